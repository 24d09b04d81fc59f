"""Host side of the device-resident dataset loader (no GPU): the numpy oracle of the sampled collation against the
reference's own output, the quality of the key hash, epoch_plan, and the declared entry points."""
import ctypes
import os

import numpy as np
import pytest

import cova_amd  # noqa: F401
from cova_web_object_detection_amd import _lib, pipeline
from cova_web_object_detection_amd.trainer import shard_pages

import sampling_oracle as SO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_fixture():
    fx = np.load(GOLDEN + "/collate_sampled.npz")
    cuts = np.cumsum(fx["counts"])[:-1]
    return fx, np.split(fx["rows"], cuts), np.split(fx["additional_feats_in"], cuts)


@pytest.mark.parametrize("f", [0, 1])
def test_oracle_reproduces_the_reference_sampled_collation_bit_exact(f):
    fx, rows, addl = load_fixture()
    assert len(fx["counts"]) >= 4 and len(set(fx["counts"].tolist())) > 1 and int(fx["context_size"]) > 0
    assert list(fx["fractions"]) == [0.9, 0.5] and fx["additional_feats_in"].shape[1] > 0
    sf = float(fx["fractions"][f])
    perms = np.split(fx["sf%d/perms" % f], np.cumsum(fx["counts"])[:-1])
    keys = [SO.keys_from_permutation(p) for p in perms]
    got = SO.collate(fx["u8_pages"], rows, int(fx["context_size"]), sf, keys_per_page=keys, additional_feats=addl)
    assert [len(k) for k in got["kept"]] == fx["sf%d/kept_per_page" % f].tolist()
    assert sum(len(k) for k in got["kept"]) < fx["rows"].shape[0]               # something was dropped
    for k in ("bboxes", "labels", "context_indices", "additional_feats"):
        ref = fx["sf%d/%s" % (f, k)]
        assert got[k].dtype == ref.dtype and np.array_equal(got[k], ref), k
    assert np.array_equal(got["images"], fx["images"])


@pytest.mark.parametrize("n", [1, 2, 11, 84, 90, 230])
@pytest.mark.parametrize("sf", [0.9, 0.5, 0.3, 0.999])
def test_key_restatement_selects_the_reference_index_set(n, sf):
    """datasets.py:102-108 written out, against ``select`` with key[perm[j]] = j."""
    rs = np.random.RandomState(n * 7 + int(sf * 1000))
    rows = np.zeros((n, 5), np.float32)
    rows[rs.permutation(n)[:min(3, n)], 4] = [1, 2, 3][:min(3, n)]
    for _ in range(20):
        perm = rs.permutation(n)
        ref = np.unique(np.concatenate((np.where(rows[:, -1] != 0)[0], perm[:int(sf * n)])))
        assert np.array_equal(SO.select(rows, int(sf * n), SO.keys_from_permutation(perm)), ref)


def test_select_breaks_key_ties_towards_the_lower_index():
    rows = np.zeros((6, 5), np.float32)
    assert SO.select(rows, 2, np.zeros(6, np.int64)).tolist() == [0, 1]
    assert SO.select(rows, 3, np.asarray([5, 1, 5, 1, 0, 5])).tolist() == [1, 3, 4]
    rows[5, 4] = 2.0
    assert SO.select(rows, 0, np.zeros(6, np.int64)).tolist() == [5]


def test_host_key_formula_is_the_oracle_formula():
    for seed, epoch in ((0, 0), (1, 0), (0, 1), (123456789, 77), (2 ** 63 + 5, 2 ** 40)):
        assert pipeline.stream_seed(seed, epoch) == int(SO.stream_seed(seed, epoch))
    assert pipeline.mix64(3, 4) == int(SO.mix(3, 4))
    k = SO.hash_keys(5, 2, 17, 1000)
    assert k.dtype == np.int64 and (k >= 0).all() and len(set(k.tolist())) == 1000
    assert not np.array_equal(k[:90], SO.hash_keys(5, 3, 17, 90)) and not np.array_equal(k[:90], SO.hash_keys(5, 2, 18, 90))
    assert [pipeline.keep_count(0.9, n) for n in (0, 1, 10, 11, 90, 230)] == [0, 0, 9, 9, 81, 207]


def test_hash_sampling_frequencies_on_a_90_box_page():
    """4 000 (seed, epoch) draws of a 90-box page at sf 0.9: labelled boxes always kept, every background box kept with
    frequency m/n = 0.9 within 4.5 binomial standard deviations (sd = sqrt(0.9 * 0.1 / 4000) = 0.00474)."""
    n, sf, draws = 90, 0.9, 4000
    m = int(sf * n)
    rows = np.zeros((n, 5), np.float32)
    labelled = [7, 40, 88]
    rows[labelled, 4] = [1, 2, 3]
    hits = np.zeros(n, np.int64)
    for d in range(draws):
        seed, epoch = d // 50, d % 50
        kept = SO.select(rows, m, SO.hash_keys(seed, epoch, 3, n))
        assert m <= kept.shape[0] <= m + 3
        hits[kept] += 1
    assert (hits[labelled] == draws).all()
    bg = np.setdiff1d(np.arange(n), labelled)
    sd = np.sqrt((m / n) * (1 - m / n) / draws)
    dev = np.abs(hits[bg] / draws - m / n) / sd
    print("largest deviation of a background box: %.2f sd" % dev.max())
    assert dev.max() <= 4.5, dev.max()


def test_epoch_plan_covers_every_page_once_and_keeps_the_short_batch():
    plan = pipeline.epoch_plan(37, 8, True, 3, 0)
    assert [len(b) for b in plan] == [8, 8, 8, 8, 5] and all(b.dtype == np.int64 for b in plan)
    assert sorted(np.concatenate(plan).tolist()) == list(range(37))
    assert [len(b) for b in pipeline.epoch_plan(37, 8, True, 3, 0, drop_last=True)] == [8, 8, 8, 8]
    assert [b.tolist() for b in pipeline.epoch_plan(5, 2, False, 3, 9)] == [[0, 1], [2, 3], [4]]
    assert pipeline.epoch_plan(0, 4, True, 0, 0) == []


def test_epoch_plan_is_a_function_of_seed_and_epoch():
    cat = lambda p: np.concatenate(p).tolist()
    a = cat(pipeline.epoch_plan(200, 16, True, 5, 2))
    assert a == cat(pipeline.epoch_plan(200, 16, True, 5, 2)) == cat(pipeline.epoch_plan(200, 7, True, 5, 2))
    assert a != cat(pipeline.epoch_plan(200, 16, True, 5, 3)) and a != cat(pipeline.epoch_plan(200, 16, True, 6, 2))
    assert a != list(range(200))


def test_epoch_plan_honours_an_injected_order():
    order = [4, 0, 3, 3, 1]
    assert [b.tolist() for b in pipeline.epoch_plan(5, 2, True, 0, 0, order=order)] == [[4, 0], [3, 3], [1]]
    for bad in ([0, 5], [-1], [0.5]):
        with pytest.raises(ValueError, match="order"):
            pipeline.epoch_plan(5, 2, False, 0, 0, order=bad)
    with pytest.raises(ValueError):
        pipeline.epoch_plan(5, 0, False, 0, 0)
    with pytest.raises(ValueError):
        pipeline.epoch_plan(5, 2, False, 0, 0, rank=2, world_size=2)


@pytest.mark.parametrize("world", [2, 3])
def test_epoch_plan_shards_concatenate_to_the_single_process_plan(world):
    n, bs = 53, 4                                    # the short last global batch (5 pages) still feeds every rank
    single = pipeline.epoch_plan(n, bs * world, True, 11, 4)                  # the global batches
    shards = [pipeline.epoch_plan(n, bs, True, 11, 4, rank=r, world_size=world) for r in range(world)]
    assert all(len(s) == len(single) for s in shards)
    for step, glob in enumerate(single):
        assert np.concatenate([s[step] for s in shards]).tolist() == glob.tolist()
        for r in range(world):
            lo, hi = shard_pages(len(glob), r, world)
            assert shards[r][step].tolist() == glob[lo:hi].tolist()


def test_epoch_plan_drops_a_global_batch_smaller_than_the_world():
    # 13 pages, 4 ranks x 3 pages: the 13th page alone cannot feed 4 ranks
    plans = [pipeline.epoch_plan(13, 3, False, 0, 0, rank=r, world_size=4) for r in range(4)]
    assert all(len(p) == 1 for p in plans)
    assert np.concatenate([p[0] for p in plans]).tolist() == list(range(12))
    # 14 pages, 2 ranks x 3: the last global batch of 2 pages is kept, one page per rank
    plans = [pipeline.epoch_plan(14, 3, False, 0, 0, rank=r, world_size=2) for r in range(2)]
    assert [p[-1].tolist() for p in plans] == [[12], [13]]
    assert all(len(pipeline.epoch_plan(14, 3, False, 0, 0, True, r, 2)) == 2 for r in range(2))


def test_sampling_arguments_are_checked_on_the_host():
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="sampling_fraction"):
            pipeline.DeviceCollate(3, "cpu", sampling_fraction=bad)
    c = pipeline.DeviceCollate(3, "cpu")
    assert c.sf == 1.0 and c.seed == 0
    good = np.zeros((2, 4, 4, 3), np.uint8)
    rows = [np.zeros((3, 5), np.float32), np.zeros((0, 5), np.float32)]
    for pages, r, kw, match in (
            (np.zeros((2, 4, 4, 3), np.float32), rows, {}, "uint8"),
            (np.zeros((2, 4, 4), np.uint8), rows, {}, "uint8"),
            ([good[0], np.zeros((5, 4, 3), np.uint8)], rows, {}, "equal-shape"),
            (good, rows[:1], {}, "one \\[n,5\\] array per page"),
            (good, [np.zeros((3, 4), np.float32), rows[1]], {}, "page 0"),
            (good, [np.full((3, 5), np.nan, np.float32), rows[1]], {}, "non-finite"),
            (good, rows, dict(additional_feats=np.zeros((4, 2), np.float32)), "additional_feats"),
            (good, rows, dict(img_ids=["a"]), "img_ids")):
        with pytest.raises(ValueError, match=match):
            pipeline.DeviceDataset(pages, r, 2, "cpu", **kw)
    with pytest.raises(ValueError, match="context_size"):
        pipeline.DeviceDataset(good, rows, -1, "cpu")


def test_sampling_entry_points_are_declared_and_exported():
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    protos = _lib.parse_header()
    for name, n_args in (("cova_pages_u8_gather_f32", 8), ("cova_sample_boxes", 13), ("cova_collate_selected", 13),
                         ("cova_sample_boxes_workspace_ints", 2)):
        assert name in protos and hasattr(cdll, name), name
        assert len(protos[name]) == n_args, name
    assert protos["cova_sample_boxes"][8] is ctypes.c_ulonglong            # the stream seed is a full 64-bit word
    for (b, n), ints in (((1, 0), 1), ((16, 1440), 1456), ((200, 5000), 5200)):
        assert _lib.query("cova_sample_boxes_workspace_ints", b, n) == ints
    assert len(protos["cova_images_u8_to_f32"]) == 6 and len(protos["cova_collate_boxes"]) == 9      # unchanged
