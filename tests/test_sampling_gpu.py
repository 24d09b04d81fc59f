"""GPU tests of the device-resident dataset loader: the page gather, background-box sampling and the collation of the
kept boxes against the reference's own output (tests/golden/collate_sampled.npz) and the numpy oracle
(tests/sampling_oracle.py), DeviceDataset against DeviceCollate, and a training trajectory fed both ways.  Everything
here is integer / byte work or bit-reproducible arithmetic: every comparison is exact."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import engine, pipeline, weights  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceCollate, DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
from oracle import cova_oracle as O  # noqa: E402
import sampling_oracle as SO  # noqa: E402
from config_cases import SPLIT_CFG as CFG  # noqa: E402
from helpers import DEV, profiled  # noqa: E402
from trainer_cases import page_set  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("images", "bboxes", "labels", "context_indices", "additional_feats", "page_start")


def make_rows(rs, n, labelled, size=500.0):
    """[n,5] rows with ``labelled`` boxes (an int count, or "all") at random positions."""
    r = np.zeros((n, 5), np.float32)
    r[:, :4] = rs.uniform(1, size, (n, 4))
    if labelled == "all":
        r[:, 4] = rs.randint(1, 4, n)
    else:
        k = min(int(labelled), n)
        r[rs.permutation(n)[:k], 4] = (np.arange(k) % 3) + 1
    return r


def assert_batch_equals(got, ref, keys=KEYS):
    for k in keys:
        g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else np.asarray(got[k])
        r = ref[k].cpu().numpy() if torch.is_tensor(ref[k]) else np.asarray(ref[k])
        assert g.shape == r.shape and g.dtype == r.dtype and np.array_equal(g, r), k


# ---------------------------------------------------------------- 5. injected keys against the reference's output
@pytest.mark.parametrize("f", [0, 1])
def test_injected_keys_reproduce_the_reference_fixture_bit_exact(f):
    fx = np.load(GOLDEN + "/collate_sampled.npz")
    cuts = np.cumsum(fx["counts"])[:-1]
    rows = np.split(fx["rows"], cuts)
    keys = np.concatenate([SO.keys_from_permutation(p) for p in np.split(fx["sf%d/perms" % f], cuts)])
    sf, A = float(fx["fractions"][f]), fx["additional_feats_in"].shape[1]
    got = DeviceCollate(int(fx["context_size"]), DEV, n_additional_feat=A, sampling_fraction=sf)(
        fx["u8_pages"], rows, additional_feats=fx["additional_feats_in"], keys=keys)
    assert np.array_equal(got["images"].cpu().numpy(), fx["images"])
    for k in ("bboxes", "labels", "context_indices", "additional_feats"):
        ref = fx["sf%d/%s" % (f, k)]
        g = got[k].cpu().numpy()
        assert g.dtype == ref.dtype and np.array_equal(g, ref), k
    assert got["page_start"].cpu().tolist() == [0] + np.cumsum(fx["sf%d/kept_per_page" % f]).tolist()


# ---------------------------------------------------------------- 6. hash path against the oracle
HASH_CASES = {
    # name: (counts, labelled per page, context_size, A, sampling_fraction)
    "one_box_pages": ([1, 1, 1, 4], [0, 1, 0, 1], 3, 0, 0.9),                  # m = int(0.9 * 1) = 0
    "all_background_may_empty": ([1, 3, 2, 30, 3], [0, 0, 0, 0, 0], 2, 0, 0.3),      # pages of 1..3 boxes keep nothing
    "nothing_kept_at_all": ([1], [0], 4, 2, 0.5),                               # N_out = 0
    "all_labelled": ([5, 17, 1], ["all", "all", "all"], 3, 0, 0.5),
    "context_0": ([12, 7, 33], [3, 3, 3], 0, 0, 0.9),
    "context_larger_than_page": ([4, 9, 2], [1, 2, 0], 12, 0, 0.9),
    "single_page": ([90], [3], 12, 0, 0.9),
    "additional_feats": ([11, 84, 0, 23], [3, 3, 0, 3], 5, 7, 0.9),
    "page_of_5000": ([13, 5000, 40], [3, 3, 3], 6, 1, 0.9),                    # three LDS tiles, 20 chunks of 256 boxes
    "page_of_2048_and_2049": ([2048, 2049], [3, 3], 2, 0, 0.5),                # the tile boundary
    "batch_of_200": (None, None, 12, 0, 0.9),
}


@pytest.mark.parametrize("name", list(HASH_CASES))
def test_hash_sampling_matches_the_oracle_bit_exact(name):
    counts, labelled, cs, A, sf = HASH_CASES[name]
    rs = np.random.RandomState(len(name) * 13 + 1)
    if counts is None:
        counts = rs.randint(0, 231, 200).tolist()
        labelled = [3] * 200
    B, seed, epoch = len(counts), 41, 6
    u8 = rs.randint(0, 256, (B, 4, 6, 3)).astype(np.uint8)
    rows = [make_rows(rs, n, l) for n, l in zip(counts, labelled)]
    addl = [rs.standard_normal((n, A)).astype(np.float32) for n in counts] if A else None
    page_ids = rs.permutation(7000)[:B]
    got = DeviceCollate(cs, DEV, n_additional_feat=A, sampling_fraction=sf, seed=seed)(
        u8, rows, additional_feats=np.concatenate(addl, 0) if A else None, page_ids=page_ids, epoch=epoch)
    ref = SO.collate(u8, rows, cs, sf, seed=seed, epoch=epoch, page_ids=page_ids, additional_feats=addl)
    assert_batch_equals(got, ref)
    if name in ("one_box_pages", "all_background_may_empty"):
        assert (np.diff(ref["page_start"]) == 0).any()                         # an empty page is among the cases
    if name == "nothing_kept_at_all":
        assert ref["page_start"].tolist() == [0, 0] and tuple(got["bboxes"].shape) == (0, 5)
    if name == "all_labelled":
        assert ref["page_start"][-1] == sum(counts)
    # default page ids are the batch positions
    got = DeviceCollate(cs, DEV, n_additional_feat=A, sampling_fraction=sf, seed=seed)(
        u8, rows, additional_feats=np.concatenate(addl, 0) if A else None, epoch=epoch)
    assert_batch_equals(got, SO.collate(u8, rows, cs, sf, seed=seed, epoch=epoch, additional_feats=addl))


def test_injected_keys_with_ties_go_to_the_lower_index():
    rs = np.random.RandomState(3)
    counts = [40, 300]
    rows = [make_rows(rs, n, 2) for n in counts]
    keys = [rs.randint(0, 5, n).astype(np.int64) for n in counts]            # heavy ties
    u8 = rs.randint(0, 256, (2, 4, 4, 3)).astype(np.uint8)
    got = DeviceCollate(3, DEV, sampling_fraction=0.5)(u8, rows, keys=np.concatenate(keys))
    assert_batch_equals(got, SO.collate(u8, rows, 3, 0.5, keys_per_page=keys))
    with pytest.raises(ValueError, match="keys"):
        DeviceCollate(3, DEV, sampling_fraction=0.5)(u8, rows, keys=-np.concatenate(keys) - 1)
    with pytest.raises(ValueError, match="page_ids"):
        DeviceCollate(3, DEV, sampling_fraction=0.5)(u8, rows, page_ids=[1])


# ---------------------------------------------------------------- 7. sampling_fraction = 1 is today's path
def test_fraction_one_is_the_unsampled_path_without_a_sampling_launch():
    rs = np.random.RandomState(8)
    counts = [7, 40, 2, 13]
    u8 = rs.randint(0, 256, (4, 24, 36, 3)).astype(np.uint8)
    rows = [make_rows(rs, n, 3) for n in counts]
    got, launches = profiled(lambda: DeviceCollate(5, DEV, sampling_fraction=1.0, seed=9)(u8, rows, page_ids=[5, 6, 7, 8],
                                                                                        epoch=3))
    assert launches == {"cova_images_u8_to_f32": 1, "cova_collate_boxes": 1}
    ref = O.collate_reference(u8, rows, 5)
    for k in ("images", "bboxes", "labels", "context_indices", "additional_feats"):
        assert np.array_equal(got[k].cpu().numpy(), ref[k].numpy()), k
    assert got["page_start"].cpu().tolist() == [0] + np.cumsum(counts).tolist()
    fx = np.load(GOLDEN + "/collate_raw.npz")
    got = DeviceCollate(int(fx["context_size"]), DEV, sampling_fraction=1)(
        fx["u8_pages"], np.split(fx["rows"], np.cumsum(fx["counts"])[:-1]))
    for k in ("images", "bboxes", "labels", "context_indices"):
        assert np.array_equal(got[k].cpu().numpy(), fx[k]), k
    # and a sampled call does issue the sampling entry points, once each
    _, launches = profiled(lambda: DeviceCollate(5, DEV, sampling_fraction=0.9)(u8, rows))
    assert launches == {"cova_images_u8_to_f32": 1, "cova_sample_boxes": 1, "cova_collate_selected": 1}


# ---------------------------------------------------------------- 8. page gather
def to_f32(u8):
    out = torch.empty((u8.shape[0], 3, u8.shape[1], u8.shape[2]), dtype=torch.float32, device=DEV)
    engine.call("cova_images_u8_to_f32", u8.contiguous(), out, u8.shape[0], u8.shape[1], u8.shape[2])
    return out


def gather(store, idx):
    P, H, W, _ = store.shape
    idx_d = torch.tensor(idx, dtype=torch.int32, device=DEV)
    out = torch.empty((len(idx), 3, H, W), dtype=torch.float32, device=DEV)
    engine.call("cova_pages_u8_gather_f32", store, idx_d, P, len(idx), H, W, out)
    return out


@pytest.mark.parametrize("P,H,W", [(9, 32, 48), (9, 5, 7), (6, 33, 35), (3, 1280, 1280)])   # vector path; H*W % 4 != 0: scalar path
def test_gather_equals_totensor_of_the_same_pages(P, H, W):
    rs = np.random.RandomState(P * H)
    store = torch.from_numpy(rs.randint(0, 256, (P, H, W, 3)).astype(np.uint8)).to(DEV)
    idx = [P - 1, 0, 2, 2, 1, P - 1, 0, 2]                                   # repeated and permuted
    got = gather(store, idx)
    ref = to_f32(torch.stack([store[i] for i in idx]))
    assert torch.equal(got, ref)
    host = np.transpose(store.cpu().numpy()[idx], (0, 3, 1, 2)).astype(np.float32) / np.float32(255)     # IEEE division
    assert np.array_equal(got.cpu().numpy(), host)


def test_gather_from_a_store_above_4_gib():
    H = W = 1024
    page = H * W * 3
    P = (4 << 30) // page + 36                                               # 1401 pages, 4.1 GiB
    edge = (4 << 30) // page                                                 # page 1365 straddles the 4 GiB offset
    store = torch.empty((P, H, W, 3), dtype=torch.uint8, device=DEV)
    assert store.numel() > (4 << 30)
    g = torch.Generator(device=DEV).manual_seed(5)
    for lo in range(0, P, 100):
        n = min(100, P - lo)
        store[lo:lo + n] = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=DEV, generator=g)
    idx = [edge + 1, 0, edge - 1, edge, P - 1, 3, edge, edge + 20]
    got = gather(store, idx)
    ref = to_f32(torch.stack([store[i] for i in idx]))
    assert torch.equal(got, ref)
    assert not torch.equal(got[0], got[1])
    del store, got, ref
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 9. DeviceDataset
def small_dataset(P=13, H=16, W=20, A=2, seed=21):
    rs = np.random.RandomState(seed)
    u8 = rs.randint(0, 256, (P, H, W, 3)).astype(np.uint8)
    counts = rs.randint(0, 60, P).tolist()
    counts[1], counts[4] = 1, 0
    rows = [make_rows(rs, n, 3, size=10.0) for n in counts]
    addl = [rs.standard_normal((n, A)).astype(np.float32) for n in counts] if A else None
    return u8, rows, addl


def host_batch(u8, rows, addl, ids, cs, sf, seed, epoch):
    A = addl[0].shape[1] if addl else 0
    af = np.concatenate([addl[i] for i in ids], 0) if addl else None
    return DeviceCollate(cs, DEV, n_additional_feat=A, sampling_fraction=sf, seed=seed)(
        u8[ids], [rows[i] for i in ids], additional_feats=af, page_ids=ids, epoch=epoch)


@pytest.mark.parametrize("sf", [0.9, 0.5, 1.0])
def test_dataset_batches_equal_device_collate_on_the_same_pages(sf):
    u8, rows, addl = small_dataset()
    names = ["page-%02d" % i for i in range(len(rows))]
    ds = DeviceDataset(u8, rows, 4, DEV, additional_feats=addl, img_ids=names)
    plan = pipeline.epoch_plan(len(ds), 5, True, 17, 2)
    n = 0
    for ids, got in zip(plan, ds.batches(5, shuffle=True, sampling_fraction=sf, seed=17, epoch=2)):
        ref = host_batch(u8, rows, addl, ids, 4, sf, 17, 2)
        assert_batch_equals(got, ref)
        assert got["page_ids"].dtype == torch.int64 and got["page_ids"].cpu().tolist() == ids.tolist()
        assert got["img_ids"].tolist() == [names[i] for i in ids]
        if sf == 1.0:
            assert got["labels"].numel() == sum(rows[i].shape[0] for i in ids)
        n += 1
    assert n == len(plan) == 3 and sorted(np.concatenate(plan).tolist()) == list(range(13))
    # val / test loaders: batch 10, in order, nothing sampled (datasets.py:236-258)
    got = list(ds.batches(10))
    assert [b["page_ids"].cpu().tolist() for b in got] == [list(range(10)), [10, 11, 12]]
    assert_batch_equals(got[1], host_batch(u8, rows, addl, np.arange(10, 13), 4, 1.0, 0, 0))


def test_dataset_accepts_numpy_host_device_tensors_and_lists():
    u8, rows, _ = small_dataset(P=5, A=0)
    stores = [DeviceDataset(src, rows, 2, DEV).store for src in
              (u8, torch.from_numpy(u8), torch.from_numpy(u8).to(DEV), [p for p in u8], [torch.from_numpy(p) for p in u8])]
    for s in stores:
        assert s.dtype == torch.uint8 and s.is_cuda and np.array_equal(s.cpu().numpy(), u8)
    old, DeviceDataset.STAGING_BYTES = DeviceDataset.STAGING_BYTES, 2 * u8[0].nbytes      # staging of two pages: three chunks
    try:
        assert np.array_equal(DeviceDataset(u8, rows, 2, DEV).store.cpu().numpy(), u8)
    finally:
        DeviceDataset.STAGING_BYTES = old
    ds = DeviceDataset(u8, rows, 2, DEV)
    with pytest.raises(ValueError, match="order"):
        list(ds.batches(2, order=[0, 5]))
    with pytest.raises(ValueError, match="sampling_fraction"):
        ds.batches(2, sampling_fraction=0.0)


def test_dataset_without_sampling_reads_nothing_back(monkeypatch):
    u8, rows, addl = small_dataset()
    ds = DeviceDataset(u8, rows, 4, DEV, additional_feats=addl)

    def refuse(*a):
        raise AssertionError("host read with sampling_fraction == 1")
    monkeypatch.setattr(pipeline, "_read_kept_total", refuse)
    for prefetch in (False, True):
        assert len(list(ds.batches(4, shuffle=True, seed=1, prefetch=prefetch))) == 4
    with pytest.raises(AssertionError, match="host read"):
        list(ds.batches(4, sampling_fraction=0.9, prefetch=False))


def epoch_tensors(ds, **kw):
    out = []
    for b in ds.batches(**kw):
        out.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()})
    torch.cuda.synchronize()
    return out


def test_dataset_epochs_are_reproducible_and_prefetch_changes_nothing():
    u8, rows, addl = small_dataset()
    ds = DeviceDataset(u8, rows, 4, DEV, additional_feats=addl)
    kw = dict(batch_size=3, shuffle=True, sampling_fraction=0.9, seed=5)
    a = epoch_tensors(ds, epoch=0, prefetch=True, **kw)
    b = epoch_tensors(ds, epoch=0, prefetch=False, **kw)
    c = epoch_tensors(ds, epoch=0, prefetch=True, **kw)
    d = epoch_tensors(ds, epoch=1, prefetch=True, **kw)
    assert len(a) == len(b) == len(c) == len(d) == 5
    for x, y, z in zip(a, b, c):
        assert_batch_equals(x, y, KEYS + ("page_ids", "img_ids"))
        assert_batch_equals(x, z, KEYS + ("page_ids", "img_ids"))
    assert [x["page_ids"].tolist() for x in a] != [x["page_ids"].tolist() for x in d]           # another order ...
    kept = lambda ep: {int(p): x["bboxes"][int(x["page_start"][i]):int(x["page_start"][i + 1]), 1:].cpu().numpy()
                       for x in ep for i, p in enumerate(x["page_ids"].tolist())}
    ka, kd = kept(a), kept(d)
    assert set(ka) == set(kd) == set(range(13))
    assert any(ka[p].shape != kd[p].shape or not np.array_equal(ka[p], kd[p]) for p in ka)       # ... and another sample


def test_a_pages_sample_does_not_depend_on_batch_size_or_position():
    u8, rows, addl = small_dataset()
    ds = DeviceDataset(u8, rows, 4, DEV, additional_feats=addl)

    def kept(**kw):
        out = {}
        for x in ds.batches(sampling_fraction=0.5, seed=3, epoch=7, **kw):
            ps = x["page_start"].tolist()
            for i, p in enumerate(x["page_ids"].tolist()):
                out[p] = (x["bboxes"][ps[i]:ps[i + 1], 1:].cpu().numpy(), x["labels"][ps[i]:ps[i + 1]].cpu().numpy(),
                          x["additional_feats"][ps[i]:ps[i + 1]].cpu().numpy())
        return out
    ref = kept(batch_size=13)
    for kw in (dict(batch_size=1), dict(batch_size=5), dict(batch_size=4, order=list(range(12, -1, -1))),
               dict(batch_size=3, shuffle=True), dict(batch_size=2, rank=1, world_size=2, order=list(range(13)) + [0])):
        got = kept(**kw)
        assert got and set(got) <= set(ref)
        for p, parts in got.items():
            for g, r in zip(parts, ref[p]):
                assert np.array_equal(g, r), (kw, p)
    for p, (bb, lab, _) in ref.items():                                   # and it is the oracle's sample of that page
        idx = SO.select(rows[p], int(0.5 * rows[p].shape[0]), SO.hash_keys(3, 7, p, rows[p].shape[0]))
        assert np.array_equal(lab, rows[p][idx, 4].astype(np.int64)) and np.array_equal(bb[:, :2], rows[p][idx, :2])


# ---------------------------------------------------------------- 10. trajectory
def test_ten_train_steps_fed_by_the_dataset_equal_host_fed_steps_bit_for_bit():
    u8, rows = page_set()
    sd = weights.seeded_state_dict(77, logit_gain=2.0, **{k: v for k, v in CFG.items() if k != "drop_prob"})
    cs, bs, sf, seed = 6, 3, 0.9, 12
    ds = DeviceDataset(u8, rows, cs, DEV)
    a, b = HotPathTrainer(CFG, sd, DEV), HotPathTrainer(CFG, sd, DEV)
    losses_a, losses_b, boxes = [], [], 0
    for epoch in range(2):                                                    # 5 steps per epoch
        for batch in ds.batches(bs, shuffle=True, sampling_fraction=sf, seed=seed, epoch=epoch):
            losses_a.append(a.train_step(batch)[0])
            boxes += batch["labels"].numel()
        for ids in pipeline.epoch_plan(len(ds), bs, True, seed, epoch):
            losses_b.append(b.train_step(host_batch(u8, rows, None, ids, cs, sf, seed, epoch))[0])
    assert len(losses_a) == len(losses_b) == 10 and boxes < 2 * sum(r.shape[0] for r in rows)
    assert [float(x) for x in losses_a] == [float(x) for x in losses_b]
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and any("running_mean" in k for k in sa)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert not torch.equal(sa["convnet.0.weight"], sd["convnet.0.weight"].to(DEV))          # the steps did train
    # evaluation over the resident split at batch 10 against the same batches collated from the host
    for got in ds.batches(10):
        ids = got["page_ids"].cpu().numpy()
        ref = host_batch(u8, rows, None, ids, cs, 1.0, 0, 0)
        for k in (1, 3):
            topk_a, ok_a = a.evaluate(got, got["page_start"], k=k)
            topk_b, ok_b = b.evaluate(ref, ref["page_start"], k=k)
            assert torch.equal(topk_a, topk_b) and torch.equal(ok_a, ok_b)
