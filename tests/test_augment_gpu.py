"""GPU tests of the page augmentation: cova_pages_u8_augment_f32 and cova_boxes_translate through the C ABI against the numpy
oracle (tests/augment_oracle.py), DeviceDataset.batches(augment=) / DeviceCollate(augment=) against the oracle applied to the
unaugmented batch, launch counts, and a training trajectory.  Byte moves and bit-reproducible float32 arithmetic: every
comparison is exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import _lib, engine, evaluation, pipeline  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceCollate, DeviceDataset, PageAugment  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
import augment_oracle as AO  # noqa: E402
import graph_oracle as GO  # noqa: E402
from helpers import DEV, load_case, profiled  # noqa: E402

SENTINEL = 7.0
FILLS = (0x000000, 0xFFFFFF, 0x010203)
KEYS = ("images", "bboxes", "labels", "context_indices", "additional_feats", "page_start")


def same(a, b):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def run(store, idx, B, shift, color, fill, out=None):
    """One cova_pages_u8_augment_f32 launch into a sentinel-prefilled (or the given) output -> numpy [B,3,H,W]."""
    P, H, W, _ = store.shape
    idx_d = None if idx is None else torch.tensor(list(idx), dtype=torch.int32, device=DEV)
    sh_d = None if shift is None else torch.from_numpy(np.asarray(shift, dtype=np.int64).astype(np.int32).reshape(B, 2)).to(DEV)
    co_d = None if color is None else torch.from_numpy(np.ascontiguousarray(color, dtype=np.float32).reshape(B, 12)).to(DEV)
    if out is None:
        out = torch.full((B, 3, H, W), SENTINEL, dtype=torch.float32, device=DEV)
    engine.call("cova_pages_u8_augment_f32", store, idx_d, P, B, H, W, sh_d, co_d, fill, out)
    return out.cpu().numpy()


def gather(store, idx):
    P, H, W, _ = store.shape
    out = torch.full((len(idx), 3, H, W), SENTINEL, dtype=torch.float32, device=DEV)
    engine.call("cova_pages_u8_gather_f32", store, torch.tensor(list(idx), dtype=torch.int32, device=DEV), P, len(idx), H, W, out)
    return out.cpu().numpy()


def deltas(n):
    return sorted({0, 1, -1, 2, -2, 3, -3, 4, -4, 5, -5, n - 1, 1 - n, n, -n, n + 3, -n - 3})


def shift_list(H, W):
    dxs, dys = deltas(W), deltas(H)
    mixed = [(dxs[i % len(dxs)], dys[(3 * i + 1) % len(dys)]) for i in range(max(len(dxs), len(dys)))]
    return [(dx, 0) for dx in dxs] + [(0, dy) for dy in dys] + mixed + [(AO.INT_MAX, -AO.INT_MAX)]


def random_color(rs, B):
    """Matrices in [-2,2], offsets in [-1,1]: both clamps and negative intermediates occur."""
    m = rs.uniform(-2, 2, (B, 12)).astype(np.float32)
    m[:, 3::4] = rs.uniform(-1, 1, (B, 3))
    return m


def make_store(rs, P, H, W):
    store = rs.randint(0, 256, (P, H, W, 3)).astype(np.uint8)
    if H * W == 256:                                         # every byte value in every channel, in three different orders
        for c, (mul, off) in enumerate(((1, 0), (7, 3), (-5, 100))):
            store[0, :, :, c] = ((np.arange(256) * mul + off) % 256).reshape(H, W)
    return store


# ---------------------------------------------------------------- 1. the kernel against the oracle
@pytest.mark.parametrize("H,W", [(1, 1), (3, 4), (5, 7), (6, 12), (8, 8), (16, 16), (64, 64)])
def test_augment_kernel_matches_the_oracle_bit_exact(H, W):
    rs = np.random.RandomState(H * 100 + W)
    P = 3
    store = make_store(rs, P, H, W)
    store_d = torch.from_numpy(store).to(DEV)
    shifts = shift_list(H, W)
    B = len(shifts)
    idx = [b % P for b in range(B)]                          # B > P: every source page repeated
    tables = {"null": None, "identity": AO.identity(B), "random": random_color(rs, B), "inversion": AO.inversion(B)}
    for fill in FILLS:
        for name, color in tables.items():
            got = run(store_d, idx, B, shifts, color, fill)
            ref = AO.pages(store, idx, shifts, color, fill)
            assert got.dtype == ref.dtype and np.array_equal(got, ref), (hex(fill), name)
            assert not np.signbit(got).any(), (hex(fill), name)
    fb = (AO.fill_bytes(0x010203).astype(np.float32) / np.float32(255))[:, None, None]
    assert np.array_equal(got[-1], np.broadcast_to(np.float32(1) - fb, (3, H, W)))   # +-(2**31-1): all fill (inverted here)
    assert H * W != 256 or all(len(np.unique(store[0, :, :, c])) == 256 for c in range(3))


def test_augment_without_parameters_is_the_plain_gather():
    for P, H, W in ((5, 8, 8), (4, 5, 7), (3, 6, 12), (3, 33, 36)):
        rs = np.random.RandomState(P + H)
        store = rs.randint(0, 256, (P, H, W, 3)).astype(np.uint8)
        store_d = torch.from_numpy(store).to(DEV)
        idx = [P - 1, 0, 2, 2, 1, P - 1, 0]
        ref = gather(store_d, idx)
        assert np.array_equal(run(store_d, idx, len(idx), None, None, 0x123456), ref)
        assert np.array_equal(run(store_d, idx, len(idx), np.zeros((len(idx), 2)), None, 0), ref)
        assert np.array_equal(run(store_d, idx, len(idx), np.zeros((len(idx), 2)), AO.identity(len(idx)), 0xFFFFFF), ref)
        # page_idx NULL: the pages in place (B <= P)
        assert np.array_equal(run(store_d, None, P - 1, None, None, 0), gather(store_d, range(P - 1)))
        sh = [(1, -1)] * P
        assert np.array_equal(run(store_d, None, P, sh, None, 0x0A0B0C), AO.pages(store, None, sh, None, 0x0A0B0C))


def test_an_index_outside_the_store_leaves_its_page_unwritten():
    rs = np.random.RandomState(3)
    for H, W in ((8, 8), (5, 7)):
        store = rs.randint(0, 256, (4, H, W, 3)).astype(np.uint8)
        idx, shifts = [0, 4, -1, 3, 2 ** 31 - 1, 1], [(1, 1), (0, 0), (2, 0), (-3, 2), (0, 0), (0, -1)]
        color = random_color(rs, 6)
        got = run(torch.from_numpy(store).to(DEV), idx, 6, shifts, color, 0x808080)
        ref = AO.pages(store, idx, shifts, color, 0x808080, out=np.full((6, 3, H, W), SENTINEL, np.float32))
        assert np.array_equal(got, ref)
        assert (got[[1, 2, 4]] == SENTINEL).all() and not (got[[0, 3, 5]] == SENTINEL).any()


def test_a_store_at_an_odd_address_takes_the_scalar_path_with_the_same_bytes():
    rs = np.random.RandomState(4)
    P, H, W = 3, 8, 12
    store = rs.randint(0, 256, (P, H, W, 3)).astype(np.uint8)
    buf = torch.zeros(P * H * W * 3 + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = torch.from_numpy(store).to(DEV).reshape(-1)
    view = buf[1:].view(P, H, W, 3)
    assert view.data_ptr() % 2 == 1
    shifts, idx = [(1, 0), (-2, 1), (3, -1), (4, 2), (0, 0), (-5, -3)], [2, 2, 1, 0, 2, 1]
    color = random_color(rs, 6)
    got = run(view, idx, 6, shifts, color, 0x010203)
    assert np.array_equal(got, AO.pages(store, idx, shifts, color, 0x010203))
    assert np.array_equal(got, run(torch.from_numpy(store).to(DEV), idx, 6, shifts, color, 0x010203))     # the vector path


def test_the_last_page_of_the_store_at_every_byte_residue():
    rs = np.random.RandomState(5)
    P, H, W = 2, 4, 8
    store = rs.randint(0, 256, (P, H, W, 3)).astype(np.uint8)
    store_d = torch.from_numpy(store).to(DEV)                # an allocation of exactly the store's size
    shifts = [(d, 0) for d in (1, 2, 3, -1, -2, -3, 0, 4, -4, 5, -7)]
    idx = [P - 1] * len(shifts)
    for color in (None, random_color(rs, len(shifts))):
        assert np.array_equal(run(store_d, idx, len(shifts), shifts, color, 0x010203),
                              AO.pages(store, idx, shifts, color, 0x010203))


def test_two_full_size_pages():
    rs = np.random.RandomState(6)
    store = rs.randint(0, 256, (2, 1280, 1280, 3)).astype(np.uint8)
    shifts, color = [(37, -501), (37, -501)], random_color(rs, 2)
    got = run(torch.from_numpy(store).to(DEV), [1, 0], 2, shifts, color, 0xFFFFFF)
    assert np.array_equal(got, AO.pages(store, [1, 0], shifts, color, 0xFFFFFF))


def test_the_last_page_of_a_store_above_4_gib():
    H = W = 1024
    page = H * W * 3
    P = (4 << 30) // page + 36                               # 1401 pages, 4.1 GiB
    store = torch.empty((P, H, W, 3), dtype=torch.uint8, device=DEV)
    assert store.numel() > (4 << 30)
    last = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    store[P - 1] = last
    rs = np.random.RandomState(7)
    shifts, color = [(-3, 2), (0, 0)], random_color(rs, 2)
    got = run(store, [P - 1, P - 1], 2, shifts, color, 0x010203)
    assert np.array_equal(got, AO.pages(last.cpu().numpy()[None], [0, 0], shifts, color, 0x010203))
    del store
    torch.cuda.empty_cache()


def test_augment_status_returns():
    store = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device=DEV)
    out = torch.full((3, 3, 4, 4), SENTINEL, dtype=torch.float32, device=DEV)
    idx = torch.zeros(3, dtype=torch.int32, device=DEV)
    call = lambda *a: engine.call("cova_pages_u8_augment_f32", *a)  # noqa: E731
    for args in ((store, idx, 2, 3, 0, 4, None, None, 0, out), (store, idx, 2, 3, 4, 0, None, None, 0, out),
                 (store, idx, 0, 3, 4, 4, None, None, 0, out), (None, idx, 2, 3, 4, 4, None, None, 0, out),
                 (store, idx, 2, 3, 4, 4, None, None, 0, None), (store, None, 2, 3, 4, 4, None, None, 0, out),
                 (store, idx, 2, -1, 4, 4, None, None, 0, out)):
        with pytest.raises(_lib.CovaHipError):
            call(*args)
    call(store, idx, 2, 0, 4, 4, None, None, 0, out)                                          # B == 0: accepted, no launch
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    with pytest.raises(_lib.CovaHipError):
        engine.call("cova_boxes_translate", None, 3, idx, 1)
    with pytest.raises(_lib.CovaHipError):
        engine.call("cova_boxes_translate", out, 3, None, 1)


# ---------------------------------------------------------------- 2. boxes
def translate(bb, shift):
    bb_d = torch.from_numpy(np.ascontiguousarray(bb, dtype=np.float32)).to(DEV)
    sh_d = torch.from_numpy(np.asarray(shift, dtype=np.int32).reshape(-1, 2)).to(DEV)
    engine.call("cova_boxes_translate", bb_d if bb_d.numel() else None, bb_d.shape[0], sh_d, sh_d.shape[0])
    return bb_d.cpu().numpy()


def test_boxes_translate_matches_the_oracle():
    rs = np.random.RandomState(8)
    for counts in ([0], [1], [5, 0, 17, 1, 300], rs.randint(0, 9, 200).tolist()):
        B = len(counts)
        bb = rs.uniform(-50, 1500, (sum(counts), 5)).astype(np.float32)            # non-integer coordinates
        bb[:, 0] = np.repeat(np.arange(B), counts)
        shift = rs.randint(-2000, 2001, (B, 2))
        shift[0] = (2000, -2000)
        got = translate(bb, shift)
        assert got.dtype == np.float32 and np.array_equal(got, AO.translate(bb, shift))
        assert sum(counts) == 0 or not np.array_equal(got, bb)
    # rows of a foreign page stay as they are; the page column truncates towards zero
    bb = rs.uniform(0, 100, (8, 5)).astype(np.float32)
    bb[:, 0] = [0, 2, 3, -1, 1e9, 2.9, -0.5, -1.5]
    got = translate(bb, [(1, 2), (3, 4), (5, 6)])
    assert np.array_equal(got, AO.translate(bb, [(1, 2), (3, 4), (5, 6)]))
    assert np.array_equal(got[[2, 3, 4, 7]], bb[[2, 3, 4, 7]]) and not np.array_equal(got[[0, 1, 5, 6]], bb[[0, 1, 5, 6]])


# ---------------------------------------------------------------- 3. DeviceDataset / DeviceCollate
AUG = dict(max_shift=(5, 7), brightness=0.2, contrast=0.3, saturation=0.4, channel_gain=0.1, invert_prob=0.3, fill=(1, 2, 3),
           seed=11)
CS = 2


def make_rows(rs, n, H, W):
    wh = rs.uniform(2, 12, (n, 2))
    xy = rs.uniform(0, 1, (n, 2)) * (np.asarray([W, H]) - wh)
    lab = np.zeros((n, 1))
    lab[rs.permutation(n)[:min(3, n)], 0] = [1, 2, 3][:min(3, n)]
    return np.concatenate([xy, wh, lab], 1).astype(np.float32)


@pytest.fixture(scope="module")
def split():
    rs = np.random.RandomState(9)
    H, W = 32, 48
    u8 = rs.randint(0, 256, (8, H, W, 3)).astype(np.uint8)
    rows = [make_rows(rs, n, H, W) for n in (9, 0, 14, 1, 22, 6, 11, 17)]
    return u8, rows


def epoch_tensors(ds, **kw):
    out = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()} for b in ds.batches(**kw)]
    torch.cuda.synchronize()
    return out


def per_page(batches):
    out = {}
    for x in batches:
        ps = x["page_start"].tolist()
        for i, p in enumerate(x["page_ids"].tolist()):
            out[p] = (x["images"][i].cpu().numpy(), x["bboxes"][ps[i]:ps[i + 1], 1:].cpu().numpy(),
                      x["labels"][ps[i]:ps[i + 1]].cpu().numpy(), x["aug_shift"][i].cpu().numpy())
    return out


@pytest.mark.parametrize("ks", [0, 3])
@pytest.mark.parametrize("sf", [1.0, 0.5])
def test_augmented_batches_are_the_oracle_applied_to_the_plain_batches(split, sf, ks):
    u8, rows = split
    ds = DeviceDataset(u8, rows, CS, DEV, spatial_k=ks)
    aug = PageAugment(**AUG)
    kw = dict(batch_size=3, shuffle=True, sampling_fraction=sf, seed=4, epoch=2)
    plain, got = epoch_tensors(ds, **kw), epoch_tensors(ds, augment=aug, **kw)
    assert len(plain) == len(got) == 3
    for a, g in zip(plain, got):
        ids = a["page_ids"].cpu().numpy()
        shift, color = aug.params(ids, 2)
        assert set(g) == set(a) | {"aug_shift"}
        assert g["aug_shift"].dtype == torch.int32 and g["aug_shift"].is_cuda and same(g["aug_shift"], shift)
        assert same(g["images"], AO.pages(u8, ids, shift, color, 0x010203))
        boxes = AO.translate(a["bboxes"].cpu().numpy(), shift)
        assert same(g["bboxes"], boxes)
        if ks:
            assert same(g["context_indices"], GO.batch_graph(boxes, a["page_start"].cpu().numpy(), CS, ks))
        for k in a:
            if k not in ("images", "bboxes") and not (ks and k == "context_indices"):
                assert same(g[k], a[k]) if torch.is_tensor(a[k]) or isinstance(a[k], np.ndarray) else g[k] == a[k], k
        # DeviceCollate on the same pages and ids
        ref = DeviceCollate(CS, DEV, sampling_fraction=sf, seed=4, spatial_k=ks, augment=aug)(
            u8[ids], [rows[i] for i in ids], page_ids=ids, epoch=2)
        for k in KEYS + ("aug_shift",):
            assert same(g[k], ref[k]), k
    # the default page ids of DeviceCollate are the positions
    ref = DeviceCollate(CS, DEV, spatial_k=ks, augment=aug)(u8[:3], rows[:3], epoch=5)
    shift, color = aug.params(np.arange(3), 5)
    assert same(ref["images"], AO.pages(u8[:3], None, shift, color, 0x010203)) and same(ref["aug_shift"], shift)


def test_a_pages_augmentation_does_not_depend_on_batch_size_rank_or_prefetch(split):
    u8, rows = split
    ds = DeviceDataset(u8, rows, CS, DEV, spatial_k=3)
    aug = PageAugment(**AUG)
    kw = dict(sampling_fraction=0.5, seed=4, epoch=1, augment=aug)
    ref = per_page(epoch_tensors(ds, batch_size=3, **kw))
    assert set(ref) == set(range(8))
    ranks = {}
    for r in (0, 1):
        ranks.update(per_page(epoch_tensors(ds, batch_size=2, rank=r, world_size=2, **kw)))
    for other in (per_page(epoch_tensors(ds, batch_size=5, shuffle=True, **kw)), ranks,
                  per_page(epoch_tensors(ds, batch_size=3, prefetch=False, **kw))):
        assert set(other) == set(ref)
        for p in ref:
            assert all(np.array_equal(x, y) for x, y in zip(other[p], ref[p])), p
    a = epoch_tensors(ds, batch_size=3, prefetch=True, **kw)
    b = epoch_tensors(ds, batch_size=3, prefetch=False, **kw)
    for x, y in zip(a, b):
        for k in KEYS + ("aug_shift", "page_ids"):
            assert same(x[k], y[k]), k
    nxt = per_page(epoch_tensors(ds, batch_size=3, **dict(kw, epoch=2)))
    assert any(not np.array_equal(nxt[p][0], ref[p][0]) for p in ref) and any(not np.array_equal(nxt[p][3], ref[p][3]) for p in ref)


def test_zero_magnitudes_equal_no_augmentation_and_launch_counts(split):
    u8, rows = split
    ds = DeviceDataset(u8, rows, CS, DEV, spatial_k=3)
    kw = dict(batch_size=3, shuffle=True, sampling_fraction=0.5, seed=4, epoch=2)
    plain, lp = profiled(lambda: epoch_tensors(ds, **kw))
    zero, lz = profiled(lambda: epoch_tensors(ds, augment=PageAugment(fill=(9, 9, 9), seed=3), **kw))
    for a, z in zip(plain, zero):
        for k in a:
            assert same(z[k], a[k]) if torch.is_tensor(a[k]) or isinstance(a[k], np.ndarray) else z[k] == a[k], k
        assert not z["aug_shift"].any()
    _, lc = profiled(lambda: epoch_tensors(ds, augment=PageAugment(contrast=0.5, invert_prob=0.5), **kw))
    _, ls = profiled(lambda: epoch_tensors(ds, augment=PageAugment(max_shift=(0, 1)), **kw))
    assert lp["cova_pages_u8_gather_f32"] == 3 and "cova_pages_u8_augment_f32" not in lp and "cova_boxes_translate" not in lp
    rest = {k: v for k, v in lp.items() if k != "cova_pages_u8_gather_f32"}
    assert lz == lc == dict(rest, cova_pages_u8_augment_f32=3)                  # colour only: the boxes stay, no launch for them
    assert ls == dict(rest, cova_pages_u8_augment_f32=3, cova_boxes_translate=3)
    with pytest.raises(ValueError, match="max_shift"):
        ds.batches(3, augment=PageAugment(max_shift=(48, 0)))
    with pytest.raises(ValueError, match="features"):
        ds.batches(3, features=object(), augment=PageAugment())


# ---------------------------------------------------------------- 4. training
@pytest.fixture(scope="module")
def small_model():
    fx, cfg, sd, _ = load_case("cova_h64_n11")
    rs = np.random.RandomState(12)
    u8 = rs.randint(0, 256, (6, 64, 64, 3)).astype(np.uint8)
    rows = [make_rows(rs, int(n), 64, 64) for n in rs.randint(8, 20, 6)]
    return cfg, sd, int(fx["meta/context_size"]), u8, rows


def test_three_augmented_train_steps_are_reproducible_and_differ_from_plain_ones(small_model):
    cfg, sd, cs, u8, rows = small_model
    ds = DeviceDataset(u8, rows, cs, DEV)
    aug = PageAugment(max_shift=(6, 6), brightness=0.2, contrast=0.3, saturation=0.3, invert_prob=0.5, seed=2)

    def trained(augment):
        tr = HotPathTrainer(cfg, sd, DEV)
        n = 0
        for batch in ds.batches(2, shuffle=True, sampling_fraction=0.9, seed=1, epoch=0, augment=augment):
            tr.train_step(batch)
            n += 1
        assert n == 3
        return tr.state_dict()
    a, b, c = trained(aug), trained(aug), trained(None)
    assert list(a) == list(b) == list(c)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["convnet.0.weight"], c["convnet.0.weight"])


def test_fit_augments_the_training_batches_and_never_the_evaluation(small_model, monkeypatch):
    cfg, sd, cs, u8, rows = small_model
    train, val = DeviceDataset(u8, rows, cs, DEV), DeviceDataset(u8[:4], rows[:4], cs, DEV)
    tr = HotPathTrainer(cfg, sd, DEV, track_metrics=True)
    seen = []
    real = evaluation.evaluate_split
    count = lambda n: len(_lib.PROFILE[n])  # noqa: E731

    def watched(*a, **kw):
        before = (count("cova_pages_u8_augment_f32"), count("cova_boxes_translate"), count("cova_pages_u8_gather_f32"))
        out = real(*a, **kw)
        seen.append((before, (count("cova_pages_u8_augment_f32"), count("cova_boxes_translate"),
                              count("cova_pages_u8_gather_f32"))))
        return out
    monkeypatch.setattr(evaluation, "evaluate_split", watched)
    res, launches = profiled(lambda: evaluation.fit(tr, train, val, n_epochs=1, batch_size=2, seed=3,
                                                    augment=PageAugment(max_shift=(4, 4), contrast=0.2)))
    assert res.epochs_run == 1 and len(seen) == 1
    (before, after), = seen
    assert before == (3, 3, 0) and after == (3, 3, 1)                         # 3 training steps; one evaluation batch, plain
    assert launches["cova_pages_u8_augment_f32"] == 3 and launches["cova_pages_u8_gather_f32"] == 1
    with pytest.raises(ValueError, match="train_features"):
        evaluation.fit(tr, train, val, 1, 2, train_features=object(), augment=PageAugment())
