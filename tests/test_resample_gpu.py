"""GPU tests of the page zoom: cova_pages_u8_resample_f32 and cova_boxes_affine through the C ABI against the numpy oracle
(tests/resample_oracle.py) and, at step 65536, against cova_pages_u8_augment_f32 itself; DeviceDataset.batches(augment=) /
DeviceCollate(augment=) with a zooming PageAugment against the oracle applied to the unaugmented batch; launch counts; a
training trajectory.  Integer taps, one correctly rounded division, unfused float32 after it: every comparison is exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import _lib, engine, evaluation  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceCollate, DeviceDataset, PageAugment  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
import augment_oracle as AO  # noqa: E402
import graph_oracle as GO  # noqa: E402
import resample_oracle as RO  # noqa: E402
from helpers import DEV, load_case, np_bits as bits, profiled  # noqa: E402

SENTINEL = 7.0
FILLS = (0x000000, 0xFFFFFF, 0x123456)
KEYS = ("images", "bboxes", "labels", "context_indices", "additional_feats", "page_start")
STEPS = [(v, v) for v in (65536, 65535, 65537, 32768, 131072, 43691, 98304, 1, 1 << 22)] + [(32768, 131072), (131072, 43691)]


def same(a, b):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    if a.dtype == np.float32 and b.dtype == np.float32:
        return a.shape == b.shape and np.array_equal(bits(a), bits(b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def run(store, idx, B, step, origin, color, fill, out=None):
    """One cova_pages_u8_resample_f32 launch into a sentinel-prefilled (or the given) output -> numpy [B,3,H,W]."""
    P, H, W, _ = store.shape
    idx_d = None if idx is None else torch.tensor(list(idx), dtype=torch.int32, device=DEV)
    st_d = torch.from_numpy(np.asarray(step, dtype=np.int64).astype(np.int32).reshape(B, 2)).to(DEV)
    or_d = torch.from_numpy(np.asarray(origin, dtype=np.int64).reshape(B, 2)).to(DEV)
    co_d = None if color is None else torch.from_numpy(np.ascontiguousarray(color, dtype=np.float32).reshape(B, 12)).to(DEV)
    if out is None:
        out = torch.full((B, 3, H, W), SENTINEL, dtype=torch.float32, device=DEV)
    engine.call("cova_pages_u8_resample_f32", store, idx_d, P, B, H, W, st_d, or_d, co_d, fill, out)
    return out.cpu().numpy()


def run_shift(store, idx, B, shift, color, fill):
    P, H, W, _ = store.shape
    idx_d = torch.tensor(list(idx), dtype=torch.int32, device=DEV)
    sh_d = torch.from_numpy(np.asarray(shift, dtype=np.int32).reshape(B, 2)).to(DEV)
    co_d = None if color is None else torch.from_numpy(np.ascontiguousarray(color, dtype=np.float32).reshape(B, 12)).to(DEV)
    out = torch.full((B, 3, H, W), SENTINEL, dtype=torch.float32, device=DEV)
    engine.call("cova_pages_u8_augment_f32", store, idx_d, P, B, H, W, sh_d, co_d, fill, out)
    return out.cpu().numpy()


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


def origin_list(H, W):
    """Per axis: 0; fraction 255; tap -1 with fraction 255; the first sample exactly on the last pixel (its second tap outside
    with weight 0); three pixels before the page; far outside on either side."""
    kinds = [lambda n: 0, lambda n: 0xFF00, lambda n: -1, lambda n: (n - 1) << 16, lambda n: -(3 << 16), lambda n: 1 << 40,
             lambda n: -(1 << 40)]
    return [(k(W), k(H)) for k in kinds]


def cases(H, W):
    steps, origins = [], []
    for i, st in enumerate(STEPS):
        org = origin_list(H, W)
        for j, o in enumerate(org):
            steps.append(st)
            origins.append(o if (i + j) % 3 else (o[0], org[(j + 2) % 5][1]))      # some pairs mix the kinds of the two axes
    return steps, origins


# ---------------------------------------------------------------- 1. the kernel against the oracle
@pytest.mark.parametrize("H,W", [(1, 1), (1, 4), (4, 1), (5, 7), (3, 4), (8, 8), (6, 12), (16, 16), (64, 64), (4, 260)])
def test_resample_kernel_matches_the_oracle_bit_exact(H, W):
    rs = np.random.RandomState(H * 1000 + W)
    P = 3
    store = make_store(rs, P, H, W)
    store_d = torch.from_numpy(store).to(DEV)
    steps, origins = cases(H, W)
    B = len(steps)
    assert B == 77
    idx = [b % P for b in range(B)]                          # B > P: every source page repeated
    for fill in FILLS:
        for name, color in (("null", None), ("random", random_color(rs, B))):
            got = run(store_d, idx, B, steps, origins, color, fill)
            ref = RO.pages(store, idx, steps, origins, color, fill)
            assert got.dtype == ref.dtype and np.array_equal(bits(got), bits(ref)), (hex(fill), name)
            assert not np.signbit(got).any(), (hex(fill), name)
    assert H * W != 256 or all(len(np.unique(store[0, :, :, c])) == 256 for c in range(3))


def test_page_idx_null_repeated_and_outside_the_store():
    rs = np.random.RandomState(3)
    for H, W in ((8, 8), (5, 7)):
        P = 4
        store = rs.randint(0, 256, (P, H, W, 3)).astype(np.uint8)
        store_d = torch.from_numpy(store).to(DEV)
        # NULL: the pages in place (B <= P)
        st, org = [(43691, 98304)] * P, [(-(1 << 15), 3000)] * P
        assert np.array_equal(bits(run(store_d, None, P, st, org, None, 0x0A0B0C)), bits(RO.pages(store, None, st, org, None, 0x0A0B0C)))
        assert np.array_equal(bits(run(store_d, None, P - 1, st[:-1], org[:-1], None, 0)),
                              bits(RO.pages(store, None, st[:-1], org[:-1], None, 0)))
        # repeated, B > P, and indices outside the store on a prefilled output
        idx = [0, 4, -1, 3, 2 ** 31 - 1, 1, 3, 3]
        st = [(65536, 65536), (1, 1), (32768, 32768), (131072, 65535), (65536, 65536), (43691, 43691), (1 << 22, 1), (98304, 32768)]
        org = [(0, 0), (0, 0), (5, 5), (-70000, 1 << 16), (0, 0), (0xFF00, -1), (0, 0), (-(3 << 16), 0xFF00)]
        color = random_color(rs, 8)
        got = run(store_d, idx, 8, st, org, color, 0x808080)
        ref = RO.pages(store, idx, st, org, color, 0x808080, out=np.full((8, 3, H, W), SENTINEL, np.float32))
        assert np.array_equal(bits(got), bits(ref))
        assert (got[[1, 2, 4]] == SENTINEL).all() and not (got[[0, 3, 5, 6, 7]] == SENTINEL).any()


def test_a_store_at_an_odd_address_takes_the_scalar_path_with_the_same_bytes():
    rs = np.random.RandomState(4)
    P, H, W = 3, 8, 12
    store = rs.randint(0, 256, (P, H, W, 3)).astype(np.uint8)
    buf = torch.zeros(P * H * W * 3 + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = torch.from_numpy(store).to(DEV).reshape(-1)
    view = buf[1:].view(P, H, W, 3)
    assert view.data_ptr() % 2 == 1
    steps, origins = cases(H, W)
    idx = [b % P for b in range(len(steps))]
    color = random_color(rs, len(steps))
    got = run(view, idx, len(steps), steps, origins, color, 0x123456)
    assert np.array_equal(bits(got), bits(RO.pages(store, idx, steps, origins, color, 0x123456)))
    assert np.array_equal(bits(got), bits(run(torch.from_numpy(store).to(DEV), idx, len(steps), steps, origins, color, 0x123456)))


def test_the_last_page_of_the_store_at_every_byte_residue():
    rs = np.random.RandomState(5)
    P, H, W = 2, 4, 8
    store = rs.randint(0, 256, (P, H, W, 3)).astype(np.uint8)
    store_d = torch.from_numpy(store).to(DEV)                # an allocation of exactly the store's size
    steps, origins = [], []
    for inv in (65536, 43691, 131072, 32768):
        for d in (1, 2, 3, -1, -2, -3, 0, 4, -4, 5, -7):     # the segment's first byte at every residue modulo 4
            steps.append((inv, inv))
            origins.append((-d * 65536 + 0x8000, 0x4000))
    idx = [P - 1] * len(steps)
    for color in (None, random_color(rs, len(steps))):
        assert np.array_equal(bits(run(store_d, idx, len(steps), steps, origins, color, 0x123456)),
                              bits(RO.pages(store, idx, steps, origins, color, 0x123456)))


def test_resample_status_returns():
    store = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device=DEV)
    out = torch.full((3, 3, 4, 4), SENTINEL, dtype=torch.float32, device=DEV)
    idx = torch.zeros(3, dtype=torch.int32, device=DEV)
    st = torch.full((3, 2), 65536, dtype=torch.int32, device=DEV)
    org = torch.zeros((3, 2), dtype=torch.int64, device=DEV)
    call = lambda *a: engine.call("cova_pages_u8_resample_f32", *a)  # noqa: E731
    for args in ((store, idx, 2, 3, 0, 4, st, org, None, 0, out), (store, idx, 2, 3, 4, 0, st, org, None, 0, out),
                 (store, idx, 0, 3, 4, 4, st, org, None, 0, out), (None, idx, 2, 3, 4, 4, st, org, None, 0, out),
                 (store, idx, 2, 3, 4, 4, st, org, None, 0, None), (store, None, 2, 3, 4, 4, st, org, None, 0, out),
                 (store, idx, 2, -1, 4, 4, st, org, None, 0, out), (store, idx, 2, 3, 4, 4, None, org, None, 0, out),
                 (store, idx, 2, 3, 4, 4, st, None, None, 0, out)):
        with pytest.raises(_lib.CovaHipError):
            call(*args)
    call(store, idx, 2, 0, 4, 4, st, org, None, 0, out)                                       # B == 0: accepted, no launch
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    with pytest.raises(_lib.CovaHipError):
        engine.call("cova_boxes_affine", None, 3, out, 1)
    with pytest.raises(_lib.CovaHipError):
        engine.call("cova_boxes_affine", out, 3, None, 1)
    with pytest.raises(_lib.CovaHipError):
        engine.call("cova_boxes_affine", out, 3, out, 0)


def test_two_full_size_pages():
    rs = np.random.RandomState(6)
    store = rs.randint(0, 256, (2, 1280, 1280, 3)).astype(np.uint8)
    steps, origins, color = [(47836, 47836)] * 2, [(11184811, -1234567), (-40000000, 777)], random_color(rs, 2)
    got = run(torch.from_numpy(store).to(DEV), [1, 0], 2, steps, origins, color, 0xFFFFFF)
    assert np.array_equal(bits(got), bits(RO.pages(store, [1, 0], steps, origins, color, 0xFFFFFF)))


# ---------------------------------------------------------------- 2. identity with the shift
@pytest.mark.parametrize("H,W", [(16, 16), (6, 12)])
def test_step_65536_is_the_shift_kernel_bit_for_bit(H, W):
    rs = np.random.RandomState(H)
    store = rs.randint(16, 256, (2, H, W, 3)).astype(np.uint8)          # no pixel has a byte of the fill colour
    store_d = torch.from_numpy(store).to(DEV)
    ds = lambda n: [0, 1, -1, 3, -3, n - 1, 1 - n, n, -n, n + 3, -n - 3]  # noqa: E731
    dxs, dys = ds(W), ds(H)
    shifts = [(d, 0) for d in dxs] + [(0, d) for d in dys] + [(dxs[i], dys[(3 * i + 1) % len(dys)]) for i in range(len(dxs))]
    B = len(shifts)
    idx = [b % 2 for b in range(B)]
    steps, origins = [(65536, 65536)] * B, [(-dx * 65536, -dy * 65536) for dx, dy in shifts]
    for color in (None, random_color(rs, B)):
        got = run(store_d, idx, B, steps, origins, color, 0x010203)
        assert np.array_equal(bits(got), bits(run_shift(store_d, idx, B, shifts, color, 0x010203)))
        assert np.array_equal(bits(got), bits(AO.pages(store, idx, shifts, color, 0x010203)))


# ---------------------------------------------------------------- 3. boxes
def affine_boxes(bb, affine):
    bb_d = torch.from_numpy(np.ascontiguousarray(bb, dtype=np.float32)).to(DEV)
    af_d = torch.from_numpy(np.ascontiguousarray(affine, dtype=np.float32).reshape(-1, 4)).to(DEV)
    engine.call("cova_boxes_affine", bb_d if bb_d.numel() else None, bb_d.shape[0], af_d, af_d.shape[0])
    return bb_d.cpu().numpy()


def test_boxes_affine_matches_the_oracle_and_the_translation_at_scale_one():
    rs = np.random.RandomState(8)
    for counts in ([0], [1], [5, 0, 17, 1, 300], rs.randint(0, 9, 200).tolist()):
        B = len(counts)
        bb = rs.uniform(-50, 1500, (sum(counts), 5)).astype(np.float32)            # non-integer coordinates
        bb[:, 0] = np.repeat(np.arange(B), counts)
        affine = np.concatenate([rs.uniform(0.5, 2, (B, 2)), rs.uniform(-700, 700, (B, 2))], 1).astype(np.float32)
        got = affine_boxes(bb, affine)
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(RO.affine_boxes(bb, affine)))
        assert sum(counts) == 0 or not np.array_equal(got, bb)
        shift = rs.randint(-2000, 2001, (B, 2))
        unit = np.concatenate([np.ones((B, 2)), shift], 1).astype(np.float32)
        sh_d = torch.from_numpy(shift.astype(np.int32)).to(DEV)
        tr_d = torch.from_numpy(bb).to(DEV)
        engine.call("cova_boxes_translate", tr_d if tr_d.numel() else None, tr_d.shape[0], sh_d, B)
        assert np.array_equal(bits(affine_boxes(bb, unit)), bits(tr_d))
    # rows of a foreign page stay as they are; the page column truncates towards zero; NaN stays
    bb = rs.uniform(0, 100, (9, 5)).astype(np.float32)
    bb[:, 0] = [0, 2, 3, -1, 1e9, 2.9, -0.5, -1.5, np.nan]
    affine = [(2, 0.5, 1, 2), (1.25, 1.25, 3, 4), (0.75, 1.5, 5, 6)]
    got = affine_boxes(bb, affine)
    assert np.array_equal(bits(got), bits(RO.affine_boxes(bb, affine)))
    assert np.array_equal(bits(got[[2, 3, 4, 7, 8]]), bits(bb[[2, 3, 4, 7, 8]]))
    assert not np.array_equal(got[[0, 1, 5, 6]], bb[[0, 1, 5, 6]])


# ---------------------------------------------------------------- 4. DeviceDataset / DeviceCollate
AUG = dict(max_shift=(5, 7), brightness=0.2, contrast=0.3, saturation=0.4, channel_gain=0.1, invert_prob=0.3, fill=(1, 2, 3),
           seed=11)
ZOOM = dict(AUG, scale=(0.6, 1.8))
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
            out[p] = (bits(x["images"][i]), bits(x["bboxes"][ps[i]:ps[i + 1], 1:]), x["labels"][ps[i]:ps[i + 1]].cpu().numpy(),
                      x["aug_shift"][i].cpu().numpy(), bits(x["aug_affine"][i]))
    return out


@pytest.mark.parametrize("ks", [0, 3])
@pytest.mark.parametrize("sf", [1.0, 0.5])
def test_zoomed_batches_are_the_oracle_applied_to_the_plain_batches(split, sf, ks):
    u8, rows = split
    W = u8.shape[2]
    ds = DeviceDataset(u8, rows, CS, DEV, spatial_k=ks)
    aug = PageAugment(**ZOOM)
    kw = dict(batch_size=3, shuffle=True, sampling_fraction=sf, seed=4, epoch=2)
    plain, got = epoch_tensors(ds, **kw), epoch_tensors(ds, augment=aug, **kw)
    assert len(plain) == len(got) == 3
    zoomed = 0
    for a, g in zip(plain, got):
        ids = a["page_ids"].cpu().numpy()
        shift, color = aug.params(ids, 2)
        step, origin, affine = aug.resample_params(ids, 2, W)
        zoomed += int((step != 65536).sum())
        assert set(g) == set(a) | {"aug_shift", "aug_affine"}
        assert g["aug_shift"].dtype == torch.int32 and g["aug_shift"].is_cuda and same(g["aug_shift"], shift)
        assert g["aug_affine"].dtype == torch.float32 and g["aug_affine"].is_cuda and same(g["aug_affine"], affine)
        assert same(g["images"], RO.pages(u8, ids, step, origin, color, 0x010203))
        boxes = RO.affine_boxes(a["bboxes"].cpu().numpy(), affine)
        assert same(g["bboxes"], boxes)
        if ks:
            assert same(g["context_indices"], GO.batch_graph(boxes, a["page_start"].cpu().numpy(), CS, ks))
        for k in a:
            if k not in ("images", "bboxes") and not (ks and k == "context_indices"):
                assert same(g[k], a[k]) if torch.is_tensor(a[k]) or isinstance(a[k], np.ndarray) else g[k] == a[k], k
        # DeviceCollate on the same pages and ids
        ref = DeviceCollate(CS, DEV, sampling_fraction=sf, seed=4, spatial_k=ks, augment=aug)(
            u8[ids], [rows[i] for i in ids], page_ids=ids, epoch=2)
        for k in KEYS + ("aug_shift", "aug_affine"):
            assert same(g[k], ref[k]), k
    assert zoomed
    # the default page ids of DeviceCollate are the positions
    ref = DeviceCollate(CS, DEV, spatial_k=ks, augment=aug)(u8[:3], rows[:3], epoch=5)
    _, color = aug.params(np.arange(3), 5)
    step, origin, affine = aug.resample_params(np.arange(3), 5, W)
    assert same(ref["images"], RO.pages(u8[:3], None, step, origin, color, 0x010203)) and same(ref["aug_affine"], affine)


def test_a_pages_zoom_does_not_depend_on_batch_size_rank_or_prefetch(split):
    u8, rows = split
    ds = DeviceDataset(u8, rows, CS, DEV, spatial_k=3)
    aug = PageAugment(**ZOOM)
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
        for k in KEYS + ("aug_shift", "aug_affine", "page_ids"):
            assert same(x[k], y[k]), k
    nxt = per_page(epoch_tensors(ds, batch_size=3, **dict(kw, epoch=2)))
    assert any(not np.array_equal(nxt[p][0], ref[p][0]) for p in ref) and any(not np.array_equal(nxt[p][4], ref[p][4]) for p in ref)


def test_scale_one_keeps_todays_launches_and_a_zoom_swaps_two_of_them(split):
    u8, rows = split
    ds = DeviceDataset(u8, rows, CS, DEV, spatial_k=3)
    kw = dict(batch_size=3, shuffle=True, sampling_fraction=0.5, seed=4, epoch=2)
    plain, lp = profiled(lambda: epoch_tensors(ds, **kw))
    rest = {k: v for k, v in lp.items() if k != "cova_pages_u8_gather_f32"}
    assert lp["cova_pages_u8_gather_f32"] == 3 and not any("resample" in k or "affine" in k for k in lp)
    today, lt = profiled(lambda: epoch_tensors(ds, augment=PageAugment(**AUG), **kw))
    one, l1 = profiled(lambda: epoch_tensors(ds, augment=PageAugment(scale=(1, 1), **AUG), **kw))
    assert lt == l1 == dict(rest, cova_pages_u8_augment_f32=3, cova_boxes_translate=3)
    for a, z in zip(today, one):
        assert set(a) == set(z) and "aug_affine" not in z
        for k in a:
            assert same(z[k], a[k]) if torch.is_tensor(a[k]) or isinstance(a[k], np.ndarray) else z[k] == a[k], k
    _, lc = profiled(lambda: epoch_tensors(ds, augment=PageAugment(contrast=0.5, scale=(1.0, 1.0)), **kw))
    assert lc == dict(rest, cova_pages_u8_augment_f32=3)                        # colour only: no launch for the boxes
    _, lz = profiled(lambda: epoch_tensors(ds, augment=PageAugment(**ZOOM), **kw))
    _, ln = profiled(lambda: epoch_tensors(ds, augment=PageAugment(scale=(0.9, 1.1)), **kw))
    assert lz == ln == dict(rest, cova_pages_u8_resample_f32=3, cova_boxes_affine=3)     # in their places, one launch each
    with pytest.raises(ValueError, match="features"):
        ds.batches(3, features=object(), augment=PageAugment(**ZOOM))


# ---------------------------------------------------------------- 5. training
@pytest.fixture(scope="module")
def small_model():
    fx, cfg, sd, _ = load_case("cova_h64_n11")
    rs = np.random.RandomState(12)
    u8 = rs.randint(0, 256, (6, 64, 64, 3)).astype(np.uint8)
    rows = [make_rows(rs, int(n), 64, 64) for n in rs.randint(8, 20, 6)]
    return cfg, sd, int(fx["meta/context_size"]), u8, rows


def test_three_zoomed_train_steps_are_reproducible_and_differ_from_unzoomed_ones(small_model):
    cfg, sd, cs, u8, rows = small_model
    ds = DeviceDataset(u8, rows, cs, DEV)
    kw = dict(max_shift=(6, 6), brightness=0.2, contrast=0.3, saturation=0.3, invert_prob=0.5, seed=2)

    def trained(augment):
        tr = HotPathTrainer(cfg, sd, DEV)
        n = 0
        for batch in ds.batches(2, shuffle=True, sampling_fraction=0.9, seed=1, epoch=0, augment=augment):
            tr.train_step(batch)
            n += 1
        assert n == 3
        return tr.state_dict()
    a, b, c = trained(PageAugment(scale=(0.6, 1.8), **kw)), trained(PageAugment(scale=(0.6, 1.8), **kw)), trained(PageAugment(**kw))
    assert list(a) == list(b) == list(c)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["convnet.0.weight"], c["convnet.0.weight"])


def test_fit_zooms_the_training_batches_and_never_the_evaluation(small_model, monkeypatch):
    cfg, sd, cs, u8, rows = small_model
    train, val = DeviceDataset(u8, rows, cs, DEV), DeviceDataset(u8[:4], rows[:4], cs, DEV)
    tr = HotPathTrainer(cfg, sd, DEV, track_metrics=True)
    seen = []
    real = evaluation.evaluate_split
    names = ("cova_pages_u8_resample_f32", "cova_boxes_affine", "cova_pages_u8_gather_f32", "cova_pages_u8_augment_f32",
             "cova_boxes_translate")
    counts = lambda: tuple(len(_lib.PROFILE[n]) for n in names)  # noqa: E731

    def watched(*a, **kw):
        before = counts()
        out = real(*a, **kw)
        seen.append((before, counts()))
        return out
    monkeypatch.setattr(evaluation, "evaluate_split", watched)
    res, launches = profiled(lambda: evaluation.fit(tr, train, val, n_epochs=1, batch_size=2, seed=3,
                                                    augment=PageAugment(max_shift=(4, 4), contrast=0.2, scale=(0.7, 1.4))))
    assert res.epochs_run == 1 and len(seen) == 1
    (before, after), = seen
    assert before == (3, 3, 0, 0, 0) and after == (3, 3, 1, 0, 0)              # 3 training steps; one evaluation batch, plain
    assert launches["cova_pages_u8_resample_f32"] == 3 and launches["cova_pages_u8_gather_f32"] == 1
    with pytest.raises(ValueError, match="train_features"):
        evaluation.fit(tr, train, val, 1, 2, train_features=object(), augment=PageAugment(scale=(0.7, 1.4)))
