"""Host side of the page zoom (no GPU): the numpy oracle against the contract written out pixel by pixel and against the shift
oracle at scale 1, the kernel's quotient form against the exact quotient for every tap sum, PageAugment.resample_params against
the oracle's formulas, what the default leaves as it was, the argument checks, the geometry of the box map against the
resampled content, and the declared entry points."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import cova_amd  # noqa: F401
from cova_web_object_detection_amd import _lib, evaluation, pipeline
from cova_web_object_detection_amd.pipeline import PageAugment

import augment_oracle as AO
import resample_oracle as RO
from helpers import np_bits as bits

MAGS = dict(max_shift=(3, 5), brightness=0.2, contrast=0.3, saturation=0.4, channel_gain=0.15, invert_prob=0.3)
DEN = 255 * 65536


def random_color(rs, B):
    m = rs.uniform(-2, 2, (B, 12)).astype(np.float32)
    m[:, 3::4] = rs.uniform(-1, 1, (B, 3))
    return m


# ---------------------------------------------------------------- the oracle
@pytest.mark.parametrize("H,W", [(1, 1), (3, 4), (5, 7), (9, 12)])
def test_the_vectorised_oracle_equals_the_contract_pixel_by_pixel(H, W):
    rs = np.random.RandomState(H * 31 + W)
    P = 3
    store = rs.randint(0, 256, (P, H, W, 3)).astype(np.uint8)
    steps = [(65536, 65536), (65535, 65537), (32768, 131072), (131072, 43691), (1, 1 << 22), (1 << 22, 1), (98304, 47836)]
    steps += [tuple(int(v) for v in rs.randint(1, 1 << 18, 2)) for _ in range(9)]
    origins = [(0, 0), (0xFF00, 0xFF00), (-1, -1), ((W - 1) << 16, (H - 1) << 16), (-(3 << 16), 5 << 16),
               (1 << 40, 0), (0, -(1 << 40)), (-(1 << 61), 1 << 61)]
    origins += [tuple(int(v) for v in rs.randint(-(W + H) << 16, (W + H) << 16, 2)) for _ in range(8)]
    assert len(steps) == len(origins)
    idx = [b % P for b in range(len(steps))]
    color = random_color(rs, len(steps))
    color[0], color[1] = AO.identity(1)[0], AO.inversion(1)[0]
    for fill in (0x000000, 0xFFFFFF, 0x123456):
        got = RO.pages(store, idx, steps, origins, color, fill)
        ref = RO.pages_naive(store, idx, steps, origins, color, fill)
        assert got.dtype == ref.dtype == np.float32 and np.array_equal(bits(got), bits(ref)), hex(fill)
        assert not np.signbit(got).any()
    # far outside: the fill colour alone; an index outside the store keeps the prefilled page
    far = RO.pages(store, [0], [(65536, 65536)], [(1 << 40, 0)], None, 0x123456)
    assert np.array_equal(far[0], np.broadcast_to((np.float32([0x12, 0x34, 0x56]) / np.float32(255))[:, None, None], (3, H, W)))
    kept = RO.pages(store, [P, 1, -1], steps[:3], origins[:3], None, 0, out=np.full((3, 3, H, W), 7, np.float32))
    assert (kept[[0, 2]] == 7).all() and not (kept[1] == 7).any()


@pytest.mark.parametrize("H,W", [(5, 7), (6, 12), (16, 16)])
def test_at_step_65536_the_oracle_is_the_shift_oracle(H, W):
    rs = np.random.RandomState(H + W)
    store = rs.randint(0, 256, (2, H, W, 3)).astype(np.uint8)
    ds = [0, 1, -1, 3, -3, W - 1, 1 - W, W, -W, W + 3, -W - 3]
    shifts = [(d, 0) for d in ds] + [(0, d) for d in ds] + [(ds[i], ds[(3 * i + 1) % len(ds)]) for i in range(len(ds))]
    idx = [b % 2 for b in range(len(shifts))]
    color = random_color(rs, len(shifts))
    steps = [(65536, 65536)] * len(shifts)
    origins = [(-dx * 65536, -dy * 65536) for dx, dy in shifts]
    for fill in (0x010203, 0xFFFFFF):
        for table in (None, color):
            assert np.array_equal(bits(RO.pages(store, idx, steps, origins, table, fill)),
                                  bits(AO.pages(store, idx, shifts, table, fill)))


# ---------------------------------------------------------------- the quotient
def nearest_f32(fr):
    """An exact rational -> the nearest float32, ties to even."""
    x = np.float32(float(fr))
    best = None
    for c in (x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))):
        key = (abs(Fraction(float(c)) - fr), int(np.float32(c).view(np.uint32)) & 1)
        if best is None or key < best[0]:
            best = (key, np.float32(c))
    return best[1]


def test_a_byte_times_65536_over_the_tap_denominator_is_the_byte_over_255():
    v = np.arange(256)
    assert np.array_equal(bits(np.float32(v * 65536) / np.float32(DEN)), bits(np.float32(v) / np.float32(255)))
    assert DEN < 2 ** 24 and np.float32(DEN) == DEN


def test_the_three_operation_quotient_of_the_kernel_is_the_ieee_division_for_every_tap_sum():
    """csrc/augment.hip tap_unit: t = q*c, e = fma(-D, t, q), out = fma(e, c, t) with D = 16711680, c = fl(1/D), for EVERY
    integer q in [0, D] (a superset of the sums the four taps can produce), each step rounded once.

    Exact arithmetic without a rational per q: q, t, c and e are float32 values, so q*c (48 significant bits), D*t (32 bits)
    and q - D*t (at most 33 bits on one grid) are EXACT in float64 and a conversion to float32 is the one rounding of the
    step.  The last step rounds t + e*c: e*c is exact in float64, the float64 sum is within 2**-53 of the exact one, and it is
    shown to lie further than that from every float32 midpoint, so rounding it to float32 is rounding the exact sum.  numpy's
    own float32 division, the statement of the contract, is held to the exact quotient the same way (|ref*D - q| against
    half a gap times D, all exact), and spot-checked with Fractions."""
    c = np.float32(1) / np.float32(DEN)
    assert c == nearest_f32(Fraction(1, DEN))
    c64, D = float(c), float(DEN)
    plain_differs = 0
    for lo in range(0, DEN + 1, 1 << 22):
        q = np.arange(lo, min(lo + (1 << 22), DEN + 1), dtype=np.int64)
        f = q.astype(np.float64)                                           # q < 2**24: also an exact float32
        assert np.array_equal(f.astype(np.float32).astype(np.int64), q)
        t = (f * c64).astype(np.float32)
        t64 = t.astype(np.float64)
        e = (f - D * t64).astype(np.float32)
        assert np.array_equal(e.astype(np.float64), f - D * t64)           # the residual is a float32: that fma is exact
        ec = e.astype(np.float64) * c64
        s = t64 + ec                                                       # the one inexact float64 operation: within 2**-53 |s|
        out = s.astype(np.float32)
        o64 = out.astype(np.float64)
        mid_up = (o64 + np.nextafter(out, np.float32(np.inf)).astype(np.float64)) / 2
        mid_dn = (o64 + np.nextafter(out, np.float32(-np.inf)).astype(np.float64)) / 2
        assert (np.minimum(mid_up - s, s - mid_dn) > np.abs(s) * 2.0 ** -51).all()        # ... of no float32 midpoint
        ref = q.astype(np.float32) / np.float32(DEN)
        r64 = ref.astype(np.float64)
        err = f - r64 * D                                                  # exact: D times the signed error of ref
        rup = np.nextafter(ref, np.float32(np.inf)).astype(np.float64) - r64
        rdn = r64 - np.nextafter(ref, np.float32(-np.inf)).astype(np.float64)
        assert (err < rup / 2 * D).all() and (-err < rdn / 2 * D).all()     # ref is the one nearest float32 of q / D
        assert np.array_equal(bits(out), bits(ref))
        plain_differs += int((t != ref).sum())
    assert plain_differs > 0                                               # the product with the reciprocal alone is not enough
    for q in (0, 1, 2, 255, 65535, 65536, 65537, 8355840, 12345678, DEN - 1, DEN):
        assert np.float32(q) / np.float32(DEN) == nearest_f32(Fraction(q, DEN)), q


# ---------------------------------------------------------------- parameters
@pytest.mark.parametrize("W", [4, 7, 1280])
def test_resample_params_follow_the_stated_formulas(W):
    pids = np.concatenate([np.arange(120), [7699, 2 ** 31 - 1, 123456789]])
    for seed, scale in ((7, (0.6, 1.8)), (0, (0.5, 2.0)), (3, (1.37, 1.37))):
        aug = PageAugment(seed=seed, scale=scale, **MAGS)
        assert aug.scales
        for epoch in (0, 17):
            step, origin, affine = aug.resample_params(pids, epoch, W)
            rs, ro, ra = RO.resample_params(pids, epoch, W, seed=seed, scale=scale, **MAGS)
            assert step.dtype == np.int32 and step.shape == (123, 2) and np.array_equal(step, rs)
            assert origin.dtype == np.int64 and origin.shape == (123, 2) and np.array_equal(origin, ro)
            assert affine.dtype == np.float32 and affine.shape == (123, 4) and np.array_equal(bits(affine), bits(ra))
            assert (step[:, 0] == step[:, 1]).all() and step.min() >= 32768 and step.max() <= 131072
            # slots 0-8 are untouched: the shifts and colours of the same pages are those without a zoom
            shift, color = aug.params(pids, epoch)
            s0, c0 = PageAugment(seed=seed, **MAGS).params(pids, epoch)
            assert np.array_equal(shift, s0) and np.array_equal(bits(color), bits(c0))
            assert np.array_equal(affine[:, 3], shift[:, 1].astype(np.float32))
            tab = aug.resample_table(pids, epoch, W)
            assert tab.dtype == np.int32 and np.array_equal(tab, np.concatenate(
                [step.reshape(-1), origin.reshape(-1).view(np.int32), affine.reshape(-1).view(np.int32)]))
    step = PageAugment(scale=(0.5, 2.0), seed=1).resample_params(np.arange(2000), 0, W)[0]
    assert step.min() < 36000 and step.max() > 120000                      # the whole range of zooms occurs
    assert PageAugment(scale=(0.5, 2.0)).resample_params(np.zeros(0, np.int64), 0, W)[2].shape == (0, 4)


def test_the_default_scale_changes_no_table_byte():
    pids = np.concatenate([np.arange(300), [7699, 2 ** 31 - 1]])
    for kw in (dict(seed=7, **MAGS), dict(seed=7, scale=(1, 1), **MAGS), dict(seed=7, scale=[1.0, 1.0], **MAGS)):
        aug = PageAugment(**kw)
        assert not aug.scales and aug.scale == (1.0, 1.0)
        for epoch in (0, 5):
            shift, color = aug.params(pids, epoch)
            rs, rc = AO.params(pids, epoch, seed=7, **MAGS)
            assert shift.dtype == np.int32 and np.array_equal(shift, rs)
            assert color.dtype == np.float32 and np.allclose(color, rc, rtol=1e-6, atol=1e-7)
            tab = aug.table(pids, epoch)
            assert tab.dtype == np.int32 and tab.shape == (302 * 14,)
            assert np.array_equal(tab, np.concatenate([shift.reshape(-1), color.reshape(-1).view(np.int32)]))
    # the identical bytes with a zoom switched on: the zoom tables are extra arrays, never a change to these
    a, b = PageAugment(seed=7, **MAGS), PageAugment(seed=7, scale=(0.6, 1.8), **MAGS)
    assert b.scales and np.array_equal(a.table(pids, 3), b.table(pids, 3))
    assert not PageAugment().scales and PageAugment(scale=(1.0, 1.5)).scales and PageAugment(scale=(0.5, 1.0)).scales


@pytest.mark.parametrize("scale", [(0.4, 1.0), (1.0, 2.5), (1.5, 1.2), (float("nan"), 1.0), (1.0, float("inf")), 1.0, (1.0,),
                                   (1.0, 1.0, 1.0), ("a", "b"), None, (0.0, 0.0), (-1.0, 1.0)])
def test_page_augment_refuses_a_bad_scale(scale):
    with pytest.raises(ValueError, match="scale"):
        PageAugment(scale=scale)


def test_valid_scales_are_accepted():
    for scale in ((0.5, 2.0), (0.5, 0.5), (2.0, 2.0), (1, 1), [0.75, 1.25]):
        assert PageAugment(scale=scale).scale == (float(scale[0]), float(scale[1]))


@pytest.mark.parametrize("W", [4, 7, 1280])
def test_scale_one_with_shifts_is_the_shift(W):
    aug = PageAugment(max_shift=(3, 5), seed=2, scale=(1, 1))
    pids = np.arange(200)
    shift, _ = aug.params(pids, 4)
    assert shift.any()
    step, origin, affine = aug.resample_params(pids, 4, W)
    assert (step == 65536).all()
    assert np.array_equal(origin, -shift.astype(np.int64) * 65536)
    assert np.array_equal(bits(affine), bits(np.stack([np.ones(200), np.ones(200), shift[:, 0], shift[:, 1]], 1)))


# ---------------------------------------------------------------- geometry
def page_with_shift(aug, epoch, want):
    """The id of a page whose viewport shift is ``want`` (a search: the shift is a draw)."""
    pids = np.arange(20000)
    shift, _ = aug.params(pids, epoch)
    hit = np.nonzero((shift == np.asarray(want)).all(1))[0]
    assert hit.size
    return int(hit[0])


@pytest.mark.parametrize("s,want", [(0.5, (3, -2)), (0.73, (0, 0)), (1.0, (5, 7)), (1.37, (-4, 3)), (2.0, (6, -5))])
def test_the_box_map_lands_on_the_resampled_content(s, want):
    """Nothing of the formulas is restated here: a black rectangle on a white page, its box the rectangle's exact edges; after
    the resample every output pixel whose centre lies more than 1.5 px inside the mapped box is exactly black, every one more
    than 1.5 px outside exactly white (a tap pair reaches one source pixel beyond the sample, which is at most 2 output
    pixels at zoom 2, less the half pixel between a pixel's edge and its centre)."""
    H = W = 64
    page = np.full((1, H, W, 3), 255, np.uint8)
    x1, y1, x2, y2 = 20, 10, 40, 30
    page[0, y1:y2, x1:x2] = 0
    aug = PageAugment(max_shift=(6, 7), scale=(s, s), seed=5)
    pid = page_with_shift(aug, 1, want)
    step, origin, affine = aug.resample_params([pid], 1, W)
    img = RO.pages(page, [0], step, origin, None, 0xFFFFFF)[0]
    box = RO.affine_boxes(np.asarray([[0, x1, y1, x2, y2]], np.float32), affine)[0, 1:].astype(np.float64)
    cx, cy = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    inside = (cx > box[0] + 1.5) & (cx < box[2] - 1.5) & (cy > box[1] + 1.5) & (cy < box[3] - 1.5)
    outside = (cx < box[0] - 1.5) | (cx > box[2] + 1.5) | (cy < box[1] - 1.5) | (cy > box[3] + 1.5)
    assert inside.any() and outside.any()
    assert (img[:, inside] == 0).all() and (img[:, outside] == 1).all()
    assert abs((box[2] - box[0]) / (x2 - x1) - s) < 0.01 and abs((box[3] - box[1]) / (y2 - y1) - s) < 0.01


def test_oracle_affine_moves_the_boxes_of_a_page_and_leaves_foreign_rows():
    bb = np.asarray([[0, 1.5, 2.25, 3, 4], [1, 0, 0, 10, 10], [2, 1, 1, 2, 2], [-1, 1, 1, 2, 2], [0.9, 5, 5, 6, 6],
                     [np.nan, 1, 1, 2, 2]], np.float32)
    got = RO.affine_boxes(bb, [[2, 0.5, 3, -4], [1, 1, -2000, 2000]])
    assert got.dtype == np.float32
    assert got[:5].tolist() == [[0, 6, -2.875, 9, -2], [1, -2000, 2000, -1990, 2010], [2, 1, 1, 2, 2], [-1, 1, 1, 2, 2],
                                [np.float32(0.9), 13, -1.5, 15, -1]]
    assert np.isnan(got[5, 0]) and got[5, 1:].tolist() == [1, 1, 2, 2]
    # scale 1 and integer offsets: the translation's bits
    rs = np.random.RandomState(1)
    bb = rs.uniform(-50, 1500, (300, 5)).astype(np.float32)
    bb[:, 0] = rs.randint(-1, 5, 300)
    shift = rs.randint(-2000, 2001, (4, 2))
    affine = np.concatenate([np.ones((4, 2)), shift], 1).astype(np.float32)
    assert np.array_equal(bits(RO.affine_boxes(bb, affine)), bits(AO.translate(bb, shift)))


# ---------------------------------------------------------------- argument checks, entry points
def resident_stub(P=4, H=32, W=48):
    """A DeviceDataset without its device part: what batches() checks before any device work."""
    ds = object.__new__(pipeline.DeviceDataset)
    ds.P, ds.H, ds.W = P, H, W
    return ds


def test_batches_and_fit_refuse_a_zoom_with_cached_features():
    ds = resident_stub()
    zoom = PageAugment(scale=(0.6, 1.8))
    with pytest.raises(ValueError, match="features"):
        ds.batches(2, features=object(), augment=zoom)
    with pytest.raises(ValueError, match="train_features"):
        evaluation.fit(None, ds, ds, 1, 2, train_features=object(), augment=zoom)
    with pytest.raises(ValueError, match="max_shift"):
        ds.batches(2, augment=PageAugment(max_shift=(48, 0), scale=(0.6, 1.8)))


def test_resample_entry_points_are_declared_and_exported():
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    protos = _lib.parse_header()
    p, i = ctypes.c_void_p, ctypes.c_int
    # store, page_idx, P, B, H, W, step, origin, color, fill_rgb, out, stream
    assert protos["cova_pages_u8_resample_f32"] == [p, p, i, i, i, i, p, p, p, i, p, p]
    assert protos["cova_boxes_affine"] == [p, i, p, i, p]
    assert protos["cova_pages_u8_augment_f32"] == [p, p, i, i, i, i, p, p, i, p, p]                      # unchanged
    assert protos["cova_boxes_translate"] == [p, i, p, i, p]
    fn = cdll.cova_pages_u8_resample_f32
    fn.argtypes, fn.restype = protos["cova_pages_u8_resample_f32"], ctypes.c_int
    assert fn(None, None, 1, 1, 4, 4, None, None, None, 0, None, None) != 0                              # a status, no launch
    af = cdll.cova_boxes_affine
    af.argtypes, af.restype = protos["cova_boxes_affine"], ctypes.c_int
    assert af(None, 0, None, 3, None) == 0 and af(None, 2, None, 3, None) != 0 and af(None, -1, None, 3, None) != 0
