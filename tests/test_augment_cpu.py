"""Host side of the page augmentation (no GPU): the numpy oracle against the contract written out pixel by pixel,
pipeline.PageAugment.params against the oracle's formulas, the argument checks, and the declared entry points."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import cova_amd  # noqa: F401
from cova_web_object_detection_amd import _lib, evaluation, pipeline
from cova_web_object_detection_amd.pipeline import PageAugment

import augment_oracle as AO

MAGS = dict(max_shift=(3, 5), brightness=0.2, contrast=0.3, saturation=0.4, channel_gain=0.15, invert_prob=0.3)


def test_oracle_pages_equal_the_contract_pixel_by_pixel():
    rs = np.random.RandomState(0)
    store = rs.randint(0, 256, (3, 5, 7, 3)).astype(np.uint8)
    shifts = [(0, 0), (1, 0), (-1, 0), (0, 2), (0, -2), (6, 4), (-6, -4), (7, 0), (0, 5), (-7, -5), (3, -2), (-2, 3),
              (AO.INT_MAX, -AO.INT_MAX)]
    idx = [b % 3 for b in range(len(shifts))]
    color = rs.uniform(-2, 2, (len(shifts), 12)).astype(np.float32)
    color[:, 3::4] = rs.uniform(-1, 1, (len(shifts), 3))
    color[0], color[1] = AO.identity(1)[0], AO.inversion(1)[0]
    for fill in (0x000000, 0xFFFFFF, 0x010203):
        got = AO.pages(store, idx, shifts, color, fill)
        ref = AO.pages_naive(store, idx, shifts, color, fill)
        assert got.dtype == ref.dtype == np.float32 and np.array_equal(got, ref)
        assert not np.signbit(got).any() and got.min() == 0.0 and got.max() == 1.0       # both clamps occur
    # the identity is the plain ToTensor, the last page is all fill, a shift moves the content right / down
    plain = np.transpose(store[idx], (0, 3, 1, 2)).astype(np.float32) / np.float32(255)
    got = AO.pages(store, idx, shifts, None, 0x010203)
    assert np.array_equal(got[0], plain[0])
    assert np.array_equal(got[-1], np.broadcast_to((np.float32([1, 2, 3]) / np.float32(255))[:, None, None], (3, 5, 7)))
    assert np.array_equal(got[1][:, :, 1:], plain[1][:, :, :-1]) and np.array_equal(got[3][:, 2:, :], plain[3][:, :-2, :])
    assert np.array_equal(got[1][:, :, 0], np.broadcast_to((np.float32([1, 2, 3]) / np.float32(255))[:, None], (3, 5)))


def nearest_f32(fr):
    """An exact rational -> the nearest float32, ties to even."""
    x = np.float32(float(fr))
    best = None
    for c in (x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))):
        key = (abs(Fraction(float(c)) - fr), int(np.float32(c).view(np.uint32)) & 1)
        if best is None or key < best[0]:
            best = (key, np.float32(c))
    return best[1]


def test_the_three_operation_quotient_of_the_kernel_is_the_ieee_division_for_every_byte():
    """csrc/augment.hip byte_unit: q = v*c, e = fma(-255, q, v), t = fma(e, c, q) with c = fl(1/255), every step rounded once
    (exact rationals here) -- against numpy's float32 division, the statement of the contract.  The plain product is not enough."""
    c = np.float32(1) / np.float32(255)
    assert c == nearest_f32(Fraction(1, 255))
    plain_differs = 0
    for v in range(256):
        q = nearest_f32(Fraction(v) * Fraction(float(c)))
        e = nearest_f32(Fraction(v) - 255 * Fraction(float(q)))
        t = nearest_f32(Fraction(float(q)) + Fraction(float(e)) * Fraction(float(c)))
        ref = np.float32(v) / np.float32(255)
        assert ref == nearest_f32(Fraction(v, 255)) and t == ref, v
        plain_differs += int(q != ref)
    assert plain_differs > 0


def test_oracle_translate_moves_the_boxes_of_a_page_and_leaves_foreign_rows():
    bb = np.asarray([[0, 1.5, 2.25, 3, 4], [1, 0, 0, 10, 10], [2, 1, 1, 2, 2], [-1, 1, 1, 2, 2], [0.9, 5, 5, 6, 6]], np.float32)
    got = AO.translate(bb, [[3, -4], [-2000, 2000]])
    assert got.dtype == np.float32
    assert got.tolist() == [[0, 4.5, -1.75, 6, 0], [1, -2000, 2000, -1990, 2010], [2, 1, 1, 2, 2], [-1, 1, 1, 2, 2],
                            [np.float32(0.9), 8, 1, 9, 2]]


def test_params_follow_the_stated_formulas():
    aug = PageAugment(seed=7, **MAGS)
    pids = np.concatenate([np.arange(300), [7699, 2 ** 31 - 1, 123456789]])
    for epoch in (0, 1, 17):
        shift, color = aug.params(pids, epoch)
        rs, rc = AO.params(pids, epoch, seed=7, **MAGS)
        assert shift.dtype == np.int32 and shift.shape == (303, 2) and np.array_equal(shift, rs)
        # both sides round a ten-operation float64 expression to float32: one float32 ulp of O(1) values at the most
        assert color.dtype == np.float32 and color.shape == (303, 12)
        assert np.allclose(color, rc, rtol=1e-6, atol=1e-7)
    assert (color[:, 0] < 0).any() and (color[:, 0] > 0).any()            # inverted and plain pages both occur
    inv = color[:, 0] < 0
    assert (color[inv][:, 3::4] > 0.4).all() and (np.abs(color[~inv][:, 3::4]) < 0.4).all()


def test_shifts_cover_the_whole_range_and_stay_inside():
    aug = PageAugment(max_shift=(3, 3), seed=1)
    shift, color = aug.params(np.arange(2000), 0)
    assert shift.min(0).tolist() == [-3, -3] and shift.max(0).tolist() == [3, 3]
    assert np.array_equal(color, AO.identity(2000))
    counts = np.bincount(shift[:, 0] + 3, minlength=7)
    assert counts.min() > 200                                              # 2000 / 7 = 286 expected a value
    only_x = PageAugment(max_shift=(4, 0)).params(np.arange(50), 3)[0]
    assert (only_x[:, 1] == 0).all() and (only_x[:, 0] != 0).any()


def test_zero_magnitudes_are_zero_shifts_and_the_exact_identity():
    for kw in (dict(), dict(seed=5, fill=(0, 0, 0)), dict(invert_prob=0.0, brightness=0.0)):
        shift, color = PageAugment(**kw).params(np.arange(500), 9)
        assert not shift.any() and np.array_equal(color, AO.identity(500)) and not np.signbit(color).any()
    assert not PageAugment().shifts and PageAugment(max_shift=(0, 1)).shifts
    assert PageAugment(fill=(1, 2, 3)).fill_rgb == 0x010203
    assert PageAugment().params(np.zeros(0, np.int64), 0)[1].shape == (0, 12)


def test_params_depend_on_seed_epoch_and_page_id_alone():
    aug = PageAugment(seed=3, **MAGS)
    pids = np.arange(40)
    shift, color = aug.params(pids, 5)
    # another batch composition, another order, a rank's share: the same rows for the same page ids
    for part in (pids[::-1], pids[7:19], pids[1::2], np.asarray([33, 2, 33, 2])):
        s, c = aug.params(part, 5)
        assert np.array_equal(s, shift[part]) and np.array_equal(c, color[part])
    s2, c2 = aug.params(pids, 6)
    assert not np.array_equal(s2, shift) and not np.array_equal(c2, color)
    s3, c3 = PageAugment(seed=4, **MAGS).params(pids, 5)
    assert not np.array_equal(s3, shift) and not np.array_equal(c3, color)
    # a stream of its own: not the box sampler's keys of the same (seed, epoch, page)
    u0 = (pipeline.mix64(pipeline.mix64(pipeline.stream_seed(3, 5), 0), 0) >> 11) * 2.0 ** -53
    assert AO.uniform(3, 5, 0, 0) != u0
    assert np.array_equal(aug.table(pids, 5), np.concatenate([shift.reshape(-1), color.reshape(-1).view(np.int32)]))


def test_certain_inversion_turns_a_white_page_black():
    shift, color = PageAugment(invert_prob=1.0, seed=2).params(np.arange(6), 1)
    assert np.array_equal(color, AO.inversion(6))
    white = np.full((6, 4, 4, 3), 255, np.uint8)
    assert not AO.pages(white, None, shift, color, 0xFFFFFF).any()
    assert np.array_equal(AO.pages(np.zeros_like(white), None, shift, color, 0), np.ones((6, 3, 4, 4), np.float32))


@pytest.mark.parametrize("kw,match", [
    (dict(max_shift=(-1, 0)), "max_shift"), (dict(max_shift=(0, -2)), "max_shift"), (dict(max_shift=3), "max_shift"),
    (dict(brightness=-0.1), "brightness"), (dict(contrast=-0.1), "contrast"), (dict(saturation=-1), "saturation"),
    (dict(channel_gain=-0.5), "channel_gain"), (dict(contrast=1.0), "contrast"), (dict(saturation=1.5), "saturation"),
    (dict(channel_gain=1.0), "channel_gain"), (dict(invert_prob=-0.01), "invert_prob"), (dict(invert_prob=1.01), "invert_prob"),
    (dict(fill=(256, 0, 0)), "fill"), (dict(fill=(0, -1, 0)), "fill"), (dict(fill=(0, 0)), "fill"),
    (dict(brightness=float("nan")), "brightness")])
def test_page_augment_refuses_bad_arguments(kw, match):
    with pytest.raises(ValueError, match=match):
        PageAugment(**kw)


def resident_stub(P=4, H=32, W=48):
    """A DeviceDataset without its device part: what batches() checks before any device work.  Only P, H and W exist, so a
    check that moved behind anything else would show up here as an AttributeError, not as a pass; tests/test_augment_gpu.py
    repeats both checks on a real dataset."""
    ds = object.__new__(pipeline.DeviceDataset)
    ds.P, ds.H, ds.W = P, H, W
    return ds


def test_batches_and_fit_refuse_augment_with_cached_features_and_too_large_shifts():
    PageAugment(brightness=5.0, contrast=0.99, invert_prob=1.0, fill=(0, 128, 255))                # all valid
    ds = resident_stub()
    with pytest.raises(ValueError, match="features"):
        ds.batches(2, features=object(), augment=PageAugment(brightness=0.1))
    for bad in ((48, 0), (0, 32), (100, 100)):
        with pytest.raises(ValueError, match="max_shift"):
            ds.batches(2, augment=PageAugment(max_shift=bad))
    with pytest.raises(ValueError, match="train_features"):
        evaluation.fit(None, ds, ds, 1, 2, train_features=object(), augment=PageAugment())
    collate = pipeline.DeviceCollate(2, "cpu", augment=PageAugment(max_shift=(4, 4)))
    with pytest.raises(ValueError, match="max_shift"):
        collate(np.zeros((1, 4, 4, 3), np.uint8), [np.zeros((0, 5), np.float32)])


def test_augment_entry_points_are_declared_and_exported():
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    protos = _lib.parse_header()
    # the augment prototype as the header states it: store, page_idx, P, B, H, W, shift, color, fill_rgb, out, stream
    for name, n_args in (("cova_pages_u8_augment_f32", 11), ("cova_boxes_translate", 5)):
        assert name in protos and hasattr(cdll, name), name
        assert len(protos[name]) == n_args, name
    p, i = ctypes.c_void_p, ctypes.c_int
    assert protos["cova_pages_u8_augment_f32"] == [p, p, i, i, i, i, p, p, i, p, p]
    assert protos["cova_boxes_translate"] == [p, i, p, i, p]
    assert len(protos["cova_pages_u8_gather_f32"]) == 8 and len(protos["cova_images_u8_to_f32"]) == 6      # unchanged
    # argument checks that need no device: a status, no launch
    fn = cdll.cova_pages_u8_augment_f32
    fn.argtypes, fn.restype = protos["cova_pages_u8_augment_f32"], ctypes.c_int
    assert fn(None, None, 1, 1, 4, 4, None, None, 0, None, None) != 0
    tr = cdll.cova_boxes_translate
    tr.argtypes, tr.restype = protos["cova_boxes_translate"], ctypes.c_int
    assert tr(None, 0, None, 3, None) == 0 and tr(None, 2, None, 3, None) != 0 and tr(None, -1, None, 3, None) != 0
