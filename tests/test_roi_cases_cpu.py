"""Checks on the case table of tests/roi_cases.py itself (no GPU), with the oracle alone: every item is a condition the
inputs must meet so that tests/test_roi_paths_gpu.py cannot pass vacuously -- tied maxima in every pixel phase and in the
later trips of the forward's scan, every listed window size, empty bins, an empty page, bad page indices, every kernel
instantiation reached, and the exactness claims behind the bit-for-bit comparisons."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
import roi_cases as RC  # noqa: E402

TIE_CASES = [k for k, c in RC.FWD_CASES.items() if c.kind in RC.TIE_KINDS]


def tie_stats(case, feat, rois, arg):
    """over the (box, bin, channel) entries of the non-empty bins: how many, how many with a tied maximum, how many with
    the first maximum at window index i with i % 4 == 1, 2, 3, with i >= 16 and with i >= 32; the oracle's argmax must
    be that first maximum"""
    hs, he, ws, we = RC.windows(rois, case.PH, case.PW, case.H, case.W)
    st = dict(entries=0, tied=0, phase=[0, 0, 0, 0], ge16=0, ge32=0)
    for i in np.nonzero(RC.good_page(rois, case.B))[0]:
        b = int(rois[i, 0])
        for p in range(case.PH):
            for q in range(case.PW):
                if he[i, p] <= hs[i, p] or we[i, q] <= ws[i, q]:
                    assert (arg[i, :, p, q] == -1).all()
                    continue
                win = feat[b, :, hs[i, p]:he[i, p], ws[i, q]:we[i, q]].reshape(case.C, -1)
                first = win.argmax(1)
                nw = we[i, q] - ws[i, q]
                assert np.array_equal(arg[i, :, p, q], (hs[i, p] + first // nw) * case.W + ws[i, q] + first % nw)
                st["entries"] += case.C
                st["tied"] += int(((win == win.max(1, keepdims=True)).sum(1) > 1).sum())
                for k in range(4):
                    st["phase"][k] += int((first % 4 == k).sum())
                st["ge16"] += int((first >= 16).sum())
                st["ge32"] += int((first >= 32).sum())
    return st


@pytest.mark.parametrize("lazy", [0, 1])
@pytest.mark.parametrize("name", TIE_CASES)
def test_tie_cases_exercise_the_merge_rule_and_the_later_trips(name, lazy):
    case = RC.FWD_CASES[name]
    feat, rois, out, arg = RC.forward_reference(name, lazy)
    st = tie_stats(case, feat, rois, arg)
    print("%s lazy=%d: %r" % (name, lazy, st))
    assert 4 * st["tied"] >= st["entries"] > 0
    assert min(st["phase"][1:]) >= 20 and st["ge16"] >= 20 and st["ge32"] >= 20
    if lazy:                                         # ties at positive values, as behind a ReLU
        assert (out > 0).any()


@pytest.mark.parametrize("name", list(RC.FWD_CASES))
def test_forward_cases_hold_every_window_size_and_the_degenerate_boxes(name):
    case = RC.FWD_CASES[name]
    _, rois, out, arg = RC.forward_reference(name, 0)
    npx = RC.window_sizes(rois, case.PH, case.PW, case.H, case.W)[RC.good_page(rois, case.B)]
    have = sorted(set(npx.reshape(-1).tolist()) & set(RC.WINDOW_SIZES))
    pages = rois[:, 0].astype(int)
    print("%s: window sizes %r, %d empty bins, pages %r, grid %d" % (name, have, int((npx == 0).sum()),
                                                                     sorted(set(pages.tolist())), RC.fwd_grid(case)))
    assert have == sorted(RC.WINDOW_SIZES)
    assert (npx == 0).any() and (arg == -1).any()
    assert set(range(case.B)) - set(pages.tolist()), "no page without a box"
    assert {-2, case.B + 3} <= set(pages.tolist())
    good = pages[(pages >= 0) & (pages < case.B)]
    assert (np.diff(good) < 0).any(), "page indices are sorted"
    if case.n >= 40:                                 # boxes wholly left of / above the map, inverted, zero-area
        x1, y1, x2, y2 = rois[:, 1], rois[:, 2], rois[:, 3], rois[:, 4]
        assert ((x2 < 0) & (x1 < 0)).any() and ((y2 < 0) & (y1 < 0)).any()
        assert ((x2 < x1) & (y2 < y1)).any() and ((x2 == x1) & (y2 == y1)).any()


def test_forward_grids_cover_the_block_remap():
    """C == 64 launches remap blocks over eight XCDs: grids below 8, multiples of 8, others, and a partial last block"""
    grids = {RC.fwd_grid(c): (c.n * c.PH * c.PW) % 4 for c in RC.FWD_CASES.values() if c.C == 64}
    print("forward grids (blocks: tasks in the last block mod 4): %r" % grids)
    assert any(g < 8 for g in grids) and any(g >= 8 and g % 8 == 0 for g in grids)
    assert any(g > 8 and g % 8 for g in grids) and any(r for r in grids.values())
    assert {c.C for c in RC.FWD_CASES.values()} == {64, 128}


def test_every_kernel_instantiation_is_reached():
    hit = set()
    for c in list(RC.FWD_CASES.values()) + list(RC.BWD_CASES.values()) + [a.case for a in RC.ALIGN_CASES.values()]:
        hit |= set(RC.variants(c))
    hit |= set(RC.variants(RC.ALIGN_LONG.case))
    print("\n".join(sorted(hit)))
    assert len(RC.ALL_VARIANTS) == 14 and sorted(hit) == RC.ALL_VARIANTS, sorted(set(RC.ALL_VARIANTS) - hit)
    bwd = RC.BWD_CASES.values()
    assert {(c.PH, c.PW) for c in bwd} >= {(3, 3), (2, 5), (1, 1), (7, 7)} and {c.C for c in bwd} == {64, 128}
    assert {c.W for c in bwd} >= {1, 39, 40, 41, 81} and {c.H for c in bwd} >= {1, 9}


@pytest.mark.parametrize("name", list(RC.BWD_CASES))
def test_exact_gradients_are_exact(name):
    """the oracle's sequential float32 scatter of the masked integer gradients equals the float64 scatter exactly, the
    float32 sums of the BatchNorm statistics in two orders equal the float64 sums, and the masks are not trivial"""
    case = RC.BWD_CASES[name]
    d = RC.backward_inputs(name)
    gout, mean, invstd = RC.gradients(case, True)
    g = gout.reshape(d["argmax"].shape)
    keep = (d["pooled"] > 0) & (d["argmax"] >= 0)
    gm = np.where(keep, g, np.float32(0))
    for grad in (g, gm):
        ref = RC.scatter64(grad, d["rois"], d["argmax"], case.B, case.H, case.W)
        got = RC.oracle_roipool_bwd(grad, d["rois"], d["argmax"], case.B, case.H, case.W)
        assert np.array_equal(got.astype(np.float64), ref)
    (s0, s1), _ = RC.stat_sums64(gm, d["zmax"], mean, invstd)
    t = gm * ((d["zmax"] - mean.reshape(1, -1, 1, 1)) * invstd.reshape(1, -1, 1, 1))          # float32 throughout
    for order in (1, -1):
        acc = np.zeros(case.C, np.float32)
        for row in t.transpose(0, 2, 3, 1).reshape(-1, case.C)[::order]:
            acc += row
        assert np.array_equal(acc.astype(np.float64), s1)
    assert np.array_equal(gm.sum((0, 2, 3), dtype=np.float32).astype(np.float64), s0)
    valid = d["argmax"] >= 0
    hits = RC.max_hits(d["rois"], d["argmax"], case.B, case.H, case.W)
    print("%s: %d entries, %d with an arg-max, %d masked by pooled <= 0, most contributions to one element %d" % (
        name, valid.size, int(valid.sum()), int((valid & ~keep).sum()), hits))
    assert valid.any() and (~valid).any() and (valid & ~keep).any() and (valid & keep).any() and hits > 1
    pages = d["rois"][:, 0].astype(int)
    assert set(range(case.B)) - set(pages.tolist()) and {-2, case.B + 3} <= set(pages.tolist())


@pytest.mark.parametrize("name", list(RC.FWD_CASES) + list(RC.BWD_CASES))
def test_lazy_map_is_exact_in_float32(name):
    case = RC.FWD_CASES.get(name) or RC.BWD_CASES[name]
    ops = RC.lazy_operands(case)
    for k in ("z", "x", "shift"):
        assert np.array_equal(ops[k] * 8, np.round(ops[k] * 8)) and np.abs(ops[k]).max() <= 4
    assert set(ops["scale"].tolist()) <= {-1.0, -0.5, 0.5, 1.0, 2.0}
    m32, m64 = RC.lazy_map(ops, np.float32), RC.lazy_map(ops, np.float64)
    assert m32.dtype == np.float32 and np.array_equal(m32.astype(np.float64), m64)
    s = ops["scale"].astype(np.float64).reshape(1, -1, 1, 1)
    fused = np.maximum(s * ops["z"] + ops["shift"].astype(np.float64).reshape(1, -1, 1, 1) + ops["x"], 0)
    assert np.array_equal(fused, m64) and (m64 > 0).any() and (m64 == 0).any()


def test_align_cases_cover_the_issue_list():
    al = list(RC.ALIGN_CASES.values())
    assert {(a.case.PH, a.case.PW) for a in al} == {(2, 5), (1, 1), (4, 1)} and {a.case.C for a in al} == {64, 128}
    assert {(a.sr, a.aligned) for a in al} == {(s, x) for s in (0, 1, 2) for x in (0, 1)}
    assert {a.case.W for a in al} >= {1, 40, 41, 121} and 1 in {a.case.H for a in al}
    for name, a in RC.ALIGN_CASES.items():
        rois = RC.align_boxes(a)
        pages = rois[:, 0].astype(int)
        assert set(range(a.case.B)) - set(pages.tolist()) and {-2, a.case.B + 3} <= set(pages.tolist())
        if a.exact:                                  # corners on multiples of 8 px, bins of a power-of-two size
            assert np.array_equal(rois[:, 1:] % 8, np.zeros_like(rois[:, 1:]))
            bw, bh = (rois[:, 3] - rois[:, 1]) / 4 / a.case.PW, (rois[:, 4] - rois[:, 2]) / 4 / a.case.PH
            lg = np.log2(np.abs(np.concatenate([bw, bh])))
            assert np.array_equal(lg, np.round(lg)) and lg.min() >= 0
    # aligned = 1 with inverted boxes wider than one owner segment and taller than 4 rows
    wide = [a for a in al if a.aligned and a.sr > 0 and a.case.W > RC.ROI_XW and a.case.H > 5]
    assert wide
    for a in wide:
        r = RC.align_boxes(a)[:-2]
        assert (((r[:, 1] - r[:, 3]) * RC.SCALE > RC.ROI_XW) & ((r[:, 2] - r[:, 4]) * RC.SCALE > 4)).any()
    real, index, feat, gout = RC.long_list()
    n = RC.ALIGN_LONG.case.n
    assert n == 2 ** 18 + 1 and index[0] == 0 and index[-1] == n - 1 and (np.diff(index) > 0).all()
    assert set(real[:, 0].astype(int).tolist()) == {0, 1} and (np.diff(real[:, 0]) < 0).any()
