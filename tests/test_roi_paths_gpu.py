"""Every RoIPool and RoIAlign launch path of csrc/roi_gat.hip against the oracle on the hard inputs of tests/roi_cases.py
(tests/test_roi_cases_cpu.py proves that the inputs are hard): tied maxima in every pixel phase and trip of the forward's
scan, every window size around the trip lengths, degenerate boxes, bad and empty pages, every bin shape and channel
count of the backward entry pass, map widths at the owner-segment edges, and the long-list page ranges of RoIAlign.

Per launch: outputs sit in wider and longer buffers pre-filled with 7.0 (head_cases.place / untouched), inputs carry NaN
wherever a correct kernel does not read (pad columns, buffer tails, map pixels outside every window, the page without a
box, gradients of skipped boxes), and every launch runs twice with bit-equal results.  Tie maps, lazy operands and exact
gradients are compared with torch.equal (roi_cases: all arithmetic on them is exact); real-valued gradients are held to
head_cases.sum_bound with L = the largest number of contributions one output receives."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import _lib, engine  # noqa: E402
import head_cases as HC  # noqa: E402
import roi_cases as RC  # noqa: E402
from helpers import DEV, NAN  # noqa: E402

I32 = torch.int32
ALIGN_GATE = 1e-5                                    # tests/test_extension_gpu.py::test_roialign_kernels_match_self_oracle
BAD_ARG = 10001                                      # COVA_ERR_BAD_ARG (include/cova_hip.h)


def call(name, *args):
    return _lib.call(name, *args)


def query(name, *args):
    return _lib.query(name, *args)


def dev_in(a, ld=None, off=0):
    """input on the device ([R, C] or [C]): NaN (integers: -1) in front of it, in the pad columns and behind the last row"""
    t = torch.as_tensor(a)
    if t.dim() == 1:
        t = t.view(1, -1)
    return HC.place(t, t.shape[1] if ld is None else ld, off, NAN if t.is_floating_point() else -1, device=DEV)[1]


def dev_out(R, C, ld=None, off=0, dtype=torch.float32, fill=HC.CANARY):
    """(flat, view): output buffer pre-filled with the canary"""
    return HC.place((R, C, dtype), C if ld is None else ld, off, fill, device=DEV)


def scratch(words):
    """workspace whose old content is NaN as a float and -1 as an int"""
    return torch.full((words,), -1, dtype=I32, device=DEV)


def twice(fn):
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y), "two runs differ"
    return a


def nhwc_dev(m, mask=None):
    """[B, C, H, W] numpy -> [B * H * W, C] on the device (16-byte aligned), NaN at the pixels outside ``mask`` [B, H, W]"""
    t = torch.from_numpy(np.ascontiguousarray(m)).permute(0, 2, 3, 1).contiguous()
    if mask is not None:
        t[~torch.from_numpy(mask)] = NAN
    return dev_in(t.reshape(-1, t.shape[-1]), off=4)


def nchw(g, case):
    return g.view(case.B, case.H, case.W, case.C).permute(0, 3, 1, 2).cpu()


def same(got, ref, name):
    ref = torch.as_tensor(ref)
    got = got.detach().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    nbad = int((got.double() != ref.double()).sum())
    assert nbad == 0, "%s: %d of %d elements differ from the reference" % (name, nbad, ref.numel())


def within_bound(got, ref, mag, L, name):
    ref, mag = torch.as_tensor(ref), torch.as_tensor(mag)
    bad, worst = HC.violations(got, ref, mag, L)
    print("%s: worst |err| / bound = %.3f over %d elements (L = %d)" % (name, worst, ref.numel(), L))
    assert bad == 0, "%s: %d of %d elements outside the f32 sum bound (worst %.3g x the bound)" % (
        name, bad, ref.numel(), worst)


def close(got, ref, tol, name):
    got, ref = got.detach().cpu().double(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-6)) if ref.numel() else 0.0
    print("%s: max|err|/max|ref| = %.3e (gate %.1e)" % (name, err, tol))
    assert err < tol, "%s: max|err|/max|ref| = %.3e" % (name, err)


def test_the_case_tables_reach_every_kernel_instantiation():
    hit = {}
    for name, c in list(RC.FWD_CASES.items()) + list(RC.BWD_CASES.items()) + [(k, a.case) for k, a in RC.ALIGN_CASES.items()] \
            + [("long_list", RC.ALIGN_LONG.case)]:
        for v in RC.variants(c):
            hit.setdefault(v, []).append(name)
    for v in RC.ALL_VARIANTS:
        print("%-40s %d cases, e.g. %s" % (v, len(hit.get(v, [])), ", ".join(hit.get(v, [])[:3])))
    assert len(RC.ALL_VARIANTS) == 14 and sorted(hit) == RC.ALL_VARIANTS


# ------------------------------------------------------------------------------------------------ RoIPool forward
@pytest.mark.parametrize("lazy", [0, 1])
@pytest.mark.parametrize("name", list(RC.FWD_CASES))
def test_roipool_forward_equals_the_oracle_bit_for_bit(name, lazy):
    case = RC.FWD_CASES[name]
    B, C, H, W, PH, PW, n, _ = case
    T = C * PH * PW
    ld = T + 5
    print("%s: %s, %d blocks" % (name, RC.variants(case)[lazy], RC.fwd_grid(case)))
    feat, rois, ref, ref_arg = RC.forward_reference(name, lazy)
    mask = RC.read_mask(case, rois)
    assert not mask[B - 1].any() and not mask.all()                  # the page without a box is NaN throughout
    r = dev_in(rois)
    if lazy:
        ops = RC.lazy_operands(case)
        z, x = nhwc_dev(ops["z"], mask), nhwc_dev(ops["x"], mask)
        scale, shift = dev_in(ops["scale"], off=4), dev_in(ops["shift"], off=8)
    else:
        f = nhwc_dev(feat, mask)

    def run():
        (fo, out), (fa, arg) = dev_out(n, T, ld, off=3), dev_out(n, T, off=3, dtype=I32)
        fz, zmax = dev_out(n, T, off=1)
        if lazy:
            call("cova_roipool_fwd_bn", z, x, scale, shift, r, n, B, C, H, W, PH, PW, RC.SCALE, out, ld, arg, zmax)
        else:
            call("cova_roipool_fwd", f, r, n, B, C, H, W, PH, PW, RC.SCALE, out, ld, arg)
        assert HC.untouched(fo, out, T) and HC.untouched(fa, arg, T), "written outside [n, C * PH * PW]"
        assert HC.untouched(fz, zmax, T if lazy else 0), "zmax: written outside [n, C * PH * PW]"
        return out[:, :T].clone(), arg.clone(), zmax.clone()
    out, arg, zmax = twice(run)
    same(arg, ref_arg.reshape(n, T), "argmax")
    same(out, ref.reshape(n, T), "pooled")
    bad = ~RC.good_page(rois, B)
    assert bad.sum() == 2 and (out.cpu()[bad] == 0).all() and (arg.cpu()[bad] == -1).all()
    if lazy:
        valid = ref_arg >= 0
        page = np.where(bad, 0, rois[:, 0]).astype(np.int64).reshape(n, 1, 1, 1)
        zref = ops["z"].reshape(B, C, -1)[page, np.arange(C).reshape(1, C, 1, 1), np.maximum(ref_arg, 0)]
        assert np.array_equal(zmax.cpu().numpy().reshape(ref_arg.shape)[valid], zref[valid])


def test_roipool_forward_without_boxes_writes_nothing():
    z = torch.zeros(64, 64, device=DEV)
    for lazy in (0, 1):
        (fo, out), (fa, arg) = dev_out(1, 64), dev_out(1, 64, dtype=I32)
        if lazy:
            call("cova_roipool_fwd_bn", z, z, z, z, z, 0, 1, 64, 8, 8, 1, 1, RC.SCALE, out, 64, arg, z)
        else:
            call("cova_roipool_fwd", z, z, 0, 1, 64, 8, 8, 1, 1, RC.SCALE, out, 64, arg)
        assert HC.untouched(fo, out, 0) and HC.untouched(fa, arg, 0)


# ------------------------------------------------------------------------------------------------ RoIPool backward
class BwdInputs:
    """device operands of the three backward entry points for one case and one gradient"""

    def __init__(self, case, d, gout, mean, invstd):
        self.case = case
        n, T = case.n, case.C * case.PH * case.PW
        self.ld_g, self.ld_p = T + 3, T + 5
        self.gout = dev_in(gout.reshape(n, T), self.ld_g, off=1)
        self.pooled = dev_in(d["pooled"].reshape(n, T), self.ld_p, off=2)
        self.zmax, self.arg = dev_in(d["zmax"].reshape(n, T)), dev_in(torch.from_numpy(d["argmax"].reshape(n, T)))
        self.rois, self.mean, self.invstd = dev_in(d["rois"]), dev_in(mean), dev_in(invstd)
        self.npart = query("cova_roipool_bwd_bn_num_partials", n)
        self.words = query("cova_roipool_bwd_workspace_words", n, case.B, case.C, case.PH, case.PW)

    def run(self, api, tail=None, expect_refusal=False):
        """-> (gfeat [B*H*W, C], partial [npart, 2, C] or None), canaries checked"""
        c = self.case
        geo = (c.n, c.B, c.C, c.H, c.W, c.PH, c.PW, RC.SCALE)
        (fg, g), (fp, part) = dev_out(c.B * c.H * c.W, c.C, off=4), dev_out(self.npart, 2 * c.C, off=4)
        ws = scratch(self.words)
        try:
            if api == "plain":
                call("cova_roipool_bwd", self.gout, self.ld_g, self.rois, self.arg, *geo, g, ws)
            else:
                args = (self.gout, self.ld_g, self.pooled, self.ld_p, self.zmax, self.rois, self.arg) + geo \
                    + (self.mean, self.invstd, g, part, ws)
                if api == "bn":
                    call("cova_roipool_bwd_bn", *args)
                else:
                    call("cova_roipool_bwd_bn_tail", *(args + (tail.ptr,)))
        except _lib.CovaHipError as e:
            assert expect_refusal and str(BAD_ARG) in str(e), e
            torch.cuda.synchronize()
            assert HC.untouched(fg, g, 0) and HC.untouched(fp, part, 0), "a refused call wrote something"
            return None, None
        assert not expect_refusal, "the call was not refused"
        assert HC.untouched(fg, g, c.C), "gfeat: written outside the map"
        assert HC.untouched(fp, part, 0 if api == "plain" else 2 * c.C), "partial: written outside [npart, 2, C]"
        return g.clone(), (None if api == "plain" else part.clone().view(self.npart, 2, c.C))


def bn_layer(C, scale, mean, invstd, count):
    st = engine.bn_state(C, scale, count, True)
    st.mean.copy_(mean.view(-1)), st.invstd.copy_(invstd.view(-1)), st.scale.copy_(scale.view(-1))
    return st


@pytest.mark.parametrize("name", list(RC.BWD_CASES))
def test_roipool_backward_entry_points_equal_the_float64_scatter(name):
    case = RC.BWD_CASES[name]
    B, C, H, W, PH, PW, n, _ = case
    print("%s: %s" % (name, ", ".join(RC.variants(case))))
    d = RC.backward_inputs(name)
    arg, rois = d["argmax"], d["rois"]
    keep = (d["pooled"] > 0) & (arg >= 0)
    L = RC.max_hits(rois, arg, B, H, W)
    scale = dev_in(RC.lazy_operands(case)["scale"])
    for exact in (True, False):
        gout, mean, invstd = RC.gradients(case, exact)
        g4 = gout.reshape(arg.shape)
        gm = np.where(keep, g4, np.float32(0))
        inp = BwdInputs(case, d, gout, mean, invstd)
        tag = "%s %s" % (name, "exact" if exact else "real")

        def check(got, grad, what):
            ref = RC.scatter64(grad, rois, arg, B, H, W)
            assert not ref[B - 1].any() and ref.any()                # the page without a box; the others are hit
            if exact:
                same(nchw(got, case), ref, what)
            else:
                within_bound(nchw(got, case), ref, RC.scatter64(np.abs(grad), rois, arg, B, H, W), L, what)

        g_plain, _ = twice(lambda: inp.run("plain"))
        check(g_plain, g4, tag + " cova_roipool_bwd gfeat")
        g_bn, part = twice(lambda: inp.run("bn"))
        check(g_bn, gm, tag + " cova_roipool_bwd_bn gfeat")
        (s0, s1), (m0, m1) = RC.stat_sums64(gm, d["zmax"], mean, invstd)
        sums = part.double().sum(0).cpu()
        if exact:
            same(sums[0], s0, tag + " sum g'"), same(sums[1], s1, tag + " sum g' xhat")
        else:                                        # n * PH * PW terms per channel; (zmax - mean) * invstd is exact
            within_bound(sums[0], s0, m0, n * PH * PW, tag + " sum g'")
            within_bound(sums[1], s1, m1, n * PH * PW, tag + " sum g' xhat")
        # the BatchNorm-backward finalize as the entry pass's tail: the separate launch, bit for bit; refused at C > 64
        st = bn_layer(C, scale, inp.mean, inp.invstd, B * H * W)
        dg_t, db_t, abc_t, tail = engine.bn_tail_bwd(st, B * H * W, None, "x.", scale)
        if C > 64:
            inp.run("tail", tail, expect_refusal=True)
            continue
        dg_r, db_r, abc_r = engine._bn_abc_from_partials(part.contiguous(), inp.npart, st, B * H * W, None, "x.", scale)
        g_t, part_t = inp.run("tail", tail)
        assert torch.equal(g_t, g_bn) and torch.equal(part_t, part), tag + ": tail against separate launch"
        assert torch.equal(abc_t, abc_r) and torch.equal(dg_t, dg_r) and torch.equal(db_t, db_r), tag + ": tail finalize"
        assert torch.isfinite(abc_t).all()


@pytest.mark.parametrize("PH,PW,C", [(3, 3, 64), (2, 5, 64), (3, 3, 128), (7, 7, 128)])
def test_roipool_backward_without_boxes_zeroes_the_map(PH, PW, C):
    """n_rois == 0: gfeat is "fully written", so a NaN-filled map comes back all zero, and so does partial row 0"""
    case = RC.Case(2, C, 3, 41, PH, PW, 0, "bwd")
    one = torch.full((8,), NAN, device=DEV)
    mean, invstd, scale = (dev_in(np.ones(C, np.float32)) for _ in range(3))
    assert query("cova_roipool_bwd_bn_num_partials", 0) == 1
    geo = (0, case.B, C, case.H, case.W, PH, PW, RC.SCALE)
    st = bn_layer(C, scale, mean, invstd, case.B * case.H * case.W)
    for api in ("plain", "bn") + (("tail",) if C == 64 else ()):
        (fg, g) = dev_out(case.B * case.H * case.W, C, off=4)
        g.fill_(NAN)
        (fp, part) = dev_out(1, 2 * C, off=4)
        ws = scratch(query("cova_roipool_bwd_workspace_words", 0, case.B, C, PH, PW))
        if api == "plain":
            call("cova_roipool_bwd", one, 0, one, one, *geo, g, ws)
        else:
            args = (one, 0, one, 0, one, one, one) + geo + (mean, invstd, g, part, ws)
            if api == "bn":
                call("cova_roipool_bwd_bn", *args)
            else:
                dg, db, abc, tail = engine.bn_tail_bwd(st, case.B * case.H * case.W, None, "x.", scale)
                call("cova_roipool_bwd_bn_tail", *(args + (tail.ptr,)))
                assert (dg == 0).all() and (db == 0).all() and torch.isfinite(abc).all()
            assert (part == 0).all() and HC.untouched(fp, part, 2 * C)
        assert (g == 0).all() and HC.untouched(fg, g, C), api


# ------------------------------------------------------------------------------------------------ RoIAlign
def run_align(a, feat_dev, rois_dev, gout_dev, ld_g, n):
    """forward and backward, twice each -> (out [n, T], gfeat [B*H*W, C])"""
    B, C, H, W, PH, PW = a.case[:6]
    T = C * PH * PW
    ld = T + 7

    def fwd():
        fo, out = dev_out(n, T, ld, off=3)
        call("cova_roialign_fwd", feat_dev, rois_dev, n, B, C, H, W, PH, PW, RC.SCALE, a.sr, a.aligned, out, ld)
        assert HC.untouched(fo, out, T), "written outside [n, C * PH * PW]"
        return (out[:, :T].clone(),)

    def bwd():
        fg, g = dev_out(B * H * W, C, off=4)
        call("cova_roialign_bwd", gout_dev, ld_g, rois_dev, n, B, C, H, W, PH, PW, RC.SCALE, a.sr, a.aligned, g,
             scratch(2 * B + 16))
        assert HC.untouched(fg, g, C), "gfeat: written outside the map"
        return (g.clone(),)
    return twice(fwd)[0], twice(bwd)[0]


@pytest.mark.parametrize("name", list(RC.ALIGN_CASES))
def test_roialign_equals_the_oracle_and_its_autograd(name):
    a = RC.ALIGN_CASES[name]
    case = a.case
    B, C, H, W, PH, PW, n, _ = case
    T = C * PH * PW
    rois = RC.align_boxes(a)
    feat, gout = RC.align_data(a)
    ref_out, ref_g = RC.align_reference(feat, rois, gout, a)
    assert ref_out.any() and ref_g.any() and not ref_g[B - 1].any()
    mask = np.ones((B, H, W), bool)
    mask[B - 1] = False                              # the page without a box
    out, g = run_align(a, nhwc_dev(feat, mask), dev_in(rois), dev_in(gout, T + 2, off=1), T + 2, n)
    bad = ~RC.good_page(rois, B)
    assert (out.cpu()[bad] == 0).all()
    if a.exact:
        same(out, ref_out, name + " forward"), same(nchw(g, case), ref_g, name + " backward")
    else:
        close(out, ref_out, ALIGN_GATE, name + " forward")
        close(nchw(g, case), ref_g, ALIGN_GATE, name + " backward")


def test_roialign_without_boxes():
    a = RC.Align(RC.Case(2, 64, 3, 41, 2, 5, 0, "align"), 2, 1, True)
    one = torch.full((8,), NAN, device=DEV)
    fo, out = dev_out(1, 640)
    call("cova_roialign_fwd", one, one, 0, 2, 64, 3, 41, 2, 5, RC.SCALE, 2, 1, out, 640)
    assert HC.untouched(fo, out, 0)
    fg, g = dev_out(2 * 3 * 41, 64, off=4)
    g.fill_(NAN)
    call("cova_roialign_bwd", one, 0, one, 0, 2, 64, 3, 41, 2, 5, RC.SCALE, 2, 1, g, scratch(2 * 2 + 16))
    assert (g == 0).all() and HC.untouched(fg, g, 64)
    assert RC.variants(a.case) == ["page_range<block>"]


def test_roialign_long_list_page_ranges():
    """n_rois = 2^18 + 1: the page ranges come from the init + grid kernels (atomics across blocks).  All boxes but twelve
    carry page index B (skipped everywhere; their gradient rows are NaN); the twelve sit at the front, the middle and
    the very last index.  Equal to the oracle on the twelve alone, and to the same twelve in a list of 2^18 boxes (one
    block finds the ranges)."""
    a = RC.ALIGN_LONG
    case = a.case
    B, C, H, W, PH, PW, n, _ = case
    assert RC.variants(case) == ["page_range<grid>"] and RC.variants(case._replace(n=n - 1)) == ["page_range<block>"]
    real, index, feat, g_real = RC.long_list()
    ref_out, ref_g = RC.align_reference(feat, real, g_real, a)
    assert ref_g[0].any() and ref_g[1].any()
    fd = nhwc_dev(feat)

    def lists(total, idx):
        rois = torch.empty(total + 2, 5, device=DEV)
        rois[:] = torch.tensor([float(B), 8.0, 8.0, 40.0, 24.0], device=DEV)
        rois[total:] = NAN
        rois[torch.from_numpy(idx).to(DEV)] = torch.from_numpy(real).to(DEV)
        gout = torch.full((total + 2, C), NAN, device=DEV)
        gout[torch.from_numpy(idx).to(DEV)] = torch.from_numpy(g_real).to(DEV)
        return rois, gout

    rois, gout = lists(n, index)
    out, g = run_align(a, fd, rois, gout, C, n)
    rows = torch.from_numpy(index).to(DEV)
    same(out[rows], ref_out, "long list forward")
    other = torch.ones(n, dtype=torch.bool, device=DEV)
    other[rows] = False
    assert (out[other] == 0).all()
    same(nchw(g, case), ref_g, "long list backward")
    cut = index - (index > 3)                         # one skipped box less: the same real boxes in the same order
    rois, gout = lists(n - 1, cut)
    out_c, g_c = run_align(a, fd, rois, gout, C, n - 1)
    assert torch.equal(g_c, g) and torch.equal(out_c[torch.from_numpy(cut).to(DEV)], out[rows])
