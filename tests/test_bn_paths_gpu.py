"""Every launch path of csrc/bn.hip and csrc/bn1d.hip on the lattice operands of tests/bn_cases.py
(tests/test_bn_cases_cpu.py proves that the cases reach every form of the host dispatch and that the checkers flag a
subtly wrong kernel).

Per launch: the operands sit in buffers that are NaN in front of them, in every pad column and behind their last row
(head_cases.place); the outputs sit in buffers filled with a sentinel and head_cases.untouched is asserted; every launch
runs twice with bit-equal results.  On the lattice every correct f32 evaluation is exact, so the statistics partials (row
by row, not only their totals), the apply passes and the whole stem pool -- pooled values, arg-max codes, ymax, backward
sums, dz, dy1 -- are compared element for element with the float64 references.  The finalize kernels are compared with
their numpy restatement: mean to the bit, invstd / abc / coef to one f32 ulp (fp64 sqrt and divide ahead of one cast),
scale and shift exactly from the kernel's own invstd and mean (shift in either of its two correct forms: the product
rounded first, or contracted into one fma)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import _lib  # noqa: E402
import bn_cases as BC  # noqa: E402
import head_cases as HC  # noqa: E402
from helpers import DEV, NAN  # noqa: E402

call, query = _lib.call, _lib.query
F32, F64 = np.float32, np.float64
S = BC.SENTINEL
assert S == HC.CANARY


def put(a, pad=0, off=0, fill=NAN):
    """an input [R, C] (a vector: [1, C]) on the device, NaN in front, in the pad columns and behind -> the view to pass"""
    a = np.ascontiguousarray(a)
    a = a.reshape(1, -1) if a.ndim == 1 else a.reshape(-1, a.shape[-1])
    view = HC.place(torch.from_numpy(a), a.shape[1] + pad, BC.OFF + off, fill, device=DEV)[1]
    assert view.data_ptr() % 16 == (4 * off) % 16 or a.dtype != F32
    return view


class Out:
    """an output [R, C] in a sentinel-filled buffer"""

    def __init__(self, R, C, pad=0, off=0, dtype=torch.float32, fill=S):
        self.C, self.fill = C, fill
        self.flat, self.view = HC.place((R, C, dtype), C + pad, BC.OFF + off, fill, device=DEV)

    def get(self):
        assert HC.untouched(self.flat, self.view, self.C, self.fill), "written outside the output"
        return self.view[:, :self.C].contiguous().cpu().numpy()


def twice(run):
    """run() -> list of Out; launched twice on fresh buffers, bit-equal -> the arrays of the first launch"""
    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x.flat.view(torch.uint8), y.flat.view(torch.uint8)), "two launches differ"
    return [x.get() for x in a]


def same(got, ref, what):
    n = BC.mismatches(got, ref)
    assert n == 0, "%s: %d of %d elements differ from the exact reference" % (what, n, np.asarray(ref).size)


# ------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("name", list(BC.STAT_CASES))
def test_statistics_partials_row_by_row(name):
    c = BC.STAT_CASES[name]
    o = BC.stat_operands(c)
    R, C, ld, lda = c.R, c.C, c.C + c.pad, c.C + c.a_pad
    rpc, nch = query("cova_colreduce_rows_per_chunk", R, C), query("cova_colreduce_num_chunks", R, C)
    assert rpc == BC.rows_per_chunk(R, C) and nch == BC.num_chunks(R, C)
    x, dout, z = (put(o[k], c.pad, c.off) for k in ("x", "dout", "z"))
    act = put(o["act"], c.a_pad, c.a_off) if c.act else None
    mean, invstd = put(o["mean"]), put(o["invstd"])

    def fwd():
        p = Out(nch * 2, C)
        call("cova_colstats", x, ld, R, C, p.view)
        return [p]

    def bwd():
        p = Out(nch * 2, C)
        call("cova_bn_bwd_reduce", dout, ld, act, lda, z, ld, mean, invstd, R, C, p.view)
        return [p]

    same(twice(fwd)[0].reshape(nch, 2, C), BC.stat_partials(o, R, C, 0), name + " colstats")
    same(twice(bwd)[0].reshape(nch, 2, C), BC.stat_partials(o, R, C, 1, c.act), name + " bwd_reduce")


# ------------------------------------------------------------------------------------------------ apply
@pytest.mark.parametrize("name", list(BC.APPLY_CASES))
def test_apply_and_backward_apply(name):
    c = BC.APPLY_CASES[name]
    o = BC.apply_operands(c.R, c.C)
    R, C, ld, ldr = c.R, c.C, c.C + c.pad, c.C + c.r_pad
    z, dout = put(o["z"], c.pad, c.off), put(o["dout"], c.pad, c.off)
    res = put(o["res"], c.r_pad, c.r_off) if c.res else None
    act = put(o["act"], c.pad, c.off) if c.relu else None
    scale, shift, mean, invstd, coef = (put(o[k]) for k in ("scale", "shift", "mean", "invstd", "coef"))

    def fwd():
        out = Out(R, C, c.pad, c.off)
        call("cova_bn_act_fwd", z, ld, scale, shift, res, ldr, out.view, ld, R, C, c.relu)
        return [out]

    def bwd():
        dz, dres = Out(R, C, c.pad, c.off), Out(R, C, c.r_pad, c.r_off)
        call("cova_bn_bwd_apply", dout, ld, act, ld, z, ld, mean, invstd, scale, coef, dz.view, ld,
             dres.view if c.dres else None, ldr, R, C)
        return [dz, dres]

    same(twice(fwd)[0], BC.act_fwd_ref(o, c.res, c.relu), name + " out")
    dz, dres = twice(bwd)
    rdz, rdy = BC.bwd_apply_ref(o, c.relu)
    same(dz, rdz, name + " dz")
    same(dres, rdy if c.dres else np.full((R, C), S), name + " dres")


@pytest.mark.parametrize("name", list(BC.BITS_CASES))
def test_act_fwd_bits(name):
    R, with_res = BC.BITS_CASES[name]
    o = BC.apply_operands(R, 64)
    z, scale, shift = put(o["z"]), put(o["scale"]), put(o["shift"])
    res = put(o["res"]) if with_res else None

    def run():
        out, bits = Out(R, 64), Out(R, 2, dtype=torch.int32, fill=7)
        call("cova_bn_act_fwd_bits", z, scale, shift, res, out.view, bits.view, R)
        return [out, bits]

    out, bits = twice(run)
    ref = BC.act_fwd_ref(o, with_res, True)
    same(out, ref, name + " out")
    assert np.array_equal(bits.view(np.uint32), BC.pack_bits(ref)) and np.array_equal(bits.view(np.uint32), BC.pack_bits(out))


@pytest.mark.parametrize("name", list(BC.ACT2_CASES))
def test_act2_fwd(name):
    R, C, relu = BC.ACT2_CASES[name]
    a, b = BC.apply_operands(R, C), BC.apply_operands(R, C, seed=17)
    ops = [put(v) for v in (a["z"], a["scale"], a["shift"], b["z"], b["scale"], b["shift"])]

    def run():
        out = Out(R, C)
        call("cova_bn_act2_fwd", *ops, out.view, R, C, relu)
        return [out]

    same(twice(run)[0], BC.act2_ref(a, b, relu), name)


# ------------------------------------------------------------------------------------------------ finalize, fold
def check_fwd_params(got, ref, gamma, beta, what):
    """mean, invstd, scale, shift [C] of a kernel against finalize_fwd_ref"""
    mean, invstd, scale, shift = got
    assert np.array_equal(mean, ref["mean"]), what + " mean"
    assert BC.within_ulps(invstd, ref["invstd"]).all(), what + " invstd"
    assert BC.within_ulps(scale, ref["scale"]).all(), what + " scale"
    assert np.array_equal(scale, gamma * invstd), what + " scale is not gamma * the invstd written next to it"
    unfused, fused = BC.shift_of(beta, mean, scale)
    assert ((shift == unfused) | (shift == fused)).all(), what + " shift is neither form of beta - mean * scale"


def check_running(got, old, ref, what):
    assert BC.within_ulps(got, ref, 2, np.maximum(np.abs(old), np.abs(ref))).all(), what


@pytest.mark.parametrize("name", list(BC.FIN_CASES))
def test_finalize_kernels_on_integer_partials(name):
    nparts, C = BC.FIN_CASES[name]
    o = BC.fin_operands(nparts, C)
    pf, pb = put(o["fwd"].reshape(nparts * 2, C)), put(o["bwd"].reshape(nparts * 2, C))
    gamma, beta, mean, invstd, scale = (put(o[k]) for k in ("gamma", "beta", "mean", "invstd", "scale"))

    def fwd():
        outs = [Out(1, C) for _ in range(4)]                     # scale, shift, mean, invstd
        rm, rv, nbt = Out(1, C), Out(1, C), Out(1, 1, dtype=torch.int64, fill=7)
        rm.view[:, :C] = torch.from_numpy(o["rm"]).to(DEV)
        rv.view[:, :C] = torch.from_numpy(o["rv"]).to(DEV)
        nbt.view[:, :1] = 0
        call("cova_bn_finalize_fwd", pf, nparts, C, o["count"], gamma, beta, rm.view, rv.view, nbt.view, float(BC.MOMENTUM),
             BC.EPS, *(t.view for t in outs))
        return outs + [rm, rv, nbt]

    sc, sh, mu, is_, rm, rv, nbt = (a[0] for a in twice(fwd))
    ref = BC.finalize_fwd_ref(BC.combine(o["fwd"]), o["count"], o["gamma"], o["beta"], o["rm"], o["rv"])
    check_fwd_params((mu, is_, sc, sh), ref, o["gamma"], o["beta"], name)
    assert is_[0] == BC.INVSTD_OF_ZERO_VAR and mu[0] == 3.0      # the constant column: var clamped at 0
    check_running(rm, o["rm"], ref["running_mean"], name + " running_mean")
    check_running(rv, o["rv"], ref["running_var"], name + " running_var")
    assert int(nbt[0]) == 1

    def fwd_no_running():
        outs = [Out(1, C) for _ in range(4)]
        call("cova_bn_finalize_fwd", pf, nparts, C, o["count"], gamma, beta, None, None, None, float(BC.MOMENTUM), BC.EPS,
             *(t.view for t in outs))
        return outs

    for a, b in zip(twice(fwd_no_running), (sc, sh, mu, is_)):
        assert np.array_equal(a[0], b)

    def bwd():
        dg, db, coef = Out(1, C), Out(1, C), Out(2, C)
        call("cova_bn_finalize_bwd", pb, nparts, C, o["count"], dg.view, db.view, coef.view)
        return [dg, db, coef]

    def bwd_abc():
        dg, db, abc = Out(1, C), Out(1, C), Out(3, C)
        call("cova_bn_finalize_bwd_abc", pb, nparts, C, o["count"], dg.view, db.view, mean, invstd, scale, abc.view)
        return [dg, db, abc]

    rb = BC.finalize_bwd_ref(BC.combine(o["bwd"]), o["count"], o["mean"], o["invstd"], o["scale"])
    dg, db, coef = twice(bwd)
    dg2, db2, abc = twice(bwd_abc)
    for g in (dg, dg2):
        same(g[0], rb["dgamma"], name + " dgamma")
    for b in (db, db2):
        same(b[0], rb["dbeta"], name + " dbeta")
    assert BC.within_ulps(coef, rb["coef"]).all() and BC.within_ulps(abc, rb["abc"]).all()
    assert np.array_equal(abc[0], o["scale"])


@pytest.mark.parametrize("name", list(BC.FOLD_CASES))
def test_partials_fold(name):
    nparts, group, width = BC.FOLD_CASES[name]
    p = BC.fold_operands(nparts, width)
    pd = put(p)

    def run():
        out = Out(BC.cdiv(nparts, group), width)
        call("cova_partials_fold", pd, nparts, width, group, out.view)
        return [out]

    same(twice(run)[0], BC.fold_ref(p, group), name)


# ------------------------------------------------------------------------------------------------ the stem pool
def pool_forward(o, c, with_ymax=True):
    B, H1, W1 = c
    H2, W2 = BC.pool_out(H1), BC.pool_out(W1)
    y, scale, shift = put(o["y"]), put(o["scale"]), put(o["shift"])

    def run():
        out, idx = Out(B * H2 * W2, 64), Out(B * H2 * W2, 64, dtype=torch.uint8, fill=99)
        ymax = Out(B * H2 * W2, 64)
        call("cova_bn_relu_maxpool_fwd", y, scale, shift, out.view, idx.view, ymax.view if with_ymax else None, B, H1, W1)
        return [out, idx, ymax]

    return [a.reshape(B, H2, W2, 64) for a in twice(run)]


def pool_backward(o, c, dp, idx):
    """-> totals [2][64] of the reduce partials (float64), dz, dy1"""
    B, H1, W1 = c
    y, dpd, idxd = put(o["y"]), put(dp), put(idx, fill=255)
    scale, shift, mean, invstd = (put(o[k]) for k in ("scale", "shift", "mean", "invstd"))
    coef = put(o["coef"])
    npart = query("cova_bn_relu_maxpool_bwd_num_partials", B, H1, W1)
    assert npart == BC.pool_bwd_num_partials(B, H1, W1)

    def run():
        part, dz = Out(npart * 2, 64), Out(B * H1 * W1, 64)
        call("cova_bn_relu_maxpool_bwd_reduce", dpd, idxd, y, scale, shift, mean, invstd, part.view, B, H1, W1)
        call("cova_bn_relu_maxpool_bwd_apply", dpd, idxd, y, scale, shift, mean, invstd, coef, dz.view, B, H1, W1)
        return [part, dz]

    part, dz = twice(run)
    dy1 = None
    if "abc" in o:
        abc = put(o["abc"])

        def run1():
            d = Out(B * H1 * W1, 64)
            call("cova_pool_bwd_dy1", dpd, idxd, y, abc, d.view, B, H1, W1)
            return [d]

        dy1 = twice(run1)[0].reshape(B, H1, W1, 64)
    return part.reshape(npart, 2, 64).astype(F64).sum(0), dz.reshape(B, H1, W1, 64), dy1


@pytest.mark.parametrize("name", list(BC.POOL_CASES))
def test_pool_forward_codes_and_backward_are_exact(name):
    c = BC.POOL_CASES[name]
    o = BC.pool_operands(c)
    rout, ridx, rymax = BC.pool_fwd_ref(o["y"], o["scale"], o["shift"])
    out, idx, ymax = pool_forward(o, c)
    same(out, rout, name + " out")
    assert np.array_equal(idx, ridx), "%s: %d arg-max codes differ" % (name, int((idx != ridx).sum()))
    same(ymax, rymax, name + " ymax")
    dead = rout == 0                                             # no positive value: 0 at the first in-bounds position
    first = np.isfinite(BC.pool_fwd_emulate(o["y"], o["scale"], o["shift"])[3]).argmax(3)
    assert dead.any() and not out[dead].any() and np.array_equal(idx[dead], first[dead])
    out2, idx2, ymax2 = pool_forward(o, c, with_ymax=False)
    same(out2, rout, name + " out (no ymax)")
    assert np.array_equal(idx2, ridx) and (ymax2 == BC.SENTINEL).all()
    dp = o["dp0"] * (rout > 0)
    rdy, rtot, rdz = BC.pool_bwd_ref(o, dp, ridx)
    tot, dz, dy1 = pool_backward(o, c, dp, idx)
    same(tot, rtot, name + " reduce totals")
    same(dz, rdz, name + " dz")
    same(dy1, BC.pool_dy1_ref(dp, ridx, o["y"], o["abc"]), name + " dy1")


def test_threshold_probe_all_three_kernels_take_the_fused_decision():
    o, c = BC.probe_operands(), BC.PROBE_MAP
    rout, ridx, rymax = BC.pool_fwd_ref(o["y"], o["scale"], o["shift"])
    out, idx, ymax = pool_forward(o, c)
    tot, dz, _ = pool_backward(o, c, o["dp"], ridx)
    rdy, rtot, rdz = BC.pool_bwd_ref(o, o["dp"], ridx)
    bad = []
    for ch, (iy, ix) in enumerate(o["pixels"]):
        pos = ch % 2 == 0
        for oy, ox in BC.windows_of(c, iy, ix):
            want = F32(2.0 ** -24) if pos else F32(0)
            if out[0, oy, ox, ch] != want or (pos and idx[0, oy, ox, ch] != (iy - 2 * oy + 1) * 3 + (ix - 2 * ox + 1)):
                bad.append(("fwd", ch, oy, ox, float(out[0, oy, ox, ch]), int(idx[0, oy, ox, ch])))
        if tot[0, ch] != (1.0 if pos else 0.0) or tot[1, ch] != 0.0:
            bad.append(("reduce", ch, float(tot[0, ch]), float(tot[1, ch])))
        if dz[0, iy, ix, ch] != F32(F64(o["scale"][ch]) * ((1.0 if pos else 0.0) - 0.125)):
            bad.append(("apply", ch, iy, ix, float(dz[0, iy, ix, ch])))
    print("threshold probe: %d findings %s" % (len(bad), bad[:8]))
    assert not bad, bad[:8]
    same(out, rout, "probe out")
    assert np.array_equal(idx, ridx)
    same(ymax, rymax, "probe ymax")
    assert not out[..., 1::2].any()                              # the negated triple: 0 everywhere
    same(tot, rtot, "probe totals")
    same(dz, rdz, "probe dz")


# ------------------------------------------------------------------------------------------------ bn1d
def option14(v):
    assert query("cova_set_option", 14, v) == 0


@pytest.mark.parametrize("name", list(BC.BN1D_CASES))
def test_bn1d_both_forms_every_mode(name):
    c = BC.BN1D_CASES[name]
    o = BC.bn1d_operands(c)
    R, C, ld, p = c.R, c.C, c.C + c.pad, BC.BN1D_P
    x, dout, z, act = (put(o[k], c.pad) for k in ("x", "dout", "z", "act"))
    keep = put(o["keep"], fill=1)
    gamma, beta, mean, invstd, scale = (put(o[k]) for k in ("gamma", "beta", "mean", "invstd", "scale"))
    fin = BC.bn1d_fwd_ref(o, R)
    assert np.array_equal(fin["mean"], o["col_mean"])
    results = {}
    try:
        for opt in (0, 1):
            option14(opt)
            for relu, drop in BC.BN1D_MODES:
                what = "%s option14=%d relu=%d drop=%d %s" % ((name, opt, relu, drop) + (BC.bn1d_forms(c, opt, relu, drop),))

                def fwd():
                    out, dropped = Out(R, C, c.pad), Out(R, C, c.pad)
                    par = [Out(1, C) for _ in range(4)]          # scale, shift, mean, invstd
                    rm, rv, nbt = Out(1, C), Out(1, C), Out(1, 1, dtype=torch.int64, fill=7)
                    rm.view[:, :C] = torch.from_numpy(o["rm"]).to(DEV)
                    rv.view[:, :C] = torch.from_numpy(o["rv"]).to(DEV)
                    nbt.view[:, :1] = 0
                    call("cova_bn1d_fwd", x, ld, R, C, gamma, beta, rm.view, rv.view, nbt.view, float(BC.MOMENTUM), BC.EPS, relu,
                         out.view, ld, dropped.view if drop else None, ld, keep if drop else None, p, 0, 1,
                         *(t.view for t in par))
                    return [out, dropped] + par + [rm, rv, nbt]

                out, dropped, sc, sh, mu, is_, rm, rv, nbt = twice(fwd)
                sc, sh, mu, is_, rm, rv = (a[0] for a in (sc, sh, mu, is_, rm, rv))
                check_fwd_params((mu, is_, sc, sh), fin, o["gamma"], o["beta"], what)
                check_running(rm, o["rm"], fin["running_mean"], what + " running_mean")
                check_running(rv, o["rv"], fin["running_var"], what + " running_var")
                assert int(nbt[0, 0]) == 1
                rout, rdropped = BC.bn1d_apply_ref(o["x"], sc, sh, relu, o["keep"] if drop else None)
                same(out, rout, what + " out")
                same(dropped, rdropped if drop else np.full((R, C), S), what + " dropped")

                def bwd():
                    dz = Out(R, C, c.pad)
                    dg, db, cs = Out(1, C), Out(1, C), Out(1, C)
                    call("cova_bn1d_bwd", dout, ld, keep if drop else None, p, act if relu else None, ld, z, ld, mean, invstd,
                         scale, R, C, dg.view, db.view, dz.view, ld, cs.view)
                    return [dz, dg, db, cs]

                dz, dg, db, cs = twice(bwd)
                rb = BC.bn1d_bwd_ref(o, R, relu, drop)
                same(db[0], rb["dbeta"], what + " dbeta")
                same(dg[0], rb["dgamma"], what + " dgamma")
                t = torch.from_numpy
                nbad, worst = HC.violations(t(dz), t(rb["dz"]), t(rb["dz_mag"]), R)
                assert nbad == 0, "%s dz: %d elements outside the bound, worst %.2f x" % (what, nbad, worst)
                same(dz[rb["dz_exact"]], rb["dz"][rb["dz_exact"]], what + " dz where every step is an f32 number")
                nbad, worst = HC.violations(t(cs[0]), t(rb["colsum"]), t(rb["colsum_mag"]), R)
                assert nbad == 0, "%s colsum: %d elements outside the bound, worst %.2f x" % (what, nbad, worst)
                results[(opt, relu, drop)] = dict(out=out, dropped=dropped, scale=sc, shift=sh, mean=mu, invstd=is_,
                                                  running_mean=rm, running_var=rv, dz=dz, dgamma=dg, dbeta=db)
    finally:
        option14(1)
    for relu, drop in BC.BN1D_MODES:                             # the two forms, bit for bit
        a, b = results[(0, relu, drop)], results[(1, relu, drop)]
        for k in a:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), "%s relu=%d drop=%d: the forms differ in %s" % (
                name, relu, drop, k)
    if R == 2:
        assert BC.bn1d_bwd_ref(o, R, 0, 0)["dz_exact"].mean() > 0.5
