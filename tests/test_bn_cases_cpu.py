"""Checks on tests/bn_cases.py itself (no GPU): the table reaches every form the restated dispatch of csrc/bn.hip and
csrc/bn1d.hip can return, its operands keep every sum exact, the references agree with torch in float64, the pool cases
hold enough exact ties, and the checkers flag every seeded fault -- the last maximum kept, `>=` for `>`, the padding as
a candidate, a row lost or counted in the neighbouring chunk, a column skipped, -0.0 taken as positive, the ReLU
decision on a rounded product, a fold group one row too long, a clamped partial row read for a valid one."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
import bn_cases as BC  # noqa: E402

F64 = np.float64


def test_the_cases_reach_every_form():
    fwd = {BC.colreduce_key(BC.stat_forms(c)[0]) for c in BC.STAT_CASES.values()}
    bwd = {BC.colreduce_key(BC.stat_forms(c)[1]) for c in BC.STAT_CASES.values()}
    for name, c in BC.STAT_CASES.items():
        print("%-26s %s  %d chunks of %d rows" % (name, BC.stat_forms(c), BC.num_chunks(c.R, c.C), BC.rows_per_chunk(c.R, c.C)))
    assert sorted(fwd, key=str) == sorted(BC.ALL_COLREDUCE, key=str) == sorted(bwd, key=str)
    # c64 forward with a generic backward by the act operand alone; one row in the last chunk for every CB; grown chunks
    assert {BC.stat_forms(BC.STAT_CASES[n]) for n in ("stat-C64-act-ld68", "stat-C64-act-off1")} == \
        {("c64", ("generic", 64, 4, 1))}
    assert BC.stat_forms(BC.STAT_CASES["stat-C64-noact"]) == ("c64", "c64")
    for cb in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        assert any(BC.pow2_cols(c.C) == cb and c.R % BC.rows_per_chunk(c.R, c.C) == 1 and c.R > 1
                   for c in BC.STAT_CASES.values()), cb
    assert {BC.rows_per_chunk(c.R, c.C) for c in BC.STAT_CASES.values() if c.R == 131073} == {68, 96}
    assert any(c.C % BC.pow2_cols(c.C) for c in BC.STAT_CASES.values() if c.C > 256)           # ragged last column block

    af = {}
    for name, c in BC.APPLY_CASES.items():
        f = BC.apply_forms(c)
        print("%-30s fwd V%d bwd V%d" % (name, *f))
        assert f == ((4, 4) if name.startswith("apply-v4") else (1, 1)), name
        af.setdefault(f[0], []).append(c)
    assert sorted(af) == BC.ALL_APPLY
    for v, cs in af.items():        # the second trip of the grid-stride loop, both switches of every flag, in each form
        assert any(c.R * c.C // v > 256 * BC.ew_grid(c.R * c.C // v) for c in cs), v
        assert all({getattr(c, k) for c in cs} == {0, 1} for k in ("res", "relu", "dres")), v
    assert all(BC.APPLY_CASES[n].pad > 0 for n in ("apply-v4-ld-pad4", "apply-v1-ld9", "apply-v1-view-1610-of-1710"))
    assert BC.ew_grid(65537 * 16) == 4096 and BC.ew_grid(1) == 1 and BC.ew_grid(7 * 16) == 1

    f1, b1 = set(), set()
    for c in BC.BN1D_CASES.values():
        for opt in (0, 1):
            for relu, drop in BC.BN1D_MODES:
                f, b = BC.bn1d_forms(c, opt, relu, drop)
                f1.add(f)
                b1.add(b)
                if opt == 0 or c.C % 4:
                    assert f[0] == b[0] == "slice"
    assert sorted(f1) == sorted(BC.ALL_BN1D_FWD) and sorted(b1) == sorted(BC.ALL_BN1D_BWD)
    # the row limits, from both sides
    for R, nf, nb in ((2, 3, 3), (1536, 3, 3), (1537, 6, 6), (3072, 6, 6), (3073, 8, None), (4096, 8, None), (4097, None, None)):
        f, b = BC.bn1d_forms(BC.Bn1d(R, 8, 4), 1, 1, 1)
        assert f == (("v4", nf, 1) if nf else ("slice", 1)) and b == (("v4", nb, 1) if nb else ("slice", 1)), R

    grids = {n: BC.pool_grid(*c) for n, c in BC.POOL_CASES.items()}
    print(grids)
    # the XCD remap of the pool forward: fewer than 8 blocks; 18 = 2 mod 8 and 36 = 4 mod 8 (a remapped part and a tail)
    assert grids["pool-1x1x1"] < 8 and grids["pool-3x16x24"] == 18 and grids["pool-3x32x24"] == 36
    assert {c[0] for c in BC.FIN_CASES.values()} == set(BC.NPARTS)
    assert len(BC.CASES) == sum(len(t) for t in (BC.STAT_CASES, BC.APPLY_CASES, BC.BITS_CASES, BC.ACT2_CASES, BC.FIN_CASES,
                                                 BC.FOLD_CASES, BC.POOL_CASES, BC.BN1D_CASES))


@pytest.mark.parametrize("name", [n for n, c in BC.STAT_CASES.items() if c.R < 100000])
def test_statistics_operands_are_exact_and_the_checker_flags_every_fault(name):
    c = BC.STAT_CASES[name]
    assert BC.exact_ok(c)
    o = BC.stat_operands(c)
    for k in ("x", "dout", "z", "mean"):
        assert np.array_equal(o[k], np.round(o[k])) and np.abs(o[k]).max() <= 7
    assert set(np.unique(o["invstd"])) <= {0.25, 0.5, 1.0, 2.0}
    if c.C >= 3:
        assert (o["x"][:, 0] == 3).all() and not o["x"][:, 1].any()
    if c.R * c.C >= 32:
        assert np.signbit(o["act"][o["act"] == 0]).any() and not np.signbit(o["act"][o["act"] == 0]).all()
    for mode in (0, 1):
        ref = BC.stat_partials(o, c.R, c.C, mode, c.act)
        assert ref.shape == (BC.num_chunks(c.R, c.C), 2, c.C)
        assert np.abs(ref).max() <= 196 * BC.rows_per_chunk(c.R, c.C) and np.array_equal(ref * 4, np.round(ref * 4))
        assert BC.mismatches(ref.astype(np.float32), ref) == 0                      # the reference is an f32 number
        # an honest f32 evaluation, row after row, is exact
        a, b = BC.stat_terms(o, mode, c.act)
        rpc = BC.rows_per_chunk(c.R, c.C)
        seq = np.zeros((2, c.C), np.float32)
        for r in range(min(rpc, c.R)):
            seq[0] += a[r].astype(np.float32)
            seq[1] += b[r].astype(np.float32)
        assert BC.mismatches(seq, ref[0]) == 0
        for fault in BC.STAT_FAULTS:
            if BC.stat_expressible(fault, c, mode):
                bad = BC.stat_partials(o, c.R, c.C, mode, c.act, fault)
                n = BC.mismatches(bad, ref)
                assert n > 0, (name, mode, fault)
                if fault == "row_in_neighbour":                                      # the totals do not see it
                    assert np.array_equal(bad.sum(0), ref.sum(0))


def test_every_statistics_fault_is_expressed():
    for mode in (0, 1):
        for fault in BC.STAT_FAULTS:
            n = sum(BC.stat_expressible(fault, c, mode) for c in BC.STAT_CASES.values())
            print("mode %d %-22s expressible on %d of %d cases" % (mode, fault, n, len(BC.STAT_CASES)))
            assert n >= 10 or (fault == "negzero_positive" and mode == 0)


@pytest.mark.parametrize("R,C", [(65, 6), (130, 64), (63, 33)])
def test_statistics_finalize_and_apply_references_agree_with_torch_float64(R, C):
    o = BC.stat_operands(BC._st(R, C))
    ap = BC.apply_operands(R, C)
    x = torch.from_numpy(o["x"].astype(F64)).requires_grad_(True)
    gamma = torch.from_numpy(ap["shift"].astype(F64) + 5.0).requires_grad_(True)
    beta = torch.from_numpy(ap["shift"].astype(F64)).requires_grad_(True)
    res = torch.from_numpy(ap["res"].astype(F64))
    rm, rv = torch.zeros(C, dtype=torch.float64) + 0.5, torch.ones(C, dtype=torch.float64) * 2
    rm0, rv0 = rm.numpy().copy(), rv.numpy().copy()
    out = F.relu(F.batch_norm(x, rm, rv, gamma, beta, True, float(BC.MOMENTUM), BC.EPS) + res)
    dout = torch.from_numpy(o["dout"].astype(F64))
    (out * dout).sum().backward()
    tot = BC.combine(BC.stat_partials(o, R, C, 0))
    fin = BC.finalize_fwd_ref(tot, float(R), gamma.detach().numpy(), beta.detach().numpy(), rm0, rv0, dt=F64)
    mine = BC.act_fwd_ref(dict(z=o["x"], scale=fin["scale"], shift=fin["shift"], res=ap["res"]))
    close = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-12 * max(1.0, np.abs(np.asarray(b)).max())
    assert close(mine, out.detach().numpy())
    assert close(fin["running_mean"], rm.numpy()) and close(fin["running_var"], rv.numpy())
    if C >= 3:
        assert fin["var"][0] == 0.0 and fin["invstd"][0] == 1.0 / np.sqrt(BC.EPS)
    bo = dict(dout=o["dout"], act=mine, z=o["x"], mean=fin["mean"], invstd=fin["invstd"], scale=fin["scale"])
    btot = BC.combine(BC.stat_partials(bo, R, C, 1))
    fb = BC.finalize_bwd_ref(btot, float(R), fin["mean"], fin["invstd"], fin["scale"], dt=F64)
    bo["coef"] = fb["coef"]
    dz, dy = BC.bwd_apply_ref(bo)
    assert close(fb["dgamma"], gamma.grad.numpy()) and close(fb["dbeta"], beta.grad.numpy()) and close(dz, x.grad.numpy())
    assert close(dy, (dout * (out > 0)).numpy())
    # the affine form of the same apply step
    abc = fb["abc"]
    assert close(abc[0] * dy + abc[1] * o["x"].astype(F64) + abc[2], dz)


@pytest.mark.parametrize("name", list(BC.APPLY_CASES)[:4] + list(BC.APPLY_CASES)[5:13])
def test_apply_operands_are_exact(name):
    c = BC.APPLY_CASES[name]
    o = BC.apply_operands(c.R, c.C)
    assert set(np.abs(o["scale"])) <= {0.0, 0.25, 0.5, 1.0, 2.0, 4.0} and (c.C < 2 or (o["scale"] == 0).sum() == 1)
    for k in ("shift", "res", "coef"):
        assert np.array_equal(o[k] * 8, np.round(o[k] * 8))
    out = BC.act_fwd_ref(o, c.res, c.relu)
    dz, dy = BC.bwd_apply_ref(o, c.relu)
    for ref in (out, dz):
        assert BC.mismatches(ref.astype(np.float32), ref) == 0
    # fused and unfused f32 evaluations give the reference
    z, sc, sh = o["z"], o["scale"], o["shift"]
    assert BC.mismatches(BC.fma32(sc, z, sh), BC.act_fwd_ref(o, False, False)) == 0
    assert BC.mismatches(BC.unfused32(sc, z, sh), BC.act_fwd_ref(o, False, False)) == 0
    xh = (o["z"] - o["mean"]) * o["invstd"]
    dy32 = dy.astype(np.float32)
    assert BC.mismatches(o["scale"] * (dy32 - o["coef"][0] - xh * o["coef"][1]), dz) == 0
    assert BC.mismatches(o["scale"] * BC.fma32(-xh, o["coef"][1], dy32 - o["coef"][0]), dz) == 0
    if c.relu:
        assert BC.mismatches(BC.bwd_apply_ref(o, True, "negzero_positive")[0], dz) > 0
    bits = BC.pack_bits(np.where(np.arange(64) % 3 == 0, 1.0, -1.0).reshape(1, 64))
    assert bits.tolist() == [[sum(1 << k for k in range(32) if k % 3 == 0), sum(1 << k for k in range(32) if (k + 32) % 3 == 0)]]


def test_fma32_rounds_once():
    y, s, sh = BC.PROBE_Y, BC.PROBE_SCALE, BC.PROBE_SHIFT
    assert BC.fma32(y, s, sh) == np.float32(2.0 ** -24) and BC.unfused32(y, s, sh) == 0.0
    assert BC.fma32(y, -s, -sh) == np.float32(-2.0 ** -24) and BC.unfused32(y, -s, -sh) == 0.0
    rs = np.random.RandomState(0)
    a, b = rs.standard_normal(20000).astype(np.float32), rs.standard_normal(20000).astype(np.float32)
    c = ((-a * b) * (1 + rs.randint(-3, 4, 20000) * 2.0 ** -22)).astype(np.float32)             # heavy cancellation
    ref = np.array([np.float32(np.longdouble(x) * np.longdouble(y) + np.longdouble(z)) for x, y, z in zip(a, b, c)])
    if np.finfo(np.longdouble).nmant >= 63:             # (80-bit long double: the sum is exact or far from a tie here)
        assert np.array_equal(BC.fma32(a, b, c), ref)
    # 1 + 2^-24 + 2^-60: rounding the float64 sum to nearest first would land on the tie and then on 1
    assert BC.fma32(np.float32(2.0 ** -30), np.float32(2.0 ** -30), np.float32(1)) == 1.0
    assert BC.fma32(np.float32(1 + 2.0 ** -23), np.float32(2.0 ** -24), np.float32(1)) == np.float32(1 + 2.0 ** -23)


@pytest.mark.parametrize("name", list(BC.FIN_CASES))
def test_finalize_references_and_the_clamped_row_fault(name):
    nparts, C = BC.FIN_CASES[name]
    o = BC.fin_operands(nparts, C)
    for k in ("fwd", "bwd"):
        tot = BC.combine(o[k])
        assert np.abs(tot).max() < 2 ** 24 and np.array_equal(tot * 4, np.round(tot * 4))
        walked = BC.combine(o[k], "walk")               # the sixteen-slice walk without a fault: every row once
        assert np.array_equal(walked, tot)
        bad = BC.combine(o[k], "clamped_row_for_last_valid")
        if nparts >= 17:                                # below that a trip holds one valid row: the clamp IS that row
            assert BC.mismatches(bad, tot) > 0
        else:
            assert np.array_equal(bad, tot)
    tot = BC.combine(o["fwd"])
    fin = BC.finalize_fwd_ref(tot, o["count"], o["gamma"], o["beta"], o["rm"], o["rv"])
    assert all(v.dtype == np.float32 for k, v in fin.items() if k != "var") and (fin["var"] >= 0).all()
    assert fin["invstd"][0] == BC.INVSTD_OF_ZERO_VAR and fin["mean"][0] == 3.0
    if nparts in (1, 16, 128, 256):                     # count a power of two: the mean is the quotient itself
        assert np.array_equal(fin["mean"].astype(F64), tot[0] / o["count"])
    # against F.batch_norm on data with these sums: two values per chunk row pair reproduce (sum, sumsq)
    s, q = o["fwd"][:, 0].astype(F64), o["fwd"][:, 1].astype(F64)
    d = np.sqrt(np.maximum(q / 64 - (s / 64) ** 2, 0.0))
    data = np.concatenate([np.repeat(s / 64 + d, 32, 0), np.repeat(s / 64 - d, 32, 0)])
    g64, b64 = torch.from_numpy(o["gamma"].astype(F64)), torch.from_numpy(o["beta"].astype(F64))
    rm, rv = torch.from_numpy(o["rm"].astype(F64)), torch.from_numpy(o["rv"].astype(F64))
    ref = F.batch_norm(torch.from_numpy(data), rm, rv, g64, b64, True, float(BC.MOMENTUM), BC.EPS).numpy()
    f64 = BC.finalize_fwd_ref(tot, o["count"], o["gamma"], o["beta"], o["rm"], o["rv"], dt=F64)
    mine = f64["scale"] * data + f64["shift"]
    assert np.abs(mine - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())   # (sqrt of the data costs digits, not the formula)
    assert np.abs(f64["running_mean"] - rm.numpy()).max() <= 1e-12 * max(1.0, np.abs(rm.numpy()).max())
    fb = BC.finalize_bwd_ref(BC.combine(o["bwd"]), o["count"], o["mean"], o["invstd"], o["scale"])
    assert BC.mismatches(fb["dbeta"], BC.combine(o["bwd"])[0]) == 0 and fb["abc"].shape == (3, C)


@pytest.mark.parametrize("name", list(BC.FOLD_CASES))
def test_fold_reference_and_the_group_fault(name):
    nparts, group, width = BC.FOLD_CASES[name]
    p = BC.fold_operands(nparts, width)
    ref = BC.fold_ref(p, group)
    assert ref.shape == (BC.cdiv(nparts, group), width) and np.array_equal(ref.sum(0), p.astype(F64).sum(0))
    assert np.abs(ref).max() < 2 ** 24
    if nparts > group:
        assert BC.mismatches(BC.fold_ref(p, group, "group_off_by_one"), ref) > 0
    else:
        assert BC.cdiv(nparts, group) == 1              # one group holds every row: a longer group reads nothing more


@pytest.mark.parametrize("name", list(BC.POOL_CASES))
def test_pool_references_agree_with_torch_and_the_checker_flags_every_fault(name):
    c = BC.POOL_CASES[name]
    o = BC.pool_operands(c)
    y, sc, sh = o["y"], o["scale"], o["shift"]
    assert np.array_equal(y * 2, np.round(y * 2)) and np.abs(y).max() <= 2 and (sc == 0).sum() == 1
    out, idx, ymax = BC.pool_fwd_ref(y, sc, sh)
    eo, ei, ey, cand = BC.pool_fwd_emulate(y, sc, sh)
    assert BC.mismatches(eo, out) == 0 and np.array_equal(ei, idx) and BC.mismatches(ey, ymax) == 0
    # all-nonpositive windows: out 0 at the first in-bounds position
    first = np.isfinite(cand).argmax(3)
    assert np.array_equal(idx[out == 0], first[out == 0])
    # backward against autograd in float64 (statistics passed in, as the kernels take them)
    yt = torch.from_numpy(y.astype(F64)).permute(0, 3, 1, 2).requires_grad_(True)
    t = yt * torch.from_numpy(sc.astype(F64)).view(1, -1, 1, 1) + torch.from_numpy(sh.astype(F64)).view(1, -1, 1, 1)
    pooled = F.max_pool2d(F.relu(t), 3, 2, 1)
    dp = o["dp0"] * (out > 0)
    (pooled * torch.from_numpy(dp.astype(F64)).permute(0, 3, 1, 2)).sum().backward()
    dy, tot, dz = BC.pool_bwd_ref(o, dp, idx)
    assert np.abs(dy * sc.astype(F64) - yt.grad.permute(0, 2, 3, 1).numpy()).max() <= 1e-12
    assert BC.mismatches(dz.astype(np.float32), dz) == 0 and BC.mismatches(tot.astype(np.float32), tot) == 0
    dy1 = BC.pool_dy1_ref(dp, idx, y, o["abc"])
    assert BC.mismatches(dy1.astype(np.float32), dy1) == 0
    flagged = {}
    for fault in ("last_max", "ge", "pad_zero"):
        fo, fi, fy, _ = BC.pool_fwd_emulate(y, sc, sh, fault)
        flagged[fault] = int((fi != idx).sum()) + BC.mismatches(fy, ymax)
        assert BC.mismatches(fo, out) == 0 or fault == "pad_zero"       # the pooled VALUES do not see a wrong tie-break
    print(name, flagged)
    assert flagged["pad_zero"] > 0                      # every map has a border, and every case a channel that is never positive
    if c.H1 * c.W1 >= 5:                                # (a window of one pixel has no tie to break)
        assert flagged["last_max"] > 0 and flagged["ge"] > 0, flagged
    if name in BC.TIE_CASES:
        tied, dead = BC.tie_density(y, sc, sh)
        print("%s: %.1f %% of windows with a tied positive maximum, %.1f %% with no positive value"
              % (name, 100 * tied, 100 * dead))
        assert tied >= 0.10 and dead >= 0.10


def test_the_threshold_probe_separates_the_two_relu_decisions():
    o = BC.probe_operands()
    c = BC.PROBE_MAP
    out, idx, ymax = BC.pool_fwd_ref(o["y"], o["scale"], o["shift"])
    kinds = set()
    for ch, (iy, ix) in enumerate(o["pixels"]):
        wins = BC.windows_of(c, iy, ix)
        kinds.add((iy in (0, c.H1 - 1)) + (ix in (0, c.W1 - 1)))
        assert o["dp"][0, :, :, ch].sum() == 1 and o["dp"][0, wins[0][0], wins[0][1], ch] == 1
        for oy, ox in wins:
            if ch % 2 == 0:
                assert out[0, oy, ox, ch] == np.float32(2.0 ** -24) and ymax[0, oy, ox, ch] == BC.PROBE_Y
                assert idx[0, oy, ox, ch] == (iy - 2 * oy + 1) * 3 + (ix - 2 * ox + 1)
        assert (out[0, :, :, ch] > 0).sum() == (len(wins) if ch % 2 == 0 else 0)
    assert kinds == {0, 1, 2} and {len(BC.windows_of(c, *p)) for p in BC.PROBE_PIXELS} == {1, 2, 4}
    dy, tot, dz = BC.pool_bwd_ref(o, o["dp"], idx)
    assert np.array_equal(tot[0], np.arange(64) % 2 == 0) and not tot[1].any()
    for ch, (iy, ix) in enumerate(o["pixels"]):
        want = np.float32(np.float64(o["scale"][ch]) * ((ch % 2 == 0) - 0.125))
        assert np.float32(dz[0, iy, ix, ch]) == want
    # the unfused decision: the forward is 0 everywhere and the gradient of every probed window is dropped
    fo, fi, fy, _ = BC.pool_fwd_emulate(o["y"], o["scale"], o["shift"], "unfused")
    assert not fo.any() and BC.mismatches(fo, out) == int((out > 0).sum()) >= 32
    bdy, btot, bdz = BC.pool_bwd_ref(o, o["dp"], idx, fused=False)
    assert BC.mismatches(btot, tot) == 32 and BC.mismatches(bdz, dz) == 32


@pytest.mark.parametrize("name", ["bn1d-R2-C8-pad0", "bn1d-R1537-C36-pad4", "bn1d-R1537-C6-unaligned", "bn1d-R4097-C8-pad0"])
def test_bn1d_operands_have_integer_means_and_exact_sums(name):
    c = BC.BN1D_CASES[name]
    o = BC.bn1d_operands(c)
    x = o["x"].astype(F64)
    assert np.array_equal(x.sum(0), c.R * o["col_mean"].astype(F64)) and np.abs(x).max() <= 7
    fin = BC.bn1d_fwd_ref(o, c.R)
    assert np.array_equal(fin["mean"], o["col_mean"])
    ref = F.batch_norm(torch.from_numpy(x), None, None, torch.from_numpy(o["gamma"].astype(F64)),
                       torch.from_numpy(o["beta"].astype(F64)), True, 0.1, BC.EPS).numpy()
    f64 = BC.finalize_fwd_ref(np.stack([x.sum(0), (x * x).sum(0)]), float(c.R), o["gamma"], o["beta"], o["rm"], o["rv"], dt=F64)
    assert np.abs(f64["scale"] * x + f64["shift"] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    out, dropped = BC.bn1d_apply_ref(o["x"], fin["scale"], fin["shift"], 1, o["keep"])
    assert np.abs(out - np.maximum(ref, 0)).max() <= 1e-5 * np.abs(ref).max()
    assert np.array_equal(dropped, np.where(o["keep"] != 0, 2 * out, 0))
    for relu, drop in BC.BN1D_MODES:
        b = BC.bn1d_bwd_ref(o, c.R, relu, drop)
        assert BC.mismatches(b["dgamma"].astype(F64) * 4, np.round(b["dgamma"].astype(F64) * 4)) == 0
        # the same formula as bwd_apply_ref (held to autograd above), with coef = the f32 quotients of the exact sums
        bo = dict(o, coef=np.stack([b["dbeta"].astype(F64) / c.R, b["dgamma"].astype(F64) / c.R]).astype(np.float32))
        if drop:
            bo["dout"] = o["dout"] * o["keep"] * 2
        assert np.array_equal(BC.bwd_apply_ref(bo, relu)[0], b["dz"]) and (b["dz_mag"] >= np.abs(b["dz"])).all()
