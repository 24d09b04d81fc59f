"""Checks on the case table of tests/head_cases.py itself (no GPU): every kernel variant of csrc/head.hip and of the
BatchNorm row kernels of csrc/bn.hip is selected by at least one case, the float64 references agree with torch autograd,
the views that are meant to lose 16-byte alignment do, and the f32 sum bound is tight enough to see one missing row."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
import head_cases as HC  # noqa: E402


def test_every_kernel_variant_is_selected_by_a_case():
    hit = set()
    for c in HC.LINEAR_CASES:
        fwd, bwd = HC.linear_variants(c)
        hit.add("linear_small_fwd " + fwd)
        if bwd is not None:
            hit.add("linear_small_bwd %s KN=%d" % bwd)
    for c in HC.COLSUM_CASES:
        hit.add("colsum " + HC.colsum_variant(c))
    for shape, layout in HC.BN_CASES:
        for entry, v in HC.bn_variants(shape, layout).items():
            hit.add("%s %s%s" % (entry, v, " C=64" if shape[1] == 64 and entry in ("colstats", "bn_bwd_reduce") else ""))
    want = {"linear_small_fwd V1", "linear_small_fwd V4",
            "linear_small_bwd V4 KN=4", "linear_small_bwd V4 KN=16", "linear_small_bwd V1 KN=4", "linear_small_bwd V1 KN=16",
            "colsum V1", "colsum V4",
            "bn_act_fwd V1", "bn_act_fwd V4", "bn_bwd_apply V1", "bn_bwd_apply V4",
            "colstats reduce64 C=64", "colstats generic C=64", "colstats generic",
            "bn_bwd_reduce reduce64 C=64", "bn_bwd_reduce generic C=64", "bn_bwd_reduce generic"}
    assert want <= hit, sorted(want - hit)


def test_each_backward_variant_sees_its_extremes():
    """per (V, KN): N = 1 and N = 1030, a partial last 64-column block, NC at both ends of the variant's range, and row
    counts on both sides of its row batch (RSTEP * U = 512 / 128 / 128 / 32)"""
    by = {}
    for c in HC.LINEAR_CASES:
        bwd = HC.linear_variants(c)[1]
        if bwd is not None:
            by.setdefault(bwd, []).append(c)
    batch = {("V4", 4): 512, ("V4", 16): 128, ("V1", 4): 128, ("V1", 16): 32}
    for v, rows in batch.items():
        cs = by[v]
        assert {1, 1030} <= {c.N for c in cs}, v
        assert any(c.Cin % 64 for c in cs), v
        assert ({1, 4} if v[1] == 4 else {5, 16}) <= {c.NC for c in cs}, v
        assert any(c.N <= rows for c in cs) and any(rows < c.N <= 2 * rows for c in cs) and any(c.N > 2 * rows for c in cs), v


def test_case_groups_hold_the_listed_values():
    L = HC.LINEAR_CASES
    assert {c.N for c in L} == {1, 3, 63, 129, 513, 1030}
    assert {c.NC for c in L} == {1, 3, 4, 5, 7, 16}
    v4 = [c for c in L if HC.linear_variants(c)[0] == "V4"]
    assert {c.Cin for c in v4} == {4, 60, 64, 68, 992}
    assert {c.Cin for c in L if c.Cin % 4} == {1, 5, 63, 65, 331}
    assert sum(1 for c in v4 if c.ldx_pad == 8) >= 2 and all(c.ldx_pad in (0, 8) for c in v4)
    lay = [c for c in L if c.Cin == 64 and HC.linear_variants(c)[0] == "V1"]
    assert any(c.ldx_pad == 2 for c in lay) and any(c.x_off == 1 for c in lay) and any(c.w_off == 1 for c in lay)
    for c in lay:                                           # one cause at a time
        assert sorted([c.ldx_pad != 0, c.x_off != 0, c.w_off != 0]) == [False, False, True], c
    assert 35 <= len(L) <= 45 and len(set(L)) == len(L)
    assert max(c.N * (c.Cin + c.ldx_pad) for c in L) == 1030 * 992
    S = HC.COLSUM_CASES
    assert {c.R for c in S} == {1, 15, 17, 65, 1030} and {c.C for c in S} == {1, 5, 64, 68, 992}
    assert {0, 4, 1} <= {c.ldx_pad for c in S} and sum(1 for c in S if c.x_off == 1) == 1
    # scalar kernel on buffers where forcing the vector kernel would stay inside the allocation
    assert any(HC.colsum_variant(c) == "V1" and (c.C + c.ldx_pad) % 4 == 0 and c.x_off == 0 and c.R > 16 for c in S)
    assert set(HC.CE_CASES) == {(n, k) for n in (1, 1023, 1025, 2500) for k in (1, 2, 5, 16)}
    assert set(HC.DROPOUT_CASES) == {(r, c, p) for (r, c) in ((1, 1), (7, 5), (311, 64)) for p in (0.0, 0.2)}
    assert set(HC.BN_SHAPES) == {(300, 64, 1, 1), (77, 32, 1, 0), (129, 992, 1, 0), (50, 6, 0, 0), (130, 64, 1, 1)}
    assert list(HC.BN_LAYOUTS) == ["ld=C", "ld=C+4", "ld=C+1", "z+1"]
    assert len(HC.BN_CASES) == len(HC.BN_SHAPES) * len(HC.BN_LAYOUTS)


def test_an_offset_z_takes_every_bn_kernel_off_the_vector_path():
    for shape in HC.BN_SHAPES:
        for layout in ("ld=C+1", "z+1"):
            v = HC.bn_variants(shape, layout)
            assert v == {"colstats": "generic", "bn_act_fwd": "V1", "bn_bwd_reduce": "generic", "bn_bwd_apply": "V1"}, \
                (shape, layout, v)
        if shape[1] % 4 == 0:
            for layout in ("ld=C", "ld=C+4"):
                v = HC.bn_variants(shape, layout)
                assert v["bn_act_fwd"] == "V4" and v["bn_bwd_apply"] == "V4", (shape, layout)
    assert HC.bn_variants((300, 64, 1, 1), "ld=C")["colstats"] == "reduce64"
    assert HC.bn_variants((300, 64, 1, 1), "ld=C+4")["colstats"] == "generic"
    assert HC.bn_variants((300, 64, 1, 1), "ld=C+4")["bn_bwd_reduce"] == "generic"


def test_variant_refuses_what_the_entry_point_refuses():
    with pytest.raises(ValueError):
        HC.variant("linear_small_bwd", Cin=64, ldx=64, x_off=0, NC=17)
    with pytest.raises(KeyError):
        HC.variant("no_such_entry")


def test_offset_views_lose_16_byte_alignment_and_the_others_keep_it():
    n = 0
    for c in HC.LINEAR_CASES:
        d = HC.linear_data(c)
        for t, ld, off in ((d["x"], c.Cin + c.ldx_pad, c.x_off), (d["W"], c.Cin, c.w_off)):
            flat, view = HC.place(t, ld, off, float("nan"))
            assert flat.data_ptr() % 16 == 0
            assert (view.data_ptr() % 16 != 0) == (off % 4 != 0) and view.data_ptr() % 4 == 0
            assert torch.equal(view[:, :t.shape[1]], t)
            n += off % 4 != 0
    for c in HC.COLSUM_CASES:
        flat, view = HC.place(HC.colsum_data(c), c.C + c.ldx_pad, c.x_off, float("nan"))
        assert (view.data_ptr() % 16 != 0) == (c.x_off % 4 != 0)
        n += c.x_off % 4 != 0
    for shape, layout in HC.BN_CASES:
        pad, zoff, off = HC.BN_LAYOUTS[layout]
        flat, view = HC.place(HC.bn_data(shape)["x"], shape[1] + pad, zoff, float("nan"))
        assert (view.data_ptr() % 16 != 0) == (zoff % 4 != 0)
        n += zoff % 4 != 0
    assert n >= 4 + 1 + len(HC.BN_SHAPES)


def test_place_and_untouched():
    flat, view = HC.place((3, 5, torch.float32), 7, 1, HC.CANARY)
    assert flat.numel() == 1 + 3 * 7 + 8 and view.shape == (3, 7) and HC.untouched(flat, view, 5)
    view[:, :5] = 1.0
    assert HC.untouched(flat, view, 5)
    for i in (0, 1 + 5, 1 + 7 + 6, 1 + 21, flat.numel() - 1):          # front, pad columns, the tail
        f2 = flat.clone()
        f2[i] = 0.0
        v2 = f2[1:22].view(3, 7)
        assert not HC.untouched(f2, v2, 5), i
    fin, vin = HC.place(torch.ones(3, 5), 7, 0, float("nan"))
    assert torch.isnan(vin[:, 5:]).all() and torch.isnan(fin[21:]).all() and not torch.isnan(vin[:, :5]).any()


# ------------------------------------------------------------------------------------------------ references
def _close64(a, b):
    scale = max(float(b.abs().max()), 1e-30)
    assert float((a - b).abs().max()) <= 1e-12 * scale


@pytest.mark.parametrize("c", [HC.LINEAR_CASES[3], HC.LINEAR_CASES[30]], ids=str)
def test_linear_references_agree_with_autograd(c):
    d = HC.linear_data(c)
    x, W, b = (d[k].double().requires_grad_(True) for k in ("x", "W", "b"))
    y = F.linear(x, W, b)
    (y * d["dy"].double()).sum().backward()
    _close64(HC.linear_fwd_ref(d["x"], d["W"], d["b"]), y.detach())
    ref, mag = HC.linear_bwd_ref(d["dy"], d["x"], d["W"])
    _close64(ref["dx"], x.grad), _close64(ref["dW"], W.grad), _close64(ref["db"], b.grad)
    for k in ref:                                       # the magnitudes dominate the sums they bound
        assert bool((mag[k] >= ref[k].abs() * (1 - 1e-12)).all())
    assert bool((HC.linear_fwd_mag(d["x"], d["W"], d["b"]) >= y.detach().abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("c", [HC.COLSUM_CASES[2], HC.COLSUM_CASES[13]], ids=str)
def test_colsum_reference_agrees_with_autograd(c):
    x = HC.colsum_data(c)
    w = torch.arange(1.0, c.C + 1, dtype=torch.float64)
    xd = x.double().requires_grad_(True)
    s = xd.sum(0)
    (s * w).sum().backward()
    ref, mag = HC.colsum_ref(x)
    _close64(ref, s.detach())
    assert torch.equal(xd.grad, w.expand(c.R, c.C))     # every row enters every column sum once
    assert bool((mag >= ref.abs()).all())


@pytest.mark.parametrize("N,NC", [(1025, 5), (1, 1), (2500, 16)])
def test_ce_reference_agrees_with_autograd(N, NC):
    logits, labels = HC.ce_data(N, NC)
    for gscale in (1.0, 1.0 / N):
        l = logits.double().requires_grad_(True)
        loss = F.cross_entropy(l, labels, reduction="sum")
        (loss * gscale).backward()
        ref_loss, ref_dl = HC.ce_ref(logits, labels, gscale)
        assert abs(float(ref_loss) - loss.item()) <= 1e-12 * max(abs(loss.item()), 1e-30)
        assert float((ref_dl - l.grad).abs().max()) <= 1e-14


@pytest.mark.parametrize("R,C,p", [(7, 5, 0.2), (311, 64, 0.0)])
def test_dropout_reference_agrees_with_autograd(R, C, p):
    d = HC.dropout_data(R, C)
    x = d["x"].double().requires_grad_(True)
    y = x * d["keep"].double() / (1.0 - p)
    (y * d["g"].double()).sum().backward()
    _close64(HC.dropout_ref(d["x"], d["keep"], p), y.detach())
    _close64(HC.dropout_ref(d["g"], d["keep"], p), x.grad)          # the backward is the same map of the gradient


@pytest.mark.parametrize("shape", [(300, 64, 1, 1), (50, 6, 0, 0)])
def test_bn_reference_agrees_with_the_closed_form(shape):
    """bn_ref is torch autograd through F.batch_norm; held against the textbook formulas written out in float64"""
    R, C, relu, res = shape
    d = HC.bn_data(shape)
    ref = HC.bn_ref(d, relu)
    x, gamma, beta, dout = (d[k].double() for k in ("x", "gamma", "beta", "dout"))
    mean, var = x.mean(0), x.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    xh = (x - mean) * invstd
    y = xh * gamma + beta
    if res:
        y = y + d["resid"].double()
    dy = dout
    if relu:
        dy = dout * (y > 0)
        y = y.clamp(min=0)
    _close64(ref["out"], y)
    _close64(ref["running_mean"], 0.9 * d["rm"].double() + 0.1 * mean)
    _close64(ref["running_var"], 0.9 * d["rv"].double() + 0.1 * x.var(0, unbiased=True))
    dbeta, dgamma = dy.sum(0), (dy * xh).sum(0)
    _close64(ref["dbeta"], dbeta), _close64(ref["dgamma"], dgamma)
    _close64(ref["dz"], gamma * invstd * (dy - dbeta / R - xh * dgamma / R))
    _close64(ref["dres"], dy)


# ------------------------------------------------------------------------------------------------ the bound
def test_f32_rounding_of_the_reference_is_inside_the_bound_and_a_missing_row_is_not():
    """The bound is the worst case of an f32 sum, so the correctly rounded reference passes it; a weight gradient, a bias
    gradient or a column sum that drops ONE of its N rows does not (checked on two cases each, the largest N included)."""
    for c in (HC.LINEAR_CASES[5], HC.LINEAR_CASES[23]):               # N = 1030 <V4, 4>; N = 129 <V1, 4>
        d = HC.linear_data(c)
        ref, mag = HC.linear_bwd_ref(d["dy"], d["x"], d["W"])
        for k, L in (("dx", c.NC), ("dW", c.N), ("db", c.N)):
            assert HC.violations(ref[k].float(), ref[k], mag[k], L)[0] == 0
        row = c.N // 2
        keep = torch.arange(c.N) != row
        short, _ = HC.linear_bwd_ref(d["dy"][keep], d["x"][keep], d["W"])
        bad_w, worst_w = HC.violations(short["dW"].float(), ref["dW"], mag["dW"], c.N)
        bad_b, worst_b = HC.violations(short["db"].float(), ref["db"], mag["db"], c.N)
        assert bad_w > 0.5 * c.NC * c.Cin and bad_b > 0, (c, bad_w, worst_w, bad_b, worst_b)
        # a dropped class in the input gradient, a dropped column in the forward
        if c.NC > 1:
            short_dx = d["dy"].double()[:, 1:] @ d["W"].double()[1:]
            assert HC.violations(short_dx.float(), ref["dx"], mag["dx"], c.NC)[0] > 0.5 * c.N * c.Cin
        y, ymag = HC.linear_fwd_ref(d["x"], d["W"], d["b"]), HC.linear_fwd_mag(d["x"], d["W"], d["b"])
        assert HC.violations(y.float(), y, ymag, c.Cin)[0] == 0
        short_y = HC.linear_fwd_ref(d["x"][:, :-1], d["W"][:, :-1], d["b"])
        assert HC.violations(short_y.float(), y, ymag, c.Cin)[0] > 0
    for c in (HC.COLSUM_CASES[13], HC.COLSUM_CASES[9]):                # 1030 x 992; 17 x 68
        x = HC.colsum_data(c)
        ref, mag = HC.colsum_ref(x)
        assert HC.violations(ref.float(), ref, mag, c.R)[0] == 0
        short, _ = HC.colsum_ref(x[1:])
        assert HC.violations(short.float(), ref, mag, c.R)[0] > 0.5 * c.C
        twice, _ = HC.colsum_ref(torch.cat((x, x[-1:])))
        assert HC.violations(twice.float(), ref, mag, c.R)[0] > 0.5 * c.C
    assert HC.violations(torch.tensor([float("nan")]), torch.zeros(1, dtype=torch.float64), torch.ones(1,
                         dtype=torch.float64), 4)[0] == 1
