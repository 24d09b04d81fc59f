"""The bf16-split products (csrc/bf3.h: three round-to-nearest bf16 pieces per f32 operand, six piece products accumulated in
f32) held to f32 on the MI355X:

* EXACT probes (tests/split_probe.py): operands for which the exact result is an f32 number and every operand piece is visible
  in it -- lattice values with a 2^24 spread of per-channel scales against power-of-two selections (x pieces, w pieces), and
  (a + 1/4)-values against each other (the second-order product x1 w1).  The assertion is bit equality; a failure names the
  row tile, the 8-channel K slot and the size of the piece product that is off.  tests/test_split_products_cpu.py shows on
  a CPU emulation that every single-term deletion and every mis-staged slot fails these checkers.
* error-class gates of the 1x1 family against fp64, with the sequential f32 chain of the same operands (computed here, on the
  CPU) as the yardstick, and the signed bias of the output over a map.

A statistical gate cannot hold the split for one-sign operands and long reductions -- the dropped terms average out of a
max-relative metric (CPU emulation, vprod at R = 60001 with ReLU-like operands: without x1 w1 P moves by 8e-8, without x2 w0
by 7e-8, the f32 GEMM's own error being 2e-7) -- which are the operand statistics the train step has.  The probes carry
that case.
The probes set every prologue and epilogue to the identity and run one tile per wave; the per-element gate with every
constant present, on every launch path and multi-trip walk, lives in tests/test_c11_paths_gpu.py (tests/c11_cases.py)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import split_probe as sp  # noqa: E402
from cova_web_object_detection_amd import engine  # noqa: E402
from cova_web_object_detection_amd._lib import call, query  # noqa: E402
from helpers import DEV  # noqa: E402

SHAPES = [(64, 64), (64, 256), (256, 64)]
R_PROBE = 256 + 13      # nine 32-row tiles: even and odd ones (odd tiles run with negated activations), a ragged last one


def d(t):
    return t.to(DEV)


def gen(*key):
    return torch.Generator().manual_seed(77 + sum((3 * i + 1) * int(k) for i, k in enumerate(key)))


def conv1x1(x, w, w_trans, **kw):
    """engine.conv1x1 on host operands; w [cout, cin] is handed over as it is or -- w_trans -- as its transpose"""
    R, cin, cout = x.shape[0], x.shape[1], w.shape[0]
    out = torch.full((R, cout), 7.0, device=DEV)
    engine.conv1x1(d(x), kw.pop("in2", None), kw.pop("abc", None), kw.pop("relu", 0),
                   d(w.t().contiguous() if w_trans else w), w_trans, out, kw.pop("part", None), R, cin, cout, **kw)
    return out


def launches(name, cin):
    """the selections t of a probe: A needs cin / 64 launches to select every input channel once; B / C select channel
    (row + t) mod cin, every K position within one launch -- a second t pairs the rows of a tile with other channels"""
    return range(cin // 64) if name == "A" else (0, 37)


# ------------------------------------------------------------------------------------ cova_conv1x1
@pytest.mark.parametrize("w_trans", [0, 1])
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_conv1x1_exact_probes(cin, cout, w_trans):
    """Probe A (x pieces), B (w pieces), C (x1 w1) on the plain product, forward and data-gradient weight layout; R = 269 and 1."""
    for R in (R_PROBE, 1):
        for n, name in enumerate("ABC"):
            for t in launches(name, cin):
                x, w, ref, k_of = sp.PROBES[name](R, cin, cout, t, gen(cin, cout, n, t, R))
                sp.check_exact(conv1x1(x, w, w_trans), ref,
                               "conv1x1 %d->%d w_trans %d R %d probe %s t %d" % (cin, cout, w_trans, R, name, t), k_of=k_of)


@pytest.mark.parametrize("cin,cout", SHAPES)
def test_conv1x1_exact_probe_through_prologues_and_epilogues(cin, cout):
    """Probe A through every prologue / epilogue variant the dispatch can launch on the bf16 path, each set to the identity:
    f(A in + C) with A = 1, C = 0 and the ReLU on a non-negative lattice; A in + B in2 + C with B = 0; statistics on (the
    output is checked); for 64 -> 256 the masked data gradient (acc + addend) * mask with addend = 0 and a pass-all mask,
    from a map and from bits."""
    R = R_PROBE
    ident = torch.stack([torch.ones(cin), torch.zeros(cin), torch.zeros(cin)])
    nparts = query("cova_conv1x1_num_partials", R, cin, cout)
    for t in launches("A", cin):
        x, w, ref, k_of = sp.probe_a(R, cin, cout, t, gen(cin, cout, t, 5), nonneg=True)
        xs, ws, refs, _ = sp.probe_a(R, cin, cout, t, gen(cin, cout, t, 6))               # signed
        what = "conv1x1 %d->%d t %d " % (cin, cout, t)
        sp.check_exact(conv1x1(x, w, 0, abc=d(ident), relu=1), ref, what + "pro 1 + relu", k_of=k_of)
        sp.check_exact(conv1x1(xs, ws, 0, abc=d(ident)), refs, what + "pro 1", k_of=k_of)
        zeros = torch.zeros((R, cin), device=DEV)
        sp.check_exact(conv1x1(xs, ws, 0, in2=zeros, abc=d(ident)), refs, what + "pro 2", k_of=k_of)
        for pro in (0, 1, 2):
            part = torch.empty((nparts, 2, cout), device=DEV)
            got = conv1x1(xs, ws, 0, in2=zeros if pro == 2 else None, abc=d(ident) if pro else None, part=part)
            sp.check_exact(got, refs, what + "statistics, pro %d" % pro, k_of=k_of)
        if cout == 256:
            addend = torch.zeros((R, cout), device=DEV)
            ones = torch.ones((R, cout), device=DEV)
            bits = torch.full((R, cout // 32), -1, dtype=torch.int32, device=DEV)
            for wt in (0, 1):
                sp.check_exact(conv1x1(xs, ws, wt, in2=zeros, abc=d(ident), addend=addend, act=ones), refs,
                               what + "masked gradient, mask map, w_trans %d" % wt, k_of=k_of)
                sp.check_exact(conv1x1(xs, ws, wt, in2=zeros, abc=d(ident), addend=addend, act_bits=bits), refs,
                               what + "masked gradient, mask bits, w_trans %d" % wt, k_of=k_of)
                sp.check_exact(conv1x1(xs, ws, wt, in2=zeros, abc=d(ident), act=ones), refs,
                               what + "masked gradient without addend, w_trans %d" % wt, k_of=k_of)


def test_conv1x1_materialize_exact_probe():
    """cova_conv1x1_materialize (256 -> 64 on relu(A in + B in2 + C), which it also writes): probe A with in2 = 0, A = 1,
    B = C = 0 on a non-negative lattice -- the side output is the input and the product is exact."""
    R = R_PROBE
    ident = d(torch.stack([torch.ones(256), torch.zeros(256), torch.zeros(256)]))
    nparts = query("cova_conv1x1_num_partials", R, 256, 64)
    for t in range(4):
        x, w, ref, k_of = sp.probe_a(R, 256, 64, t, gen(t, 9), nonneg=True)
        for stats in (False, True):
            side, out = torch.full((R, 256), 9.0, device=DEV), torch.full((R, 64), 7.0, device=DEV)
            part = torch.empty((nparts, 2, 64), device=DEV) if stats else None
            bits = torch.zeros((R, 8), dtype=torch.int32, device=DEV) if stats else None
            call("cova_conv1x1_materialize", d(x), torch.zeros((R, 256), device=DEV), ident, d(w), side, bits, out, part, R)
            assert torch.equal(side.cpu(), x), "materialised input, t %d" % t
            sp.check_exact(out, ref, "materialize t %d stats %d" % (t, stats), k_of=k_of)


# ------------------------------------------------------------------------------------ cova_conv1x1_lin_dgrad
@pytest.mark.parametrize("add", [False, True])
def test_conv1x1_lin_dgrad_exact_probes(add):
    """The 256 + 64 K channel kernel of the linear form: out = (avec . v) W + a M + cvec with avec = (1, 0, 0), cvec = 0 and
    a pass-all mask (mask_scale = 0, mask_shift = 1).  (i) W selects, M = 0: the 256 main channels; (ii) W = 0, M selects:
    the 64 extra K channels (the ci >= CIN staging path).  The operand of the silent side is a lattice too: its products
    with zero must add nothing."""
    R = R_PROBE
    avec = d(torch.stack([torch.ones(256), torch.zeros(256), torch.zeros(256)]))
    ident = d(torch.stack([torch.ones(64), torch.zeros(64), torch.zeros(64)]))
    z64, o64 = torch.zeros(64, device=DEV), torch.ones(64, device=DEV)
    zmap = torch.zeros((R, 64), device=DEV)
    addend = torch.zeros((R, 64), device=DEV) if add else None
    n = query("cova_conv1x1_lin_dgrad_num_partials", R)

    def run(v, w_sel, act, m_sel):                          # w_sel [64, 256] -> W [256, 64];  m_sel [64 co, 64 k] -> M [k, co]
        out, part = torch.full((R, 64), 7.0, device=DEV), torch.empty((n, 2, 64), device=DEV)
        call("cova_conv1x1_lin_dgrad", d(v), avec, d(w_sel.t().contiguous()), d(act), ident, 0, d(m_sel.t().contiguous()),
             z64, addend, z64, o64, zmap, z64, o64, out, part, R)
        return out

    for t in range(4):                                      # (i)
        g = gen(t, 21, add)
        v, act = sp.lattice((R, 256), g), sp.lattice((R, 64), g)
        w_sel, sel = sp.select_weight(64, 256, t, g)
        ref, _ = sp.exact(v, w_sel)
        sp.check_exact(run(v, w_sel, act, torch.zeros(64, 64)), ref, "lin_dgrad main channels t %d" % t,
                       k_of=sel.view(1, 64).expand(R, 64))
    for shift in (0, 29):                                   # (ii)
        g = gen(shift, 22, add)
        v, act = sp.lattice((R, 256), g), sp.lattice((R, 64), g)
        m_sel, sel = sp.select_weight(64, 64, 0, g, shift)
        ref, _ = sp.exact(act, m_sel)
        sp.check_exact(run(v, torch.zeros(64, 256), act, m_sel), ref, "lin_dgrad extra channels shift %d" % shift,
                       k_of=256 + sel.view(1, 64).expand(R, 64))
    g = gen(23, add)                                        # the second-order product on both operand tensors
    w_q = torch.zeros(64, 256)
    w_q[torch.arange(64), torch.arange(64) + 128] = sp.quarter((64, 1), g, -6, 6).view(64)
    v = sp.quarter((R, 256), g)
    ref, _ = sp.exact(v, w_q)
    sp.check_exact(run(v, w_q, torch.zeros(R, 64), torch.zeros(64, 64)), ref, "lin_dgrad main channels, x1 w1")
    m_q = torch.zeros(64, 64)
    m_q[torch.arange(64), (torch.arange(64) + 5) % 64] = sp.quarter((64, 1), g, -6, 6).view(64)
    act = sp.quarter((R, 64), g)
    ref, _ = sp.exact(act, m_q)
    sp.check_exact(run(torch.zeros(R, 256), torch.zeros(64, 256), act, m_q), ref, "lin_dgrad extra channels, x1 w1")


# ------------------------------------------------------------------------------------ cova_conv1x1_vprod
def vprod(v, act):
    R = v.shape[0]
    lin = torch.empty(query("cova_conv1x1_lin_floats"), device=DEV)
    ws = torch.empty(query("cova_conv1x1_vprod_workspace_floats", R), device=DEV)
    call("cova_conv1x1_vprod", d(v), d(act), None, 0, lin, ws, R)
    return lin[:16384].view(256, 64), lin[16384:20480].view(64, 64)


@pytest.mark.parametrize("R", [64, 16 * 37 + 5, 4096 + 7])
def test_conv1x1_vprod_exact_probes(R):
    """P = v^T a and G = a^T a (K = the pixel rows) with all rows zero except one window of 64: the first rows, a window across
    a block boundary, one inside an odd block (odd blocks run with the negated a) and the last 64 rows, ragged (the blocks of
    these R take 128 rows each).  P: a selects (v pieces), v selects (a pieces), quarter against quarter (the second-order
    product).  G: row r0 + i holds a lattice value at channel i and 2^k at channel i + 1 -- G[i][i+1] and its mirror are
    exact; the diagonal and the sums are not representable and not asserted."""
    i64 = torch.arange(64)
    for r0 in ([0] if R == 64 else [0, 96, 160, R - 64]):
        rows = r0 + i64
        g = gen(R, r0)
        what = "vprod R %d window %d: " % (R, r0)
        # a[r0 + i, i] = 2^k(i), v = lattice: P[cv][ca] = v[r0 + ca, cv] 2^k(ca)
        a, v = torch.zeros(R, 64), torch.zeros(R, 256)
        a[rows, i64] = sp.pow2((64,), g)
        v[rows] = sp.lattice((64, 256), g)
        P, _ = vprod(v, a)
        sp.check_exact(P, v.double().t() @ a.double(), what + "P, pieces of v", k_of=rows.view(1, 64).expand(256, 64), tile=64)
        # the roles exchanged: v[r0 + i, c] = 2^k(i) for c = i mod 64, a = lattice: P[cv][ca] = a[r0 + cv mod 64, ca] 2^k
        a, v = torch.zeros(R, 64), torch.zeros(R, 256)
        a[rows] = sp.lattice((64, 64), g)
        v[rows.repeat(4), torch.arange(256)] = sp.pow2((64,), g).repeat(4)
        P, _ = vprod(v, a)
        sp.check_exact(P, v.double().t() @ a.double(), what + "P, pieces of a",
                       k_of=rows.repeat(4).view(256, 1).expand(256, 64), tile=64)
        # quarter against quarter
        a, v = torch.zeros(R, 64), torch.zeros(R, 256)
        a[rows, i64] = sp.quarter((64, 1), g, -6, 6).view(64)
        v[rows] = sp.quarter((64, 256), g)
        P, _ = vprod(v, a)
        sp.check_exact(P, v.double().t() @ a.double(), what + "P, x1 w1", k_of=rows.view(1, 64).expand(256, 64), tile=64)
        # the Gram matrix
        a = torch.zeros(R, 64)
        a[rows, i64] = sp.lattice((64, 64), g)[i64, i64]
        a[rows, (i64 + 1) % 64] = sp.pow2((64,), g)
        _, G = vprod(torch.zeros(R, 256), a)
        probed = torch.zeros(64, 64, dtype=torch.bool)
        probed[i64, (i64 + 1) % 64] = True
        probed[(i64 + 1) % 64, i64] = True
        k_of = torch.zeros(64, 64, dtype=torch.long)
        k_of[i64, (i64 + 1) % 64] = rows
        k_of[(i64 + 1) % 64, i64] = rows
        sp.check_exact(G, a.double().t() @ a.double(), what + "G", probed=probed, k_of=k_of, tile=64)


# ------------------------------------------------------------------------------------ conv1 (7x7, stride 2)
def _nchw(x):
    return x.cpu().permute(0, 3, 1, 2).contiguous()


def _conv1_fwd(img, w, B, H, W):
    H1, W1 = (H + 1) // 2, (W + 1) // 2
    out = torch.full((B, H1, W1, 64), 7.0, device=DEV)
    part = torch.zeros(query("cova_conv1_num_partials", B, H, W), 2, 64, device=DEV)
    call("cova_conv1_fwd_tail", d(img), d(w), out, part, B, H, W, None)
    return _nchw(out)


def _conv1_wgrad(img, dy_nhwc, B, H, W):
    ws = torch.empty(query("cova_conv1_wgrad_workspace_floats", B, H, W), device=DEV)
    dw = torch.full((64, 3, 7, 7), 7.0, device=DEV)
    call("cova_conv1_wgrad", d(img), d(dy_nhwc), dw, ws, B, H, W)
    return dw


def _wgrad_exact(img, dy_nhwc):
    return torch.nn.grad.conv2d_weight(img.double(), (64, 3, 7, 7), dy_nhwc.permute(0, 3, 1, 2).double(), stride=2, padding=3)


def _image(fn, B, H, W, g):
    """NCHW image of probe values with a per-channel scale"""
    return fn((B, H, W, 3), g).permute(0, 3, 1, 2).contiguous()


def _one_pixel_per_channel(B, H1, W1, values, g):
    """dy NHWC with one non-zero pixel per output channel: corners, border and interior pixels among them"""
    dy = torch.zeros(B, H1, W1, 64)
    special = [(0, 0), (0, W1 - 1), (H1 - 1, 0), (H1 - 1, W1 - 1), (0, W1 // 2), (H1 - 1, 1), (H1 // 2, 0), (1, W1 - 1)]
    for co in range(64):
        y, x = special[co] if co < len(special) else (int(torch.randint(1, H1 - 1, (1,), generator=g)),
                                                      int(torch.randint(1, W1 - 1, (1,), generator=g)))
        dy[int(torch.randint(0, B, (1,), generator=g)), y, x, co] = values[co]
    return dy


@pytest.mark.parametrize("B,H,W", [(2, 37, 50), (1, 70, 90)])
def test_conv1_exact_probes(B, H, W):
    """cova_conv1_fwd_tail and cova_conv1_wgrad in the bf16-split form (option 7 = 0) and, as a control, on the f32 MFMA
    (option 7 = 1): both exact.  Forward: the image is a lattice with a per-channel scale, output channel co reads the one
    tap (co + 64 t) mod 147 with weight 2^j -- the output is the shifted, zero-padded image times 2^j.  Weight gradient:
    (i) dy has one non-zero pixel 2^j per output channel, image = lattice: dW is the image patch around it; (ii) the roles
    exchanged: one non-zero image pixel per input channel, dy = lattice; (iii) quarter values on both sides (x1 w1)."""
    H1, W1 = (H + 1) // 2, (W + 1) // 2
    try:
        for o7 in (0, 1):
            query("cova_set_option", 7, o7)
            what = "conv1 %dx%dx%d option 7 = %d: " % (B, H, W, o7)
            g = gen(B, H, W)
            img = _image(sp.lattice, B, H, W, g)
            for t in range(3):
                w = torch.zeros(64, 147)
                w[torch.arange(64), (torch.arange(64) + 64 * t) % 147] = sp.pow2((64,), g)
                w = w.view(64, 3, 7, 7)
                ref = F.conv2d(img.double(), w.double(), stride=2, padding=3)
                sp.check_exact(_conv1_fwd(img, w, B, H, W), ref, what + "forward, taps t %d" % t)
            dy = _one_pixel_per_channel(B, H1, W1, sp.pow2((64,), g), g)
            sp.check_exact(_conv1_wgrad(img, dy, B, H, W), _wgrad_exact(img, dy), what + "weight gradient, image pieces")
            one = torch.zeros(B, 3, H, W)
            one[0, 0, 2 * (H // 4) + 1, 2 * (W // 4) + 1] = 2.0 ** 3           # interior
            one[B - 1, 1, 0, 0] = 2.0 ** -4                                    # corner
            one[0, 2, H - 1, W // 2] = 2.0 ** 5                                # border
            dyl = sp.lattice((B, H1, W1, 64), g)
            sp.check_exact(_conv1_wgrad(one, dyl, B, H, W), _wgrad_exact(one, dyl), what + "weight gradient, dy pieces")
            imq = _image(sp.quarter, B, H, W, g)
            dyq = _one_pixel_per_channel(B, H1, W1, sp.quarter((1, 64), g, -6, 6).view(64), g)
            sp.check_exact(_conv1_wgrad(imq, dyq, B, H, W), _wgrad_exact(imq, dyq), what + "weight gradient, x1 w1")
            wq = torch.zeros(64, 147)
            wq[torch.arange(64), (torch.arange(64) + 30) % 147] = sp.quarter((1, 64), g, -6, 6).view(64)
            wq = wq.view(64, 3, 7, 7)
            sp.check_exact(_conv1_fwd(imq, wq, B, H, W), F.conv2d(imq.double(), wq.double(), stride=2, padding=3),
                           what + "forward, x1 w1")
    finally:
        query("cova_set_option", 7, 0)


# ------------------------------------------------------------------------------------ error class of the 1x1 family
@pytest.mark.parametrize("one_sign", [False, True])
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_conv1x1_error_class(cin, cout, one_sign):
    """Plain forward against fp64 at R = 2048 + 13; yardstick: the sequential FMA-free f32 chain of the same operands on the
    CPU; gate err <= 2 err(chain) + 2e-7 (the form of test_conv1_bf16_split_error_class).  For N(0,1) operands a two-piece /
    three-product emulation exceeds the gate -- the inputs can tell the classes apart, which is asserted.  For one-sign
    (ReLU-like) operands it cannot with a margin: the dropped terms average out of the max-relative metric; that case is held
    by the exact probes above."""
    R = 2048 + 13
    x, w = sp.operands(R, cin, cout, one_sign, 5 * cin + cout + one_sign)
    ref = x.double() @ w.double().t()
    gate = 2.0 * sp.max_err(sp.f32_chain(x, w), ref) + 2e-7
    two = sp.max_err(sp.emulate(sp.pieces(x), sp.pieces(w), ((1, 0), (0, 1), (0, 0))), ref)
    got = conv1x1(x, w, 0)
    err = sp.max_err(got, ref)
    print("conv1x1 %3d->%3d %s: error against fp64 %.2e   gate %.2e   two-piece emulation %.2e   bias %+.2e" % (
        cin, cout, "one-sign" if one_sign else "N(0,1)  ", err, gate, two, sp.bias(got, ref)))
    assert err <= gate, (err, gate)
    if not one_sign:
        assert two > gate, (two, gate)


@pytest.mark.parametrize("cin,cout", [(64, 256), (256, 64)])
def test_conv1x1_signed_bias_over_a_map(cin, cout):
    """One-sign operands, R = 8192 + 13 (257 row tiles): |mean(got - ref)| / mean |ref| < 1.5e-8, the bound of
    test_conv3x3_winograd_f4x4_split_error_class for the same mechanism -- the bf16 MFMA drops low product bits toward
    -infinity; odd row tiles run with negated activations.  Without the alternation the bias is about 7e-8."""
    R = 8192 + 13
    x, w = sp.operands(R, cin, cout, True, cin + 3 * cout)
    ref = x.double() @ w.double().t()
    b = sp.bias(conv1x1(x, w, 0), ref)
    print("conv1x1 %3d->%3d one-sign, R = %d: signed bias %+.2e" % (cin, cout, R, b))
    assert abs(b) < 1.5e-8, b


@pytest.mark.parametrize("one_sign", [False, True])
@pytest.mark.parametrize("R", [777, 60001])
def test_conv1x1_vprod_error_class(R, one_sign):
    """P = v^T a and G = a^T a against fp64; yardstick: torch's f32 matmul of the same operands on the CPU; gate
    err <= 2 err(f32 matmul) + 2e-7.  The signed biases are printed, not asserted (G's is a sum of squares: one sign by
    construction)."""
    g = torch.Generator().manual_seed(R + one_sign)
    a, v = torch.randn((R, 64), generator=g), torch.randn((R, 256), generator=g)
    if one_sign:
        a, v = (a + 0.5).clamp_min(0.0), (v + 0.5).clamp_min(0.0)
    P, G = vprod(v, a)
    refP, refG = v.double().t() @ a.double(), a.double().t() @ a.double()
    gateP = 2.0 * sp.max_err(v.t() @ a, refP) + 2e-7
    gateG = 2.0 * sp.max_err(a.t() @ a, refG) + 2e-7
    eP, eG = sp.max_err(P, refP), sp.max_err(G, refG)
    print("vprod R = %5d %s: P error %.2e (gate %.2e) bias %+.2e   G error %.2e (gate %.2e) bias %+.2e" % (
        R, "one-sign" if one_sign else "N(0,1)  ", eP, gateP, sp.bias(P, refP), eG, gateG, sp.bias(G, refG)))
    assert eP <= gateP, (eP, gateP)
    assert eG <= gateG, (eG, gateG)
