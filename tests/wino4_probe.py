"""Sparse probes of the F(4x4,3x3) bf16-split main loop (csrc/conv_wino4_split.h, prep_wino4s_element in csrc/conv_wino4.hip).
Host side only -- torch on the CPU, importable without a GPU; the pieces, the order of the piece products and the size hints
are those of tests/split_probe.py.

Why not bit equality, as for the 1x1 family: G holds 1/6, 1/12 and 1/24, so a transformed weight U = G g G^T is a power of two
at 4 of the 36 positions at most, and the output transform adds up to 36 rounded products -- a Winograd result is never
exact.  What these probes have instead is an error scale known BEFORE the kernel runs:

* weights: w[co][ci] != 0 only for ci = (co + t) mod 64 (a permutation: the data gradient is one-to-one too), each kernel a
  generic f32 draw N(0, 0.05) -- every U has 24 significant bits, three visible pieces;
* inputs: integers |m| < 2^17 times a per-channel power of two.  Every intermediate of B^T d B is an integer below
  100 * 2^17 < 2^24: V is an exact f32 number in any evaluation order (asserted), and its three pieces are populated;
* so one output = A^T (V (.) U) A holds ONE product per transform position, and its error is measured in units of
  2^-24 * scale, scale = |A^T| (|V| (.) |U|) |A| in float64 from the exact G:  q = |got - ref| / scale / 2^-24.
  ref is the true sparse convolution in float64 (a grouped convolution: the weights are a permutation).

Statistics of a launch: the worst q, and the largest RMS of q over the Winograd tiles of the map taken per output channel, per
in-tile coordinate (y mod 4, x mod 4) and per tile-row parity (even tile rows multiply with +U, odd ones with -U).

emulate() computes the complete split pipeline for the same operands (pieces of V and of float32(U), the six products in
TERMS order accumulated in f32, the output transform in f32 in the order of csrc/conv_wino4_epi.h) and takes fault hooks;
gates() measures its floor on every operand set the GPU test uses and derives the two gates from it."""
import functools
import itertools

import torch
import torch.nn.functional as F

from split_probe import TERMS, _hint, pieces

F64 = torch.float64
BT = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0],
                   [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], dtype=F64)
AT = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=F64)
_G_RATIONAL = [[(1, 4), (0, 1), (0, 1)], [(-1, 6), (-1, 6), (-1, 6)], [(-1, 6), (1, 6), (-1, 6)],
               [(1, 24), (1, 12), (1, 6)], [(1, 24), (-1, 12), (1, 6)], [(0, 1), (0, 1), (1, 1)]]
G = torch.tensor([[n / d for n, d in row] for row in _G_RATIONAL], dtype=F64)          # the rational G, to float64
# the constants as the prep kernel holds them (f32 quotients; it multiplies and sums in double and rounds U once)
G_F32 = torch.tensor([[float(torch.tensor(float(n)) / torch.tensor(float(d))) for n, d in row] for row in _G_RATIONAL], dtype=F64)
UNIT = 2.0 ** -24
HALF_ROWS = ((0, 1, 2), (5, 3, 4))          # transform rows of position half 0 / 1, in the order of the weight image

# (B, H, W, cova_set_option(2, .)): TH x TW = 8 x 32 pixels is one block tile of 16 Winograd tiles
SHAPE_ONE_ROW = (1, 8, 32, 0)               # one tile row: the +U image only
SHAPE_ALL_SHIFTS = (4, 16, 32, 0)           # both parities; the plain launches take all 64 shifts here
SHAPE_RAGGED = (2, 19, 45, 0)               # ragged edges, three tile rows
SHAPE_MULTI = (2, 24, 64, 2)                # several tiles per persistent block: tile-to-tile prefetch, the weight ring wraps
SHAPES = (SHAPE_ONE_ROW, SHAPE_ALL_SHIFTS, SHAPE_RAGGED, SHAPE_MULTI)
SHIFTS8 = tuple(range(0, 64, 9))            # every K-step, 8-channel group and element offset
FORMS = ("fwd", "dgrad", "pro", "pro_relu", "full", "bnact")


def shifts_of(form, shape):
    return tuple(range(64)) if form in ("fwd", "dgrad") and shape == SHAPE_ALL_SHIFTS else SHIFTS8


def launches():
    """every operand set of tests/test_wino4_probe_gpu.py: (form, shape, shift)"""
    for form in FORMS:
        for shape in SHAPES:
            for t in shifts_of(form, shape):
                yield form, shape, t


# ------------------------------------------------------------------------------------ operands
def _exp2(k):
    return torch.pow(torch.tensor(2.0, dtype=F64), k.double())


class Case:
    """One operand set and everything the host knows about it before a kernel runs.

    kernel operands: x [B, H, W, 64] f32 (NHWC), w [64, 64, 3, 3] f32 (OIHW, as cova_conv3x3_wino4_prep takes it), dgrad
    (which weight image), abc [3, 64] / relu (prologue forms), out_scale [64] (bnact), z / keep [B, H, W, 64] (full form: the
    ReLU mask is z > 0).  Tile form [B, 64, ny, nx, 4, 4] (Winograd tile (a, b) holds output rows 4a.., columns 4b..):
    ref, scale (float64), valid (inside the image and not masked)."""
    pass


def make_case(form, shape, t, seed=0):
    B, H, W, _ = shape
    gen = torch.Generator().manual_seed(40000 * (FORMS.index(form) + 1) + 1000 * SHAPES.index(shape) + 7 * t + 131071 * seed)
    c = Case()
    c.form, c.shape, c.shift, c.B, c.H, c.W = form, shape, t, B, H, W
    c.dgrad = form in ("dgrad", "full")
    # ---- weights: one generic 3x3 kernel per output channel, on input channel (co + t) mod 64
    i64 = torch.arange(64)
    w = torch.zeros(64, 64, 3, 3)
    w[i64, (i64 + t) % 64] = torch.randn(64, 3, 3, generator=gen) * 0.05
    c.w = w
    w_eff = w.flip(2, 3).transpose(0, 1).contiguous() if c.dgrad else w          # the correlation the launch computes
    nz = w_eff.abs().sum((2, 3)) != 0
    assert bool((nz.sum(1) == 1).all()) and bool((nz.sum(0) == 1).all())
    c.cin_of = nz.double().argmax(1)                                             # the one input channel behind each output channel
    c.ker = w_eff[i64, c.cin_of].double()                                        # [64, 3, 3]
    # ---- inputs
    k = torch.randint(-12, 13, (64,), generator=gen)
    c.abc, c.relu = None, 0
    if form in ("pro", "pro_relu"):          # fma(A, z, C) = (z + m) 2^a exactly, |z + m| < 2^17
        z = torch.randint(-(2 ** 16) + 1, 2 ** 16, (B, H, W, 64), generator=gen).double()
        m = torch.randint(-(2 ** 16) + 1, 2 ** 16, (64,), generator=gen).double()
        m[:8] = torch.tensor([5., -5., 60000., -60000., 1., -1., 33333., -33333.])      # relu(C) != 0 and == 0 among them
        A, C = _exp2(k), m * _exp2(k)
        c.x = z.float()
        c.abc = torch.stack([A, torch.zeros(64, dtype=F64), C]).float()
        c.relu = int(form == "pro_relu")
        d = A * z + C
        assert torch.equal(torch.addcmul(c.abc[2], c.abc[0], c.x).double(), d)       # f32 arithmetic gives it exactly
        if c.relu:
            d = d.clamp_min(0.0)
    else:
        d = torch.randint(-(2 ** 17) + 1, 2 ** 17, (B, H, W, 64), generator=gen).double() * _exp2(k)
        c.x = d.float()
        assert torch.equal(c.x.double(), d)
    d = d.permute(0, 3, 1, 2).contiguous()                                       # NCHW float64: the convolution's input
    # ---- transform-domain operands
    ny, nx = (H + 3) // 4, (W + 3) // 4
    c.ny, c.nx = ny, nx
    dp = F.pad(d, (1, 4 * nx + 1 - W, 1, 4 * ny + 1 - H))                        # zero padding: the image border and the ragged tiles
    patches = dp.unfold(2, 6, 4).unfold(3, 6, 4)                                 # [B, 64, ny, nx, 6, 6]
    V = torch.einsum("ia,bcyxae,je->bcyxij", BT, patches, BT)
    unit = _exp2(k).view(1, 64, 1, 1, 1, 1)
    assert torch.equal((V / unit).round(), V / unit)
    assert float((torch.einsum("ia,bcyxae,je->bcyxij", BT.abs(), patches.abs(), BT.abs()) / unit).max()) < 2.0 ** 24
    c.V32 = V.float()
    assert torch.equal(c.V32.double(), V)                                        # V is an f32 number in any evaluation order
    U = torch.einsum("ir,ort,jt->oij", G, c.ker, G)                              # exact G (float64)
    c.U32 = torch.einsum("ir,ort,jt->oij", G_F32, c.ker, G_F32).float()          # what the prep kernel splits
    c.scale = torch.einsum("yi,bopqij,xj->bopqyx", AT.abs(), V[:, c.cin_of].abs() * U.abs().view(1, 64, 1, 1, 6, 6), AT.abs())
    # ---- reference: the true sparse convolution, float64
    ref = F.conv2d(d[:, c.cin_of], c.ker.view(64, 1, 3, 3), padding=1, groups=64)
    c.out_scale = None
    if form == "bnact":
        c.out_scale = _exp2(torch.randint(-3, 4, (64,), generator=gen)).float()
        ref = ref * c.out_scale.double().view(1, 64, 1, 1)
        c.scale = c.scale * c.out_scale.double().view(1, 64, 1, 1, 1, 1)
    valid = torch.ones(B, 64, H, W, dtype=torch.bool)
    c.z = c.keep = None
    if form == "full":                       # the ReLU mask of the data-gradient epilogue: fma(1, z, 0) > 0
        c.keep = torch.randint(0, 2, (B, H, W, 64), generator=gen).bool()
        mag = torch.randint(1, 9, (B, H, W, 64), generator=gen).float()
        c.z = torch.where(c.keep, mag, torch.where(mag > 4, -mag, torch.zeros(())))      # masked: negative values and zeros
        valid = c.keep.permute(0, 3, 1, 2)
    c.ref = to_tiles(ref, ny, nx)
    c.valid = to_tiles(valid, ny, nx)
    ty = torch.arange(ny) // 2
    c.parity = ty % 2 if (H + 7) // 8 > 1 else torch.zeros(ny, dtype=torch.long)      # tile-row parity of a Winograd tile row
    assert not bool(c.ref[c.scale == 0].any())           # (a channel the ReLU prologue switches off: exact zeros expected)
    return c


def to_tiles(t_nchw, ny, nx):
    """[B, 64, H, W] -> [B, 64, ny, nx, 4, 4], zero (False) beyond the image"""
    H, W = t_nchw.shape[2], t_nchw.shape[3]
    return F.pad(t_nchw, (0, 4 * nx - W, 0, 4 * ny - H)).unfold(2, 4, 4).unfold(3, 4, 4)


def nhwc_to_tiles(out_nhwc, c):
    return to_tiles(out_nhwc.detach().cpu().permute(0, 3, 1, 2), c.ny, c.nx)


# ------------------------------------------------------------------------------------ the emulator
class Fault:
    """One injected fault.  kind "term": piece product `term` = (i, j) is not added; "zero" / "swap": the 8-channel slot
    `slot` (0..7 = 4 K-step + group) of piece `piece` of `operand` ("V" or "U") is not staged / changes places with its
    neighbour slot^1.  A "U" fault sits in the image of ONE wave: output channels 16 cog .. + 15, position half `half`.
    Restrictions (None = everywhere): pos = (i, j) one transform position, wtile = one Winograd tile 0..15 of every block
    tile (8 (a mod 2) + b mod 8), parity = one tile-row parity."""

    def __init__(self, kind, term=None, operand=None, piece=None, slot=None, cog=None, half=None, pos=None, wtile=None, parity=None):
        assert kind in ("term", "zero", "swap") and (kind == "term") == (term is not None)
        assert operand in (None, "V", "U") and (operand == "U") == (cog is not None)
        self.kind, self.term, self.operand, self.piece, self.slot = kind, term, operand, piece, slot
        self.cog, self.half, self.pos, self.wtile, self.parity = cog, half, pos, wtile, parity

    def __repr__(self):
        return "Fault(%s)" % ", ".join("%s=%r" % kv for kv in sorted(self.__dict__.items()) if kv[1] is not None)

    def where(self, c):
        """[ny, nx, 6, 6] bool: the (Winograd tile, position) pairs the fault applies to"""
        m = torch.ones(c.ny, c.nx, 6, 6, dtype=torch.bool)
        a, b = torch.arange(c.ny).view(-1, 1), torch.arange(c.nx).view(1, -1)
        if self.pos is not None:
            p = torch.zeros(6, 6, dtype=torch.bool)
            p[self.pos] = True
            m &= p
        if self.half is not None:
            p = torch.zeros(6, 6, dtype=torch.bool)
            p[list(HALF_ROWS[self.half])] = True
            m &= p
        if self.wtile is not None:
            m &= (8 * (a % 2) + b % 8 == self.wtile).view(c.ny, c.nx, 1, 1)
        if self.parity is not None:
            m &= (c.parity == self.parity).view(c.ny, 1, 1, 1)
        return m


def _fma(a, x, y):
    return (a * x.double() + y.double()).float()


def _at6(m):
    """at6() of csrc/conv_wino4.hip over the last dimension"""
    m0, m1, m2, m3, m4, m5 = m.unbind(-1)
    s1, d1, s2, d2 = m1 + m2, m1 - m2, m3 + m4, m3 - m4
    return torch.stack([(m0 + s1) + s2, _fma(2.0, d2, d1), _fma(4.0, s2, s1), _fma(8.0, d2, d1) + m5], -1)


def output_transform(acc):
    """Y = A^T M A in f32 the way the tile epilogue does it: A^T over j (at6), then the rows by position half -- half 0 holds
    rows (0, 1, 2), half 1 rows (5, 3, 4); each forms s = t1 + t2, d = t1 - t2 of its rows, finishes two output rows and
    hands the other two over; the sums are (rows 0-2) + (rows 3-5).  [..., 6, 6] -> [..., 4, 4]"""
    t0, t1, t2, t3, t4, t5 = _at6(acc).unbind(-2)
    sa, da, sb, db = t1 + t2, t1 - t2, t3 + t4, t3 - t4
    y0 = (sa + t0) + sb
    y1 = da + 2.0 * db
    y2 = sa + 4.0 * sb
    y3 = da + _fma(8.0, db, t5)
    return torch.stack([y0, y1, y2, y3], -2)


def emulate(c, terms=TERMS, fault=None):
    """The split pipeline on the case's operands -> outputs in tile form [B, 64, ny, nx, 4, 4] (f32).  Every MFMA of the kernel
    adds ONE non-zero, exactly representable piece product to its accumulator (the other 31 channels of the K-step and the
    whole other K-step contribute exact zeros), so the main loop is six f32 additions per position."""
    Vp, Up = pieces(c.V32), pieces(c.U32)
    ch = [c.cin_of, c.cin_of, c.cin_of]                     # the input channel whose V meets piece j of U
    mask_o = None
    if fault is not None:
        where = fault.where(c)
        if fault.operand == "V":
            lo = 8 * fault.slot
            sl, nb = slice(lo, lo + 8), slice(lo ^ 8, (lo ^ 8) + 8)
            Vp = list(Vp)
            old = Vp[fault.piece]
            new = old.clone()
            if fault.kind == "zero":
                new[:, sl] = torch.where(where, torch.zeros(()), old[:, sl])
            else:
                new[:, sl] = torch.where(where, old[:, nb], old[:, sl])
                new[:, nb] = torch.where(where, old[:, sl], old[:, nb])
            Vp[fault.piece] = new
        elif fault.operand == "U":
            o = torch.arange(64)
            in_wave = (o // 16 == fault.cog)
            hit = in_wave & (c.cin_of // 8 == fault.slot)
            if fault.kind == "swap":
                hit |= in_wave & (c.cin_of // 8 == (fault.slot ^ 1))
            mask_o = hit.view(1, 64, 1, 1, 1, 1) & where
    acc = torch.zeros((c.B, 64, c.ny, c.nx, 6, 6), dtype=torch.float32)
    for i, j in terms:
        prod = Vp[i][:, c.cin_of] * Up[j].view(1, 64, 1, 1, 6, 6)
        if fault is not None:
            if fault.kind == "term" and fault.term == (i, j):
                prod = torch.where(where, torch.zeros(()), prod)
            elif fault.operand == "U" and fault.piece == j:
                # zero: the piece is missing; swap: it meets the V of channel ci ^ 8 (and the neighbour's own piece, zero, comes here)
                moved = Vp[i][:, c.cin_of ^ 8] * Up[j].view(1, 64, 1, 1, 6, 6) if fault.kind == "swap" else torch.zeros(())
                prod = torch.where(mask_o, moved, prod)
        acc = acc + prod
    y = output_transform(acc)
    if c.out_scale is not None:
        y = y * c.out_scale.view(1, 64, 1, 1, 1, 1)
    return y


# ------------------------------------------------------------------------------------ statistics and the report
def q_of(got_tiles, c):
    """q [B, 64, ny, nx, 4, 4] (float64; 0 outside `valid`; inf for a non-finite output, and for a non-zero one where the
    scale is zero: all 36 products vanish there, the output is an exact zero)"""
    err = (got_tiles.double() - c.ref).abs()
    q = torch.where(err == 0, err, err / c.scale / UNIT)
    q = torch.where(torch.isfinite(q), q, torch.full((), float("inf"), dtype=F64))
    return torch.where(c.valid, q, torch.zeros((), dtype=F64))


def group_rms(q, c):
    """RMS of q over the valid Winograd tiles of the map per (output channel, y mod 4, x mod 4, tile-row parity): [64, 4, 4, 2];
    0 for a group without samples"""
    out = torch.zeros(64, 4, 4, 2, dtype=F64)
    for par in (0, 1):
        rows = c.parity == par
        if not bool(rows.any()):
            continue
        n = c.valid[:, :, rows].double().sum((0, 2, 3))
        s = (q[:, :, rows] ** 2).sum((0, 2, 3))
        out[..., par] = torch.sqrt(s / n.clamp_min(1.0))
    return out


def stats(got_tiles, c):
    """-> (worst q, worst group RMS)"""
    q = q_of(got_tiles, c)
    return float(q.max()), float(group_rms(q, c).max())


def best_position(res, valid):
    """The transform position whose pattern A^T[:, i] (x) A^T[:, j] explains most of a tile's residual [4, 4] (least squares on
    the valid outputs) -> ((i, j), its coefficient: the deviation of M[i][j])"""
    best = None
    for i, j in itertools.product(range(6), range(6)):
        p = torch.outer(AT[:, i], AT[:, j]) * valid
        pp = float((p * p).sum())
        if pp == 0.0:
            continue
        alpha = float((p * res).sum()) / pp
        left = float(((res * valid - alpha * p) ** 2).sum())
        if best is None or left < best[0]:
            best = (left, (i, j), alpha)
    return best[1], best[2]


def describe(got_tiles, c, gate_max, gate_rms):
    """None if the launch is inside both gates, else where it is not."""
    q = q_of(got_tiles, c)
    rms = group_rms(q, c)
    wq, wr = float(q.max()), float(rms.max())
    if wq <= gate_max and wr <= gate_rms:
        return None
    if wq > gate_max:
        b, o, a, bx, y, x = (int(v) for v in (q == q.max()).nonzero()[0])
        par = int(c.parity[a])
    else:
        o, y, x, par = (int(v) for v in (rms == rms.max()).nonzero()[0])
        sub = torch.where((c.parity == par).view(1, -1, 1), q[:, o, :, :, y, x], torch.full((), -1.0, dtype=F64))
        b, a, bx = (int(v) for v in (sub == sub.max()).nonzero()[0])
    ci = int(c.cin_of[o])
    beyond = (q[:, o][:, c.parity == par].amax((0, 1, 2)) > gate_max) | (rms[o, :, :, par] > gate_rms)
    over = [tuple(v) for v in beyond.nonzero().tolist()]
    res = (got_tiles[b, o, a, bx].double() - c.ref[b, o, a, bx])
    (pi, pj), alpha = best_position(res, c.valid[b, o, a, bx].double())
    if c.out_scale is not None:
        alpha /= float(c.out_scale[o])
    uv = abs(float(c.V32[b, ci, a, bx, pi, pj]) * float(c.U32[o, pi, pj]))
    rel = abs(alpha) / uv if uv > 0 else float("inf")
    msg = ["%s, shift %d, %dx%dx%d: worst q %.2f (gate %.2f), worst RMS %.2f (gate %.2f)" % (
        "data gradient" if c.dgrad else "forward", c.shift, c.B, c.H, c.W, wq, gate_max, wr, gate_rms)]
    msg.append("tile-row parity %d (%s image)" % (par, "-U" if par else "+U"))
    msg.append("page %d, block tile (ty %d, tx %d), Winograd tile %d of it" % (b, a // 2, bx // 8, 8 * (a % 2) + bx % 8))
    msg.append("input channel %d = (K-step %d, 8-channel group %d, element %d)" % (ci, ci // 32, (ci % 32) // 8, ci % 8))
    msg.append("output channel %d = (16-channel group %d, lane %d)" % (o, o // 16, o % 16))
    msg.append("in-tile coordinates (y, x) beyond a gate for this channel and parity: %s" % (over,))
    msg.append("residual of the worst tile best matches position (%d, %d) (half %d): deviation %.3e of |V U| there (2^%.1f): %s" % (
        pi, pj, 0 if pi < 3 else 1, rel, torch.log2(torch.tensor(rel)).item() if 0 < rel < float("inf") else 0.0, _hint(rel)))
    return "; ".join(msg)


# ------------------------------------------------------------------------------------ floor and gates
@functools.lru_cache(maxsize=None)
def floor():
    """The emulator's own worst q and worst group RMS over every operand set of the GPU test -> (floor_max, floor_rms)"""
    fm = fr = 0.0
    for form, shape, t in launches():
        c = make_case(form, shape, t)
        m, r = stats(emulate(c), c)
        fm, fr = max(fm, m), max(fr, r)
    return fm, fr


def gates():
    """(gate_max, gate_rms) = (3 floor_max, 2.5 floor_rms).  The margin is for what the emulator's round-to-nearest additions
    do not model: the bf16 MFMA's one-sided accumulate (each add can lose up to twice what round-to-nearest loses) and fma
    contraction in the device's transforms."""
    fm, fr = floor()
    return 3.0 * fm, 2.5 * fr
