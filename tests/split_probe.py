"""Deterministic probes of the bf16-split products (csrc/bf3.h: x = x0 + x1 + x2, three round-to-nearest bf16 pieces; the six
piece products of order <= 2 accumulated in f32).  Host side only -- torch on the CPU, importable without a GPU.

The operands are chosen so that the exact result is an f32 number and every piece is individually visible in it: a kernel
that drops a piece, a piece product, or mis-stages one piece of one 8-channel slot differs from the exact value by far more
than an ulp, and the assertion is torch.equal -- no measured tolerance.  tests/test_split_products_cpu.py runs the checkers
on a CPU emulation of the split (complete, and with every single fault) to show that they are sensitive;
tests/test_split_products_gpu.py runs the same builders and checkers on the kernels.

Piece product (i, j) = x_i * w_j.  TERMS is the order of the kernels (smallest first)."""
import torch

TERMS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))


# ------------------------------------------------------------------------------------ operands
def _exp2(k):
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), k.double())


def _sign(shape, gen, nonneg):
    if nonneg:
        return torch.ones(shape, dtype=torch.float64)
    return torch.randint(0, 2, shape, generator=gen).double() * 2.0 - 1.0


def lattice(shape, gen, kmin=-12, kmax=12, nonneg=False):
    """+-(a + b/256 + c/65536) * 2^k, a in [128, 255], b, c in [0, 127]; k per channel (last dimension) in [kmin, kmax].
    24 significant bits; the three RNE bf16 pieces (x0 = a 2^k; x1 != 0 unless b = c = 0, x2 != 0 for most samples) sum to x
    exactly, and every subset sum of them is a multiple of 2^(k-16) below 2^(k+8), an f32 number: accumulated in any order they
    give x bit for bit.
    Without x2 up to 7.6e-6 of x is missing, without x1 up to 3.9e-3.  A product with a power of two stays on the lattice."""
    shape = tuple(shape)
    a = torch.randint(128, 256, shape, generator=gen).double()
    b = torch.randint(0, 128, shape, generator=gen).double()
    c = torch.randint(0, 128, shape, generator=gen).double()
    k = torch.randint(kmin, kmax + 1, shape[-1:], generator=gen)
    x = _sign(shape, gen, nonneg) * (a + b / 256.0 + c / 65536.0) * _exp2(k)
    assert torch.equal(x.float().double(), x)
    return x.float()


def quarter(shape, gen, kmin=-12, kmax=12, nonneg=False):
    """+-(a + 1/4) * 2^(k-7), a in [128, 255]; k per channel (last dimension): x0 = a 2^(k-7), x1 = 2^(k-9), x2 = 0.  The product
    of two such values, (ab + (a + b)/4 + 1/16) 2^(k+j-14), has 20 significant bits (exact in f32) and its 1/16 is exactly
    x1 * w1: a kernel without that piece product is off by 2^-20 ... 2^-18 of the result."""
    shape = tuple(shape)
    a = torch.randint(128, 256, shape, generator=gen).double()
    k = torch.randint(kmin, kmax + 1, shape[-1:], generator=gen)
    x = _sign(shape, gen, nonneg) * (a + 0.25) * _exp2(k - 7)
    return x.float()


def pow2(shape, gen, jmin=-6, jmax=6):
    """2^j, j in [jmin, jmax] per element: one piece (x1 = x2 = 0)."""
    return _exp2(torch.randint(jmin, jmax + 1, tuple(shape), generator=gen)).float()


def pieces(x):
    """The three round-to-nearest-even bf16 pieces of an f32 tensor, as f32 (bf3_split_pair in csrc/bf3.h)."""
    x = x.float()
    p0 = x.bfloat16().float()
    r = x - p0
    p1 = r.bfloat16().float()
    p2 = (r - p1).bfloat16().float()
    return [p0, p1, p2]


def emulate(x_pieces, w_pieces, terms=TERMS, kstep=16):
    """out [R, N] = sum over `terms` (i, j) of x_i [R, K] . w_j [N, K]^T, accumulated in f32 the way the kernels do: K in steps
    of `kstep` channels, the terms of a step one after the other into the same accumulator (each piece product is exact in
    f32: 8 x 8 significant bits)."""
    K = x_pieces[0].shape[1]
    acc = torch.zeros((x_pieces[0].shape[0], w_pieces[0].shape[0]), dtype=torch.float32)
    for s in range(0, K, kstep):
        for i, j in terms:
            acc = acc + x_pieces[i][:, s:s + kstep] @ w_pieces[j][:, s:s + kstep].t()
    return acc


def zero_slot(pcs, piece, slot, width=8):
    """Fault: the `slot`-th group of `width` channels of one piece is not staged (zero)."""
    out = [p.clone() for p in pcs]
    out[piece][:, slot * width:(slot + 1) * width] = 0.0
    return out


def swap_slot(pcs, piece, slot, width=8):
    """Fault: the `slot`-th group of `width` channels of one piece changes places with its neighbour."""
    out = [p.clone() for p in pcs]
    nslots = pcs[0].shape[1] // width
    other = slot + 1 if slot + 1 < nslots else slot - 1
    a, b = slice(slot * width, (slot + 1) * width), slice(other * width, (other + 1) * width)
    out[piece][:, a], out[piece][:, b] = pcs[piece][:, b], pcs[piece][:, a]
    return out


# ------------------------------------------------------------------------------------ the 1x1 probes
def select_weight(cout, cin, t, gen, shift=0):
    """w [cout, cin]: w[co, ci] = 2^j(co) * [ci == (co + 64 t + shift) mod cin]; -> (w, sel [cout])."""
    sel = (torch.arange(cout) + 64 * t + shift) % cin
    w = torch.zeros((cout, cin), dtype=torch.float32)
    w[torch.arange(cout), sel] = pow2((cout,), gen)
    return w, sel


def select_rows(R, cin, t, values):
    """x [R, cin]: x[r, ci] = values[r] * [ci == (r + t) mod cin]; -> (x, sel [R])."""
    sel = (torch.arange(R) + t) % cin
    x = torch.zeros((R, cin), dtype=torch.float32)
    x[torch.arange(R), sel] = values
    return x, sel


def exact(x, w):
    """x [R, K] . w [N, K]^T in fp64, for operands whose dot products have ONE non-zero term (or few, of a common lattice): the
    fp64 value is then the exact one.  -> (ref64, representable): entries that are not f32 numbers are not to be asserted."""
    ref = x.double() @ w.double().t()
    return ref, ref.float().double() == ref


def probe_a(R, cin, cout, t, gen, nonneg=False):
    """x pieces: x = lattice, w selects one input channel per output channel.  out[r, co] = x[r, sel(co)] * 2^j(co).
    -> (x, w, ref64, k_of [R, cout])"""
    x = lattice((R, cin), gen, nonneg=nonneg)
    w, sel = select_weight(cout, cin, t, gen)
    ref, ok = exact(x, w)
    assert bool(ok.all())
    return x, w, ref, sel.view(1, cout).expand(R, cout)


def probe_b(R, cin, cout, t, gen):
    """w pieces: row r has one non-zero channel (r + t) mod cin of value 2^k(r), w = lattice.  out[r, co] = w[co, sel(r)] * 2^k(r)."""
    x, sel = select_rows(R, cin, t, pow2((R,), gen))
    w = lattice((cout, cin), gen)
    ref, ok = exact(x, w)
    assert bool(ok.all())
    return x, w, ref, sel.view(R, 1).expand(R, cout)


def probe_c(R, cin, cout, t, gen):
    """second-order product: probe B's rows with a `quarter` value, w = quarter.  The result's lowest term is x1 * w1."""
    x, sel = select_rows(R, cin, t, quarter((R, 1), gen, -6, 6).view(R))
    w = quarter((cout, cin), gen)
    ref, ok = exact(x, w)
    assert bool(ok.all())
    return x, w, ref, sel.view(R, 1).expand(R, cout)


PROBES = {"A": probe_a, "B": probe_b, "C": probe_c}


# ------------------------------------------------------------------------------------ the checker
def _hint(rel):
    if rel >= 0.5:
        return "a whole term is missing or misplaced (x0 w0, or a wrong channel)"
    if rel >= 2.0 ** -12:
        return "the size of a second piece: x1 w0 / x0 w1"
    if rel >= 2.0 ** -18:
        return "the size of a third piece: x2 w0 / x0 w2"
    if rel >= 2.0 ** -21:
        return "the size of x1 w1"
    return "below every piece product: accumulation, not a missing piece"


def mismatch(got, ref64, probed=None, k_of=None, tile=32):
    """None if got == ref64 on the probed entries (bit for bit; +0 == -0), else a description of where it is not: how many
    entries, which leading indices (row tiles of `tile` rows), which 8-channel K slots (k_of: the K index behind each
    entry), the largest relative deviation and which piece product has that size."""
    got = got.detach().cpu()
    ref = ref64.detach().cpu().double()
    assert got.dtype == torch.float32 and got.shape == ref.shape, (got.dtype, got.shape, ref.shape)
    rep = ref.float().double() == ref
    if probed is None:
        assert bool(rep.all()), "the probe's exact value is not an f32 number"
        probed = rep
    else:
        assert bool(rep[probed].all()), "the probe's exact value is not an f32 number"
    bad = (got.double() != ref) & probed
    if not bool(bad.any()):
        return None
    idx = bad.nonzero()
    rel = float(((got.double() - ref).abs() / ref.abs().clamp_min(1e-300))[bad].max()) if bool((ref[bad] != 0).any()) \
        else float("inf")
    first = tuple(int(i) for i in idx[0])
    msg = ["%d of %d probed entries differ; first at %s: got %r, exact %r" % (
        idx.shape[0], int(probed.sum()), first, float(got[first]), float(ref[first]))]
    lead = idx[:, 0].unique()
    tiles = (lead // tile).unique()
    msg.append("leading index %d..%d (%d distinct; tiles of %d: %s, %d of them odd)" % (
        int(lead.min()), int(lead.max()), lead.numel(), tile, tiles.tolist()[:12], int((tiles % 2 == 1).sum())))
    if idx.shape[1] > 1:
        last = idx[:, -1].unique()
        msg.append("last index %s%s" % (last.tolist()[:16], " ..." if last.numel() > 16 else ""))
    if k_of is not None:
        ks = k_of[bad].unique()
        msg.append("K positions %s%s = 8-channel slots %s" % (ks.tolist()[:16], " ..." if ks.numel() > 16 else "",
                                                               (ks // 8).unique().tolist()[:16]))
    msg.append("largest deviation %.3e of the value (2^%.1f): %s" % (
        rel, torch.log2(torch.tensor(rel)).item() if rel > 0 else 0.0, _hint(rel)))
    return "; ".join(msg)


def check_exact(got, ref64, what, probed=None, k_of=None, tile=32):
    m = mismatch(got, ref64, probed, k_of, tile)
    assert m is None, "%s: %s" % (what, m)


# ------------------------------------------------------------------------------------ error-class yardsticks
def f32_chain(x, w):
    """The sequential, FMA-free f32 chain acc = acc + x[:, k] * w[:, k] over k (what a plain f32 kernel computes)."""
    x, w = x.float(), w.float()
    acc = torch.zeros((x.shape[0], w.shape[0]), dtype=torch.float32)
    for k in range(x.shape[1]):
        acc = acc + x[:, k:k + 1] * w[:, k].view(1, -1)
    return acc


def max_err(got, ref64):
    ref64 = ref64.double()
    return float((got.detach().cpu().double() - ref64).abs().max() / ref64.abs().max())


def bias(got, ref64):
    ref64 = ref64.double()
    return float((got.detach().cpu().double() - ref64).mean() / ref64.abs().mean())


def operands(R, cin, cout, one_sign, seed):
    """x ~ N(0,1) [R, cin], w ~ 0.1 N(0,1) [cout, cin]; one_sign: max(. + 0.5 sigma, 0), ReLU-like, as tools/c11_error.py."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((R, cin), generator=g)
    w = torch.randn((cout, cin), generator=g) * 0.1
    if one_sign:
        x, w = (x + 0.5).clamp_min(0.0), (w + 0.05).clamp_min(0.0)
    return x, w
