"""Case table, integer probes and float64 references for the channel-generic NHWC convolutions of the layer2 stage
(csrc/conv_nhwc.hip: cova_conv_nhwc_fwd, _dgrad, _wgrad).  No GPU import: tests/test_nhwc_cases_cpu.py checks the table
itself, tests/test_nhwc_paths_gpu.py runs it on the kernels.

``tile``, ``plan``, ``class_sizes``, ``wgrad_partition`` and ``variants`` restate the HOST logic of conv_nhwc.hip: which
block tile a launch takes, which taps each pixel class of a data gradient gathers, how the grid is sized, how the weight
gradient cuts its pixels into parts.

Exactness.  Every operand (input, weight, dy, dy2, addend) holds integers in [-3, 3].  A product is an integer of
magnitude <= 9, so every partial sum of an output is an integer of magnitude <= 9 * (number of products) + 3 (addend):
``bound(case, entry)``, at most 9 * 10 taps * 192 channels + 3 = 17 283 for the forward and the data gradient and 9 * M
for the weight gradient, far below 2^24.  Integers below 2^24 are exact in f32, sums and fused multiply-adds of them
included, so ANY correct f32 evaluation -- any order, any tiling, with or without FMA -- gives the bits of the float64
reference.  One dropped, duplicated or misplaced product changes an integer and is seen.
"""
import collections
import functools

import torch
import torch.nn.functional as F

KC = 32                         # conv_nhwc.hip: reduction chunk
MAXTAP = 10                     # conv_nhwc.hip: nine 3x3 taps + one 1x1 tap
WG_ROWS, WG_COLS = 64, 128      # conv_nhwc.hip: weight-gradient block tile
EXACT_BELOW = 2 ** 24

Case = collections.namedtuple("Case", "k s p Ci Co B H W")
Tap = collections.namedtuple("Tap", "src dy dx wrow")


def case_id(c):
    return "k%ds%dp%d-%dto%d-%dx%dx%d" % c


# ------------------------------------------------------------------------------------------------ restated host logic
def out_size(n, k, s, p):
    """Ho of the header's contract; None where the map is smaller than the kernel (the entry points refuse it)"""
    if n + 2 * p < k:
        return None
    return (n + 2 * p - k) // s + 1


def shape_ok(Ci, Co, k, s, p):
    """conv_nhwc.hip shape_ok()"""
    return Ci > 0 and Co > 0 and Ci % 64 == 0 and Co % 64 == 0 and k in (1, 3) and s in (1, 2) and 0 <= p < k


def tile(N):
    """conv_nhwc.hip gather(): BN = 128 when the output width N is a multiple of 128, else 64 (BM = 8192 / BN pixels)"""
    return 128 if N % 128 == 0 else 64


def block_pixels(N):
    return 8192 // tile(N)


def joined_ok(k, s, p, H, W):
    """cova_conv_nhwc_dgrad: a second source (1x1, pad 0, same stride) needs the same output grid"""
    Ho, Wo = out_size(H, k, s, p), out_size(W, k, s, p)
    return Ho is not None and Wo is not None and (H - 1) // s + 1 == Ho and (W - 1) // s + 1 == Wo


def plan(k, stride, pad, second_source, Cs=1):
    """The tap planner of cova_conv_nhwc_dgrad (the loop over ``c < plan.ncls``): the input-gradient map splits into
    stride^2 parity classes (oy, ox); input row stride * jy + oy receives output row jy + (oy + pad - ky) / stride from
    kernel row ky when the division is exact.  A second source adds Tap(1, 0, 0, 0) to class (0, 0).
    -> [((oy, ox), [Tap(src, dy, dx, wrow), ...]), ...]; wrow = (ky * k + kx) * Cs, the first row of the tap's slice of the
    [(tap * Cs + c)][N] weight matrix.  (Python's % is the C code's ((t % s) + s) % s; // is only applied where it is exact.)"""
    classes = []
    for c in range(stride * stride):
        py, px = c // stride, c % stride
        taps = []
        for ky in range(k):
            ty = py + pad - ky
            if ty % stride:
                continue
            for kx in range(k):
                tx = px + pad - kx
                if tx % stride:
                    continue
                taps.append(Tap(0, ty // stride, tx // stride, (ky * k + kx) * Cs))
        if second_source and py == 0 and px == 0:
            taps.append(Tap(1, 0, 0, 0))
        assert len(taps) <= MAXTAP
        classes.append(((py, px), taps))
    return classes


def fwd_plan(k, stride, pad, Cs=1):
    """cova_conv_nhwc_fwd: one class, output (y, x) reads source (stride * y + ky - pad, stride * x + kx - pad)"""
    return [((0, 0), [Tap(0, ky - pad, kx - pad, (ky * k + kx) * Cs) for ky in range(k) for kx in range(k)])]


def class_sizes(B, H, W, stride):
    """conv_nhwc_gather_kernel / launch_gather: (Hc, Wc, pixels) of every parity class of a [B, H, W] map"""
    out = []
    for c in range(stride * stride):
        oy, ox = c // stride, c % stride
        hc, wc = (H - oy + stride - 1) // stride, (W - ox + stride - 1) // stride
        out.append((hc, wc, B * hc * wc if hc > 0 and wc > 0 else 0))
    return out


def _cdiv(a, b):
    return -(-a // b)


def wgrad_partition(M, Ci, Co, k):
    """conv_nhwc.hip wgrad_per_part() and cova_conv_nhwc_wgrad_num_partials: about 2048 blocks in all, at least 256 pixels
    per part, a part a multiple of the 32-pixel chunk -> (pixels per part, parts, pixels in the last part)"""
    if M <= 0:
        return (0, 1, 0)
    row_tiles, col_tiles = k * k * Ci // WG_ROWS, Co // WG_COLS
    parts = max(min(_cdiv(2048, row_tiles * col_tiles), _cdiv(M, 256)), 1)
    per = _cdiv(_cdiv(M, parts), KC) * KC
    nparts = _cdiv(M, per)
    return per, nparts, M - (nparts - 1) * per


def workspace_floats(c):
    M = c.B * out_size(c.H, c.k, c.s, c.p) * out_size(c.W, c.k, c.s, c.p)
    return wgrad_partition(M, c.Ci, c.Co, c.k)[1] * c.k * c.k * c.Ci * c.Co


def has_wgrad(c):
    return c.Co % WG_COLS == 0


def has_joined(c):
    return joined_ok(c.k, c.s, c.p, c.H, c.W)


def variants(c):
    """What the restated dispatch says the launches of one case take:
    fwd    (BN, blocks along pixels, taps)
    dgrad  (BN, blocks along pixels, (taps, Hc, Wc, pixels, blocks that do work) per class); with a second source the first
           class has one tap more
    wgrad  (pixels per part, parts, pixels in the last part) or None"""
    Ho, Wo = out_size(c.H, c.k, c.s, c.p), out_size(c.W, c.k, c.s, c.p)
    M = c.B * Ho * Wo
    bm_f, bm_d = block_pixels(c.Co), block_pixels(c.Ci)
    sizes = class_sizes(c.B, c.H, c.W, c.s)
    gx = _cdiv(max(m for _, _, m in sizes), bm_d) if c.B else 0
    cls = [(len(taps), hc, wc, m, _cdiv(m, bm_d)) for (_, taps), (hc, wc, m) in zip(plan(c.k, c.s, c.p, False), sizes)]
    return {"fwd": (tile(c.Co), _cdiv(M, bm_f), c.k * c.k),
            "dgrad": (tile(c.Ci), gx, cls),
            "wgrad": wgrad_partition(M, c.Ci, c.Co, c.k) if has_wgrad(c) else None}


# ------------------------------------------------------------------------------------------------ cases
GEOMETRIES = [(1, 1, 0), (1, 2, 0), (3, 1, 0), (3, 2, 0), (3, 1, 1), (3, 2, 1), (3, 1, 2), (3, 2, 2)]      # (k, stride, pad)
CHANNELS = [(64, 128), (128, 128), (64, 64), (128, 64), (192, 64), (192, 128), (64, 192), (128, 192)]      # (Ci, Co)
# (64, 128): forward BN = 128, data gradient BN = 64; (128, 64): the other way round.  These two take every map size.
FULL_CHANNELS = [(64, 128), (128, 64)]
SMALL_MAPS = [(1, 1, 1), (1, 1, 5), (1, 5, 1), (2, 2, 2), (1, 3, 3), (3, 4, 7)]                             # (B, H, W)
RAGGED_MAP = (2, 23, 29)
STRIDE2_MAPS = [(2, 4, 6), (1, 5, 7), (2, 4, 7)]                  # even x even, odd x odd, even x odd
REDUCED_MAPS = [(2, 2, 2), (3, 4, 7), (2, 9, 11)]                 # the other channel pairs


def valid(k, s, p, H, W):
    return H + 2 * p >= k and W + 2 * p >= k


@functools.lru_cache(maxsize=None)
def map_with_pixels(k, s, p, T, entry):
    """The smallest (B, H, W) (two rows at least where there is one) whose launch has exactly T pixels: output pixels
    B * Ho * Wo for the forward, the pixels of the largest parity class B * ceil(H / s) * ceil(W / s) for the data gradient;
    None where there is none (127 is prime: no map of three rows and columns or more has 127 pixels)"""
    best = None
    for B in (1, 2):
        for H in range(1, 24):
            for W in range(1, 300):
                if not valid(k, s, p, H, W):
                    continue
                if entry == "fwd":
                    n = B * out_size(H, k, s, p) * out_size(W, k, s, p)
                else:
                    n = B * _cdiv(H, s) * _cdiv(W, s)
                if n == T:
                    key = (H == 1, B * H * W, B, H, W)
                    if best is None or key < best:
                        best = key
    return None if best is None else best[2:]


def tile_maps(k, s, p, Ci, Co):
    """maps whose launch has one pixel less than, exactly, and one pixel more than the block tile"""
    out = []
    for entry, N in (("fwd", Co), ("dgrad", Ci)):
        bm = block_pixels(N)
        maps = [map_with_pixels(k, s, p, T, entry) for T in (bm - 1, bm, bm + 1)]
        assert maps[1] is not None and maps[2] is not None
        out += [m for m in maps if m is not None]
    return out


def _build_cases():
    cases = []
    for (k, s, p) in GEOMETRIES:
        for (Ci, Co) in CHANNELS:
            if (Ci, Co) in FULL_CHANNELS:
                maps = SMALL_MAPS + [RAGGED_MAP] + (STRIDE2_MAPS if s == 2 else []) + tile_maps(k, s, p, Ci, Co)
            else:
                maps = REDUCED_MAPS
            seen = []
            for m in maps:
                if valid(k, s, p, m[1], m[2]) and m not in seen:
                    seen.append(m)
                    cases.append(Case(k, s, p, Ci, Co, *m))
    return cases


CASES = _build_cases()
GROUPS = collections.OrderedDict()
for _c in CASES:
    GROUPS.setdefault(_c[:5], []).append(_c)

# weight-gradient pixel counts: case -> (pixels per part, parts, pixels in the last part)
WGRAD_CASES = collections.OrderedDict([
    (Case(3, 1, 1, 128, 128, 1, 3, 5), (32, 1, 15)),              # fewer than 32 pixels in all
    (Case(3, 1, 1, 128, 128, 1, 4, 8), (32, 1, 32)),              # one full chunk
    (Case(3, 1, 1, 128, 128, 1, 16, 16), (256, 1, 256)),          # the last count with one part
    (Case(3, 1, 1, 128, 128, 1, 1, 257), (160, 2, 97)),           # the first with two
    (Case(1, 2, 0, 64, 128, 1, 1, 513), (160, 2, 97)),            # the same step on the 1x1 stride-2 kernel (one row tile)
    (Case(3, 1, 1, 128, 128, 1, 3, 683), (256, 9, 1)),            # the last part holds a single pixel
    (Case(3, 1, 1, 128, 128, 2, 16, 16), (256, 2, 256)),          # every part full
    (Case(3, 2, 1, 192, 128, 1, 31, 33), (160, 2, 112)),          # three row tiles per tap, ragged last part
])

# B = 0: every entry point returns OK, the weight gradient zero-fills dw, nothing else is written
EMPTY_CASES = [Case(3, 2, 1, 64, 128, 0, 5, 7), Case(1, 2, 0, 64, 128, 0, 4, 4), Case(3, 1, 1, 128, 128, 0, 3, 3),
               Case(3, 1, 0, 128, 64, 0, 3, 3)]

# the large test: [2, 5792, 5795, 64] -- each page has 2 148 136 960 elements, 2^31 + 653 312; the second page starts beyond
# the 2^31st element, the whole input is above 2^32 elements
LARGE = dict(B=2, H=5792, W=5795, Ci=64, Co=128, geometries=[(1, 2, 0), (3, 2, 1)], wgrad_pixels=50000)


# ------------------------------------------------------------------------------------------------ probes
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 10007 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def ints(shape, g):
    """integer-valued f32 in [-3, 3]"""
    return torch.randint(-3, 4, shape, generator=g).float()


@functools.lru_cache(maxsize=None)
def probe(c):
    """dict of NCHW / OIHW f32 tensors with integer values in [-3, 3]: x, w, dy; w1, dy2 (the 1x1 second source, only where
    the geometry admits it); add (addend of the data gradient).  Shared between tests: not to be modified."""
    g = _gen(7, *c)
    Ho, Wo = out_size(c.H, c.k, c.s, c.p), out_size(c.W, c.k, c.s, c.p)
    d = dict(x=ints((c.B, c.Ci, c.H, c.W), g), w=ints((c.Co, c.Ci, c.k, c.k), g), dy=ints((c.B, c.Co, Ho, Wo), g),
             add=ints((c.B, c.Ci, c.H, c.W), g))
    if has_joined(c):
        d["w1"], d["dy2"] = ints((c.Co, c.Ci, 1, 1), g), ints((c.B, c.Co, Ho, Wo), g)
    return d


def bound(c, entry):
    """the largest magnitude a partial sum of one output can reach (see the module docstring)"""
    if entry == "fwd":
        return 9 * c.k * c.k * c.Ci
    if entry == "dgrad":                                        # every tap, the second source's, the addend
        return 9 * (c.k * c.k + 1) * c.Co + 3
    if entry == "wgrad":
        return 9 * c.B * out_size(c.H, c.k, c.s, c.p) * out_size(c.W, c.k, c.s, c.p)
    raise KeyError(entry)


# ------------------------------------------------------------------------------------------------ references
def ref_fwd(c, d, dtype=torch.float64):
    return F.conv2d(d["x"].to(dtype), d["w"].to(dtype), stride=c.s, padding=c.p)


def ref_dgrad(c, d, joined=False, addend=False, dtype=torch.float64):
    shape = (c.B, c.Ci, c.H, c.W)
    r = torch.nn.grad.conv2d_input(shape, d["w"].to(dtype), d["dy"].to(dtype), stride=c.s, padding=c.p)
    if joined:
        r = r + torch.nn.grad.conv2d_input(shape, d["w1"].to(dtype), d["dy2"].to(dtype), stride=c.s, padding=0)
    if addend:
        r = r + d["add"].to(dtype)
    return r


def ref_wgrad(c, d, dtype=torch.float64):
    return torch.nn.grad.conv2d_weight(d["x"].to(dtype), (c.Co, c.Ci, c.k, c.k), d["dy"].to(dtype), stride=c.s,
                                       padding=c.p)


def dgrad_operand(w):
    """cova_conv_nhwc_prep's data-gradient operand of an OIHW weight: [(tap * Co + co)][Ci]"""
    co, ci, k, _ = w.shape
    return w.permute(2, 3, 0, 1).reshape(k * k * co, ci)


def apply_plan(classes, stride, srcs, wds, shape, addend=None):
    """The gather of conv_nhwc_gather_kernel written out with the planner's taps in plain torch (float64):
    out[b, :, stride * jy + oy, stride * jx + ox] = sum over the class's taps of
    src_t[b, :, jy + dy_t, jx + dx_t] @ wd_t[wrow_t : wrow_t + Cs] (zero outside the source) (+ addend).
    srcs: NCHW sources, wds: their [(tap * Cs + c)][N] operands."""
    B, N, H, W = shape
    out = torch.zeros(shape, dtype=torch.float64)
    for (oy, ox), taps in classes:
        hc, wc = len(range(oy, H, stride)), len(range(ox, W, stride))
        if hc <= 0 or wc <= 0:
            continue
        for t in taps:
            src, wd = srcs[t.src].double(), wds[t.src].double()
            Cs, Hs, Ws = src.shape[1:]
            sy, sx = torch.arange(hc) + t.dy, torch.arange(wc) + t.dx
            ok = ((sy >= 0) & (sy < Hs)).view(-1, 1) & ((sx >= 0) & (sx < Ws)).view(1, -1)
            g = src[:, :, sy.clamp(0, Hs - 1)][:, :, :, sx.clamp(0, Ws - 1)] * ok
            out[:, :, oy::stride, ox::stride] += torch.einsum("bchw,cn->bnhw", g, wd[t.wrow:t.wrow + Cs])
    if addend is not None:
        out = out + addend.double()
    return out
