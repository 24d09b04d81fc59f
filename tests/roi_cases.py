"""Case table, deterministic generators and float64 references for the RoIPool / RoIAlign launch paths of
csrc/roi_gat.hip.  No device work: tests/test_roi_cases_cpu.py checks the table itself with the oracle alone,
tests/test_roi_paths_gpu.py runs it on the kernels.

``variants(case)`` restates the HOST dispatch of roi_gat.hip: which template instantiation a call takes follows from
C, PH * PW, n_rois and the presence of ``partial`` / ``tail``:

    roipool_fwd_kernel<LAZY, U, XCD>        C == 64 -> <.., 8, true>, C > 64 -> <.., 4, false>; LAZY = the _bn entry
    roipool_bwd_prep_kernel<STATS, TAIL, NB> NB = 9 iff PH * PW == 9; STATS iff partial; TAIL iff tail (C == 64 only)
    roipool_bwd_rows_kernel<P33>            P33 iff PH == 3 and PW == 3
    page ranges of cova_roialign_bwd        n_rois <= 2^18: one block; above: init + grid kernels with atomics

Exactness.  Tie maps hold small integers.  The lazy operands are multiples of 1/8 of magnitude <= 4 with scale in
{-1, -0.5, 0.5, 1, 2}: fmaf(scale, z, shift) + x is a multiple of 1/16 below 2^5, exact in f32.  Exact gradients are
integers in [-8, 8], mean a multiple of 1/8, invstd in {0.5, 1, 2}: every contribution g and g * (zmax - mean) * invstd
is a multiple of 1/16 below 2^8, so an f32 sum of up to n * PH * PW <= 2^12 of them stays below 2^24 units and is exact
in any order -- the float64 reference then equals the kernel bit for bit.  Real-valued gradients are held to
head_cases.sum_bound with L = the largest number of contributions one output receives (from the oracle's argmax).
"""
import collections
import functools

import numpy as np
import torch

from oracle import cova_oracle as O

SCALE = 0.25
ROI_XW = 40                                          # pixels per owner wave of the rows kernels
LONG_LIST = 1 << 18                                  # roipool_page_ranges: above this the grid kernels run
WINDOW_SIZES = (1, 3, 4, 15, 16, 17, 31, 32, 33, 63, 64, 65)
BAD_PAGES = (-2, 3)                                  # as offsets: -2 and B + 3
F32 = np.float32

Case = collections.namedtuple("Case", "B C H W PH PW n kind")
TIE_KINDS = ("quant", "page")
FWD_KINDS = TIE_KINDS + ("edge",)

# ------------------------------------------------------------------------------------------------ cases
# forward: n * PH * PW / 4 blocks -- 144 (% 8 == 0), 153 (% 8 != 0, last block partial), 7 (< 8: no remap, partial),
# 19 (% 8 != 0, partial), 135 (% 8 != 0, full)
_FWD = [("quant33", 13, 50, 3, 3, 64, "quant"), ("page25", 13, 50, 2, 5, 61, "page"), ("quant11_small", 13, 50, 1, 1, 27, "quant"),
        ("page11", 11, 41, 1, 1, 75, "page"), ("edge33", 13, 50, 3, 3, 60, "edge"), ("edge25", 9, 81, 2, 5, 61, "edge")]
FWD_CASES = collections.OrderedDict(
    ("%s_c%d" % (name, C), Case(3, C, H, W, PH, PW, n, kind)) for (name, H, W, PH, PW, n, kind) in _FWD for C in (64, 128))

# backward: bins x C on a map of two owner segments (40 + 1 pixels), then W in {1, 39, 40, 41, 81} and H in {1, 9};
# (1, 9): NB = 9 in the entry pass with the generic rows kernel
_BWD = [(9, 41, 3, 3, 64), (9, 41, 3, 3, 128), (9, 41, 2, 5, 64), (9, 41, 2, 5, 128), (9, 41, 1, 1, 64), (9, 41, 1, 1, 128),
        (9, 41, 7, 7, 64), (9, 41, 7, 7, 128), (9, 1, 3, 3, 64), (1, 39, 2, 5, 64), (1, 40, 3, 3, 128), (9, 81, 2, 5, 128),
        (1, 1, 1, 1, 64), (9, 81, 3, 3, 64), (9, 40, 1, 9, 64)]
BWD_CASES = collections.OrderedDict(
    ("h%dw%d_%dx%d_c%d" % (H, W, PH, PW, C), Case(3, C, H, W, PH, PW, 45, "bwd")) for (H, W, PH, PW, C) in _BWD)

# RoIAlign: name -> (case, sampling_ratio, aligned, exact)
Align = collections.namedtuple("Align", "case sr aligned exact")
_ALIGN = [(14, 41, 2, 5, 64, 2, 0, 0), (14, 121, 2, 5, 128, 2, 1, 0), (14, 40, 1, 1, 64, 0, 0, 0), (9, 41, 1, 1, 128, 0, 1, 0),
          (14, 121, 4, 1, 64, 1, 1, 0), (14, 40, 4, 1, 128, 1, 0, 0), (1, 41, 2, 5, 64, 2, 1, 0), (14, 1, 4, 1, 64, 0, 0, 0),
          (1, 1, 1, 1, 64, 1, 1, 0), (14, 41, 2, 5, 64, 2, 0, 1), (14, 121, 4, 1, 128, 2, 1, 1), (14, 121, 2, 5, 64, 2, 1, 1),
          (6, 45, 1, 1, 64, 2, 0, 1)]
ALIGN_CASES = collections.OrderedDict(
    ("h%dw%d_%dx%d_c%d_sr%d_al%d%s" % (H, W, PH, PW, C, sr, al, "_exact" if ex else ""),
     Align(Case(3, C, H, W, PH, PW, 30, "align"), sr, al, bool(ex))) for (H, W, PH, PW, C, sr, al, ex) in _ALIGN)
# the long list: every box but a dozen carries page index B and is skipped everywhere
ALIGN_LONG = Align(Case(2, 64, 6, 45, 1, 1, LONG_LIST + 1, "align"), 2, 0, True)

ALL_VARIANTS = sorted(
    ["roipool_fwd<LAZY=%d,U=%d,XCD=%d>" % (l, u, x) for l in (0, 1) for (u, x) in ((8, 1), (4, 0))]
    + ["roipool_bwd_prep<STATS=%d,TAIL=%d,NB=%d>" % (s, t, nb) for (s, t) in ((0, 0), (1, 0), (1, 1)) for nb in (9, 0)]
    + ["roipool_bwd_rows<P33=%d>" % p for p in (0, 1)] + ["page_range<block>", "page_range<grid>"])


def variants(case):
    """the kernel instantiations the launches of the GPU test take for one case (host dispatch of roi_gat.hip)"""
    bins = case.PH * case.PW
    if case.kind in FWD_KINDS:                       # cova_roipool_fwd and cova_roipool_fwd_bn
        u, xcd = (4, 0) if case.C > 64 else (8, 1)
        return sorted("roipool_fwd<LAZY=%d,U=%d,XCD=%d>" % (l, u, xcd) for l in (0, 1))
    if case.kind == "bwd":                           # cova_roipool_bwd, _bwd_bn and (C == 64) _bwd_bn_tail
        nb = 9 if bins == 9 else 0
        v = ["roipool_bwd_prep<STATS=0,TAIL=0,NB=%d>" % nb, "roipool_bwd_prep<STATS=1,TAIL=0,NB=%d>" % nb]
        if case.C == 64:
            v.append("roipool_bwd_prep<STATS=1,TAIL=1,NB=%d>" % nb)
        return sorted(v + ["roipool_bwd_rows<P33=%d>" % (case.PH == 3 and case.PW == 3)])
    if case.kind == "align":                         # cova_roialign_bwd
        return ["page_range<%s>" % ("block" if case.n <= LONG_LIST else "grid")]
    raise KeyError(case.kind)


def fwd_grid(case):
    """blocks of the forward launch: four (box, bin) tasks per block"""
    return (case.n * case.PH * case.PW + 3) // 4


def _rs(case, salt):
    seed = salt
    for k in tuple(case[:7]) + tuple(ord(ch) for ch in case.kind):
        seed = (seed * 10007 + int(k)) % (2 ** 31 - 1)
    return np.random.RandomState(seed)


# ------------------------------------------------------------------------------------------------ geometry
def windows(rois, PH, PW, H, W, scale=SCALE):
    """The bin windows of RoIPool (torchvision 0.7.0 formulas, float32 where the C code has float), vectorised:
    -> hs, he [n, PH] and ws, we [n, PW] (clamped to the map; a bin is empty iff he <= hs or we <= ws)"""
    r = np.asarray(rois, F32).reshape(-1, 5)

    def rnd(v):                                      # C roundf on the float32 product: half away from zero
        v = v.astype(np.float64)
        return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)

    sw, sh, ew, eh = (rnd(r[:, k] * F32(scale)) for k in (1, 2, 3, 4))
    bh = np.maximum(eh - sh + 1, 1).astype(F32) / F32(PH)
    bw = np.maximum(ew - sw + 1, 1).astype(F32) / F32(PW)
    ph, pw = np.arange(PH, dtype=F32)[None], np.arange(PW, dtype=F32)[None]
    hs = np.clip(np.floor(ph * bh[:, None]).astype(np.int64) + sh[:, None], 0, H)
    he = np.clip(np.ceil((ph + F32(1)) * bh[:, None]).astype(np.int64) + sh[:, None], 0, H)
    ws = np.clip(np.floor(pw * bw[:, None]).astype(np.int64) + sw[:, None], 0, W)
    we = np.clip(np.ceil((pw + F32(1)) * bw[:, None]).astype(np.int64) + sw[:, None], 0, W)
    return hs, he, ws, we


def window_sizes(rois, PH, PW, H, W):
    """pixels (hend - hstart) * (wend - wstart) of every bin, 0 for an empty one -> [n, PH, PW]"""
    hs, he, ws, we = windows(rois, PH, PW, H, W)
    return np.maximum(he - hs, 0)[:, :, None] * np.maximum(we - ws, 0)[:, None, :]


def good_page(rois, B):
    p = np.asarray(rois)[:, 0].astype(np.int64)
    return (p >= 0) & (p < B)


def read_mask(case, rois):
    """[B, H, W] bool: the pixels a correct RoIPool forward reads (inside a non-empty bin of a box of that page)"""
    hs, he, ws, we = windows(rois, case.PH, case.PW, case.H, case.W)
    mask = np.zeros((case.B, case.H, case.W), bool)
    for i in np.nonzero(good_page(rois, case.B))[0]:
        b = int(rois[i, 0])
        for p in range(case.PH):
            for q in range(case.PW):
                mask[b, hs[i, p]:he[i, p], ws[i, q]:we[i, q]] = True
    return mask


# ------------------------------------------------------------------------------------------------ boxes
def edge_boxes(H, W):
    """[x1, y1, x2, y2] of the oracle's CPU edge test (tests/test_oracle_cpu.py): negative, outside, zero-area, inverted,
    sub-pixel and .5-rounding boxes; then boxes wholly left of and above the map (cova_boxes_translate produces them)"""
    e = [[-30, -20, 10, 14], [-8, -8, -2, -2], [60, 40, 200, 200], [66, 50, 70, 54], [10, 10, 10, 10],
         [10, 10, 10.4, 10.2], [30, 30, 10, 10], [40, 8, 8, 40], [2, 2, 6, 6], [6, 6, 10, 10], [10, 14, 30, 18],
         [0, 0, 67.9, 51.9], [0, 0, 4 * W + 40, 4 * H + 40], [17.9, 13.9, 18.1, 14.1], [1.99, 2.0, 2.01, 49.99],
         [16, 16, 31, 31], [15.9, 15.9, 28, 28]]
    e += [[-90, 4, -30, 30], [8, -70, 60, -20], [-200, -200, -100, -100], [-50, -10, -6, 4 * H + 10]]
    return e


def _window_boxes(case):
    """one box per size in WINDOW_SIZES with a bin window of exactly that many pixels, found among deterministic
    candidates with the window formulas above"""
    rs = _rs(case, 11)
    m = 20000                                        # (boxes larger than the map: the border clips single bins)
    x1, y1 = rs.randint(-case.W, case.W, m), rs.randint(-case.H, case.H, m)
    x2, y2 = x1 + rs.randint(0, case.PW * (case.W + 4), m), y1 + rs.randint(0, case.PH * (case.H + 4), m)
    cand = np.stack([np.zeros(m), 4.0 * x1, 4.0 * y1, 4.0 * x2, 4.0 * y2], 1).astype(F32)
    npx = window_sizes(cand, case.PH, case.PW, case.H, case.W).reshape(m, -1)
    out = []
    for s in WINDOW_SIZES:
        hit = np.nonzero((npx == s).any(1))[0]
        if len(hit) == 0:
            raise ValueError("no candidate box with a window of %d pixels for %r" % (s, (case,)))
        out.append(cand[hit[0], 1:].tolist())
    return out


@functools.lru_cache(maxsize=None)
def _boxes(case):
    rs = _rs(case, 12)
    H, W = case.H, case.W
    pool = (_window_boxes(case) if case.kind in FWD_KINDS else []) + edge_boxes(H, W)
    while len(pool) < case.n:                        # fill: boxes of every size up to the map, some inverted
        x1, y1 = rs.uniform(-20, 4 * W + 10), rs.uniform(-20, 4 * H + 10)
        pool.append([x1, y1, x1 + rs.uniform(-5, 4 * W + 20), y1 + rs.uniform(-5, 4 * H + 20)])
    e = edge_boxes(H, W)
    pool = pool[:case.n - 2] + [e[0], e[12]]         # the last two rows carry the bad page indices
    rois = np.zeros((case.n, 5), F32)
    rois[:, 1:] = np.asarray(pool, F32)
    rois[:, 0] = rs.randint(0, case.B - 1, case.n)   # unsorted; the last page has no box
    rois[case.n - 2, 0], rois[case.n - 1, 0] = BAD_PAGES[0], case.B + BAD_PAGES[1]
    return rois


def boxes(case):
    """[n, 5] float32 (page, x1, y1, x2, y2): window-size boxes (forward kinds), the edge list, fill; page indices
    unsorted over pages 0 .. B - 2, page B - 1 without a box, the last two rows on pages -2 and B + 3"""
    return _boxes(case).copy()


# ------------------------------------------------------------------------------------------------ maps
def _quantised(rs, shape):
    """values in {0, 1, 2, 3}, the larger the rarer: the first maximum of a window lies deep inside it"""
    return rs.choice(4, size=shape, p=[0.55, 0.3, 0.12, 0.03]).astype(F32)


def _page_like(rs, B, C, H, W):
    """piecewise-constant rectangles of levels 1 .. 3 on a zero background, every channel its own"""
    m = np.zeros((B, C, H, W), F32)
    for b in range(B):
        for c in range(C):
            for _ in range(5):
                h0, w0 = rs.randint(0, H), rs.randint(0, W)
                m[b, c, h0:h0 + rs.randint(1, max(H // 2, 2)), w0:w0 + rs.randint(1, max(W // 3, 2))] = rs.randint(1, 4)
    return m


def _levels(case, salt):
    rs = _rs(case, salt)
    if case.kind == "page":
        return _page_like(rs, case.B, case.C, case.H, case.W)
    return _quantised(rs, (case.B, case.C, case.H, case.W))


@functools.lru_cache(maxsize=None)
def _plain_map(case):
    if case.kind in TIE_KINDS:
        return _levels(case, 21)
    return _rs(case, 21).standard_normal((case.B, case.C, case.H, case.W)).astype(F32)


def plain_map(case):
    """[B, C, H, W] float32: a tie map (kinds quant / page) or a standard_normal one"""
    return _plain_map(case).copy()


@functools.lru_cache(maxsize=None)
def _lazy_operands(case):
    rs = _rs(case, 22)
    C = case.C
    zmul = rs.choice([0.125, 0.5, 1.0, 1.25], C).astype(F32).reshape(1, C, 1, 1)
    xmul = rs.choice([0.125, 0.25, 1.0], C).astype(F32).reshape(1, C, 1, 1)
    z = (_levels(case, 23) - F32(1)) * zmul           # multiples of 1/8 in [-1.25, 2.5]
    x = (_levels(case, 24) - F32(1)) * xmul
    scale = rs.choice([-1.0, -0.5, 0.5, 1.0, 2.0], C).astype(F32)
    shift = (rs.randint(-8, 9, C) / 8.0).astype(F32)
    return dict(z=z, x=x, scale=scale, shift=shift)


def lazy_operands(case):
    """z, x [B, C, H, W] multiples of 1/8 in [-4, 4], scale [C] from {-1, -0.5, 0.5, 1, 2}, shift [C] multiples of 1/8"""
    return {k: v.copy() for k, v in _lazy_operands(case).items()}


def lazy_map(ops, dtype=F32):
    """relu(fma(scale, z, shift) + x) with every operation in ``dtype`` (exact in float32 for lazy_operands)"""
    s, h = ops["scale"].astype(dtype).reshape(1, -1, 1, 1), ops["shift"].astype(dtype).reshape(1, -1, 1, 1)
    y = (s * ops["z"].astype(dtype) + h) + ops["x"].astype(dtype)
    return np.maximum(y, dtype(0))


# ------------------------------------------------------------------------------------------------ gradients
def gradients(case, exact):
    """gout [n, C * PH * PW] (integers in [-8, 8] or standard_normal), mean [C] multiples of 1/8, invstd [C] from
    {0.5, 1, 2} (both exact operands in either mode: (zmax - mean) * invstd never rounds)"""
    rs = _rs(case, 31 + int(exact))
    shape = (case.n, case.C * case.PH * case.PW)
    gout = rs.randint(-8, 9, shape).astype(F32) if exact else rs.standard_normal(shape).astype(F32)
    mean = (rs.randint(-8, 9, case.C) / 8.0).astype(F32)
    invstd = rs.choice([0.5, 1.0, 2.0], case.C).astype(F32)
    return gout, mean, invstd


# ------------------------------------------------------------------------------------------------ references
def oracle_roipool(feat, rois, size):
    """oracle/roipool_ref.c on a [B, C, H, W] map; a box on a page outside the batch pools nothing (the C code would
    read outside the map: it is handed page 0 and its rows are overwritten) -> out, argmax [n, C, PH, PW] numpy"""
    B = feat.shape[0]
    good = good_page(rois, B)
    r = np.array(rois, F32)
    r[~good, 0] = 0
    out, arg = O.roi_pool_argmax(torch.from_numpy(np.ascontiguousarray(feat, F32)), torch.from_numpy(r), size, SCALE)
    out, arg = out.numpy().copy(), arg.numpy().copy()
    out[~good], arg[~good] = 0, -1
    return out, arg


def oracle_roipool_bwd(gout, rois, arg, B, H, W):
    """the oracle's sequential float32 scatter -> [B, C, H, W]"""
    n, C, PH, PW = arg.shape
    r = np.array(rois, F32)
    r[~good_page(rois, B), 0] = 0                     # (their argmax is -1 throughout)
    g = torch.from_numpy(np.ascontiguousarray(gout, F32).reshape(n, -1))
    gin = torch.empty(B, C, H, W)
    O._lib().oracle_roipool_bwd(O._fp(g), O._fp(torch.from_numpy(r)), O._fp(torch.from_numpy(np.ascontiguousarray(arg))),
                                n, B, C, H, W, PH, PW, O._fp(gin))
    return gin.numpy()


def scatter64(g, rois, arg, B, H, W):
    """float64 scatter of g [n, C, PH, PW] to the arg-max positions -> [B, C, H, W]"""
    n, C = arg.shape[:2]
    a = arg.reshape(n, C, -1)
    valid = a >= 0
    page = np.broadcast_to(np.asarray(rois)[:, 0].astype(np.int64).reshape(n, 1, 1), a.shape)[valid]
    chan = np.broadcast_to(np.arange(C).reshape(1, C, 1), a.shape)[valid]
    out = np.zeros((B, C, H * W), np.float64)
    np.add.at(out, (page, chan, a[valid]), np.asarray(g, np.float64).reshape(a.shape)[valid])
    return out.reshape(B, C, H, W)


def max_hits(rois, arg, B, H, W):
    """the largest number of contributions one map element receives"""
    return int(scatter64(np.ones(arg.shape), rois, arg, B, H, W).max())


def stat_sums64(gm, zmax, mean, invstd):
    """(sum g', sum g' * (zmax - mean) * invstd) over boxes and bins per channel in float64, and the magnitudes
    (sum |g'|, sum |g' * (zmax - mean) * invstd|); gm, zmax [n, C, PH, PW]"""
    n, C = gm.shape[:2]
    g = np.asarray(gm, np.float64).reshape(n, C, -1)
    t = (np.asarray(zmax, np.float64).reshape(n, C, -1) - mean.astype(np.float64).reshape(1, C, 1)) \
        * invstd.astype(np.float64).reshape(1, C, 1)
    return (g.sum((0, 2)), (g * t).sum((0, 2))), (np.abs(g).sum((0, 2)), np.abs(g * t).sum((0, 2)))


@functools.lru_cache(maxsize=None)
def forward_reference(name, lazy):
    """(map, rois, out, argmax) of a forward case from the oracle; shared between tests, not to be modified"""
    case = FWD_CASES[name]
    rois = boxes(case)
    feat = lazy_map(lazy_operands(case)) if lazy else plain_map(case)
    out, arg = oracle_roipool(feat, rois, (case.PH, case.PW))
    return feat, rois, out, arg


@functools.lru_cache(maxsize=None)
def backward_inputs(name):
    """What cova_roipool_fwd_bn leaves for the backward, from the oracle on the materialised lazy map:
    dict(rois, pooled, argmax, zmax [n, C, PH, PW]; zmax = z at the arg-max, 0 where there is none, as the forward writes)"""
    case = BWD_CASES[name]
    rois, ops = boxes(case), lazy_operands(case)
    pooled, arg = oracle_roipool(lazy_map(ops), rois, (case.PH, case.PW))
    n, C = arg.shape[:2]
    page = np.where(good_page(rois, case.B), rois[:, 0], 0).astype(np.int64).reshape(n, 1, 1, 1)
    chan = np.arange(C).reshape(1, C, 1, 1)
    zmax = np.where(arg >= 0, ops["z"].reshape(case.B, C, -1)[page, chan, np.maximum(arg, 0)], F32(0)).astype(F32)
    return dict(rois=rois, pooled=pooled, argmax=arg, zmax=zmax)


# ------------------------------------------------------------------------------------------------ RoIAlign
def align_boxes(a):
    """[n, 5]: the edge list, inverted boxes wider than one owner segment and taller than 4 rows, fill; for an exact
    case corners on multiples of 8 px (2 map pixels) with bins of 1, 2 or 4 map pixels, some inverted"""
    case = a.case
    rs = _rs(case, 41 + 2 * a.sr + a.aligned)
    H, W, PH, PW = case.H, case.W, case.PH, case.PW
    if a.exact:
        pool = []
        while len(pool) < case.n:
            bh, bw = 2.0 ** rs.randint(0, 3), 2.0 ** rs.randint(0, 3)
            if (PH * bh) % 2 or (PW * bw) % 2:
                continue
            x1, y1 = 2 * rs.randint(-2, W // 2 + 2), 2 * rs.randint(-2, H // 2 + 2)
            box = [4.0 * x1, 4.0 * y1, 4.0 * (x1 + PW * bw), 4.0 * (y1 + PH * bh)]
            if a.aligned and len(pool) % 5 == 4:      # inverted: negative bin sizes, still powers of two
                box = [box[2], box[3], box[0], box[1]]
            pool.append(box)
        if a.aligned and W > 2 * ROI_XW:              # inverted, wider than one owner segment and taller than 4 rows
            bw, bh = (64.0 if PW == 1 else 16.0), 4.0
            pool[3] = [4.0 * (8 + PW * bw), 4.0 * (2 + PH * bh), 32.0, 8.0]
    else:
        pool = edge_boxes(H, W) + [[4.0 * W - 8, 4.0 * H - 6, 20, 4], [4.0 * W + 30, 30, -10, 2], [70, 4.0 * H, 74, -8],
                                   [10.2, 10.1, 10.4, 10.3]]
        while len(pool) < case.n:
            x1, y1 = rs.uniform(-20, 4 * W + 10), rs.uniform(-12, 4 * H + 10)
            pool.append([x1, y1, x1 + rs.uniform(-40, 150), y1 + rs.uniform(-20, 40)])
    pool = pool[:case.n - 2] + [pool[0], pool[1]]
    rois = np.zeros((case.n, 5), F32)
    rois[:, 1:] = np.asarray(pool, F32)
    rois[:, 0] = rs.randint(0, case.B - 1, case.n)
    rois[case.n - 2, 0], rois[case.n - 1, 0] = BAD_PAGES[0], case.B + BAD_PAGES[1]
    return rois


def align_data(a):
    """(feat [B, C, H, W], gout [n, C * PH * PW]): small integers for an exact case, standard_normal otherwise"""
    case = a.case
    rs = _rs(case, 51 + 2 * a.sr + a.aligned)
    fs, gs = (case.B, case.C, case.H, case.W), (case.n, case.C * case.PH * case.PW)
    if a.exact:
        return _quantised(rs, fs), rs.randint(-8, 9, gs).astype(F32)
    return rs.standard_normal(fs).astype(F32), rs.standard_normal(gs).astype(F32)


def align_reference(feat, rois, gout, a):
    """O.roi_align and its autograd -> (out [n, C * PH * PW], gfeat [B, C, H, W]) as float32 numpy"""
    f = torch.from_numpy(np.ascontiguousarray(feat, F32)).requires_grad_(True)
    out = O.roi_align(f, torch.from_numpy(np.ascontiguousarray(rois, F32)), (a.case.PH, a.case.PW), SCALE, a.sr,
                      bool(a.aligned)).reshape(len(rois), -1)
    (out * torch.from_numpy(np.ascontiguousarray(gout, F32))).sum().backward()
    return out.detach().numpy(), f.grad.numpy()


def long_list():
    """The long-list case: (real [12, 5], index of each real box in the list of n = 2^18 + 1, feat, gout of the real
    boxes).  Real boxes sit at the front, the middle and the very last index, on both pages, pages unsorted; every
    other row carries page index B."""
    a = ALIGN_LONG
    case = a.case
    rs = _rs(case, 61)
    real = np.zeros((12, 5), F32)
    for i in range(12):
        bw, bh = 2.0 ** rs.randint(1, 4), 2.0 ** rs.randint(1, 3)
        x1, y1 = 2 * rs.randint(-1, case.W // 2), 2 * rs.randint(-1, case.H // 2)
        real[i] = [(i + i // 3) % case.B, 4.0 * x1, 4.0 * y1, 4.0 * (x1 + bw), 4.0 * (y1 + bh)]
    mid = case.n // 2
    index = np.array([0, 1, 2, 5, mid - 1, mid, mid + 1, mid + 300, case.n - 70, case.n - 3, case.n - 2, case.n - 1])
    feat = _quantised(rs, (case.B, case.C, case.H, case.W))
    gout = rs.randint(-8, 9, (12, case.C)).astype(F32)
    return real, index, feat, gout
