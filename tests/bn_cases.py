"""Case table, lattice operands and float64 references for BatchNorm and the stem's BatchNorm + ReLU + MaxPool:
csrc/bn.hip, csrc/bn1d.hip and csrc/bn_tail.h.  No GPU import: tests/test_bn_cases_cpu.py checks this file itself (the
forms the table reaches, the exactness of the operands, the references against torch in float64, and that the checkers
flag a set of seeded faults); tests/test_bn_paths_gpu.py runs the table on the kernels.

The ``*_form`` functions restate the HOST dispatch of the two files, each line citing the line it restates.  Alignment
is a base offset in floats from a 16-byte aligned allocation (``None`` = a NULL pointer), as in tests/head_cases.py.

Every operand lies on a lattice on which each correct f32 evaluation is exact -- in any summation order, with or
without FMA -- so the kernels are compared with ``mismatches`` (element for element) and not against a tolerance:
  statistics  x, dout, z integers in [-7, 7]; mean an integer in [-2, 2]; invstd in {1/4, 1/2, 1, 2}; act in
              {-1, -0.0, 0, 1}.  xhat is then a multiple of 1/4 with |xhat| <= 18, every term of a sum a multiple of 1/4
              of magnitude <= 196, and a chunk's sums are exact while 4 * 196 * rows < 2^24 (``exact_ok``).
  apply       scale = +-2^j, j in [-2, 2], one entry exactly 0; shift, residual, coef multiples of 1/8.
  pool        y a multiple of 1/2 in [-2, 2] (nine values: ties are dense); scale as above, shift a multiple of 1/2;
              dp an integer.
"""
import collections

import numpy as np
import torch
import torch.nn.functional as F

F32, F64 = np.float32, np.float64
EPS = float(F32(1e-5))                     # what the kernels receive: float32(1e-5) widened to double
MOMENTUM = F32(0.1)
SENTINEL = 7.0                             # = head_cases.CANARY: what output buffers hold before a launch


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ dispatch
def vec4_ok(off, ld):
    """common.h:169  a NULL pointer passes; otherwise 16-byte aligned and ld % 4 == 0"""
    return off is None or (off % 4 == 0 and ld % 4 == 0)


def pow2_cols(C):
    """bn.hip:24-29"""
    cb = 1
    while cb < C and cb < 256:
        cb <<= 1
    return cb


def rows_per_chunk(R, C):
    rpb = 256 // pow2_cols(C)              # bn.hip:623
    rows = cdiv(R, 2048)                   # bn.hip:624
    rows = max(rows, 64)                   # bn.hip:625
    return cdiv(rows, rpb) * rpb           # bn.hip:626


def num_chunks(R, C):
    return cdiv(R, rows_per_chunk(R, C))   # bn.hip:632


def ew_grid(n):
    return min(max(cdiv(n, 256), 1), 256 * 16)     # common.h:172-177


def pool_out(n):
    return (n + 2 - 3) // 2 + 1            # bn.hip:815


def pool_grid(B, H1, W1):
    return min(cdiv(B * pool_out(H1) * pool_out(W1) * 16, 256), 0x7fffffff)        # bn.hip:817-818


def pool_bwd_num_partials(B, H1, W1):
    return min(max(cdiv(B * H1 * W1, 16 * 64), 1), 4096)                           # bn.hip:827-829


def _generic(C):
    cb = pow2_cols(C)
    return ("generic", cb, 256 // cb, cdiv(C, cb))                                 # bn.hip:41-42, :652


def colstats_form(C, ld, off):
    if C == 64 and ld == 64 and vec4_ok(off, ld):                                  # bn.hip:653
        return "c64"
    return _generic(C)                                                             # bn.hip:660


def bwd_reduce_form(C, ldd, d_off, lda, a_off, ldz, z_off):
    if (C == 64 and ldd == 64 and ldz == 64 and (a_off is None or lda == 64) and vec4_ok(d_off, ldd)
            and vec4_ok(z_off, ldz) and vec4_ok(a_off, lda)):                      # bn.hip:746-747
        return "c64"
    return _generic(C)                                                             # bn.hip:753


def act_form(C, ldz, z_off, ldres, res_off, ldo, o_off, scale_off=0, shift_off=0):
    v4 = (C % 4 == 0 and vec4_ok(z_off, ldz) and vec4_ok(res_off, ldres) and vec4_ok(o_off, ldo)
          and vec4_ok(scale_off, 0) and vec4_ok(shift_off, 0))                     # bn.hip:700-701
    return 4 if v4 else 1                                                          # bn.hip:702-707


def bwd_apply_form(C, ldd, d_off, lda, a_off, ldz, z_off, lddz, dz_off, lddres, dres_off):
    v4 = (C % 4 == 0 and vec4_ok(d_off, ldd) and vec4_ok(a_off, lda) and vec4_ok(z_off, ldz)
          and vec4_ok(dz_off, lddz) and vec4_ok(dres_off, lddres))                 # bn.hip:792-793
    return 4 if v4 else 1                                                          # bn.hip:794-801


V4_SLICES = 512                            # bn1d.hip:158


def bn1d_fwd_form(option14, R, C, ldx, x_off, ldo, o_off, drop, ldd=0, d_off=0, mask_off=0):
    """mask_off in BYTES from a 4-byte aligned address"""
    v4 = (option14 != 0 and C % 4 == 0 and ldx % 4 == 0 and ldo % 4 == 0 and x_off % 4 == 0 and o_off % 4 == 0
          and (not drop or (ldd % 4 == 0 and d_off % 4 == 0 and mask_off % 4 == 0))
          and R <= 8 * V4_SLICES)                                                  # bn1d.hip:361-363
    if not v4:
        return ("slice", int(bool(drop)))                                          # bn1d.hip:377-385
    nr = 3 if R <= 3 * V4_SLICES else 6 if R <= 6 * V4_SLICES else 8               # bn1d.hip:370-372
    return ("v4", nr, int(bool(drop)))


def bn1d_bwd_form(option14, R, C, ldg, g_off, ldz, z_off, lddz, dz_off, lda, a_off, mask_off):
    """a_off None: no act; mask_off None: no Dropout mask (bytes otherwise)"""
    v4 = (option14 != 0 and C % 4 == 0 and ldg % 4 == 0 and ldz % 4 == 0 and lddz % 4 == 0 and g_off % 4 == 0
          and z_off % 4 == 0 and dz_off % 4 == 0 and (a_off is None or (lda % 4 == 0 and a_off % 4 == 0))
          and (mask_off is None or mask_off % 4 == 0) and R <= 6 * V4_SLICES)      # bn1d.hip:396-398
    drop = int(mask_off is not None)
    if not v4:
        return ("slice", drop)                                                     # bn1d.hip:410-416
    return ("v4", 3 if R <= 3 * V4_SLICES else 6, drop)                            # bn1d.hip:404-405


def colreduce_key(form):
    """a generic form with its column blocks counted as 1 or 2 (= two or more)"""
    return form if form == "c64" else form[:3] + (min(form[3], 2),)


ALL_COLREDUCE = ["c64"] + [("generic", cb, 256 // cb, 1) for cb in (1, 2, 4, 8, 16, 32, 64, 128, 256)] + \
                [("generic", 256, 1, 2)]
ALL_APPLY = [1, 4]
ALL_BN1D_FWD = [("slice", d) for d in (0, 1)] + [("v4", nr, d) for nr in (3, 6, 8) for d in (0, 1)]
ALL_BN1D_BWD = [("slice", d) for d in (0, 1)] + [("v4", nr, d) for nr in (3, 6) for d in (0, 1)]

# ------------------------------------------------------------------------------------------------ cases
OFF = 4                                    # floats of NaN in front of every aligned operand (place() fills them)

# statistics: x (and dout, z) [R, C] with leading dimension C + pad at OFF + off floats; act (MODE 1, if act) with its own
Stat = collections.namedtuple("Stat", "R C pad off act a_pad a_off")


def _st(R, C, pad=0, off=0, act=1, a_pad=None, a_off=None):
    return Stat(R, C, pad, off, act, pad if a_pad is None else a_pad, off if a_off is None else a_off)


def _one_row_last(C):
    return rows_per_chunk(1, C) + 1


STAT_CASES = collections.OrderedDict()
for _C in (1, 2, 3, 6, 12, 24, 33, 100, 200, 257):                                 # every CB; RPB = 256 .. 1; two column blocks
    STAT_CASES["stat-C%d-lastrow1" % _C] = _st(_one_row_last(_C), _C)
for _R in (1, 63, 64, 65):
    STAT_CASES["stat-C6-R%d" % _R] = _st(_R, 6, act=_R % 2)
    STAT_CASES["stat-c64-R%d" % _R] = _st(_R, 64, act=1 - _R % 2)
STAT_CASES.update([
    ("stat-C3-ld4", _st(65, 3, pad=1)),
    ("stat-C33-R63-ld40", _st(63, 33, pad=7)),
    ("stat-C64-ld68", _st(65, 64, pad=4)),
    ("stat-C64-off1", _st(65, 64, off=1)),
    ("stat-C64-act-ld68", _st(65, 64, a_pad=4)),                                   # forward c64, backward generic by act alone
    ("stat-C64-act-off1", _st(65, 64, a_off=1)),
    ("stat-C64-noact", _st(130, 64, act=0)),
    ("stat-C257-R1", _st(1, 257)),
    ("stat-C1710", _st(65, 1710)),
    ("stat-C1610-ld1710", _st(65, 1610, pad=100, act=0)),                          # comb[:, :1610] of the engine
    ("stat-c64-R131073", _st(131073, 64)),                                         # R > 2048 * 64: rows per chunk grow
    ("stat-C6-R131073", _st(131073, 6, pad=2)),
])

# apply / bwd-apply: z, out (dout, act, dz) at (pad, off); the residual (dres) at (r_pad, r_off)
Apply = collections.namedtuple("Apply", "R C pad off res r_pad r_off relu dres")


def _ap(R, C, pad=0, off=0, res=1, r_pad=None, r_off=None, relu=1, dres=1):
    return Apply(R, C, pad, off, res, pad if r_pad is None else r_pad, off if r_off is None else r_off, relu, dres)


APPLY_CASES = collections.OrderedDict([
    ("apply-v4-dense", _ap(7, 8)),
    ("apply-v4-c64", _ap(300, 64, relu=0, dres=0)),
    ("apply-v4-nores", _ap(9, 8, res=0, dres=0)),
    ("apply-v4-ld-pad4", _ap(9, 8, pad=4)),
    ("apply-v4-second-trip", _ap(16400, 256, res=0, dres=0)),                      # R * C / 4 > 4096 * 256
    ("apply-v1-C6", _ap(9, 6)),
    ("apply-v1-C1", _ap(5, 1, res=0, relu=0, dres=0)),
    ("apply-v1-C257", _ap(3, 257, relu=0)),
    ("apply-v1-ld9", _ap(9, 8, pad=1)),
    ("apply-v1-off1", _ap(9, 8, off=1, dres=0)),
    ("apply-v1-res-ld-alone", _ap(9, 8, r_pad=1)),
    ("apply-v1-res-off-alone", _ap(9, 8, r_off=1)),
    ("apply-v1-view-1610-of-1710", _ap(83, 1610, pad=100, res=0)),
    ("apply-v1-second-trip", _ap(16200, 65, res=0, dres=0)),                       # R * C > 4096 * 256
])

BITS_CASES = collections.OrderedDict(("bits-R%d-res%d" % (R, res), (R, res)) for R in (1, 7, 65537) for res in (0, 1))
ACT2_CASES = collections.OrderedDict(("act2-R%d-C%d-relu%d" % (R, C, relu), (R, C, relu))
                                     for R in (1, 8200) for C in (4, 128) for relu in (0, 1))

NPARTS = (1, 15, 16, 17, 127, 128, 129, 255, 256)
FIN_CASES = collections.OrderedDict(("fin-n%d-C%d" % (n, C), (n, C)) for n in NPARTS for C in (6, 64, 992))
FOLD_CASES = collections.OrderedDict(("fold-%d-%d-%d" % c, c) for c in ((257, 64, 128), (64, 64, 12), (5, 9, 1984),
                                                                        (300, 300, 128)))   # (nparts, group, width)

Pool = collections.namedtuple("Pool", "B H1 W1")
POOL_CASES = collections.OrderedDict(("pool-%dx%dx%d" % c, Pool(*c)) for c in (
    (1, 1, 1), (1, 1, 5), (1, 5, 1), (2, 2, 3), (1, 3, 2), (2, 13, 21), (1, 16, 18), (3, 16, 24), (3, 32, 24)))
TIE_CASES = ("pool-2x13x21", "pool-1x16x18")
PROBE_MAP = Pool(1, 7, 10)
# (iy, ix) of the probed pixel, by channel pair: corners, borders, interior; even and odd coordinates (one, two or four
# windows contain the pixel)
PROBE_PIXELS = ((0, 0), (0, 9), (6, 0), (6, 9), (0, 4), (3, 0), (6, 5), (2, 9), (2, 4), (3, 5), (4, 3), (1, 1))

# bn1d: x [R, C], every leading dimension C + pad.  Each case runs under option 14 = 0 and 1, ReLU on / off, Dropout
# (given mask) on / off.
Bn1d = collections.namedtuple("Bn1d", "R C pad")
BN1D_ROWS = (2, 1536, 1537, 3072, 3073, 4096, 4097)
BN1D_CASES = collections.OrderedDict(("bn1d-R%d-C%d-pad%d" % (R, C, pad), Bn1d(R, C, pad))
                                     for R in BN1D_ROWS for C in (8, 36) for pad in (0, 4))
BN1D_CASES["bn1d-R1537-C6-unaligned"] = Bn1d(1537, 6, 0)
BN1D_MODES = [(relu, drop) for relu in (0, 1) for drop in (0, 1)]
BN1D_P = 0.5                               # 1 / (1 - p) = 2: the Dropout scaling is exact

CASES = collections.OrderedDict()
for _t in (STAT_CASES, APPLY_CASES, BITS_CASES, ACT2_CASES, FIN_CASES, FOLD_CASES, POOL_CASES, BN1D_CASES):
    CASES.update(_t)


def stat_forms(c):
    """(forward form, backward-reduce form) of a statistics case"""
    ld, o = c.C + c.pad, OFF + c.off
    return (colstats_form(c.C, ld, o),
            bwd_reduce_form(c.C, ld, o, c.C + c.a_pad, OFF + c.a_off if c.act else None, ld, o))


def apply_forms(c):
    """(bn_act_fwd form, bn_bwd_apply form) of an apply case"""
    ld, o, ldr, orr = c.C + c.pad, OFF + c.off, c.C + c.r_pad, OFF + c.r_off
    return (act_form(c.C, ld, o, ldr, orr if c.res else None, ld, o),
            bwd_apply_form(c.C, ld, o, ld, o if c.relu else None, ld, o, ld, o, ldr, orr if c.dres else None))


def bn1d_forms(c, option14, relu, drop):
    ld = c.C + c.pad
    return (bn1d_fwd_form(option14, c.R, c.C, ld, OFF, ld, OFF, drop, ld, OFF, 0),
            bn1d_bwd_form(option14, c.R, c.C, ld, OFF, ld, OFF, ld, OFF, ld, OFF if relu else None, 0 if drop else None))


def exact_ok(c):
    """every chunk sum of a statistics case is an exact f32 number in any order: multiples of 1/4 below 2^24 / 4"""
    return 4 * 196 * rows_per_chunk(c.R, c.C) < 2 ** 24


# ------------------------------------------------------------------------------------------------ operands
def _rs(*key):
    seed = 0
    for k in key:
        seed = (seed * 10007 + int(k)) % (2 ** 31 - 1)
    return np.random.RandomState(seed)


def _ints(rs, shape, lim=7):
    return rs.randint(-lim, lim + 1, shape).astype(F32)


def _pow2(rs, n, lo=-2, hi=2, signed=True):
    v = np.ldexp(1.0, rs.randint(lo, hi + 1, n)).astype(F32)
    return v * rs.choice([-1.0, 1.0], n).astype(F32) if signed else v


def _eighths(rs, shape, lim):
    return (rs.randint(-lim, lim + 1, shape) / 8.0).astype(F32)


ACT_VALUES = np.array([-1.0, -0.0, 0.0, 1.0], F32)


def stat_operands(c):
    """x, dout, z, act [R, C]; mean, invstd [C].  With C >= 3 column 0 is constant and column 1 all zero; rows 0 and
    rows_per_chunk - 1 carry known non-zero terms in the last column (so that losing one of them shows)."""
    rs = _rs(11, c.R, c.C, c.pad, c.off)
    x, dout, z = _ints(rs, (c.R, c.C)), _ints(rs, (c.R, c.C)), _ints(rs, (c.R, c.C))
    act = ACT_VALUES[rs.randint(0, 4, (c.R, c.C))]
    mean, invstd = _ints(rs, c.C, 2), _pow2(rs, c.C, -2, 1, signed=False)
    if c.C >= 3:
        x[:, 0], z[:, 0] = 3.0, -2.0
        x[:, 1], dout[:, 1] = 0.0, 0.0
    for r in {0, min(rows_per_chunk(c.R, c.C), c.R) - 1}:
        x[r, -1], dout[r, -1], act[r, -1], z[r, -1] = 5.0, 3.0, 1.0, mean[-1] + 1.0
    return dict(x=x, dout=dout, z=z, act=act, mean=mean, invstd=invstd)


def apply_operands(R, C, seed=12):
    rs = _rs(seed, R, C)
    scale = _pow2(rs, C)
    if C >= 2:
        scale[C // 2] = 0.0
    return dict(z=_ints(rs, (R, C)), scale=scale, shift=_eighths(rs, C, 32), res=_eighths(rs, (R, C), 32),
                dout=_ints(rs, (R, C)), act=ACT_VALUES[rs.randint(0, 4, (R, C))], mean=_ints(rs, C, 2),
                invstd=_pow2(rs, C, -2, 1, signed=False), coef=_eighths(rs, (2, C), 16))


def fin_operands(nparts, C, rows=64):
    """Synthetic integer partial rows of `rows` data rows each.  fwd [nparts][2][C]: sums and sums of squares that some
    data could have produced (sumsq >= sum^2 / rows per chunk, so the variance is >= 0); column 0 is a constant 3, column
    1 all zero.  bwd: sums of dy (integers) and of dy * xhat (multiples of 1/4)."""
    rs = _rs(13, nparts, C)
    s = rs.randint(-7 * rows, 7 * rows + 1, (nparts, C)).astype(F64)
    lo = np.ceil(s * s / rows)
    q = lo + np.floor(rs.uniform(0, 1, (nparts, C)) * (49 * rows - lo))
    s[:, 0], q[:, 0] = 3.0 * rows, 9.0 * rows
    if C >= 2:
        s[:, 1], q[:, 1] = 0.0, 0.0
    fwd = np.stack([s, q], 1).astype(F32)
    bwd = np.stack([rs.randint(-7 * rows, 7 * rows + 1, (nparts, C)),
                    rs.randint(-4 * 126 * rows, 4 * 126 * rows + 1, (nparts, C)) / 4.0], 1).astype(F32)
    return dict(fwd=fwd, bwd=bwd, count=float(nparts * rows), gamma=_eighths(rs, C, 16), beta=_eighths(rs, C, 16),
                rm=_eighths(rs, C, 16), rv=np.abs(_eighths(rs, C, 16)) + F32(0.125), mean=_ints(rs, C, 2),
                invstd=_pow2(rs, C, -2, 1, signed=False), scale=_pow2(rs, C))


def fold_operands(nparts, width):
    return _ints(_rs(14, nparts, width), (nparts, width), 1000)


def pool_operands(c):
    """y [B, H1, W1, 64] multiples of 1/2 in [-2, 2]; per channel scale (+-2^j, one zero), shift (multiple of 1/2), mean
    (integer), invstd (power of two), coef (multiples of 1/8), abc (A = +-2^j, B and C multiples of 1/8); dp0
    [B, H2, W2, 64] integers (the caller masks them by out > 0)"""
    rs = _rs(15, c.B, c.H1, c.W1)
    scale = _pow2(rs, 64)
    scale[37] = 0.0
    abc = np.stack([_pow2(rs, 64), _eighths(rs, 64, 16), _eighths(rs, 64, 16)])
    return dict(y=(rs.randint(-4, 5, (c.B, c.H1, c.W1, 64)) / 2.0).astype(F32), scale=scale,
                shift=(rs.randint(-4, 5, 64) / 2.0).astype(F32), mean=_ints(rs, 64, 2),
                invstd=_pow2(rs, 64, -2, 1, signed=False), coef=_eighths(rs, (2, 64), 16), abc=abc,
                dp0=_ints(rs, (c.B, pool_out(c.H1), pool_out(c.W1), 64)))


PROBE_Y, PROBE_SCALE, PROBE_SHIFT = F32(1 + 2.0 ** -12), F32(1 + 2.0 ** -12), F32(-(1 + 2.0 ** -11))


def probe_operands():
    """The threshold probe on PROBE_MAP.  Even channels: y = scale = 1 + 2^-12 and shift = -(1 + 2^-11) at one pixel,
    y = 0 elsewhere; fma(y, scale, shift) = 2^-24 at the pixel, while the rounded product plus shift is 0.  Odd channels:
    scale and shift negated (-2^-24 at the pixel) and y = 2 elsewhere (-1): nothing is positive.  dp = 1 in the first
    window that contains the pixel, in every channel (the kernels take the decision themselves).  mean = the probed y
    (xhat = 0 there), invstd = 1, coef = (1/8, 0): dz is one rounding of scale * (dy - 1/8)."""
    c = PROBE_MAP
    H2, W2 = pool_out(c.H1), pool_out(c.W1)
    y = np.zeros((1, c.H1, c.W1, 64), F32)
    y[..., 1::2] = 2.0
    dp = np.zeros((1, H2, W2, 64), F32)
    pix = []
    for ch in range(64):
        iy, ix = PROBE_PIXELS[(ch // 2) % len(PROBE_PIXELS)]
        y[0, iy, ix, ch] = PROBE_Y
        oy, ox = windows_of(c, iy, ix)[0]
        dp[0, oy, ox, ch] = 1.0
        pix.append((iy, ix))
    sign = np.where(np.arange(64) % 2 == 0, 1.0, -1.0).astype(F32)
    coef = np.zeros((2, 64), F32)
    coef[0] = 0.125
    return dict(y=y, scale=sign * PROBE_SCALE, shift=sign * PROBE_SHIFT, mean=np.full(64, PROBE_Y, F32),
                invstd=np.ones(64, F32), coef=coef, dp=dp, pixels=pix)


def windows_of(c, iy, ix):
    """the (oy, ox) of the pooling windows that contain pixel (iy, ix), row-major"""
    H2, W2 = pool_out(c.H1), pool_out(c.W1)
    return [(oy, ox) for oy in range(H2) for ox in range(W2) if abs(iy - 2 * oy) <= 1 and abs(ix - 2 * ox) <= 1]


def bn1d_operands(c):
    """x [R, C] integers whose column means are integers: rows come in pairs (v, 2 m - v), an odd row count leaves one
    row at m.  Then mean is exact, z - mean is an integer, and every fp64 sum of the kernels is exact whatever its order,
    so the two kernel forms must agree bit for bit.  For the backward called on its own: lattice mean / invstd / scale."""
    rs = _rs(16, c.R, c.C, c.pad)
    m = _ints(rs, c.C, 1)
    half = rs.randint(-6, 7, (c.R // 2, c.C)).astype(F32)
    x = np.empty((c.R, c.C), F32)
    x[0:2 * (c.R // 2):2] = m + half
    x[1:2 * (c.R // 2):2] = m - half
    if c.R % 2:
        x[-1] = m
    x = x[rs.permutation(c.R)]
    return dict(x=x, col_mean=m, gamma=_eighths(rs, c.C, 16), beta=_eighths(rs, c.C, 16), rm=_eighths(rs, c.C, 16),
                rv=np.abs(_eighths(rs, c.C, 16)) + F32(0.125), keep=rs.randint(0, 2, (c.R, c.C)).astype(np.uint8),
                dout=_ints(rs, (c.R, c.C)), act=ACT_VALUES[rs.randint(0, 4, (c.R, c.C))], z=_ints(rs, (c.R, c.C)),
                mean=_ints(rs, c.C, 2), invstd=_pow2(rs, c.C, -2, 1, signed=False), scale=_pow2(rs, c.C))


# ------------------------------------------------------------------------------------------------ f32 arithmetic, restated
def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays: the product is exact in float64; the sum is rounded to ODD in float64 (TwoSum
    gives its error), after which the cast to float32 is the single correct rounding (Boldo & Melquiond, 2008)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32).astype(F64), np.asarray(b, F32).astype(F64),
                                  np.asarray(c, F32).astype(F64))
    p = a * b
    s = np.ascontiguousarray(p + c)
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def unfused32(a, b, c):
    """a * b + c with the product rounded to float32 first"""
    return (np.asarray(a, F32) * np.asarray(b, F32)).astype(F32) + np.asarray(c, F32)


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, F32))).astype(F64)


def within_ulps(got, ref, n=1, scale=None):
    """|got - ref| <= n f32 ulps of ref (or of ``scale``), element-wise -> bool array; a NaN is outside"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    return np.abs(got - ref) <= n * ulp32(ref if scale is None else scale)


def mismatches(got, ref):
    """number of elements of ``got`` that differ in value from ``ref`` (a NaN differs; -0.0 equals 0.0)"""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    ref = ref.detach().cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return int((~(got.astype(F64) == ref.astype(F64))).sum())


# ------------------------------------------------------------------------------------------------ references
def chunk_sums(a, rpc):
    """[R, C] -> [chunks, C]: sums over `rpc` consecutive rows"""
    return np.add.reduceat(np.asarray(a, F64), np.arange(0, a.shape[0], rpc), axis=0)


def relu_mask(act, fault=None):
    act = np.asarray(act)
    if fault == "negzero_positive":
        return (act > 0) | ((act == 0) & np.signbit(act))
    return act > 0


def stat_terms(o, mode, act=True, fault=None):
    """the two per-element terms a statistics kernel sums, float64 [R, C] each"""
    if mode == 0:
        x = o["x"].astype(F64)
        return x, x * x
    dy = o["dout"].astype(F64)
    if act:
        dy = dy * relu_mask(o["act"], fault)
    xh = (o["z"].astype(F64) - o["mean"].astype(F64)) * o["invstd"].astype(F64)
    return dy, dy * xh


def stat_partials(o, R, C, mode, act=True, fault=None):
    """partial [chunks][2][C] of cova_colstats (mode 0) / cova_bn_bwd_reduce (mode 1) in float64.  Faults: a row dropped
    from chunk 0; the last row of chunk 0 counted in chunk 1; the last column never written (it keeps the sentinel);
    act == -0.0 taken as positive."""
    rpc = rows_per_chunk(R, C)
    a, b = stat_terms(o, mode, act, fault)
    out = np.stack([chunk_sums(a, rpc), chunk_sums(b, rpc)], 1)
    if fault == "row_dropped":
        out[0, 0] -= a[0]
        out[0, 1] -= b[0]
    elif fault == "row_in_neighbour":
        r = rpc - 1
        out[0, 0] -= a[r]; out[0, 1] -= b[r]
        out[1, 0] += a[r]; out[1, 1] += b[r]
    elif fault == "last_column_skipped":
        out[:, :, -1] = SENTINEL
    return out


STAT_FAULTS = ("row_dropped", "row_in_neighbour", "last_column_skipped", "negzero_positive")


def stat_expressible(fault, c, mode):
    if fault == "row_in_neighbour":
        return num_chunks(c.R, c.C) >= 2
    if fault == "negzero_positive":
        return mode == 1 and bool(c.act) and c.R * c.C >= 32
    return True


def act_fwd_ref(o, res=True, relu=True):
    y = o["scale"].astype(F64) * o["z"].astype(F64) + o["shift"].astype(F64)
    if res:
        y = y + o["res"].astype(F64)
    return np.maximum(y, 0.0) if relu else y


def bwd_apply_ref(o, act=True, fault=None):
    """-> (dz, dy): dz = scale * (dy - c1 - xhat * c2), dy = dout * (act > 0)"""
    dy, dyxh = stat_terms(o, 1, act, fault)
    xh = (o["z"].astype(F64) - o["mean"].astype(F64)) * o["invstd"].astype(F64)
    coef = o["coef"].astype(F64)
    return o["scale"].astype(F64) * (dy - coef[0] - xh * coef[1]), dy


def pack_bits(out):
    """[R, 64] -> uint32 [R, 2]: bit k of word w = out[r, 32 w + k] > 0"""
    b = (np.asarray(out) > 0).reshape(out.shape[0], 2, 32).astype(np.uint64)
    return (b << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)


def act2_ref(a, b, relu):
    y = act_fwd_ref(a, res=False, relu=False) + act_fwd_ref(b, res=False, relu=False)
    return np.maximum(y, 0.0) if relu else y


def combine(partial, fault=None):
    """totals [2][C] of partial [nparts][2][C] in float64, as combine_partials (bn.hip:76-107) and bn_tail_run
    (bn_tail.h:108-137) form them: 16 slices, eight rows of a slice in flight, the index of a row past the end clamped to
    the trip's first row and its value not added.  fault "walk": that walk, row by row (the same totals); fault
    "clamped_row_for_last_valid": the last valid of the eight rows is read through the clamp (row p0) instead."""
    partial = np.asarray(partial, F64)
    n = partial.shape[0]
    if fault is None:
        return partial.sum(0)
    tot = np.zeros(partial.shape[1:], F64)
    for sl in range(16):
        for p0 in range(sl, n, 128):
            valid = [u for u in range(8) if p0 + 16 * u < n]
            for u in valid:
                tot += partial[p0 if fault == "clamped_row_for_last_valid" and u == valid[-1] else p0 + 16 * u]
    return tot


def finalize_fwd_ref(tot, count, gamma, beta, rm, rv, dt=F32):
    """bn_fwd_channel_v (bn_tail.h:14-33) from the fp64 totals [2][C], with the kernel's float casts (dt = float32) or
    without any (float64, for the comparison with torch).  shift and the running statistics are given as the kernel
    writes them without contraction; ``shift_of`` gives both forms from the kernel's own scale."""
    gamma, beta, rm, rv = (np.asarray(v, dt) for v in (gamma, beta, rm, rv))
    mu = tot[0] / count
    var = np.maximum(tot[1] / count - mu * mu, 0.0)
    invstd = (1.0 / np.sqrt(var + EPS)).astype(dt)
    scale = gamma * invstd
    mean = mu.astype(dt)
    unbiased = var * count / (count - 1.0) if count > 1.0 else var
    mom = dt(MOMENTUM)
    return dict(mean=mean, invstd=invstd, scale=scale, shift=beta - mean * scale, var=var,
                running_mean=(dt(1) - mom) * rm + mom * mean, running_var=(dt(1) - mom) * rv + mom * unbiased.astype(dt))


def shift_of(beta, mean, scale):
    """the two correct f32 values of beta - mean * scale: product rounded first, and contracted to one fma"""
    mean, scale, beta = np.asarray(mean, F32), np.asarray(scale, F32), np.asarray(beta, F32)
    return beta - (mean * scale).astype(F32), fma32(-mean, scale, beta)


INVSTD_OF_ZERO_VAR = F32(1.0 / np.sqrt(F64(F32(1e-5))))


def finalize_bwd_ref(tot, count, mean=None, invstd=None, scale=None, dt=F32):
    """bn_finalize_bwd_kernel (bn.hip:217-231) and bn_bwd_abc_channel_v (bn_tail.h:45-55)"""
    c1, c2 = tot[0] / count, tot[1] / count
    r = dict(dbeta=tot[0].astype(dt), dgamma=tot[1].astype(dt), coef=np.stack([c1, c2]).astype(dt))
    if mean is not None:
        mu, is_, sc = (np.asarray(v, dt).astype(F64) for v in (mean, invstd, scale))
        r["abc"] = np.stack([sc, -sc * is_ * c2, sc * (mu * is_ * c2 - c1)]).astype(dt)
    return r


def fold_ref(partial, group, fault=None):
    """cova_partials_fold: sums of `group` consecutive rows; fault: groups of group + 1 rows"""
    if fault == "group_off_by_one":
        n = partial.shape[0]
        return np.stack([np.asarray(partial[p:min(p + group + 1, n)], F64).sum(0) for p in range(0, n, group)])
    return chunk_sums(partial, group)


# ---- pool
def pool_t(y, scale, shift, fused=True):
    """the pre-activation the three pool kernels decide on, float32"""
    return fma32(y, scale, shift) if fused else unfused32(y, scale, shift)


def pool_fwd_ref(y, scale, shift):
    """-> out, idx (window code ky * 3 + kx of the first maximum), ymax through F.max_pool2d on the CPU in float64"""
    B, H1, W1, C = y.shape
    a = np.maximum(pool_t(y, scale, shift).astype(F64), 0.0)
    out, flat = F.max_pool2d(torch.from_numpy(a).permute(0, 3, 1, 2).contiguous(), 3, 2, 1, return_indices=True)
    out, flat = out.permute(0, 2, 3, 1).numpy(), flat.permute(0, 2, 3, 1).numpy()
    iy, ix = flat // W1, flat % W1
    oy = np.arange(out.shape[1]).reshape(1, -1, 1, 1)
    ox = np.arange(out.shape[2]).reshape(1, 1, -1, 1)
    ky, kx = iy - (2 * oy - 1), ix - (2 * ox - 1)
    assert ky.min() >= 0 and ky.max() <= 2 and kx.min() >= 0 and kx.max() <= 2
    b = np.arange(B).reshape(-1, 1, 1, 1)
    ch = np.arange(C).reshape(1, 1, 1, -1)
    return out.astype(F32), (ky * 3 + kx).astype(np.uint8), y[b, iy, ix, ch]


def _windows(a, fill):
    """[B, H1, W1, C] -> [B, H2, W2, 9, C], positions in the padding = fill"""
    B, H1, W1, C = a.shape
    H2, W2 = pool_out(H1), pool_out(W1)
    p = np.full((B, 2 * H2 + 1, 2 * W2 + 1, C), fill, a.dtype)
    p[:, 1:H1 + 1, 1:W1 + 1] = a
    return np.stack([p[:, ky:ky + 2 * H2:2, kx:kx + 2 * W2:2] for ky in range(3) for kx in range(3)], 3)


POOL_FAULTS = ("last_max", "ge", "pad_zero", "unfused")


def pool_fwd_emulate(y, scale, shift, fault=None):
    """The forward kernel's scan, window by window (-> out, idx, ymax, and the [.., 9, C] candidates with the padding at
    -inf).  Faults: the last maximum kept; `>=` in place of `>`; the padding a candidate of value 0; the pre-activation
    as a rounded product plus shift."""
    t = pool_t(y, scale, shift, fused=fault != "unfused")
    a = _windows(np.maximum(t, F32(0)), F32(0))
    yw = _windows(np.asarray(y, F32), F32(0))
    valid = _windows(np.ones(y.shape, bool), False)
    if fault == "pad_zero":
        valid = np.ones_like(valid)
    m = np.full(a[:, :, :, 0].shape, -np.inf, F32)
    idx = np.zeros(m.shape, np.uint8)
    ym = np.zeros(m.shape, F32)
    for k in (range(8, -1, -1) if fault == "last_max" else range(9)):
        upd = valid[:, :, :, k] & ((a[:, :, :, k] >= m) if fault == "ge" else (a[:, :, :, k] > m))
        m, idx, ym = np.where(upd, a[:, :, :, k], m), np.where(upd, np.uint8(k), idx), np.where(upd, yw[:, :, :, k], ym)
    return m, idx, ym, np.where(_windows(np.ones(y.shape, bool), False), a, -np.inf)


def tie_density(y, scale, shift):
    """-> (fraction of windows whose POSITIVE maximum is taken at two or more positions, fraction of windows with no
    positive value)"""
    out, _, _, cand = pool_fwd_emulate(y, scale, shift)
    tied = ((cand == out[:, :, :, None]).sum(3) >= 2) & (out > 0)
    return float(tied.mean()), float((out == 0).mean())


def pool_route(dp, idx, H1, W1):
    """scatter dp [B, H2, W2, C] to the pixel each window's code points at -> [B, H1, W1, C] float64"""
    B, H2, W2, C = dp.shape
    b, oy, ox, ch = np.meshgrid(np.arange(B), np.arange(H2), np.arange(W2), np.arange(C), indexing="ij")
    iy, ix = 2 * oy - 1 + idx // 3, 2 * ox - 1 + idx % 3
    g = np.zeros((B, H1, W1, C), F64)
    np.add.at(g, (b, iy, ix, ch), np.asarray(dp, F64))
    return g


def pool_bwd_ref(o, dp, idx, fused=True):
    """-> dy [B, H1, W1, 64] (routed, masked by the pre-activation), totals [2][64] (sum dy, sum dy * xhat), dz"""
    y = o["y"]
    dy = pool_route(dp, idx, y.shape[1], y.shape[2]) * (pool_t(y, o["scale"], o["shift"], fused) > 0)
    xh = (y.astype(F64) - o["mean"].astype(F64)) * o["invstd"].astype(F64)
    coef = o["coef"].astype(F64)
    dz = o["scale"].astype(F64) * (dy - coef[0] - xh * coef[1])
    return dy, np.stack([dy.sum((0, 1, 2)), (dy * xh).sum((0, 1, 2))]), dz


def pool_dy1_ref(dp, idx, y, abc):
    abc = abc.astype(F64)
    return abc[0] * pool_route(dp, idx, y.shape[1], y.shape[2]) + abc[1] * y.astype(F64) + abc[2]


# ---- bn1d
def bn1d_fwd_ref(o, R):
    """finalize_fwd_ref on the exact column sums of o["x"]"""
    x = o["x"].astype(F64)
    return finalize_fwd_ref(np.stack([x.sum(0), (x * x).sum(0)]), float(R), o["gamma"], o["beta"], o["rm"], o["rv"])


def bn1d_apply_ref(x, scale, shift, relu, keep=None):
    """out = fmaf(scale, x, shift) (ReLU) and dropped = out * keep * 2, from the scale / shift a kernel returned"""
    y = fma32(scale, x, shift)
    if relu:
        y = np.maximum(y, F32(0))
    return y, None if keep is None else y * keep.astype(F32) * F32(2)


def bn1d_bwd_ref(o, R, relu, drop):
    """cova_bn1d_bwd on the lattice mean / invstd / scale -> dict(dbeta, dgamma: exact sums; dz, colsum: float64, with
    the magnitudes dz_mag / colsum_mag their f32 evaluation's bound scales with)"""
    dy = o["dout"].astype(F64)
    if drop:
        dy = dy * o["keep"] * 2.0
    if relu:
        dy = dy * relu_mask(o["act"])
    xh = (o["z"].astype(F64) - o["mean"].astype(F64)) * o["invstd"].astype(F64)
    s1, s2 = dy.sum(0), (dy * xh).sum(0)
    c1, c2 = (s1 / R).astype(F32).astype(F64), (s2 / R).astype(F32).astype(F64)
    sc = o["scale"].astype(F64)
    dz = sc * (dy - c1 - xh * c2)
    dz_mag = np.abs(sc) * (np.abs(dy) + np.abs(c1) + np.abs(xh * c2))
    rep = lambda v: v.astype(F32).astype(F64) == v
    # where dy - c1, xhat * c2 and their difference are f32 numbers, every f32 evaluation (fused or not) gives dz itself
    exact = rep(dy - c1) & rep(xh * c2) & rep(dy - c1 - xh * c2)
    return dict(dbeta=s1.astype(F32), dgamma=s2.astype(F32), dz=dz, dz_mag=dz_mag, dz_exact=exact, colsum=dz.sum(0),
                colsum_mag=dz_mag.sum(0))
