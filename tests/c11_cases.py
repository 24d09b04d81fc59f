"""Case table, lattice operands, float64 references and checkers for the 1x1 convolution family of the ResNet-50
extension: csrc/conv1x1.hip (conv1x1_kernel, conv1x1_wgrad_kernel and their reduce) and csrc/conv1x1_lin.hip
(conv1x1_vprod_kernel, lin_bnsums_kernel, lin_finish_kernel).  No GPU import: tests/test_c11_cases_cpu.py checks this
file itself (the forms and walk paths the table reaches, the exactness of the operands, the mask shares, the references
against a tile-by-tile evaluation, and that the checkers flag a set of seeded faults); tests/test_c11_paths_gpu.py runs
the table on the kernels.

``*_form`` restate the HOST dispatch, each line citing the line of conv1x1.hip it restates; ``*Walk`` restate how the
kernels divide the rows among blocks, waves and trips, from the kernels' own constants.

Every operand lies on a lattice on which each correct f32 evaluation is exact -- in any summation order, with FMA or
without, on the bf16-split path (every value is ONE bf16 piece: at most 8 significant bits) or the f32 MFMA, per tile
or carried across tiles:
  maps        in, in2, dz, dz2, v, act, z, z2: integers in [-3, 3]; the mask map `act` with -0.0 and +0.0 for its zeros
  weights     integers in [-2, 2] ([-1, 1] behind 256 input channels, where a forward's sum of y^2 would outgrow 2^24)
  prologues   A = +-{1/2, 1, 2}, B = +-{1/2, 1}, C a non-zero multiple of 1/2 up to 3/2: values are multiples of 1/2, |.| <= 10.5
              (a forward that sums y^2 behind a prologue: maps in [-2, 2] and A = +-{1/2, 1}; behind the ReLU the
              operand has one sign, y a per-channel offset, and sum y^2 is the budget that comes nearest to 2^24)
  epilogues   addend, cvec multiples of 1/2; mean, mean2 integers in [-2, 2]; invstd, invstd2 in {1/2, 1, 2};
              mask_scale = +-{1/2, 1, 2}, mask_shift = -mask_scale * z0 with z0 in [-1, 1]: 1/7 of the decisions are
              exactly 0.  Channel FMA_CH of a `fma` mask carries the one off-lattice triple on which the fused and the
              unfused decision differ (fmaf = 2^-24 > 0, rounded product + shift = 0); its xhat stays a multiple of 2^-4.
``exact_ok`` states the condition: for every accumulated quantity the sum of the absolute values of its terms, in units
of the quantity's lattice quantum, is below 2^24."""
import collections

import numpy as np

import bn_cases as BC

F32, F64 = np.float32, np.float64
CUS = 256                                  # compute units of the MI355X (the GPU test asserts the grids it derives from this)
BAD_ARG = 10001                            # common.h:12
SHAPES = ((64, 64), (64, 256), (256, 64))  # (Cin, Cout) of cova_conv1x1; (Ci, Co) of the weight gradient
TILE, NW = 32, 8                           # rows per wave tile, waves per block (conv1x1.hip:152-153, :753)
FMA_CH = 5


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ dispatch restated
Form = collections.namedtuple("Form", "kernel cin cout pro epi add mask_act x2 ext side")


def _c11(cin, cout, pro, epi, add=0, mask_act=0, x2=0, ext=0, side=0):
    return Form("c11", cin, cout, pro, epi, int(bool(add)), int(bool(mask_act)), int(bool(x2)), ext, side)


def launch_form(cin, cout, pro, epi, add, mask_act, x2, side=False):
    """launch_c11<CIN, COUT> (conv1x1.hip:745-802)"""
    if side:                                                                       # :757
        if cin != 256 or pro != 2 or epi > 1:                                      # :758-759, :768
            return BAD_ARG
        return _c11(256, cout, 2, epi, side=1)                                     # :760-766
    if epi in (0, 1):
        return _c11(cin, cout, pro, epi)                                           # :770-779
    if pro != 2:                                                                   # :781
        return BAD_ARG
    if epi == 3:                                                                   # :782
        if cout != 256 or not mask_act or x2:                                      # :783-784, :788
            return BAD_ARG
        return _c11(cin, cout, 2, 3, add, 1)                                       # :785-786
    if add:                                                                        # :790
        if mask_act:
            return _c11(cin, cout, 2, 2, 1, 1, x2)                                 # :791-794
        if x2:                                                                     # :795
            return BAD_ARG
        return _c11(cin, cout, 2, 2, 1)                                            # :796
    if x2:                                                                         # :798
        return BAD_ARG
    return _c11(cin, cout, 2, 2, 0, mask_act)                                      # :799-800


def conv1x1_form(cin, cout, R=1, in2=0, abc=0, addend=0, act=0, act_bits=0, msc=0, z=0, mean=0, z2=0, mean2=0, part=0,
                 need=1):
    """cova_conv1x1 (conv1x1.hip:826-862) by which pointers are given: msc = mask_scale and mask_shift, mean = mean and
    invstd, mean2 = mean2, invstd2 and stat_part2, need = in, w and out"""
    if not need or R <= 0:                                                         # :833
        return BAD_ARG
    if in2 and not abc:                                                            # :834
        return BAD_ARG
    if act_bits and z:                                                             # :835
        return BAD_ARG
    pro = 0 if not abc else (2 if in2 else 1)                                      # :836
    if z:
        if not (mean and part and (act or msc)):                                   # :839
            return BAD_ARG
        if z2 and not mean2:                                                       # :840
            return BAD_ARG
        epi = 2
    elif act or act_bits:
        if z2 or part or cout != 256 or (act and act_bits):                        # :843
            return BAD_ARG
        epi = 3
    else:
        if addend or z2:                                                           # :846
            return BAD_ARG
        epi = 1 if part else 0                                                     # :847
    if (cin, cout) not in SHAPES:                                                  # :855-859
        return BAD_ARG
    return launch_form(cin, cout, pro, epi, addend, act or act_bits, z2)           # :852, :856-858


def materialize_form(part, given=1, R=1):
    """cova_conv1x1_materialize (conv1x1.hip:870-882); side_bits is a runtime pointer (:415)"""
    if not given or R <= 0:                                                        # :874
        return BAD_ARG
    return launch_form(256, 64, 2, 1 if part else 0, 0, 0, 0, side=True)           # :878


def lin_dgrad_form(addend, given=1, R=1):
    """cova_conv1x1_lin_dgrad (conv1x1.hip:897-916)"""
    if not given or R <= 0:                                                        # :903-904
        return BAD_ARG
    return _c11(256, 64, 1, 2, addend, 0, 0, ext=1)                                # :910-913


def wgrad_form(co, ci, dz2=0, dz_abc=0, act_abc=0, R=1, need=1):
    """cova_conv1x1_wgrad (conv1x1.hip:927-955); act_relu is a runtime switch (:651)"""
    if not need or R <= 0:                                                         # :931
        return BAD_ARG
    if dz_abc and not dz2:                                                         # :932
        return BAD_ARG
    if (ci, co) not in SHAPES:                                                     # :945-948
        return BAD_ARG
    return ("wgrad", co, ci, int(bool(dz_abc)), int(bool(act_abc)))                # :937, :940-943


VPROD_FORM = ("vprod",)                    # conv1x1_lin.hip:305: one instantiation; act_abc and act_relu at run time (:53, :72)


def derived(f):
    """the flags conv1x1_kernel derives from its template arguments"""
    bf = not (f.epi == 2 and f.cout == 256)                                        # :91
    prefetch = not (f.epi in (2, 3) and f.cout == 256)                             # :312
    tr = f.epi == 3 and f.cout == 256 and not f.ext                                # :317
    return dict(BF=bf, PREFETCH=prefetch, TR=tr, EARLY=bf and tr)                  # :321


EPI2_FLAGS = ((1, 1, 1), (1, 1, 0), (1, 0, 0), (0, 1, 0), (0, 0, 0))              # (add, mask_act, x2) of launch_c11
ALL_C11 = [_c11(ci, co, pro, epi) for ci, co in SHAPES for epi in (0, 1) for pro in (0, 1, 2)] + \
          [_c11(ci, co, 2, 2, *f) for ci, co in SHAPES for f in EPI2_FLAGS] + \
          [_c11(64, 256, 2, 3, add, 1) for add in (0, 1)] + \
          [_c11(256, 64, 2, epi, side=1) for epi in (0, 1)] + \
          [_c11(256, 64, 1, 2, add, ext=1) for add in (0, 1)]
ALL_WGRAD = [("wgrad", co, ci, pz, pa) for ci, co in SHAPES for pz in (0, 1) for pa in (0, 1)]
ALL_FORMS = ALL_C11 + ALL_WGRAD + [VPROD_FORM]

# refused argument combinations: (entry, keyword arguments of its *_form).  The GPU test builds the call from these.
REFUSALS = [
    ("conv1x1", dict(cin=64, cout=64, R=0)),
    ("conv1x1", dict(cin=64, cout=64, need=0)),
    ("conv1x1", dict(cin=64, cout=64, in2=1)),                                     # in2 without a table
    ("conv1x1", dict(cin=64, cout=256, in2=1, abc=1, act_bits=1, z=1, mean=1, part=1)),
    ("conv1x1", dict(cin=64, cout=64, in2=1, abc=1, z=1, mean=1, part=1)),          # sums without a mask source
    ("conv1x1", dict(cin=64, cout=64, in2=1, abc=1, z=1, act=1, part=1)),           # ... without mean / invstd
    ("conv1x1", dict(cin=64, cout=64, in2=1, abc=1, z=1, act=1, mean=1)),           # ... without a buffer for them
    ("conv1x1", dict(cin=64, cout=64, in2=1, abc=1, addend=1, z=1, act=1, mean=1, part=1, z2=1)),
    ("conv1x1", dict(cin=256, cout=64, in2=1, abc=1, act=1)),                       # sum-free gradient: 256 outputs only
    ("conv1x1", dict(cin=64, cout=256, in2=1, abc=1, act=1, act_bits=1)),
    ("conv1x1", dict(cin=64, cout=256, in2=1, abc=1, act=1, part=1)),
    ("conv1x1", dict(cin=64, cout=256, in2=1, abc=1, act=1, z2=1, mean2=1)),
    ("conv1x1", dict(cin=64, cout=64, addend=1)),
    ("conv1x1", dict(cin=64, cout=64, z2=1, mean2=1)),
    ("conv1x1", dict(cin=256, cout=256)),
    ("conv1x1", dict(cin=128, cout=64)),
    ("conv1x1", dict(cin=64, cout=64, abc=1, z=1, act=1, mean=1, part=1)),          # a data gradient needs both inputs (:781)
    ("conv1x1", dict(cin=64, cout=256, abc=1, act=1)),                              # (:781 on the sum-free form)
    ("conv1x1", dict(cin=64, cout=64, in2=1, abc=1, z=1, msc=1, mean=1, part=1, addend=1, z2=1, mean2=1)),   # :795
    ("conv1x1", dict(cin=64, cout=64, in2=1, abc=1, z=1, act=1, mean=1, part=1, z2=1, mean2=1)),             # :798
    ("materialize", dict(part=1, given=0)),
    ("materialize", dict(part=0, R=0)),
    ("lin_dgrad", dict(addend=0, given=0)),
    ("lin_dgrad", dict(addend=1, R=0)),
    ("wgrad", dict(co=64, ci=64, dz_abc=1)),
    ("wgrad", dict(co=256, ci=256)),
    ("wgrad", dict(co=64, ci=64, R=0)),
    ("wgrad", dict(co=64, ci=64, need=0)),
]
FORM_OF = dict(conv1x1=conv1x1_form, materialize=materialize_form, lin_dgrad=lin_dgrad_form, wgrad=wgrad_form,
               vprod=lambda: VPROD_FORM)


def form(entry, **kw):
    """the instantiation the host code of ``entry`` selects for the pointers given (or BAD_ARG)"""
    return FORM_OF[entry](**kw)


# ------------------------------------------------------------------------------------------------ the walks restated
def persistent_grid(want, blocks_per_cu, cap=0, cus=CUS):
    g = min(want, cus * blocks_per_cu)                                             # conv.hip:1413
    return min(g, cap) if cap > 0 else g                                           # conv.hip:1414-1415


class C11Walk:
    """conv1x1_kernel: 32-row tiles; wave w of block b takes tiles 8 b + w, + 8 grid, ... (conv1x1.hip:152-153, :324-327)"""

    def __init__(self, R, cap=0, cus=CUS):
        self.R, self.cap = R, cap
        self.ntiles = cdiv(R, TILE)                                                # :152
        self.grid = persistent_grid(min(cdiv(self.ntiles, NW), 1 << 30), 1, cap, cus)     # :804-808
        self.stride = NW * self.grid                                               # :153
        self.ragged = self.ntiles - 1 if R % TILE else None

    def tiles_of(self, b, w):
        return list(range(b * NW + w, self.ntiles, self.stride))

    def owner(self, tile):
        """-> (block, wave, trip)"""
        first = tile % self.stride
        return first // NW, first % NW, tile // self.stride

    def rows_of_block(self, b):
        """bool [R]: the rows whose tile block b owns"""
        t = np.arange(self.R) // TILE
        return (t % self.stride) // NW == b

    def paths(self):
        p = set()
        trips = [[len(self.tiles_of(b, w)) for w in range(NW)] for b in range(self.grid)]
        for b, row in enumerate(trips):
            p.add("even-block" if b % 2 == 0 else "odd-block")
            p.update({0: "wave-no-tile", 1: "wave-one-tile", 2: "wave-two-trips"}.get(n, "wave-3+-trips") for n in row)
            if max(row) >= 2 and min(row) < max(row):
                p.add("last-trip-some-waves")
        if len({max(r) for r in trips}) > 1 or len({sum(r) for r in trips}) > 1:
            p.add("blocks-differ")
        p.update("even-tile" if t % 2 == 0 else "odd-tile" for t in range(self.ntiles))
        if self.ragged is not None:
            b, w, trip = self.owner(self.ragged)
            p.add("ragged-first-trip" if trip == 0 else "ragged-later-trip")
            p.add("ragged-even-tile" if self.ragged % 2 == 0 else "ragged-odd-tile")
            if trip and b % 2:
                p.add("ragged-later-trip-odd-block")
        if self.R == 1:
            p.add("one-row")
        return p


C11_REQUIRED = {"wave-no-tile", "wave-one-tile", "wave-3+-trips", "ragged-first-trip", "ragged-later-trip",
                "last-trip-some-waves", "blocks-differ", "even-tile", "odd-tile", "even-block", "odd-block", "one-row"}


class WgradWalk:
    """conv1x1_wgrad_kernel: pixel pairs in contiguous per-block ranges, batches of 8 pairs; with one 64 x 64 unit the four
    waves interleave the batches of the range, with four units every wave walks all of them (conv1x1.hip:621-695)"""
    U = 8                                                                          # :626

    def __init__(self, R, units, cap=0, cus=CUS):
        self.R, self.units, self.cap = R, units, cap
        self.npairs = (R + 1) // 2                                                 # :621
        self.want = cdiv(self.npairs, 64)                                          # :934
        self.grid = persistent_grid(min(self.want, 1 << 30), 2, cap, cus)          # :935
        self.per = cdiv(self.npairs, self.grid)                                    # :622

    def block(self, b):
        """-> (s_lo, s_hi, [per wave: (full batches, first pair of the tail batch or None, its valid pixel rows)])"""
        lo = b * self.per                                                          # :623
        hi = min(lo + self.per, self.npairs)                                       # :624-625
        full_hi = min(hi, self.R // 2) if 2 * hi > self.R else hi                  # :666-667
        wstep = 4 if self.units == 1 else 1                                        # :627
        waves = []
        for w in range(4):
            s0 = lo + (w if self.units == 1 else 0) * self.U                       # :628, :668
            nfull = 0
            while s0 + self.U <= full_hi:                                          # :670
                nfull, s0 = nfull + 1, s0 + wstep * self.U
            tail = [r for sp in range(s0, min(s0 + self.U, hi)) for r in (2 * sp, 2 * sp + 1) if r < self.R]   # :683-688
            waves.append((nfull, s0 if s0 < hi else None, tail))
        return lo, hi, waves

    def tail_rows(self):
        """the pixel rows that go through the clamped, predicated tail loop (once each: per unit, one wave owns them)"""
        rows = []
        for b in range(self.grid):
            _, _, waves = self.block(b)
            seen = set()
            for nfull, s0, tail in waves:
                if s0 is not None and s0 not in seen:
                    rows += tail
                    seen.add(s0)
        return rows

    def paths(self):
        p = set()
        per_block = []
        for b in range(self.grid):
            lo, hi, waves = self.block(b)
            p.add("even-block" if b % 2 == 0 else "odd-block")
            if hi <= lo:
                p.add("empty-block")
            counts = []
            for nfull, s0, tail in waves:
                n = nfull + (s0 is not None)
                counts.append(n)
                p.add({0: "wave-no-batch", 1: "wave-one-batch", 2: "wave-two-batches"}.get(n, "wave-3+-batches"))
                if s0 is not None:
                    p.add("tail-first-trip" if nfull == 0 else "tail-later-trip")
                    if len(tail) % 2:
                        p.add("half-pair")
                    if len(tail) < 2 * self.U:
                        p.add("tail-short")
                if nfull >= 2:
                    p.add("second-buffer")
            if max(counts) >= 2 and min(counts) < max(counts):
                p.add("last-trip-some-waves")
            per_block.append(tuple(counts))
        if len(set(per_block)) > 1:
            p.add("blocks-differ")
        if self.R == 1:
            p.add("one-row")
        return p


WGRAD_REQUIRED = {1: {"wave-no-batch", "wave-one-batch", "wave-3+-batches", "tail-first-trip", "tail-later-trip",
                      "last-trip-some-waves", "blocks-differ", "even-block", "odd-block", "one-row", "half-pair",
                      "second-buffer"},
                  4: {"wave-one-batch", "wave-3+-batches", "tail-first-trip", "tail-later-trip", "blocks-differ",
                      "even-block", "odd-block", "one-row", "half-pair", "second-buffer"}}


class VprodWalk:
    """conv1x1_vprod_kernel: K-steps of 16 rows in contiguous per-block ranges; wave (step & 3) takes the step's sums of
    a and its Gram quadrant; odd blocks run negated (conv1x1_lin.hip:74-83, :97, :156-173)"""

    def __init__(self, R, cap=0, cus=CUS):
        self.R, self.cap = R, cap
        self.nsteps = cdiv(R, 16)                                                  # :79
        self.grid = persistent_grid(min(cdiv((R + 1) // 2, 64), 1 << 30), 2, cap, cus)    # :276-280
        self.per = cdiv(self.nsteps, self.grid)                                    # :80

    def block(self, b):
        """-> (k_lo, k_hi, k_full, ragged): full steps [k_lo, k_full), then the ragged one at k_full"""
        lo = b * self.per                                                          # :81
        hi = min(lo + self.per, self.nsteps)                                       # :82-83
        full = min(self.R // 16, hi)                                               # :156-157
        return lo, hi, full, full < hi and full >= lo                              # :163

    def paths(self):
        p = set()
        counts = []
        for b in range(self.grid):
            lo, hi, full, ragged = self.block(b)
            p.add("even-block" if b % 2 == 0 else "odd-block")
            n = max(hi - lo, 0)
            counts.append(n)
            p.add({0: "empty-block", 1: "block-one-step", 2: "block-two-steps"}.get(n, "block-3+-steps"))
            if n and n < 4:
                p.add("wave-no-step")
            if n % 4:
                p.add("last-round-some-waves")
            if ragged:
                p.add("ragged-first-step" if full == lo else "ragged-later-step")
                p.add("ragged-even-block" if b % 2 == 0 else "ragged-odd-block")
            if full - lo >= 2:
                p.add("prefetch-next-step")
        if len(set(counts)) > 1:
            p.add("blocks-differ")
        if self.R == 1:
            p.add("one-row")
        return p


VPROD_REQUIRED = {"wave-no-step", "block-one-step", "block-3+-steps", "ragged-first-step", "ragged-later-step",
                  "last-round-some-waves", "blocks-differ", "even-block", "odd-block", "one-row", "empty-block"}

# ------------------------------------------------------------------------------------------------ cases
# (R, grid cap; 0 = none).  Beyond the listed shapes: (869, 2) puts the ragged tile on a later trip of an ODD block -- in
# the others it is owned by block 0 or sits on a first trip; (1577, 12) leaves the last vprod block WITHOUT a K-step
# and (8450, 66) the last weight-gradient block without a pixel pair (a block behind the end of the range: with a cap c
# it needs ceil(n / c) * (c - 1) >= n, which no smaller shape gives; uncapped, full-size maps have such blocks).
C11_WALKS = [(1, 0), (31, 0), (32, 0), (33, 0), (255, 0), (256, 0), (257, 0), (613, 1), (613, 2), (773, 1), (869, 2)]
WGRAD_WALKS = [(1, 0), (2, 0), (15, 0), (16, 0), (17, 0), (63, 0), (64, 0), (65, 0), (129, 0), (613, 1), (613, 3),
               (1031, 1), (1031, 3)]
WGRAD_EMPTY_BLOCK = (8450, 66)
VPROD_WALKS = [(1, 0), (15, 0), (16, 0), (17, 0), (64, 0), (597, 0), (613, 1), (613, 2), (613, 3), (1577, 12)]
RELU_OFF_WALK = (613, 1)                   # prologue forms run with the ReLU everywhere and without it at this walk

Spec = collections.namedtuple("Spec", "entry form mask bits relu step")
SPECS = collections.OrderedDict()


def _step(f, mask, bits):
    """launched by the engine's train step (engine.py:588-782)"""
    if f.ext:
        return True                                                                # engine.py:732, :779
    if f.side:
        return True                                                                # engine.py:623 (bits: :621-622)
    if f.epi in (0, 1) and (f.cin, f.cout, f.pro) in ((64, 64, 0), (64, 256, 1), (64, 256, 0)):
        return True                                                                # engine.py:615, :635, :642
    if f.epi == 3 and f.add:
        return True                                                                # engine.py:762, :764
    return f.epi == 0 and (f.cin, f.cout, f.pro) == (64, 64, 2)                    # engine.py:776


def _add_spec(entry, f, mask=None, bits=0):
    name = "%s-%dx%d-p%d-e%d" % (entry, f.cin, f.cout, f.pro, f.epi)
    name += ("-add" if f.add else "") + ("-" + mask if mask else "") + ("-x2" if f.x2 else "") + ("-bits" if bits else "")
    assert name not in SPECS
    SPECS[name] = Spec(entry, f, mask, bits, 1 if f.pro else 0, _step(f, mask, bits))


for _f in ALL_C11:
    if _f.side:
        for _b in (0, 1):
            _add_spec("materialize", _f, bits=_b)
    elif _f.ext:
        _add_spec("lin_dgrad", _f, "fma")
    elif _f.epi == 3:
        for _m in ("act", "bits"):
            _add_spec("conv1x1", _f, _m)
    else:
        _add_spec("conv1x1", _f, ("act" if _f.mask_act else "fma") if _f.epi == 2 else None)

Case = collections.namedtuple("Case", "spec R cap relu")


def c11_cases(name):
    s = SPECS[name]
    out = [Case(name, R, cap, s.relu) for R, cap in C11_WALKS]
    if s.form.pro and not s.form.side:
        out.append(Case(name, RELU_OFF_WALK[0], RELU_OFF_WALK[1], 0))
    return out


def spec_form(s):
    """the form the restated dispatch gives for a spec's arguments"""
    f = s.form
    if s.entry == "materialize":
        return materialize_form(f.epi == 1)
    if s.entry == "lin_dgrad":
        return lin_dgrad_form(f.add)
    return conv1x1_form(f.cin, f.cout, in2=f.pro == 2, abc=f.pro >= 1, addend=f.add, act=s.mask == "act",
                        act_bits=s.mask == "bits", msc=s.mask == "fma", z=f.epi == 2, mean=f.epi == 2, z2=f.x2,
                        mean2=f.x2, part=f.epi in (1, 2))


WSpec = collections.namedtuple("WSpec", "co ci pz pa relu step")
WGRAD_SPECS = collections.OrderedDict()
for _ci, _co in SHAPES:
    for _pz in (0, 1):
        for _pa in (0, 1):
            for _relu in ((0, 1) if _pa else (0,)):
                # engine.py:755: conv1's weight gradient, dz = abc1 . (dy1, z1), the block input as it is
                WGRAD_SPECS["wgrad-%dx%d-pz%d-pa%d-relu%d" % (_co, _ci, _pz, _pa, _relu)] = WSpec(
                    _co, _ci, _pz, _pa, _relu, bool(_pz and not _pa and _co == 64))


def wgrad_walks(name):
    extra = [WGRAD_EMPTY_BLOCK] if name == "wgrad-64x64-pz1-pa0-relu0" else []
    return WGRAD_WALKS + extra


VSpec = collections.namedtuple("VSpec", "abc relu step")
VPROD_SPECS = collections.OrderedDict([("vprod-plain", VSpec(0, 0, True)),          # engine.py:771 (downsample branch)
                                       ("vprod-abc", VSpec(1, 0, False)),
                                       ("vprod-abc-relu", VSpec(1, 1, True))])      # engine.py:728
LIN_CASES = ("lin-small", "lin-wide")      # lin_bnsums / lin_finish do not depend on R


# ------------------------------------------------------------------------------------------------ operands
def _rs(*key):
    seed = 0
    for k in key:
        seed = (seed * 10007 + int(k)) % (2 ** 31 - 1)
    return np.random.RandomState(seed)


def _ints(rs, shape, lim=3):
    return rs.randint(-lim, lim + 1, shape).astype(F32)


def _pm(rs, n, mags):
    return (rs.choice(mags, n) * rs.choice([-1.0, 1.0], n)).astype(F32)


def _abc(rs, C, with_b=True, a_mags=(0.5, 1.0, 2.0)):
    """A | B | C; without B its row is NaN: nothing may read it"""
    b = _pm(rs, C, [0.5, 1.0]) if with_b else np.full(C, np.nan, F32)
    return np.stack([_pm(rs, C, list(a_mags)), b, _pm(rs, C, [0.5, 1.0, 1.5])])


def _halves(rs, shape, lim=4):
    return (rs.randint(-lim, lim + 1, shape) / 2.0).astype(F32)


def _signed_zeros(rs, a):
    """an integer map whose zeros are -0.0 and +0.0, half each"""
    a = a.copy()
    zero = a == 0
    a[zero & (rs.randint(0, 2, a.shape) == 1)] = -0.0
    return a


def pack_bits(a):
    """[R, C] -> uint32 [R, C / 32]: bit (c & 31) of word c >> 5 = a[r, c] > 0, built on the host"""
    b = (np.asarray(a) > 0).reshape(a.shape[0], -1, 32).astype(np.uint64)
    return (b << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)


FMA_Z, FMA_SC = F32(1 + 2.0 ** -4), F32(1 + 2.0 ** -20)
FMA_SH = F32(-(1 + 2.0 ** -4 + 2.0 ** -20))           # fmaf(SC, Z, SH) = 2^-24; float(SC * Z) + SH = 0 (the tie goes to even)


def c11_operands(case):
    s = SPECS[case.spec]
    f, R = s.form, case.R
    rs = _rs(31, list(SPECS).index(case.spec), R, case.cap)
    small = f.epi == 1 and f.pro != 0      # a forward with statistics behind a prologue: sum y^2 is the tightest budget
    lim = 2 if small else 3
    o = dict(inp=_ints(rs, (R, f.cin), lim), w=_ints(rs, (f.cout, f.cin), 1 if f.cin == 256 else 2))     # w: logical [Cout][Cin]
    if f.pro == 2:
        o["in2"] = _ints(rs, (R, f.cin), lim)
    if f.ext:
        o["abc"] = np.stack([_pm(rs, 256, [0.5, 1.0, 2.0]), np.zeros(256, F32), np.zeros(256, F32)])   # avec = A | 0 | 0
        o["in3"], o["abc3"] = _ints(rs, (R, 64)), _abc(rs, 64, False)
        o["m"], o["cvec"] = _ints(rs, (64, f.cout), 2), _pm(rs, f.cout, [0.5, 1.0, 1.5])               # m [k][co]
    elif f.pro:
        o["abc"] = _abc(rs, f.cin, f.pro == 2, [0.5, 1.0] if small else [0.5, 1.0, 2.0])
    if f.add:
        o["addend"] = _halves(rs, (R, f.cout))
        o["addend"][o["addend"] == 0] = 0.5
    if s.mask in ("act", "bits"):
        o["act"] = _signed_zeros(rs, _ints(rs, (R, f.cout)))
        if s.mask == "bits":
            o["act_bits"] = pack_bits(o["act"])
    if f.epi == 2:
        o["z"], o["mean"], o["invstd"] = _ints(rs, (R, f.cout)), _ints(rs, f.cout, 2), _pm(rs, f.cout, [0.5, 1.0, 2.0])
        o["invstd"] = np.abs(o["invstd"])
        o["mean"][1], o["invstd"][1], o["mean"][2], o["invstd"][2] = 1.0, 0.5, -2.0, 2.0    # distinct whatever the draw
        if s.mask == "fma":
            o["msc"] = _pm(rs, f.cout, [0.5, 1.0, 2.0])
            o["msh"] = (-o["msc"] * rs.randint(-1, 2, f.cout)).astype(F32)
            ch = FMA_CH
            o["z"][:, ch] = rs.choice([FMA_Z, F32(1), F32(2)], R, p=[0.5, 0.25, 0.25])
            o["z"][R - 1, ch] = FMA_Z
            o["msc"][ch], o["msh"][ch], o["mean"][ch], o["invstd"][ch] = FMA_SC, FMA_SH, 1.0, 1.0
        if f.x2:
            o["z2"], o["mean2"] = _ints(rs, (R, f.cout)), _ints(rs, f.cout, 2)
            o["invstd2"] = np.abs(_pm(rs, f.cout, [0.5, 1.0, 2.0]))
            o["mean2"][1], o["invstd2"][1], o["mean2"][2], o["invstd2"][2] = -1.0, 2.0, 2.0, 0.5
    return o


def wgrad_operands(name, R, cap):
    s = WGRAD_SPECS[name]
    rs = _rs(32, list(WGRAD_SPECS).index(name), R, cap)
    o = dict(dz=_ints(rs, (R, s.co)), act=_ints(rs, (R, s.ci)))
    if s.pz:
        o["dz2"], o["dz_abc"] = _ints(rs, (R, s.co)), _abc(rs, s.co)
    if s.pa:
        o["act_abc"] = _abc(rs, s.ci, False)
    return o


def vprod_operands(name, R, cap):
    s = VPROD_SPECS[name]
    rs = _rs(33, list(VPROD_SPECS).index(name), R, cap)
    o = dict(v=_ints(rs, (R, 256)), act=_ints(rs, (R, 64)))
    if s.abc:
        o["act_abc"] = _abc(rs, 64, False)
    return o


LIN_P, LIN_G, LIN_S, LIN_SU, LIN_FLOATS = 0, 16384, 20480, 20544, 20800           # conv1x1_lin.hip:24


def lin_operands(name):
    """integer lin = P | G | S | SU (lin-wide: up to 2^20, so that the results need more than 24 bits and the single
    rounding of the double value shows), w, abc = A | B | C, mean, invstd"""
    wide = name == "lin-wide"
    rs = _rs(34, wide)
    lim = 2 ** 20 if wide else 50
    return dict(lin=_ints(rs, LIN_FLOATS, lim), w=_ints(rs, (256, 64), 1000 if wide else 2), abc=_abc(rs, 256),
                mean=_ints(rs, 256, 2), invstd=np.abs(_pm(rs, 256, [0.5, 1.0, 2.0])))


# ------------------------------------------------------------------------------------------------ references (float64)
def prologue(f, o, relu, rows=None):
    """f(A in + B in2 + C) [rows, Cin] and, with EXT, the extra 64 channels relu?(A3 in3 + C3) (None otherwise)"""
    sel = slice(None) if rows is None else rows
    x = o["inp"][sel].astype(F64)
    if f.pro:
        abc = o["abc"].astype(F64)
        x = abc[0] * x + abc[2]
        if f.pro == 2:
            x = x + abc[1] * o["in2"][sel].astype(F64)
        if relu and not f.ext:                                   # (the linear form's main operand: pro_relu = 0, :906)
            x = np.maximum(x, 0.0)
    x3 = None
    if f.ext:
        a3 = o["abc3"].astype(F64)
        x3 = np.maximum(a3[0] * o["in3"][sel].astype(F64) + a3[2], 0.0) if relu else a3[0] * o["in3"][sel].astype(F64) + a3[2]
    return x, x3


def mask_of(s, o, rows=None, fault=None):
    """bool [rows, Cout]: the elements the epilogue keeps"""
    sel = slice(None) if rows is None else rows
    if s.mask in ("act", "bits"):
        m = o["act"][sel]
    else:
        m = (BC.unfused32 if fault == "mask_unfused" else BC.fma32)(o["msc"], o["z"][sel], o["msh"])
    return m >= 0 if fault == "mask_ge" else m > 0


def xhat(o, k="", rows=None):
    sel = slice(None) if rows is None else rows
    return (o["z" + k][sel].astype(F64) - o["mean" + k].astype(F64)) * o["invstd" + k].astype(F64)


def tile_result(s, o, relu, rows, xrows=None, fault=None):
    """one row set through prologue, product and epilogue -> dict(out, side, terms: the per-element summands of the
    statistics rows).  xrows: the rows the MFMA operand is taken from (a stale operand: another tile's)."""
    f = s.form
    x, x3 = prologue(f, o, relu, rows if xrows is None else xrows)
    side = prologue(f, o, relu, rows)[0] if f.side else None
    if fault == "chunks_swapped" and f.cin == 256:
        x = x.copy()
        x[:, 32:64], x[:, 64:96] = x[:, 64:96].copy(), x[:, 32:64].copy()
    y = x @ o["w"].astype(F64).T
    if f.ext:
        if fault != "ext_dropped":
            y = y + x3 @ o["m"].astype(F64)
        if fault != "cvec_dropped":
            y = y + o["cvec"].astype(F64)
    terms = []
    if f.epi == 1:
        terms = [y, y * y]
    elif f.epi in (2, 3):
        keep = mask_of(s, o, rows, fault)
        add = o["addend"][rows].astype(F64) if f.add else 0.0
        pre = y + add
        y = np.where(keep, y, 0.0) + add if fault == "addend_after_mask" else np.where(keep, pre, 0.0)
        if f.epi == 2:
            v = pre if fault == "sums_before_mask" else y
            terms = [v, v * xhat(o, "", rows)]
            if f.x2:
                terms += [v, v * xhat(o, "" if fault == "x2_uses_xhat1" else "2", rows)]
    return dict(out=y, side=side, terms=terms)


def side_words(side, fault=None):
    w = pack_bits(side)
    if fault == "side_bits_wrong_chunk":
        w = w[:, [1, 0, 2, 3, 4, 5, 6, 7]]
    return w


def c11_ref(case, o):
    """-> dict(out [R, Cout]; part / part2 [grid, 2, Cout]: the statistics row of every block; side, side_bits)"""
    s = SPECS[case.spec]
    walk = C11Walk(case.R, case.cap)
    t = tile_result(s, o, case.relu, np.arange(case.R))
    ref = dict(out=t["out"])
    if s.form.side:
        ref["side"] = t["side"]
        if s.bits:
            ref["side_bits"] = side_words(t["side"])
    if t["terms"]:
        owned = [walk.rows_of_block(b) for b in range(walk.grid)]
        ref["part"] = np.stack([np.stack([t["terms"][0][m].sum(0), t["terms"][1][m].sum(0)]) for m in owned])
        if s.form.x2:
            ref["part2"] = np.stack([np.stack([t["terms"][2][m].sum(0), t["terms"][3][m].sum(0)]) for m in owned])
    return ref


C11_FAULTS = ("tile_skipped", "stale_prefetch", "clamped_rows_counted", "ragged_not_stored", "row_beyond_R",
              "addend_after_mask", "mask_ge", "mask_unfused", "sums_before_mask", "x2_uses_xhat1", "odd_tile_not_negated",
              "chunks_swapped", "ext_dropped", "cvec_dropped", "part_row_unwritten", "side_bits_wrong_chunk")


def fault_applies(fault, case):
    """whether a fault can be expressed on a case at all (a later trip, a ragged tile, the slot it breaks)"""
    s = SPECS[case.spec]
    f, walk = s.form, C11Walk(case.R, case.cap)
    later = walk.ntiles > walk.stride
    return {"tile_skipped": later, "stale_prefetch": later,
            "clamped_rows_counted": walk.ragged is not None and f.epi in (1, 2),
            "ragged_not_stored": walk.ragged is not None, "row_beyond_R": walk.ragged is not None,
            "addend_after_mask": f.add and case.R >= 8, "mask_ge": f.epi in (2, 3) and case.R >= 8,
            "mask_unfused": s.mask == "fma", "sums_before_mask": f.epi == 2 and case.R >= 8,
            "x2_uses_xhat1": f.x2, "odd_tile_not_negated": walk.ntiles >= 2 and derived(f)["BF"],
            "chunks_swapped": f.cin == 256, "ext_dropped": f.ext, "cvec_dropped": f.ext,
            "part_row_unwritten": f.epi in (1, 2), "side_bits_wrong_chunk": bool(s.bits)}[fault]


def c11_emulate(case, o, fault=None):
    """The tile walk of conv1x1_kernel restated in numpy: blocks, waves, trips, the clamped rows of the ragged tile, sums
    carried across a wave's tiles and folded per block.  Without a fault: a second, tile-by-tile evaluation of c11_ref.
    -> the dict c11_ref gives, the outputs NaN where nothing was stored, plus `frame`: whether nothing was stored behind
    row R - 1."""
    s = SPECS[case.spec]
    f, R, walk = s.form, case.R, C11Walk(case.R, case.cap)
    out = np.full((R + TILE, f.cout), np.nan)
    got = dict(out=out)
    if f.side:
        got["side"] = np.full((R + TILE, f.cin), np.nan)
    nsum = 0 if f.epi not in (1, 2) else (4 if f.x2 else 2)
    parts = np.full((walk.grid, nsum, f.cout), np.nan)
    for b in range(walk.grid):
        sums = np.zeros((nsum, f.cout))
        for w in range(NW):
            prev = None
            for trip, tile in enumerate(walk.tiles_of(b, w)):
                idx = tile * TILE + np.arange(TILE)
                valid = idx < R
                rows = np.minimum(idx, R - 1)                                      # clamped: loads stay unconditional
                if fault == "tile_skipped" and trip >= 1:
                    continue
                t = tile_result(s, o, case.relu, rows, prev if fault == "stale_prefetch" and trip >= 1 else None, fault)
                prev = rows
                if fault == "odd_tile_not_negated" and tile % 2:
                    t["out"] = -t["out"]
                    t["terms"] = [-a for a in t["terms"]]
                count = np.ones(TILE, bool) if fault == "clamped_rows_counted" else valid
                for k, a in enumerate(t["terms"]):
                    sums[k] += a[count].sum(0)
                store = valid
                if fault == "ragged_not_stored" and tile == walk.ragged:
                    store = np.zeros(TILE, bool)
                if fault == "row_beyond_R":
                    store = np.ones(TILE, bool)
                out[idx[store]] = t["out"][store]
                if f.side:
                    got["side"][idx[store]] = t["side"][store]
        if not (fault == "part_row_unwritten" and b == walk.grid - 1):
            parts[b] = sums
    got["frame"] = bool(np.isnan(out[R:]).all())
    got["out"] = out[:R]
    if f.side:
        got["side"] = got["side"][:R]
        if s.bits:
            got["side_bits"] = side_words(np.nan_to_num(got["side"]), fault)
    if nsum:
        got["part"] = parts[:, :2]
        if f.x2:
            got["part2"] = parts[:, 2:]
    return got


def fz_fa(s, o, rows=None):
    sel = slice(None) if rows is None else rows
    fz, fa = o["dz"][sel].astype(F64), o["act"][sel].astype(F64)
    if s.pz:
        a = o["dz_abc"].astype(F64)
        fz = a[0] * fz + a[1] * o["dz2"][sel].astype(F64) + a[2]
    if s.pa:
        a = o["act_abc"].astype(F64)
        fa = a[0] * fa + a[2]
        if s.relu:
            fa = np.maximum(fa, 0.0)
    return fz, fa


def wgrad_ref(name, o):
    fz, fa = fz_fa(WGRAD_SPECS[name], o)
    return fz.T @ fa


def wgrad_emulate(name, o, R, cap, fault=None):
    """dw as the fold of the per-block partials of the restated walk: full batches, then the tail rows of each block.
    Fault "tail_twice": one batch of the tail is counted twice."""
    s = WGRAD_SPECS[name]
    walk = WgradWalk(R, 1 if (s.co, s.ci) == (64, 64) else 4, cap)
    dw = np.zeros((s.co, s.ci))
    for b in range(walk.grid):
        lo, hi, waves = walk.block(b)
        tails = {s0: tail for _, s0, tail in waves if s0 is not None}
        tail_rows = sorted(r for t in tails.values() for r in t)
        full_rows = [r for r in range(2 * lo, min(2 * hi, R)) if r not in set(tail_rows)]
        for rows in (full_rows, tail_rows) + ((tail_rows,) if fault == "tail_twice" else ()):
            if rows:
                fz, fa = fz_fa(s, o, np.asarray(rows))
                dw += fz.T @ fa
    return dw


def vprod_a(s, o, rows=None):
    a = o["act"][slice(None) if rows is None else rows].astype(F64)
    if s.abc:
        t = o["act_abc"].astype(F64)
        a = t[0] * a + t[2]
        if s.relu:
            a = np.maximum(a, 0.0)
    return a


def vprod_ref(name, o):
    """lin = P [256, 64] | G [64, 64] | S [64] | SU [256]"""
    a, v = vprod_a(VPROD_SPECS[name], o), o["v"].astype(F64)
    return np.concatenate([(v.T @ a).ravel(), (a.T @ a).ravel(), a.sum(0), v.sum(0)])


def vprod_emulate(name, o, R, cap, fault=None):
    """lin as the fold of the per-block, per-wave partials of the restated walk.  Faults: "s_every_wave" (the sums of a
    are taken by all four waves of a step), "odd_block_p_not_negated"."""
    s, walk = VPROD_SPECS[name], VprodWalk(R, cap)
    P, G, S, SU = np.zeros((256, 64)), np.zeros((64, 64)), np.zeros(64), np.zeros(256)
    for b in range(walk.grid):
        lo, hi, full, ragged = walk.block(b)
        sgn = -1.0 if b % 2 else 1.0
        Pb = np.zeros((256, 64))
        for ks in range(lo, max(hi, lo)):
            rows = np.arange(16 * ks, min(16 * ks + 16, R))
            a, v = vprod_a(s, o, rows), o["v"][rows].astype(F64)
            Pb += v.T @ (sgn * a)
            G += sgn * (a.T @ (sgn * a))
            S += a.sum(0) * (4 if fault == "s_every_wave" else 1)
            SU += v.sum(0)
        P += Pb if fault == "odd_block_p_not_negated" else sgn * Pb
    return np.concatenate([P.ravel(), G.ravel(), S, SU])


def lin_bnsums_ref(o):
    """part [2][256] as float32(the double value) (conv1x1_lin.hip:233-243)"""
    lin, w = o["lin"].astype(F64), o["w"].astype(F64)
    dot = (w * lin[LIN_P:LIN_G].reshape(256, 64)).sum(1)
    su = lin[LIN_SU:]
    return np.stack([su, o["invstd"].astype(F64) * (dot - o["mean"].astype(F64) * su)]).astype(F32)


def lin_finish_ref(o):
    """dw [256, 64], m [64, 64], cvec [64], avec [3, 256] as float32(the double value) (conv1x1_lin.hip:247-274)"""
    lin, w, abc = o["lin"].astype(F64), o["w"].astype(F64), o["abc"].astype(F64)
    P, G, S = lin[LIN_P:LIN_G].reshape(256, 64), lin[LIN_G:LIN_S].reshape(64, 64), lin[LIN_S:LIN_SU]
    dw = abc[0][:, None] * P + abc[1][:, None] * (w @ G) + abc[2][:, None] * S[None, :]
    m = w.T @ (abc[1][:, None] * w)
    avec = np.stack([abc[0], np.zeros(256), np.zeros(256)])
    return dict(dw=dw.astype(F32), m=m.astype(F32), cvec=(abc[2] @ w).astype(F32), avec=avec.astype(F32))


def lin_exact(o):
    """every double sum of the two kernels is exact in any order: every term is a multiple of 1/4 (at most two of the
    half-integer constants A, B, C, invstd meet in one), and the sums of their absolute values stay below 2^53 / 8"""
    lin, w, abc = np.abs(o["lin"].astype(F64)), np.abs(o["w"].astype(F64)), np.abs(o["abc"].astype(F64))
    worst = max((w * lin[LIN_P:LIN_G].reshape(256, 64)).sum(1).max() + 2 * lin[LIN_SU:].max(),
                (abc[0][:, None] * lin[:LIN_G].reshape(256, 64) + abc[1][:, None] * (w @ lin[LIN_G:LIN_S].reshape(64, 64))
                 + abc[2][:, None] * lin[LIN_S:LIN_SU][None, :]).max(), (w.T @ (abc[1][:, None] * w)).max())
    return 8 * worst < 2.0 ** 53


# ------------------------------------------------------------------------------------------------ exactness, mask shares
LIMIT = 2.0 ** 24


def _one_piece(a, q):
    """every value is a multiple of q with at most 8 significant bits: one bf16 piece, products of two exact in f32"""
    u = np.abs(np.asarray(a, F64)) / q
    return bool(np.array_equal(u, np.round(u)) and u.max() < 256)


def c11_budget(case, o):
    """-> {quantity: the largest sum of |terms| in units of the quantity's quantum} of a conv1x1_kernel case"""
    s = SPECS[case.spec]
    f = s.form
    x, x3 = prologue(f, o, case.relu)
    qx = 0.5 if f.pro else 1.0
    assert _one_piece(x, qx) and _one_piece(o["w"], 1.0) and (x3 is None or (_one_piece(x3, 0.5) and _one_piece(o["m"], 1.0)))
    mag = np.abs(x) @ np.abs(o["w"].astype(F64)).T
    if f.ext:
        mag = mag + np.abs(x3) @ np.abs(o["m"].astype(F64)) + np.abs(o["cvec"].astype(F64))
    if f.add:
        mag = mag + np.abs(o["addend"].astype(F64))
    b = {"out": mag.max() / 0.5}
    t = tile_result(s, o, case.relu, np.arange(case.R))
    if f.epi == 1:
        b["sum y"], b["sum y^2"] = np.abs(t["terms"][0]).sum(0).max() / 0.5, t["terms"][1].sum(0).max() / 0.25
    if f.epi == 2:
        for k, key in ((1, ""), (3, "2")):
            if k < len(t["terms"]):
                qz = np.where(np.arange(f.cout) == FMA_CH, 2.0 ** -4, 1.0) if s.mask == "fma" and key == "" else 1.0
                q = 0.5 * o["invstd" + key].astype(F64) * qz
                assert np.array_equal(t["terms"][k] / q, np.round(t["terms"][k] / q))
                b["sum dy*xhat" + key] = (np.abs(t["terms"][k]).sum(0) / q).max()
        b["sum dy"] = np.abs(t["terms"][0]).sum(0).max() / 0.5
    return b


def exact_ok(case, o=None):
    return max(c11_budget(case, c11_operands(case) if o is None else o).values()) < LIMIT


def wgrad_budget(name, o):
    fz, fa = fz_fa(WGRAD_SPECS[name], o)
    assert np.array_equal(fz * 2, np.round(fz * 2)) and np.array_equal(fa * 2, np.round(fa * 2))
    return {"dw": (np.abs(fz).T @ np.abs(fa)).max() / 0.25}


def vprod_budget(name, o):
    a, v = vprod_a(VPROD_SPECS[name], o), o["v"].astype(F64)
    assert _one_piece(a, 0.5) and _one_piece(v, 1.0)
    return {"P": (np.abs(v).T @ np.abs(a)).max() / 0.5, "G": (np.abs(a).T @ np.abs(a)).max() / 0.25,
            "S": np.abs(a).sum(0).max() / 0.5, "SU": np.abs(v).sum(0).max()}


def mask_shares(case, o):
    """-> dict(kept, dropped: shares of the elements; zero: share of fma decisions that are exactly 0 (None for a map);
    neg_zero, pos_zero: whether the mask map holds both zeros)"""
    s = SPECS[case.spec]
    keep = mask_of(s, o)
    r = dict(kept=float(keep.mean()), dropped=float(1 - keep.mean()), zero=None, neg_zero=None, pos_zero=None)
    if s.mask == "fma":
        r["zero"] = float((BC.fma32(o["msc"], o["z"], o["msh"]) == 0).mean())
    else:
        zero = o["act"] == 0
        r["neg_zero"], r["pos_zero"] = bool((zero & np.signbit(o["act"])).any()), bool((zero & ~np.signbit(o["act"])).any())
        assert not keep[zero].any()
    return r


# ------------------------------------------------------------------------------------------------ checkers
def _differs(got, ref):
    return ~(np.asarray(got, F64) == np.asarray(ref, F64))                         # a NaN differs; -0.0 equals 0.0


def describe_rows(walk, bad, what):
    """where a [R, C] result differs: row tiles, the (block, wave, trip) that owns each, 32-channel blocks"""
    rows, cols = np.nonzero(bad)
    tiles = sorted(set((rows // TILE).tolist()))
    owners = ["tile %d = block %d wave %d trip %d%s" % ((t,) + walk.owner(t) + (" (ragged)" if t == walk.ragged else "",))
              for t in tiles[:6]]
    return "%s: %d of %d elements differ; first (row %d, channel %d); %d tiles: %s%s; channel blocks %s" % (
        what, int(bad.sum()), bad.size, rows[0], cols[0], len(tiles), "; ".join(owners), " ..." if len(tiles) > 6 else "",
        sorted(set((cols // 32).tolist())))


def check_c11(case, got, ref):
    """-> the list of findings (empty: every output equals the exact reference element for element).  Statistics: every
    row finite, the float64 fold of the rows exact, and each block's row the sum over the tiles the walk gives it."""
    walk = C11Walk(case.R, case.cap)
    msgs = []
    for k in ("out", "side"):
        if k in ref:
            bad = _differs(got[k], ref[k])
            if bad.any():
                msgs.append(describe_rows(walk, bad, "%s %s" % (case.spec, k)))
    if "side_bits" in ref:
        bad = got["side_bits"] != ref["side_bits"]
        if bad.any():
            msgs.append(describe_rows(walk, bad, "%s side_bits (words)" % case.spec))
    for k in ("part", "part2"):
        if k in ref:
            g = np.asarray(got[k], F64)
            if g.shape != ref[k].shape:
                msgs.append("%s %s: %s rows, expected %s" % (case.spec, k, g.shape, ref[k].shape))
                continue
            if not np.isfinite(g).all():
                msgs.append("%s %s: blocks %s left a statistics row unwritten" % (
                    case.spec, k, sorted(set(np.nonzero(~np.isfinite(g))[0].tolist()))))
            bad = _differs(g.sum(0), ref[k].sum(0))
            if bad.any():
                msgs.append("%s %s: the fold over %d blocks differs in %d of %d sums (sum index %s, channel blocks %s)" % (
                    case.spec, k, g.shape[0], int(bad.sum()), bad.size, sorted(set(np.nonzero(bad)[0].tolist())),
                    sorted(set((np.nonzero(bad)[1] // 32).tolist()))))
            bad = _differs(g, ref[k])
            if bad.any():
                msgs.append("%s %s: the rows of blocks %s are not the sums over their own tiles" % (
                    case.spec, k, sorted(set(np.nonzero(bad)[0].tolist()))))
    if not got.get("frame", True):
        msgs.append("%s: a row behind R - 1 was written" % case.spec)
    return msgs


def check_matrix(got, ref, what, rows_name="row"):
    bad = _differs(got, ref)
    if not bad.any():
        return []
    idx = np.argwhere(bad)
    return ["%s: %d of %d elements differ; first at %s: got %r, exact %r; %s blocks of 64: %s" % (
        what, int(bad.sum()), bad.size, tuple(idx[0]), float(np.asarray(got)[tuple(idx[0])]), float(ref[tuple(idx[0])]),
        rows_name, sorted(set((idx[:, 0] // 64).tolist())))]


def check_lin(got, ref, what):
    """lin = P | G | S | SU, each part named"""
    msgs = []
    for k, lo, hi in (("P", LIN_P, LIN_G), ("G", LIN_G, LIN_S), ("S", LIN_S, LIN_SU), ("SU", LIN_SU, LIN_FLOATS)):
        msgs += check_matrix(np.asarray(got)[lo:hi].reshape(-1, 64), ref[lo:hi].reshape(-1, 64), "%s %s" % (what, k))
    return msgs
