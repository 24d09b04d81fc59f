"""Case table, hard operands and float64 references for cova_sgemm / cova_sgemm_dropout_bwd (csrc/gemm.hip).  No GPU
import: tests/test_gemm_cases_cpu.py checks the table and the checkers themselves, tests/test_gemm_paths_gpu.py runs it.

``form(...)`` restates the HOST rule of sgemm_launch: which of the 20 kernel instantiations a call takes follows from the
shape, the 16-byte alignment of the two operands, their leading dimensions and option 22.  Alignment is described by the
operand's offset in floats from a 16-byte boundary, as in tests/head_cases.py.

Two kinds of operands, both seeded per case and transposition form:

* ``integer_operands``: A and B hold non-zero integers in [-8, 8], bias and the old content of C integers in
  [-1000, 1000].  Every partial sum of a product, in any order, is an integer of magnitude <= 64 K + 2000 < 2^24
  (``exact_ok``), so every correct f32 summation order -- with or without FMA, one accumulator or four -- returns the exact
  result: the comparison is element for element.
* ``scaled_operands``: entries +-[0.5, 1), row m of op(A) times 2^e(m), column n of op(B) times 2^f(n), e and f in
  [-10, 10] with both ends present whenever there are two rows / columns: no denormals, magnitudes 2^40 apart inside one
  matrix.  bias[n] carries 2^f(n), the old C[m, n] carries 2^(e(m) + f(n)).  The result is held element by element to
  head_cases.sum_bound with L = K + 2 (K products, the bias, the old value) and
  mag = |op(A)| |op(B)| + |bias| + |old|: a derived bound, no measured tolerance.

The Dropout epilogue is stated in float32 exactly as the kernel writes it: einv = float32(1) / (float32(1) - float32(p)),
one rounded multiply of the (exact) product on the kept elements, 0 elsewhere.
"""
import collections

import numpy as np
import torch

import head_cases as HC

NAN = float("nan")
BM = BN = BK = 64                                   # gemm.hip:25   block tile and k-tile of sgemm_kernel
KT = 32                                             # gemm.hip:205  k-tile of sgemm_dma_kernel
TRANS = [(0, 0), (0, 1), (1, 0), (1, 1)]


# ------------------------------------------------------------------------------------------------ dispatch
def _cdiv(a, b):
    return (a + b - 1) // b


def form(ta, tb, M, N, K, a_off, lda, b_off, ldb, option22=1):
    """The kernel instantiation sgemm_launch selects (csrc/gemm.hip):
    None (M == 0 or N == 0: nothing is launched), ("reg", ta, tb, KS) = sgemm_kernel<TA, TB, KS>, or
    ("dma", ta, tb, shape) = sgemm_dma_kernel: shape 0 = <2, 1, 4> (64 x 64 tile), 1 = <2, 2, 3> (64 x 64, two k-groups),
    2 = <1, 2, 4> (32 x 64, two k-groups)."""
    ta, tb = int(bool(ta)), int(bool(tb))
    if M == 0 or N == 0:                                                        # :358
        return None
    va = a_off % 4 == 0 and lda % 4 == 0                                        # :361  vec4_ok (common.h)
    vb = b_off % 4 == 0 and ldb % 4 == 0
    a_bytes = 4 * (K * lda if ta else M * lda)                                  # :364
    b_bytes = 4 * (N * ldb if tb else K * ldb)
    dma = (bool(option22) and va and vb and K % 4 == 0 and K >= 4               # :365-366
           and (not ta or (M % 4 == 0 and M >= 4)) and (tb or (N % 4 == 0 and N >= 4))
           and a_bytes < 2 ** 31 and b_bytes < 2 ** 31)
    if dma:
        blocks64 = _cdiv(M, 64) * _cdiv(N, 64)                                  # :372
        blocks32 = _cdiv(M, 32) * _cdiv(N, 64)
        shape = 2 if blocks32 <= 256 and K >= 8 * 32 else (1 if blocks64 <= 256 and K >= 16 * 32 else 0)     # :373
        return ("dma", ta, tb, shape)
    split = K >= 4 * BK and _cdiv(N, BN) * _cdiv(M, BM) < 2 * 4 * 256           # :390
    return ("reg", ta, tb, 2 if split else 1)


ALL_FORMS = sorted([("reg", ta, tb, ks) for ta, tb in TRANS for ks in (1, 2)]
                   + [("dma", ta, tb, s) for ta, tb in TRANS for s in (0, 1, 2)])


# ------------------------------------------------------------------------------------------------ cases
# a_al / b_al: the operand sits on a 16-byte boundary (else one float -- or an odd number of floats -- behind one);
# view: every operand and C are column blocks of wider matrices
Case = collections.namedtuple("Case", "name M N K a_al b_al option22 view")
Lay = collections.namedtuple("Lay", "rows cols ld off")          # off: floats from the 16-byte aligned start of the buffer

DMA0 = [(4, 4, 4), (36, 68, 36), (68, 36, 64), (64, 64, 96), (100, 132, 252)]          # K < 256; (64, 64, 96): the ring never full
DMA2 = [(36, 68, 256), (100, 132, 260), (32, 64, 288), (68, 100, 292)]                # 32 x 64 tiles: 8 k-tiles, 9 with a tail of 4, 9, 10
DMA1 = [(516, 964, 516), (544, 1024, 512)]                                            # more than 256 tiles of 32 x 64, K >= 512
REG = [(1, 1, 1), (5, 3, 0), (33, 65, 17), (63, 31, 64), (65, 33, 65), (100, 70, 255), (31, 63, 257), (64, 64, 256),
       (65, 100, 321)]                                                                # (65, 100, 321): five k-tiles under KS = 2
MIXED = [(36, 68, 260), (65, 100, 321)]


def _table():
    out = collections.OrderedDict()

    def add(tag, shape, a_al, b_al, option22, view):
        name = "%s-%dx%dx%d%s" % (tag, shape[0], shape[1], shape[2], "-view" if view else "")
        assert name not in out
        out[name] = Case(name, shape[0], shape[1], shape[2], a_al, b_al, option22, view)

    for view in (0, 1):
        for tag, shapes in (("dma0", DMA0), ("dma2", DMA2), ("dma1", DMA1)):
            for s in shapes:
                add(tag, s, True, True, 1, view)
                add(tag + "-opt22off", s, True, True, 0, view)            # the register kernel with vector fetches
        for s in REG:
            add("reg", s, False, False, 1, view)
        for s in MIXED:
            add("mixedA", s, True, False, 1, view)
            add("mixedB", s, False, True, 1, view)
    return out


CASES = _table()


def _lay(rows, cols, aligned, view, odd):
    """plain: rows at leading dimension cols, 4 floats (aligned) or 1 float behind the start of the buffer; view: a column
    block at column 4 of rows 8 longer (aligned), or at column ``odd`` = 3 or 5 with 8 - odd columns behind it"""
    if view:
        return Lay(rows, cols, cols + 8, 4 + (4 if aligned else odd))
    return Lay(rows, cols, cols, 4 if aligned else 1)


def layout(case, ta, tb):
    """-> (A, B, C) as Lay: the stored shapes, leading dimensions and buffer offsets of one call"""
    M, N, K = case.M, case.N, case.K
    ra, ca = (K, M) if ta else (M, K)
    rb, cb = (N, K) if tb else (K, N)
    return (_lay(ra, ca, case.a_al, case.view, 3), _lay(rb, cb, case.b_al, case.view, 5),
            _lay(M, N, case.a_al and case.b_al, case.view, 3))


def dropout_c_layout(case, ta, tb):
    """C of cova_sgemm_dropout_bwd: always ldc > N (the keep mask stays contiguous [M, N])"""
    C = layout(case, ta, tb)[2]
    return C if C.ld > C.cols else C._replace(ld=C.cols + 3)


def dropout_ldc(case, ta, tb):
    return dropout_c_layout(case, ta, tb).ld


def case_form(case, ta, tb):
    A, B, _ = layout(case, ta, tb)
    return form(ta, tb, case.M, case.N, case.K, A.off % 4, A.ld, B.off % 4, B.ld, case.option22)


def exact_ok(case):
    """every partial sum of the integer operands is an integer below 2^24"""
    return 64 * case.K + 2000 < 2 ** 24


assert all(exact_ok(c) for c in CASES.values())


# ------------------------------------------------------------------------------------------------ operands
# opA [M, K], opB [K, N] float64; A, B the float32 matrices as stored (transposed where the form says so);
# prod = op(A) op(B) and absprod = |op(A)| |op(B)| in float64, formed once
Operands = collections.namedtuple("Operands", "opA opB A B bias old prod absprod")


def _rs(case, ta, tb, kind):
    return np.random.RandomState((case.M * 1009 + case.N * 917 + case.K * 31 + ta * 2 + tb + 7 * kind
                                  + 13 * case.a_al + 17 * case.b_al) % (2 ** 31 - 1))


def _pack(opA, opB, bias, old, ta, tb):
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    A, B = f(opA.T if ta else opA), f(opB.T if tb else opB)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).double()        # (what the kernel is given)
    a, b = d(opA), d(opB)
    return Operands(a, b, A, B, f(bias), f(old), a @ b, a.abs() @ b.abs())


def integer_operands(case, ta, tb):
    rs = _rs(case, ta, tb, 0)

    def ints(lim, shape):
        a = rs.randint(-lim, lim + 1, shape)
        a[a == 0] = 1                                # (no zeros: a dropped or doubled term always shows)
        return a
    assert exact_ok(case)
    return _pack(ints(8, (case.M, case.K)), ints(8, (case.K, case.N)), ints(1000, case.N), ints(1000, (case.M, case.N)),
                 ta, tb)


def _exponents(rs, n):
    e = rs.randint(-10, 11, n)
    if n >= 2:                                       # both ends present; the smallest scale on the LAST row / column
        e[0], e[n - 1] = 10, -10                     # (the one the clamped loads of the kernels read again)
    return e


def scaled_operands(case, ta, tb):
    rs = _rs(case, ta, tb, 1)
    unit = lambda shape: rs.choice([-1.0, 1.0], shape) * rs.uniform(0.5, 1.0, shape)
    e, f = _exponents(rs, case.M), _exponents(rs, case.N)
    se, sf = np.exp2(e.astype(np.float64)).reshape(-1, 1), np.exp2(f.astype(np.float64)).reshape(1, -1)
    return _pack(unit((case.M, case.K)) * se, unit((case.K, case.N)) * sf, unit(case.N) * sf.reshape(-1),
                 unit((case.M, case.N)) * se * sf, ta, tb)


def smallest_row(o):
    """the row of op(A) with the smallest scale (scaled operands)"""
    return int(o.old.double().abs().sum(1).argmin())


def keep_mask(case, p, ta=0, tb=0):
    """uint8 [M, N]: random with keep probability 1 - p, row (M - 1) // 2 and column N - 1 dropped as a whole wherever the
    matrix has a second row / column"""
    rs = _rs(case, ta, tb, 2 + int(p * 10))
    keep = (rs.uniform(size=(case.M, case.N)) >= p).astype(np.uint8)
    if case.M >= 2:
        keep[(case.M - 1) // 2] = 0
    if case.N >= 2:
        keep[:, case.N - 1] = 0
    return torch.from_numpy(keep)


# ------------------------------------------------------------------------------------------------ references
MODES = [(0, 0), (1, 0), (0, 1), (1, 1)]             # (bias, accumulate)


def reference(o, use_bias, accumulate):
    """float64 (exact on the integer operands): op(A) op(B) (+ bias) (+ old C)"""
    ref = o.prod
    if use_bias:
        ref = ref + o.bias.double()
    if accumulate:
        ref = ref + o.old.double()
    return ref


def magnitude(o, use_bias, accumulate):
    mag = o.absprod
    if use_bias:
        mag = mag + o.bias.double().abs()
    if accumulate:
        mag = mag + o.old.double().abs()
    return mag


def einv32(p):
    return np.float32(1) / (np.float32(1) - np.float32(p))


def dropout_reference(o, keep, p):
    """float32, as the epilogue writes it (integer operands: the product is exact)"""
    prod = o.prod.numpy().astype(np.float32)
    return torch.from_numpy(np.where(keep.numpy() != 0, prod * einv32(p), np.float32(0)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ checkers
def mismatches(got, ref):
    """number of elements of ``got`` that are not equal to the reference (a NaN never is)"""
    got, ref = got.detach().cpu().double(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return int((~(got == ref)).sum())


def violations(got, o, use_bias, accumulate, K):
    """(elements outside head_cases.sum_bound, worst error over its bound) for the scaled operands: L = K + 2"""
    return HC.violations(got, reference(o, use_bias, accumulate), magnitude(o, use_bias, accumulate), K + 2)


# ------------------------------------------------------------------------------------------------ emulation with faults
FAULTS = ["last_k_dropped", "last_piece_twice", "group1_lost_32", "group1_lost_64", "bias_twice", "old_ignored",
          "pad_column_read", "row_written_twice"]
DROPOUT_FAULTS = ["mask_indexed_with_ldc"]


def expressible(fault, case, use_bias=1, accumulate=1):
    M, K = case.M, case.K
    return {"last_k_dropped": K >= 1, "last_piece_twice": K >= 4, "group1_lost_32": K > 32, "group1_lost_64": K > 64,
            "bias_twice": bool(use_bias and accumulate), "old_ignored": bool(accumulate), "pad_column_read": True,
            "row_written_twice": M >= 2 and (K >= 1 or bool(accumulate)),      # (K = 0: every row is the bias)
            "mask_indexed_with_ldc": M >= 2 and K >= 1}[fault]


def _pad_column(o, lay, ta, M, K):
    """what a kernel reads as op(A)[m, K] out of A's buffer (head_cases.place, NaN outside the data): a pad column, the next
    row, or the NaN behind the last row"""
    flat, _ = HC.place(o.A, lay.ld, lay.off, NAN)
    idx = lay.off + (K * lay.ld + np.arange(M) if ta else np.arange(M) * lay.ld + K)
    out = np.full(M, NAN)
    ok = idx < flat.numel()
    out[ok] = flat.numpy()[idx[ok]]
    return torch.from_numpy(out)


def emulate(o, case, ta, tb, use_bias, accumulate, fault=None):
    """The product as float32 [M, N], from float64 sums (one rounding: an honest result for both checkers), with one
    seeded fault of FAULTS or none."""
    A, B, K = o.opA, o.opB, case.K
    if fault == "last_k_dropped":
        prod = A[:, :K - 1] @ B[:K - 1]
    elif fault == "last_piece_twice":
        prod = A @ B + A[:, K - 4:] @ B[K - 4:]
    elif fault in ("group1_lost_32", "group1_lost_64"):          # the odd k-tiles of the DMA kernels / of sgemm_kernel
        sel = torch.from_numpy((np.arange(K) // int(fault[-2:])) % 2 == 0)
        prod = A[:, sel] @ B[sel]
    elif fault == "pad_column_read":                             # one more k, the matching element of B taken as 1
        prod = A @ B + _pad_column(o, layout(case, ta, tb)[0], ta, case.M, K).view(-1, 1)
    else:
        prod = A @ B
    if use_bias:
        prod = prod + o.bias.double() * (2 if fault == "bias_twice" else 1)
    if accumulate and fault != "old_ignored":
        prod = prod + o.old.double()
    out = prod.float()
    if fault == "row_written_twice":
        out[case.M - 2] = out[case.M - 1]
    return out


def emulate_dropout(o, case, keep, p, ldc, fault=None):
    """cova_sgemm_dropout_bwd on the integer operands [M, N]; ``mask_indexed_with_ldc`` reads keep[m * ldc + n] (an index
    past the mask reads "kept")"""
    M, N = case.M, case.N
    k = keep
    if fault == "mask_indexed_with_ldc":
        idx = np.arange(M).reshape(-1, 1) * ldc + np.arange(N).reshape(1, -1)
        flat = np.concatenate([keep.numpy().reshape(-1), np.ones(M * ldc + N, np.uint8)])
        k = torch.from_numpy(flat[idx])
    return dropout_reference(o, k, p)
