"""Every launch path of cova_sgemm and cova_sgemm_dropout_bwd (csrc/gemm.hip: 8 instantiations of sgemm_kernel, 12 of
sgemm_dma_kernel, three epilogues each) on the hard operands of tests/gemm_cases.py (tests/test_gemm_cases_cpu.py proves
that the cases reach all 20 forms and that the checkers flag a subtly wrong product).

Per launch: the operands sit in buffers that are NaN in front of them, in every pad column and behind their last row
(head_cases.place), C sits in a buffer filled with 7.0 and is NaN itself wherever the call overwrites without reading,
head_cases.untouched is asserted, and every launch runs twice with bit-equal output.  On the integer operands the result
equals the float64 reference element for element (every f32 summation order is exact there); on the scaled operands every
element is inside head_cases.sum_bound around it.  The Dropout epilogue runs on every case of the table too, dense and
view, in all four transposition forms, always with ldc > N (gemm_cases.dropout_c_layout).  Which form a case takes is stated by gemm_cases.form alone."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import _lib  # noqa: E402
import gemm_cases as GC  # noqa: E402
import head_cases as HC  # noqa: E402
from helpers import DEV, NAN  # noqa: E402

BAD_ARG = 10001                                      # COVA_ERR_BAD_ARG (include/cova_hip.h)
NAMES = list(GC.CASES)
FORM_IDS = ["nn", "nt", "tn", "tt"]


class Placed:
    """a [rows, cols] matrix on the device at a Lay's leading dimension and offset; ``ptr`` is what the call gets (an
    empty operand has no view to ask)"""

    def __init__(self, data, lay, fill=NAN):
        self.lay = lay
        self.flat, self.view = HC.place(data, lay.ld, lay.off, fill, device=DEV)
        self.ptr = self.flat.data_ptr() + 4 * lay.off
        assert self.ptr % 16 == 4 * (lay.off % 4)


def vector(v):
    """bias [N]: one float behind a 16-byte boundary, NaN on both sides"""
    return Placed(v.view(1, -1), GC.Lay(1, v.numel(), v.numel(), 1))


def status(name, *args):
    """the entry point's return code (0 = launched)"""
    args = [a.ptr if isinstance(a, Placed) else a.data_ptr() if torch.is_tensor(a) else a for a in args]
    return _lib.lib().fn[name](*args, torch.cuda.current_stream().cuda_stream)


def option22(case):
    return _lib.query("cova_set_option", 22, int(case.option22))


class Launch:
    """the device operands of one case and transposition form"""

    def __init__(self, case, ta, tb, o):
        self.case, self.ta, self.tb, self.o = case, ta, tb, o
        self.la, self.lb, self.lc = GC.layout(case, ta, tb)
        self.A, self.B, self.bias = Placed(o.A, self.la), Placed(o.B, self.lb), vector(o.bias)
        self.old = o.old.to(DEV)

    def sgemm(self, use_bias, acc):
        """one cova_sgemm -> [M, N]; C is NaN where the call overwrites, the old content under ``acc``"""
        c = self.case
        C = Placed((c.M, c.N, torch.float32), self.lc, HC.CANARY)
        C.view[:, :c.N] = self.old if acc else NAN
        assert option22(c) == 0
        try:
            rc = status("cova_sgemm", self.ta, self.tb, c.M, c.N, c.K, self.A, self.la.ld, self.B, self.lb.ld, C,
                        self.lc.ld, self.bias if use_bias else None, acc)
        finally:
            _lib.query("cova_set_option", 22, 1)
        assert rc == 0, rc
        assert HC.untouched(C.flat, C.view, c.N), "written outside C [M, N]"
        return C.view[:, :c.N].clone()

    def dropout(self, keep, p):
        c = self.case
        lay = GC.dropout_c_layout(c, self.ta, self.tb)
        C = Placed((c.M, c.N, torch.float32), lay, HC.CANARY)
        C.view[:, :c.N] = NAN
        assert option22(c) == 0
        try:
            rc = status("cova_sgemm_dropout_bwd", self.ta, self.tb, c.M, c.N, c.K, self.A, self.la.ld, self.B,
                        self.lb.ld, C, lay.ld, keep, float(p))
        finally:
            _lib.query("cova_set_option", 22, 1)
        assert rc == 0, rc
        assert HC.untouched(C.flat, C.view, c.N), "written outside C [M, N]"
        return C.view[:, :c.N].clone()


def twice(fn):
    a, b = fn(), fn()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two runs differ"
    return a.cpu()


def same(got, ref, what):
    n = GC.mismatches(got, ref)
    assert n == 0, "%s: %d of %d elements differ from the exact result" % (what, n, got.numel())


@pytest.mark.parametrize("ta,tb", GC.TRANS, ids=FORM_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_sgemm_equals_the_exact_product_and_stays_inside_the_bound(name, ta, tb):
    c = GC.CASES[name]
    f = GC.case_form(c, ta, tb)
    exact = Launch(c, ta, tb, GC.integer_operands(c, ta, tb))
    for use_bias, acc in GC.MODES:
        what = "%s %r bias %d accumulate %d" % (name, f, use_bias, acc)
        same(twice(lambda: exact.sgemm(use_bias, acc)), GC.reference(exact.o, use_bias, acc), what)
    scaled = Launch(c, ta, tb, GC.scaled_operands(c, ta, tb))
    for use_bias, acc in GC.MODES:
        what = "%s %r bias %d accumulate %d" % (name, f, use_bias, acc)
        bad, worst = GC.violations(twice(lambda: scaled.sgemm(use_bias, acc)), scaled.o, use_bias, acc, c.K)
        print("%s: worst |err| / bound = %.3f over %d elements (L = %d)" % (what, worst, c.M * c.N, c.K + 2))
        assert bad == 0, "%s: %d of %d elements outside the f32 sum bound (worst %.3g x the bound)" % (
            what, bad, c.M * c.N, worst)


@pytest.mark.parametrize("ta,tb", GC.TRANS, ids=FORM_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_dropout_epilogue_equals_its_float32_statement(name, ta, tb):
    c = GC.CASES[name]
    run = Launch(c, ta, tb, GC.integer_operands(c, ta, tb))
    assert GC.dropout_ldc(c, ta, tb) > c.N
    for p in (0.5, 0.2):
        keep = GC.keep_mask(c, p, ta, tb)
        kd = keep.to(DEV)
        assert kd.is_contiguous() and kd.shape == (c.M, c.N)
        got = twice(lambda: run.dropout(kd, p))
        what = "%s %r p %.1f" % (name, GC.case_form(c, ta, tb), p)
        same(got, GC.dropout_reference(run.o, keep, p), what)
        dropped = got[keep == 0]
        assert bool((dropped.view(torch.int32) == 0).all()), what + ": a dropped element is not +0"


@pytest.mark.parametrize("ta,tb", GC.TRANS, ids=FORM_IDS)
def test_k_zero_leaves_the_bias_or_zero(ta, tb):
    """K = 0: no operand access (sgemm_kernel's fetches are all predicated off); C = bias or 0, += under accumulate"""
    for name in ("reg-5x3x0", "reg-5x3x0-view"):
        c = GC.CASES[name]
        assert c.K == 0 and GC.case_form(c, ta, tb) == ("reg", ta, tb, 1)
        run = Launch(c, ta, tb, GC.integer_operands(c, ta, tb))
        o = run.o
        zero = torch.zeros(c.M, c.N)
        assert torch.equal(twice(lambda: run.sgemm(0, 0)), zero)
        assert torch.equal(twice(lambda: run.sgemm(1, 0)), zero + o.bias)
        assert torch.equal(twice(lambda: run.sgemm(0, 1)), o.old)
        assert torch.equal(twice(lambda: run.sgemm(1, 1)), o.old + o.bias)


# one case per form: the first view case that reaches it
NAN_CASES = {}
for _name in NAMES:
    for _ta, _tb in GC.TRANS:
        if GC.CASES[_name].view and GC.CASES[_name].K >= 1:
            NAN_CASES.setdefault(GC.case_form(GC.CASES[_name], _ta, _tb), _name)
assert sorted(NAN_CASES) == GC.ALL_FORMS


@pytest.mark.parametrize("f", GC.ALL_FORMS, ids=["%s%d%d-%d" % f for f in GC.ALL_FORMS])
def test_a_nan_in_the_last_row_and_k_poisons_exactly_its_row_or_column(f):
    """op(A)[M-1, K-1] and op(B)[K-1, N-1]: the row / column that the clamped loads read again for the rows past M / N,
    and the k piece they read again for the k past K"""
    name = NAN_CASES[f]
    c, (_, ta, tb, _) = GC.CASES[name], f
    assert GC.case_form(c, ta, tb) == f
    o = GC.integer_operands(c, ta, tb)
    ref = GC.reference(o, 1, 0)
    for which in "AB":
        A, B = o.A.clone(), o.B.clone()
        if which == "A":
            A[(c.K - 1, c.M - 1) if ta else (c.M - 1, c.K - 1)] = NAN
        else:
            B[(c.N - 1, c.K - 1) if tb else (c.K - 1, c.N - 1)] = NAN
        got = twice(lambda: Launch(c, ta, tb, o._replace(A=A, B=B)).sgemm(1, 0))
        poisoned = torch.zeros(c.M, c.N, dtype=torch.bool)
        if which == "A":
            poisoned[c.M - 1] = True
        else:
            poisoned[:, c.N - 1] = True
        what = "%s %r NaN in %s" % (name, f, which)
        assert torch.equal(torch.isnan(got), poisoned), "%s: %d NaN elements, %d expected" % (
            what, int(torch.isnan(got).sum()), int(poisoned.sum()))
        same(got[~poisoned], ref[~poisoned], what)


# ------------------------------------------------------------------------------------------------ refusals
def refusal_setup(ta, tb):
    c = GC.CASES["dma0-36x68x36-view"]
    run = Launch(c, ta, tb, GC.integer_operands(c, ta, tb))
    C = Placed((c.M, c.N, torch.float32), run.lc, HC.CANARY)
    keep = torch.ones(c.M, c.N, dtype=torch.uint8, device=DEV)
    good = dict(ta=ta, tb=tb, M=c.M, N=c.N, K=c.K, A=run.A, lda=run.la.ld, B=run.B, ldb=run.lb.ld, C=C, ldc=run.lc.ld)
    return c, run, C, keep, good


def launch(good, keep=None, p=0.2, **change):
    a = dict(good, **change)
    head = (a["ta"], a["tb"], a["M"], a["N"], a["K"], a["A"], a["lda"], a["B"], a["ldb"], a["C"], a["ldc"])
    if keep is None:
        return status("cova_sgemm", *head, None, 0)
    return status("cova_sgemm_dropout_bwd", *head, keep, float(p))


@pytest.mark.parametrize("ta,tb", GC.TRANS, ids=FORM_IDS)
def test_bad_arguments_are_refused_and_nothing_is_written(ta, tb):
    c, run, C, keep, good = refusal_setup(ta, tb)
    bad = [dict(M=-1), dict(N=-1), dict(K=-1), dict(A=None), dict(B=None), dict(C=None),
           # a leading dimension shorter than the operand's row (the buffers are those of the valid call: no access could
           # leave them either way)
           dict(lda=run.la.cols - 1), dict(ldb=run.lb.cols - 1), dict(ldc=c.N - 1)]
    for change in bad:
        for mask in (None, keep):
            assert launch(good, mask, **change) == BAD_ARG, (change, mask is not None)
    assert run.la.cols == (c.M if ta else c.K) and run.lb.cols == (c.K if tb else c.N)
    for which, lay, data in (("A", run.la, run.o.A), ("B", run.lb, run.o.B)):     # the shortest allowed is accepted: a dense operand
        dense = Placed(data, GC.Lay(lay.rows, lay.cols, lay.cols, 4))
        out = Placed((c.M, c.N, torch.float32), run.lc, HC.CANARY)
        assert launch(good, **{which: dense, "ld" + which.lower(): lay.cols, "C": out}) == 0
        assert GC.mismatches(out.view[:, :c.N], GC.reference(run.o, 0, 0)) == 0
    # the Dropout entry point's own arguments
    head = (ta, tb, c.M, c.N, c.K, run.A, run.la.ld, run.B, run.lb.ld, C, run.lc.ld)
    for mask, p in ((None, 0.2), (keep, -0.1), (keep, 1.0), (keep, 1.5)):
        assert status("cova_sgemm_dropout_bwd", *head, mask, p) == BAD_ARG, (mask is not None, p)
    torch.cuda.synchronize()
    assert bool((C.flat == HC.CANARY).all()), "a refused call wrote to C"
    # M == 0 or N == 0: accepted, nothing launched, nothing written
    for change in (dict(M=0), dict(N=0), dict(M=0, N=0)):
        assert launch(good, **change) == 0 and launch(good, keep, **change) == 0, change
    torch.cuda.synchronize()
    assert bool((C.flat == HC.CANARY).all()), "an empty product wrote to C"
    assert launch(good) == 0 and GC.mismatches(C.view[:, :c.N], GC.reference(run.o, 0, 0)) == 0      # the valid call itself
