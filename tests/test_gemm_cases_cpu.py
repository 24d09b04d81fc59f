"""Checks on the case table of tests/gemm_cases.py itself (no GPU): the cases reach all 20 kernel instantiations behind
cova_sgemm, the integer operands keep every partial sum exact, an honest float32 product passes both checkers (so the
references alone stay inside them), and the checkers flag every seeded fault -- a dropped or doubled k piece, a lost
k-group, a wrong epilogue, a pad column read, a row written twice.  The last test records the gap these files close: a
relative error of 1e-4 in the row of smallest scale violates the per-element bound and is invisible to the whole-matrix
gate of tests/test_kernels_gpu.py (helpers.close at SGEMM_TOL)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
import gemm_cases as GC  # noqa: E402
import helpers  # noqa: E402

NAMES = list(GC.CASES)


def test_the_cases_reach_all_twenty_forms():
    hit = {}
    for name, c in GC.CASES.items():
        forms = [GC.case_form(c, ta, tb) for ta, tb in GC.TRANS]
        print("%-34s %s" % (name, "  ".join("%s<%d,%d>%d" % f for f in forms)))
        for f in forms:
            hit.setdefault(f, set()).add((c.M, c.N, c.K))
    for f in GC.ALL_FORMS:
        print("%-22r %d shapes" % (f, len(hit.get(f, ()))))
    print("%d of %d forms" % (len(set(hit) & set(GC.ALL_FORMS)), len(GC.ALL_FORMS)))
    assert len(GC.ALL_FORMS) == 20 and sorted(hit) == GC.ALL_FORMS, sorted(set(GC.ALL_FORMS) ^ set(hit))
    assert all(len(hit[f]) >= 2 for f in GC.ALL_FORMS), {f: len(s) for f, s in hit.items()}
    # the groups land where the table says
    for name, c in GC.CASES.items():
        kinds = {GC.case_form(c, ta, tb)[0::3] for ta, tb in GC.TRANS}
        if name.startswith(("dma0-", "dma1-", "dma2-")) and c.option22:
            assert kinds == {("dma", int(name[3]))}, (name, kinds)
        else:
            assert kinds == {("reg", 2 if c.K >= 256 else 1)}, (name, kinds)
    # register kernel with vecA != vecB, both ways; the listed shapes are all there, in plain and view layout
    mixed = {(c.a_al, c.b_al) for c in GC.CASES.values() if c.a_al != c.b_al and c.K % 4 == 0}
    assert mixed == {(True, False), (False, True)}
    for shapes in (GC.DMA0, GC.DMA1, GC.DMA2, GC.REG, GC.MIXED):
        for s in shapes:
            assert {c.view for c in GC.CASES.values() if (c.M, c.N, c.K) == s} == {0, 1}, s
    assert GC.form(0, 0, 0, 5, 3, 0, 4, 0, 8) is None and GC.form(1, 1, 5, 0, 3, 0, 8, 0, 4) is None


def test_layouts_put_nan_on_every_side_and_keep_the_alignment_the_table_names():
    for c in GC.CASES.values():
        for ta, tb in GC.TRANS:
            A, B, C = GC.layout(c, ta, tb)
            assert (A.off % 4 == 0) == c.a_al and (B.off % 4 == 0) == c.b_al and (C.off % 4 == 0) == (c.a_al and c.b_al)
            for lay in (A, B, C):
                assert lay.off > 0 and lay.ld >= lay.cols and (lay.ld > lay.cols) == bool(c.view)
            if c.view:
                assert {A.ld - A.cols, B.ld - B.cols, C.ld - C.cols} == {8}
                assert A.off - 4 == (4 if c.a_al else 3) and B.off - 4 == (4 if c.b_al else 5)      # the column offset
            assert GC.dropout_ldc(c, ta, tb) > c.N


@pytest.mark.parametrize("name", NAMES)
def test_integer_operands_keep_every_partial_sum_exact(name):
    c = GC.CASES[name]
    assert GC.exact_ok(c)
    o = GC.integer_operands(c, 0, 1)
    for t, lim in ((o.A, 8), (o.B, 8), (o.bias, 1000), (o.old, 1000)):
        assert torch.equal(t, t.round()) and (t.numel() == 0 or (0 < float(t.abs().min()) and float(t.abs().max()) <= lim))
    worst = GC.magnitude(o, 1, 1)
    assert worst.numel() and float(worst.max()) <= 64 * c.K + 2000 < 2 ** 24
    s = GC.scaled_operands(c, 1, 0)
    for t in (s.A, s.B, s.bias, s.old):
        if t.numel():
            assert 2.0 ** -21 <= float(t.abs().min()) and float(t.abs().max()) < 2.0 ** 20     # normal numbers only
    if c.M >= 2 and c.N >= 2 and c.K >= 1:
        rows = s.opA.abs().max(1).values
        assert float(rows.max() / rows.min()) >= 2.0 ** 19 and float(s.old.abs().max() / s.old.abs().min()) >= 2.0 ** 38


@pytest.mark.parametrize("name", NAMES)
def test_an_honest_float32_product_passes_both_checkers(name):
    c = GC.CASES[name]
    for ta, tb in GC.TRANS:
        for kind, make in (("integer", GC.integer_operands), ("scaled", GC.scaled_operands)):
            o = make(c, ta, tb)
            prod = torch.matmul(o.A.t() if ta else o.A, o.B.t() if tb else o.B)             # float32 on the CPU
            assert prod.dtype == torch.float32 and prod.shape == (c.M, c.N)
            for use_bias, acc in GC.MODES:
                got = prod
                if use_bias:
                    got = got + o.bias
                if acc:
                    got = got + o.old
                if kind == "integer":
                    assert GC.mismatches(got, GC.reference(o, use_bias, acc)) == 0, (name, ta, tb, use_bias, acc)
                    assert GC.mismatches(GC.emulate(o, c, ta, tb, use_bias, acc), GC.reference(o, use_bias, acc)) == 0
                else:
                    bad, worst = GC.violations(got, o, use_bias, acc, c.K)
                    assert bad == 0 and worst <= 1.0, (name, ta, tb, use_bias, acc, bad, worst)
                    assert GC.violations(GC.emulate(o, c, ta, tb, use_bias, acc), o, use_bias, acc, c.K)[0] == 0
    o = GC.integer_operands(c, 0, 0)
    for p in (0.5, 0.2):
        keep = GC.keep_mask(c, p)
        ref = GC.dropout_reference(o, keep, p)
        assert ref.dtype == torch.float32 and bool((ref[keep == 0] == 0).all())
        assert torch.equal(ref, torch.where(keep != 0, (o.opA @ o.opB).float() * float(GC.einv32(p)), torch.zeros(())))
        if c.M >= 2 and c.N >= 2:
            assert not keep[(c.M - 1) // 2].any() and not keep[:, c.N - 1].any() and keep.any()


@pytest.mark.parametrize("name", NAMES)
def test_every_seeded_fault_is_flagged(name):
    c = GC.CASES[name]
    table = []
    for ta, tb in GC.TRANS:
        oi, os_ = GC.integer_operands(c, ta, tb), GC.scaled_operands(c, ta, tb)
        for fault in GC.FAULTS:
            for use_bias, acc in GC.MODES:
                if not GC.expressible(fault, c, use_bias, acc):
                    continue
                n_exact = GC.mismatches(GC.emulate(oi, c, ta, tb, use_bias, acc, fault), GC.reference(oi, use_bias, acc))
                n_bound = GC.violations(GC.emulate(os_, c, ta, tb, use_bias, acc, fault), os_, use_bias, acc, c.K)[0]
                table.append((fault, ta, tb, use_bias, acc, n_exact, n_bound))
                assert n_exact > 0 and n_bound > 0, (name, fault, ta, tb, use_bias, acc, n_exact, n_bound)
        ldc = GC.dropout_ldc(c, ta, tb)
        for p in (0.5, 0.2):
            keep = GC.keep_mask(c, p, ta, tb)
            assert GC.mismatches(GC.emulate_dropout(oi, c, keep, p, ldc), GC.dropout_reference(oi, keep, p)) == 0
            if GC.expressible("mask_indexed_with_ldc", c):
                n = GC.mismatches(GC.emulate_dropout(oi, c, keep, p, ldc, "mask_indexed_with_ldc"),
                                  GC.dropout_reference(oi, keep, p))
                table.append(("mask_indexed_with_ldc p=%.1f" % p, ta, tb, 0, 0, n, -1))
                assert n > 0, (name, ta, tb, p)
    seen = {}
    for fault, *_, n_exact, n_bound in table:
        a = seen.setdefault(fault, [0, 10 ** 9, 10 ** 9])
        a[0], a[1], a[2] = a[0] + 1, min(a[1], n_exact), min(a[2], n_bound)
    for fault, (runs, lo_e, lo_b) in seen.items():
        print("%-30s %-28s flagged in %3d of %3d runs (fewest elements: exact %d, bound %d)" % (name, fault, runs, runs,
                                                                                               lo_e, lo_b))
    want = [f for f in GC.FAULTS + GC.DROPOUT_FAULTS if GC.expressible(f, c)]
    assert sorted({k.split(" ")[0] for k in seen}) == sorted(want)


def test_every_fault_is_expressed_somewhere_and_most_everywhere():
    for f in GC.FAULTS + GC.DROPOUT_FAULTS:
        n = sum(GC.expressible(f, GC.CASES[name]) for name in NAMES)
        print("%-24s expressible on %d of %d cases" % (f, n, len(NAMES)))
        assert n >= len(NAMES) // 2


# A relative error r in one element shows against the bound only where r |ref| > (K + 6) u mag.  For these operands
# |ref| is about 1.04 mag / sqrt(K) at one standard deviation (E|ab| = 0.5625, E(ab)^2 = 0.34 for a, b uniform in
# +-[0.5, 1)), so r = 1e-4 is resolved where (K + 6) sqrt(K) < 1e-4 * 1.04 * 2^24 = 1745: K <= 96 with a factor 1.7 to
# spare at K = 96.  Beyond that the worst-case bound of a K-term f32 sum is itself wider than 1e-4 of the result; the
# figure is printed there and not asserted.  For K > 96 the check that carries such a fault is the element-for-element
# compare on the integer operands, where any error at all in any row is a mismatch.
SMALL_ROW_K = 96


@pytest.mark.parametrize("name", [n for n in NAMES if GC.CASES[n].M >= 2 and GC.CASES[n].K >= 1])
def test_an_error_in_the_smallest_row_violates_the_bound_and_escapes_the_whole_matrix_gate(name):
    c = GC.CASES[name]
    for ta, tb in GC.TRANS:
        o = GC.scaled_operands(c, ta, tb)
        row = GC.smallest_row(o)
        for use_bias, acc in GC.MODES:
            got = GC.emulate(o, c, ta, tb, use_bias, acc)
            assert GC.violations(got, o, use_bias, acc, c.K)[0] == 0
            got[row] *= 1.0 + 1e-4
            bad, worst = GC.violations(got, o, use_bias, acc, c.K)
            ratio = helpers.close(got, GC.reference(o, use_bias, acc).float(), helpers.SGEMM_TOL,
                                  "%s <%d,%d> bias %d acc %d (the old gate)" % (name, ta, tb, use_bias, acc))
            print("%s <%d,%d> bias %d acc %d: row %d, %d of %d elements outside the bound, worst %.2f x; the old gate "
                  "sees %.1e of %.1e" % (name, ta, tb, use_bias, acc, row, bad, c.N, worst, ratio, helpers.SGEMM_TOL))
            assert ratio <= helpers.SGEMM_TOL / 10           # helpers.close did not raise: blind, with a decade to spare
            if c.K <= SMALL_ROW_K:
                assert bad > 0 and worst > 1.0, (name, ta, tb, use_bias, acc)
