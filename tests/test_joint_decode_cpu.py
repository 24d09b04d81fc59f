"""Joint page decoding without a GPU: the numpy oracle (tests/decode_oracle.py) against the assignment optimum and against
full enumeration, the pages the definition treats one by one, the conflict share of the GPU test's inputs, EvalReport's
plumbing of the joint tables, the argument checks and the declared entry point."""
import ctypes
import itertools
import types

import numpy as np
import pytest

from cova_web_object_detection_amd import _lib, engine, evaluation
from cova_web_object_detection_amd.evaluation import EvalReport
import decode_cases as DC
import decode_oracle as DO

INF, NAN = np.inf, np.nan


def test_entry_point_is_declared_and_exported():
    protos = _lib.parse_header()
    assert len(protos["cova_page_joint_decode"]) == 12           # the stream included
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "cova_page_joint_decode")


def random_page(rs, n, nc, quantised):
    logits, _ = DC.objectness_page(rs, n, nc)
    return (np.round(logits * 2) / 2).astype(np.float32) if quantised else logits


# ---------------------------------------------------------------- the optimum
@pytest.mark.parametrize("score_mode", [0, 1])
def test_oracle_total_is_the_assignment_optimum(score_mode):
    """The candidate lists lose nothing: the best total over them is scipy's optimum over the whole page.  Both are
    float64 sums of at most 6 float32 scores of magnitude < 32 (each sum rounds by at most 2^-48 relative): 1e-9 absolute
    is far above any difference of summation order and far below the 0.5 grid of the quantised pages."""
    optimize = pytest.importorskip("scipy.optimize", reason="scipy is needed for the assignment optimum")
    rs = np.random.RandomState(100 + score_mode)
    differ = 0
    for case in range(120):
        C = 1 + case % 6
        n = int(rs.randint(C, 121))
        logits = random_page(rs, n, C + 1, quantised=case % 2 == 1)
        choice, gap, best = DO.decode_page(logits, score_mode)
        s = DO.scores(logits, score_mode).astype(np.float64)
        rows, cols = optimize.linear_sum_assignment(s, maximize=True)
        assert abs(best - s[rows, cols].sum()) <= 1e-9, (case, C, n)
        assert len(set(choice)) == C and gap >= 0
        assert abs(sum(s[b, k] for k, b in enumerate(choice)) - best) <= 1e-9
        differ += choice != DO.column_page(logits, score_mode)
    assert differ >= 40                                           # and it is not the column decision in disguise


# ---------------------------------------------------------------- the gap
def enumerate_page(logits, score_mode):
    """(best total, best of the others) over every injective choice of boxes, sums in class order."""
    s = DO.scores(logits, score_mode)
    n, C = s.shape
    totals = sorted((DO.total([s[b, k] for k, b in enumerate(boxes)]) for boxes in itertools.permutations(range(n), C)),
                    reverse=True)
    return totals[0], (totals[1] if len(totals) > 1 else None)


def test_oracle_gap_is_the_gap_of_full_enumeration():
    rs = np.random.RandomState(7)
    seen_zero = seen_positive = 0
    for case in range(300):
        C = 1 + case % 3
        n = int(rs.randint(C, 9))
        if case % 2:
            logits = rs.randint(-3, 4, (n, C + 1)).astype(np.float32)          # integer scores: ties everywhere
        else:
            logits = random_page(rs, n, C + 1, False)
        for mode in (0, 1):
            _, gap, best = DO.decode_page(logits, mode)
            ref_best, ref_other = enumerate_page(logits, mode)
            assert best == ref_best, (case, mode)
            assert gap == (INF if ref_other is None else DO.gap_of(ref_best, ref_other)), (case, mode, n, C)
            seen_zero += gap == 0
            seen_positive += 0 < gap < INF
    assert seen_zero > 50 and seen_positive > 50


# ---------------------------------------------------------------- the inputs of the GPU test
def test_gpu_cases_put_the_joint_and_the_column_decision_apart():
    apart = servable = 0
    for name, case in DC.gpu_cases().items():
        choice, _, _ = DC.oracle_tables(name)
        C = case["nc"] - 1
        for p, (logits, _) in enumerate(DC.pages_of(case)):
            if logits.shape[0] >= C:
                servable += 1
                apart += choice[p].tolist() != DO.column_page(logits, case["score_mode"])
    print("joint != column on %d of %d pages with n >= C" % (apart, servable))
    assert servable == 38 and 2 * apart >= servable              # 16 + 14 + 3 + 4 + 1 pages can serve every class


def test_gpu_cases_cover_the_sizes_and_the_unlabelled_convention():
    cases = DC.gpu_cases()
    assert cases["nc4_mode0"]["sizes"] == [0, 1, 2, 3, 4, 5, 63, 64, 65, 90, 300] == cases["nc4_mode1"]["sizes"]
    assert cases["nc7"]["sizes"] == [0, 5, 6, 7, 8, 130] and cases["nc4_2500"]["sizes"] == [2500]
    assert np.array_equal(cases["nc4_mode0"]["logits"], cases["nc4_mode1"]["logits"])
    for name in cases:
        _, hit, _ = DC.oracle_tables(name)
        assert set(np.unique(hit).tolist()) <= {-1, 0, 1}
    _, hit, _ = DC.oracle_tables("nc4_mode1")
    assert (hit == -1).any() and (hit == 0).any() and (hit == 1).any()
    assert hit[7].tolist()[2] == -1 and (hit[0] == -1).all()                   # the page without class 3, the empty page
    # with one class the joint decision is the column decision
    case = cases["nc2"]
    choice, _, gap = DC.oracle_tables("nc2")
    for p, (logits, _) in enumerate(DC.pages_of(case)):
        assert choice[p].tolist() == DO.column_page(logits, 1)
    assert gap.tolist()[:2] == [INF, INF] and 0 <= gap[2] < INF


# ---------------------------------------------------------------- the pages the definition treats one by one
def test_special_pages():
    sp = DC.special_pages()
    for mode in (0, 1):
        assert DO.decode_page(sp["empty"][0], mode)[:2] == ([-1, -1, -1], INF)
        for name in ("fewer_boxes_than_classes", "one_box"):
            choice, gap, _ = DO.decode_page(sp[name][0], mode)
            assert choice == DO.column_page(sp[name][0], mode) and gap == INF
        assert DO.decode_page(sp["one_box"][0], mode)[0] == [0, 0, 0]
        # n = C: every assignment is a permutation of the page
        logits = sp["as_many_boxes_as_classes"][0]
        choice, gap, best = DO.decode_page(logits, mode)
        ref_best, ref_other = enumerate_page(logits, mode)
        assert sorted(choice) == [0, 1, 2] and best == ref_best and gap == DO.gap_of(ref_best, ref_other)
        # all scores equal: the lexicographically smallest rank tuple with distinct boxes
        assert DO.decode_page(sp["all_scores_equal"][0], mode)[:2] == ([0, 1, 2], 0.0)
        # one box leads every column: the column decision names it three times, the joint one once
        logits = sp["one_box_leads_every_column"][0]
        choice, gap, _ = DO.decode_page(logits, mode)
        assert DO.column_page(logits, 0) == [5, 5, 5] and choice.count(5) <= 1 and len(set(choice)) == 3
        # -inf and NaN entries, a column that is all NaN: NaN scores count as -inf, the choice stays a valid assignment
        logits = sp["minus_inf_and_nan"][0]
        choice, gap, best = DO.decode_page(logits, mode)
        assert len(set(choice)) == 3 and best == -INF and gap == 0.0
        assert choice[1] == min(set(range(9)) - {choice[0]})           # the all-NaN column orders by index alone
        # +inf in one class against -inf in another: every total is NaN, which counts as -inf
        choice, gap, best = DO.decode_page(sp["plus_inf_against_minus_inf"][0], mode)
        assert (choice, gap, best) == ([0, 1, 2], 0.0, -INF)
        choice, gap, best = DO.decode_page(sp["mixed_infinities"][0], mode)
        assert choice[0] == 2 and choice[1] != 1 and best == INF and gap == 0.0
    s = DO.scores(np.array([[NAN, 1.0, INF], [INF, INF, 2.0], [1.0, NAN, -INF]], np.float32), 1)
    assert s.tolist() == [[-INF, -INF], [-INF, -INF], [-INF, -INF]]
    lab = np.array([0, 2, 1, 0, 5, -1])
    lg = np.zeros((6, 4), np.float32)
    lg[[2, 1, 3], [1, 2, 3]] = 1.0
    choice, hit, gap = DO.joint_decode(lg, lab, [0, 6], 4)
    assert choice.tolist() == [[2, 1, 3]] and hit.tolist() == [[1, 1, -1]] and gap.tolist() == [1.0]


# ---------------------------------------------------------------- EvalReport
def joint_report(with_tables=True):
    ranks = np.array([[0, 2, -1], [1, 0, 0], [-2, -2, -2], [0, 0, 3]], dtype=np.int32)
    top1 = np.array([[4, 4, 4], [2, 5, 6], [-2, -2, -2], [1, 7, 1]], dtype=np.int32)
    kw = {}
    if with_tables:
        kw = dict(joint_top1=np.array([[4, 3, 1], [9, 5, 6], [-2, -2, -2], [1, 7, 2]], dtype=np.int32),
                  joint_hit=np.array([[1, 1, -1], [1, 1, 0], [-2, -2, -2], [0, 1, 1]], dtype=np.int32),
                  joint_gap=np.array([0.5, INF, -1.0, 0.0]))
    return EvalReport(ranks, top1, ["10", "11", "12", "13"], seconds=1.5, **kw)


def test_report_hits_and_accuracies_follow_the_mode():
    rep = joint_report()
    assert rep.hits(1).tolist() == [[True, False, False], [False, True, True], [False] * 3, [True, True, False]]
    assert rep.hits(1, "joint").tolist() == [[True, True, False], [True, True, False], [False] * 3, [False, True, True]]
    assert rep.img_acc(1, "joint").tolist() == [[10, 1, 1, 0], [11, 1, 1, 0], [13, 0, 1, 1]]
    assert rep.class_acc(1, "joint").tolist() == [0.0, 2 / 3 * 100, 100.0, 1 / 3 * 100]
    assert rep.class_acc(1).tolist() == [0.0, 2 / 3 * 100, 2 / 3 * 100, 1 / 3 * 100]
    info = np.array([[10, "a"], [11, "a"], [13, "b"], [14, "b"]])
    n, acc = rep.domainwise(info, ["a", "b"], decode="joint")
    assert n.tolist() == [2, 2] and acc.tolist() == [[100.0, 100.0, 0.0], [0.0, 100.0, 100.0]]
    assert rep.macro_acc(info, ["a", "b"], decode="joint").tolist() == [0.0, 50.0, 100.0, 50.0]
    assert rep.log_lines("VAL", decode="joint")[:2] == ["[VAL] Avg_class_Accuracy: 66.67% (1.50s)", "Price top-1-Acc: 66.67%"]
    assert rep.macro_log_lines(info, ["a", "b"], decode="joint")[1] == "Title Macro Acc: 100.00%"
    assert rep.joint_gap.dtype == np.float64 and rep.joint_hit.dtype == np.int32 == rep.joint_top1.dtype


def test_report_refuses_what_joint_cannot_answer():
    rep = joint_report()
    with pytest.raises(ValueError, match="k must be 1"):
        rep.hits(3, "joint")
    with pytest.raises(ValueError, match="k must be 1"):
        rep.class_acc(2, "joint")
    with pytest.raises(ValueError, match="no joint tables"):
        joint_report(False).hits(1, "joint")
    with pytest.raises(ValueError, match="no joint tables"):
        joint_report(False).log_lines("VAL", decode="joint")
    with pytest.raises(ValueError, match="decode must be"):
        rep.hits(1, "hungarian")
    with pytest.raises(ValueError, match="shape of ranks"):
        EvalReport(np.zeros((2, 3), np.int32), joint_hit=np.zeros((2, 2), np.int32))
    with pytest.raises(ValueError, match="one value per page"):
        EvalReport(np.zeros((2, 3), np.int32), joint_gap=np.zeros(3))


def test_merge_folds_the_joint_tables_of_two_half_filled_reports():
    whole = joint_report()
    whole.joint_top1[2], whole.joint_hit[2], whole.joint_gap[2] = [0, 1, 2], [1, 0, -1], 2.5
    whole.ranks[2], whole.top1[2] = [0, 1, -1], [0, 0, 0]

    def half(pages):
        tabs = {}
        for name, fill in (("ranks", -2), ("top1", -2), ("joint_top1", -2), ("joint_hit", -2), ("joint_gap", -1.0)):
            t = np.full_like(getattr(whole, name), fill)
            t[pages] = getattr(whole, name)[pages]
            tabs[name] = t
        return EvalReport(tabs.pop("ranks"), tabs.pop("top1"), whole.img_ids, **tabs)
    merged = EvalReport.merge([half([0, 3]), half([1, 2])])
    for name in ("ranks", "top1", "joint_top1", "joint_hit", "joint_gap"):
        assert np.array_equal(getattr(merged, name), getattr(whole, name)), name
    assert merged.joint_gap[1] == INF and merged.hits(1, "joint").tolist() == whole.hits(1, "joint").tolist()
    # a report without the tables among them: the merged one has none either
    plain = EvalReport.merge([half([0, 3]), joint_report(False)])
    assert plain.joint_hit is None and plain.joint_top1 is None and plain.joint_gap is None


def test_default_outputs_do_not_see_the_joint_tables(tmp_path):
    with_tables, without = joint_report(), joint_report(False)
    info = np.array([[10, "a"], [11, "a"], [13, "b"], [14, "b"]])
    for tag, rep in (("j", with_tables), ("c", without)):
        rep.write_imgwise_csv(tmp_path / (tag + "_i.csv"), 1)
        rep.write_domainwise_csv(tmp_path / (tag + "_d.csv"), info, ["a", "b"], k=3)
    for f in ("_i.csv", "_d.csv"):
        assert (tmp_path / ("j" + f)).read_bytes() == (tmp_path / ("c" + f)).read_bytes()
    for k in (1, 3):
        assert with_tables.log_lines("VAL", k) == without.log_lines("VAL", k)
        assert with_tables.macro_log_lines(info, ["a", "b"], k) == without.macro_log_lines(info, ["a", "b"], k)
        assert np.array_equal(with_tables.img_acc(k), without.img_acc(k))
    # and the joint mode of the writers does differ
    with_tables.write_imgwise_csv(tmp_path / "jj_i.csv", 1, decode="joint")
    assert (tmp_path / "jj_i.csv").read_bytes() != (tmp_path / "j_i.csv").read_bytes()
    assert (tmp_path / "jj_i.csv").read_text().splitlines()[1] == "10,1.00,1.00,0.00"


# ---------------------------------------------------------------- argument checks
def test_check_decode():
    assert engine.check_decode("column", "map", 16, k=5) == 1 and engine.check_decode("joint", "logit", 7) == 0
    assert engine.check_decode("joint", "map", 2) == 1
    with pytest.raises(ValueError, match="decode must be"):
        engine.check_decode("both", "map", 4)
    with pytest.raises(ValueError, match="score must be"):
        engine.check_decode("joint", "softmax", 4)
    with pytest.raises(ValueError, match="score must be"):
        engine.check_decode("column", "softmax", 4)
    with pytest.raises(ValueError, match="k must be 1"):
        engine.check_decode("joint", "map", 4, k=3)
    with pytest.raises(ValueError, match="2..7 classes"):
        engine.check_decode("joint", "map", 8)


def test_host_calls_refuse_before_any_device_work():
    """The checks come first: a stand-in trainer with no device behind it is enough to reach them."""
    tr = types.SimpleNamespace(cfg=dict(n_classes=8), device="cpu", metrics=None)
    for call in (lambda: evaluation.evaluate_split(tr, [], decode="joint"),
                 lambda: evaluation.predict_split(tr, [], decode="joint"),
                 lambda: evaluation.fit(tr, None, None, 2, 3, decode="joint")):
        with pytest.raises(ValueError, match="2..7 classes"):
            call()
    tr.cfg["n_classes"] = 4
    with pytest.raises(ValueError, match="k must be 1"):
        evaluation.fit(tr, None, None, 2, 3, k=3, decode="joint")
    with pytest.raises(ValueError, match="score must be"):
        evaluation.fit(tr, None, None, 2, 3, decode="joint", decode_score="prob")
    with pytest.raises(ValueError, match="decode must be"):
        evaluation.evaluate_split(tr, [], decode="rows")
    with pytest.raises(ValueError, match="score must be"):
        evaluation.predict_split(tr, [], score="prob")
    from cova_web_object_detection_amd.trainer import HotPathTrainer
    stub = types.SimpleNamespace(cfg=dict(n_classes=8))
    with pytest.raises(ValueError, match="2..7 classes"):
        HotPathTrainer.evaluate.__wrapped__(stub, {}, None, decode="joint")
    stub.cfg["n_classes"] = 4
    with pytest.raises(ValueError, match="k must be 1"):
        HotPathTrainer.evaluate.__wrapped__(stub, {}, None, k=2, decode="joint")
