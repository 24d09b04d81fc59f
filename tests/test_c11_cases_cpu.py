"""Checks on tests/c11_cases.py itself (no GPU): the table reaches every instantiation the restated dispatch of
csrc/conv1x1.hip and csrc/conv1x1_lin.hip can launch and every path of the three restated walks, its operands keep
every accumulated quantity exact (``exact_ok``), the masks keep, drop and sit exactly on the threshold often enough, the
references agree with a second, tile-by-tile evaluation, and the checkers flag every seeded fault on the table's own
cases.

Faults no checker of this suite can see, and why:
  * a stale prefetch, a skipped tile, a clamped row counted: only on walks that have a later trip / a ragged tile
    (``fault_applies``); on the other walks of a form the fault does not exist.
  * the unfused mask decision: the lattice makes msc * z exact, so fused and unfused agree everywhere but in channel
    FMA_CH, which carries the one off-lattice triple; a kernel wrong only in other channels' rounding cannot be seen.
  * the split of a statistics sum among the WAVES of a block (the LDS fold) is internal: only the block's row is
    visible.  The per-block workspaces of the weight gradient and of vprod are internal too: dw and lin are checked."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
import c11_cases as CC  # noqa: E402
import split_probe as sp  # noqa: E402

F64 = np.float64
MULTI = [(613, 1), (613, 2), (773, 1), (869, 2)]           # the walks with a later trip


def test_the_table_reaches_every_form_and_refuses_what_the_host_refuses():
    reached = collections_of_forms()
    for name, s in CC.SPECS.items():
        print("%-34s %s %s%s" % (name, tuple(s.form), CC.derived(s.form), "  [step]" if s.step else ""))
    assert sorted(reached["c11"]) == sorted(CC.ALL_C11) and len(CC.ALL_C11) == 18 + 15 + 2 + 2 + 2
    assert sorted(reached["wgrad"]) == sorted(CC.ALL_WGRAD) and len(CC.ALL_WGRAD) == 12
    assert len(CC.ALL_FORMS) == len(set(CC.ALL_FORMS)) == len(CC.ALL_C11) + 13
    epi2 = [s for s in CC.SPECS.values() if s.form.epi == 2 and not s.form.ext]
    assert len(epi2) == 15
    # the runtime switches: both mask sources of the sum-free gradient, side_bits null and given, ReLU on and off
    assert {s.mask for s in CC.SPECS.values() if s.form.epi == 3} == {"act", "bits"}
    assert {(s.form.epi, s.bits) for s in CC.SPECS.values() if s.form.side} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {s.relu for s in CC.WGRAD_SPECS.values() if s.pa} == {0, 1}
    assert {(s.abc, s.relu) for s in CC.VPROD_SPECS.values()} == {(0, 0), (1, 0), (1, 1)}
    for name, s in CC.SPECS.items():
        if s.form.pro and not s.form.side:
            assert {c.relu for c in CC.c11_cases(name)} == {0, 1}, name
    # every derived flag of conv1x1_kernel in both states
    flags = [CC.derived(s.form) for s in CC.SPECS.values()]
    for k in ("BF", "PREFETCH", "TR", "EARLY"):
        assert {f[k] for f in flags} == {False, True}, k
    step = [n for n, s in CC.SPECS.items() if s.step]
    print("forms the train step launches: %s" % step)
    assert len(step) == 3 * 2 + 4 + 2 + 2 + 1
    for entry, kw in CC.REFUSALS:
        assert CC.form(entry, **kw) == CC.BAD_ARG, (entry, kw)
    assert len(CC.REFUSALS) == len({(e, tuple(sorted(kw.items()))) for e, kw in CC.REFUSALS})


def collections_of_forms():
    reached = {"c11": [], "wgrad": []}
    for name, s in CC.SPECS.items():
        f = CC.spec_form(s)
        assert f == s.form, (name, f, s.form)
        if f not in reached["c11"]:
            reached["c11"].append(f)
    for name, s in CC.WGRAD_SPECS.items():
        f = CC.wgrad_form(s.co, s.ci, dz2=s.pz, dz_abc=s.pz, act_abc=s.pa)
        assert f == ("wgrad", s.co, s.ci, s.pz, s.pa)
        if f not in reached["wgrad"]:
            reached["wgrad"].append(f)
    return reached


def test_the_walks_reach_every_path():
    p = {}
    for R, cap in CC.C11_WALKS:
        w = CC.C11Walk(R, cap)
        p[(R, cap)] = w.paths()
        print("conv1x1 R %4d cap %d: %2d tiles, grid %d, stride %2d, trips of block 0 %s: %s" % (
            R, cap, w.ntiles, w.grid, w.stride, [len(w.tiles_of(0, i)) for i in range(8)], sorted(p[(R, cap)])))
    reached = set().union(*p.values())
    assert CC.C11_REQUIRED <= reached, CC.C11_REQUIRED - reached
    assert {"ragged-even-tile", "ragged-odd-tile"} <= reached
    # the issue's own figures
    w = CC.C11Walk(613, 1)
    assert w.ntiles == 20 and [len(w.tiles_of(0, i)) for i in range(8)] == [3, 3, 3, 3, 2, 2, 2, 2] and w.owner(19) == (0, 3, 2)
    w = CC.C11Walk(773, 1)
    assert w.ntiles == 25 and [len(w.tiles_of(0, i)) for i in range(8)] == [4, 3, 3, 3, 3, 3, 3, 3]
    assert CC.C11Walk(40013).grid == 157                   # the largest map of the tolerance tests: one tile per wave
    # the added shape: the ragged tile on a later trip of an odd block is reached by (869, 2) alone
    assert [k for k, v in p.items() if "ragged-later-trip-odd-block" in v] == [(869, 2)]
    assert CC.C11Walk(869, 2).owner(27) == (1, 3, 1)
    for units in (1, 4):
        reached = set()
        for R, cap in CC.WGRAD_WALKS + [CC.WGRAD_EMPTY_BLOCK]:
            w = CC.WgradWalk(R, units, cap)
            reached |= w.paths()
            rows = sorted(r for b in range(w.grid) for r in range(2 * w.block(b)[0], min(2 * w.block(b)[1], R)))
            assert rows == list(range(R)) and len(set(w.tail_rows())) == len(w.tail_rows())
            print("wgrad units %d R %4d cap %2d: grid %2d, %3d pairs per block, block 0 %s: %s" % (
                units, R, cap, w.grid, w.per, [(n, len(t)) for n, _, t in w.block(0)[2]], sorted(w.paths())))
        assert CC.WGRAD_REQUIRED[units] <= reached, (units, CC.WGRAD_REQUIRED[units] - reached)
    assert "empty-block" in CC.WgradWalk(*CC.WGRAD_EMPTY_BLOCK[:1], 1, CC.WGRAD_EMPTY_BLOCK[1]).paths()
    assert not any("empty-block" in CC.WgradWalk(R, 1, cap).paths() for R, cap in CC.WGRAD_WALKS)
    assert "empty-block" in CC.WgradWalk(101400, 1).paths()          # ... which full-size maps have without a cap
    reached = set()
    for R, cap in CC.VPROD_WALKS:
        w = CC.VprodWalk(R, cap)
        reached |= w.paths()
        print("vprod R %4d cap %2d: %2d steps, grid %2d, %d per block: %s" % (R, cap, w.nsteps, w.grid, w.per, sorted(w.paths())))
    assert CC.VPROD_REQUIRED <= reached, CC.VPROD_REQUIRED - reached
    assert {"ragged-even-block", "ragged-odd-block"} <= reached
    assert [k for k in CC.VPROD_WALKS if "empty-block" in CC.VprodWalk(*k).paths()] == [(1577, 12)]
    assert "empty-block" in CC.VprodWalk(160000).paths()


@pytest.mark.parametrize("name", list(CC.SPECS))
def test_c11_operands_are_exact_masks_are_hard_and_every_fault_is_flagged(name):
    s = CC.SPECS[name]
    worst, shares, seen = {}, [], set()
    for case in CC.c11_cases(name):
        o = CC.c11_operands(case)
        budget = CC.c11_budget(case, o)
        assert CC.exact_ok(case, o), (case, budget)
        for k, v in budget.items():
            worst[k] = max(worst.get(k, 0.0), v)
        ref = CC.c11_ref(case, o)
        for k, v in ref.items():                                 # the reference is made of f32 numbers
            assert k == "side_bits" or np.array_equal(v.astype(np.float32).astype(F64), v), (case, k)
        # every non-identity constant is there
        if s.form.pro and not s.form.ext:
            assert len(set(np.abs(o["abc"][0]))) > 1 and o["abc"][0].all() and o["abc"][2].all()
            assert np.isnan(o["abc"][1]).all() if s.form.pro == 1 else o["abc"][1].all()
            if case.relu and case.R >= 8:
                pre = CC.prologue(s.form, o, 0)[0]
                assert 0.1 < (pre < 0).mean() < 0.9
        if s.form.ext:
            assert o["cvec"].all() and o["m"].any() and o["abc3"][0].all() and len(set(np.abs(o["abc"][0]))) > 1
        if s.form.add:
            assert o["addend"].all()
        if s.form.epi == 2:
            assert len(set(o["mean"])) > 1 and len(set(o["invstd"])) > 1
            if s.form.x2:
                assert len(set(o["mean2"])) > 1 and len(set(o["invstd2"])) > 1 and not np.array_equal(o["z"], o["z2"])
        if s.mask and case.R >= 31:
            m = CC.mask_shares(case, o)
            shares.append(m)
            assert m["kept"] >= 0.25 and m["dropped"] >= 0.25, (case, m)
            if s.mask == "fma":
                assert m["zero"] >= 0.05, (case, m)
            else:
                assert m["neg_zero"] and m["pos_zero"], (case, m)
        if s.mask == "bits":
            assert np.array_equal(o["act_bits"], CC.pack_bits(o["act"]))
        # a second evaluation, tile by tile in the order of the walk, gives the same values
        emu = CC.c11_emulate(case, o)
        assert CC.check_c11(case, emu, ref) == [], case
        # the product goes through the bf16-split emulation of tests/split_probe.py unchanged
        if case.R == 33 and not s.form.ext:
            import torch
            x = torch.from_numpy(CC.prologue(s.form, o, case.relu)[0]).float()
            y = sp.emulate(sp.pieces(x), sp.pieces(torch.from_numpy(o["w"])))
            assert np.array_equal(y.double().numpy(), x.double().numpy() @ o["w"].astype(F64).T)
        for fault in CC.C11_FAULTS:
            if CC.fault_applies(fault, case):
                msgs = CC.check_c11(case, CC.c11_emulate(case, o, fault), ref)
                assert msgs, "%s passes the checker on %s" % (fault, (case,))
                seen.add(fault)
    print("%s: largest budget %s of 2^24 = %.3g; faults flagged: %s" % (
        name, {k: "%.3g" % v for k, v in worst.items()}, CC.LIMIT, sorted(seen)))
    if shares:
        print("   smallest mask shares: kept %.3f dropped %.3f zero %s" % (
            min(m["kept"] for m in shares), min(m["dropped"] for m in shares),
            min((m["zero"] for m in shares if m["zero"] is not None), default=None)))
    expected = {f for f in CC.C11_FAULTS if any(CC.fault_applies(f, c) for c in CC.c11_cases(name))}
    assert seen == expected


def test_every_conv1x1_fault_is_flagged_on_some_case():
    flagged = {f for name in CC.SPECS for c in CC.c11_cases(name) for f in CC.C11_FAULTS if CC.fault_applies(f, c)}
    assert flagged == set(CC.C11_FAULTS)
    # the later-trip faults exist on the multi-trip walks only, on every form
    for name in CC.SPECS:
        assert {(c.R, c.cap) for c in CC.c11_cases(name) if CC.fault_applies("stale_prefetch", c)} == set(MULTI)


@pytest.mark.parametrize("name", list(CC.WGRAD_SPECS))
def test_wgrad_operands_are_exact_and_a_tail_counted_twice_is_flagged(name):
    s = CC.WGRAD_SPECS[name]
    worst = 0.0
    for R, cap in CC.wgrad_walks(name):
        o = CC.wgrad_operands(name, R, cap)
        b = CC.wgrad_budget(name, o)["dw"]
        worst = max(worst, b)
        assert b < CC.LIMIT
        if s.pz:
            assert o["dz_abc"].all() and len(set(np.abs(o["dz_abc"][0]))) > 1
        if s.pa:
            assert np.isnan(o["act_abc"][1]).all() and o["act_abc"][0].all() and o["act_abc"][2].all()
        ref = CC.wgrad_ref(name, o)
        assert np.array_equal(ref.astype(np.float32).astype(F64), ref)
        assert CC.check_matrix(CC.wgrad_emulate(name, o, R, cap), ref, name) == []
        walk = CC.WgradWalk(R, 1 if (s.co, s.ci) == (64, 64) else 4, cap)
        if walk.tail_rows():
            assert CC.check_matrix(CC.wgrad_emulate(name, o, R, cap, "tail_twice"), ref, name), (name, R, cap)
    print("%s: largest budget %.3g of %.3g" % (name, worst, CC.LIMIT))


@pytest.mark.parametrize("name", list(CC.VPROD_SPECS))
def test_vprod_operands_are_exact_and_its_faults_are_flagged(name):
    worst = {}
    for R, cap in CC.VPROD_WALKS:
        o = CC.vprod_operands(name, R, cap)
        for k, v in CC.vprod_budget(name, o).items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v < CC.LIMIT
        ref = CC.vprod_ref(name, o)
        assert np.array_equal(ref.astype(np.float32).astype(F64), ref) and ref.shape == (CC.LIN_FLOATS,)
        assert CC.check_lin(CC.vprod_emulate(name, o, R, cap), ref, name) == []
        msgs = CC.check_lin(CC.vprod_emulate(name, o, R, cap, "s_every_wave"), ref, name)
        assert msgs and all(" S:" in m for m in msgs), (R, cap, msgs)
        if CC.VprodWalk(R, cap).grid >= 2:
            msgs = CC.check_lin(CC.vprod_emulate(name, o, R, cap, "odd_block_p_not_negated"), ref, name)
            assert msgs and all(" P:" in m for m in msgs), (R, cap, msgs)
    print("%s: largest budgets %s of %.3g" % (name, {k: "%.3g" % v for k, v in worst.items()}, CC.LIMIT))


@pytest.mark.parametrize("name", CC.LIN_CASES)
def test_lin_references_are_single_roundings_of_exact_doubles(name):
    o = CC.lin_operands(name)
    assert CC.lin_exact(o)
    # a second evaluation in another order (torch, reversed reduction) gives the same doubles
    import torch
    lin, w, abc = (torch.from_numpy(o[k].astype(F64)) for k in ("lin", "w", "abc"))
    P, G = lin[:CC.LIN_G].view(256, 64), lin[CC.LIN_G:CC.LIN_S].view(64, 64)
    S, SU = lin[CC.LIN_S:CC.LIN_SU], lin[CC.LIN_SU:]
    dot = torch.einsum("ck,ck->c", w.flip(1), P.flip(1))
    part = torch.stack([SU, torch.from_numpy(o["invstd"].astype(F64)) * (dot - torch.from_numpy(o["mean"].astype(F64)) * SU)])
    assert np.array_equal(part.float().numpy(), CC.lin_bnsums_ref(o))
    ref = CC.lin_finish_ref(o)
    dw = abc[0].view(-1, 1) * P + abc[1].view(-1, 1) * (w.flip(1) @ G.flip(0)) + abc[2].view(-1, 1) * S.view(1, -1)
    assert np.array_equal(dw.float().numpy(), ref["dw"])
    assert np.array_equal(torch.einsum("ck,c,cj->kj", w.flip(0), abc[1].flip(0), w.flip(0)).float().numpy(), ref["m"])
    assert np.array_equal((abc[2].flip(0) @ w.flip(0)).float().numpy(), ref["cvec"])
    if name == "lin-wide":                                       # the rounding is a real one
        assert (ref["dw"].astype(F64) != dw.numpy()).any()
