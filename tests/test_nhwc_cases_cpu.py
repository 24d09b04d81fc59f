"""Checks on the case table of tests/nhwc_cases.py itself (no GPU): the table reaches every launch path of
csrc/conv_nhwc.hip it claims to reach, the premises of the integer probes hold (every bound below 2^24, torch's f32 CPU
convolutions equal their float64 forms bit for bit), the restated tap planner reproduces conv2d_input, and the restated
weight-gradient partition equals the library's own host queries."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
import nhwc_cases as NC  # noqa: E402
from cova_web_object_detection_amd import _lib  # noqa: E402

ALL = NC.CASES + list(NC.WGRAD_CASES)


def test_table_holds_the_listed_values():
    assert len(set(NC.CASES)) == len(NC.CASES)
    assert {c[:3] for c in NC.CASES} == set(NC.GEOMETRIES) == {(1, s, 0) for s in (1, 2)} | {(3, s, p) for s in (1, 2)
                                                                                                for p in (0, 1, 2)}
    assert {(c.Ci, c.Co) for c in NC.CASES} == set(NC.CHANNELS)
    assert set(NC.GROUPS) == {g + ch for g in NC.GEOMETRIES for ch in NC.CHANNELS}
    for c in ALL + NC.EMPTY_CASES:
        assert NC.shape_ok(c.Ci, c.Co, c.k, c.s, c.p) and NC.valid(c.k, c.s, c.p, c.H, c.W), c
    for (k, s, p) in NC.GEOMETRIES:
        for ch in NC.FULL_CHANNELS:
            maps = {tuple(c[5:]) for c in NC.GROUPS[(k, s, p) + ch]}
            want = {m for m in NC.SMALL_MAPS + [NC.RAGGED_MAP] if NC.valid(k, s, p, m[1], m[2])}
            if s == 2:
                want |= {m for m in NC.STRIDE2_MAPS if NC.valid(k, s, p, m[1], m[2])}
            assert want <= maps, ((k, s, p), ch, want - maps)
        # pad 0 refuses the maps smaller than the kernel and nothing else
        small = {m for m in NC.SMALL_MAPS if NC.valid(k, s, p, m[1], m[2])}
        assert small == (set(NC.SMALL_MAPS) if k == 1 or p >= 1 else {(1, 3, 3), (3, 4, 7)})
    assert all(c.B == 0 for c in NC.EMPTY_CASES) and any(NC.has_wgrad(c) for c in NC.EMPTY_CASES)


def test_every_launch_path_is_reached():
    fwd_tiles, dgrad_tiles, ntaps = set(), set(), set()
    empty_class = no_tap_class = unequal = early_return = False
    fwd_blocks, dgrad_blocks = {64: set(), 128: set()}, {64: set(), 128: set()}
    for c in NC.CASES:
        v = NC.variants(c)
        bn, blocks, _ = v["fwd"]
        fwd_tiles.add(bn)
        M = c.B * NC.out_size(c.H, c.k, c.s, c.p) * NC.out_size(c.W, c.k, c.s, c.p)
        fwd_blocks[bn].add(M - 8192 // bn)
        bn, gx, cls = v["dgrad"]
        dgrad_tiles.add(bn)
        dgrad_blocks[bn].add(max(m for *_, m, _ in cls) - 8192 // bn)
        ntaps |= {t for t, *_ in cls}
        no_tap_class |= any(t == 0 and m > 0 for t, _, _, m, _ in cls)
        empty_class |= any(hc <= 0 or wc <= 0 for _, hc, wc, _, _ in cls)
        unequal |= len({m for *_, m, _ in cls}) == 4
        early_return |= any(0 < b < gx for *_, b in cls)
        if NC.has_joined(c):
            ntaps.add(len(NC.plan(c.k, c.s, c.p, True)[0][1]))
    assert fwd_tiles == {64, 128} and dgrad_tiles == {64, 128}
    for blocks in (fwd_blocks, dgrad_blocks):           # a launch of exactly one tile of pixels, one less, one more, many
        for bn in (64, 128):
            assert {-1, 0, 1} <= blocks[bn] and max(blocks[bn]) > 2 * 8192 // bn, (bn, sorted(blocks[bn]))
    assert NC.MAXTAP in ntaps and {1, 2, 4, 9} <= ntaps, ntaps
    assert no_tap_class and empty_class and unequal and early_return
    # negative tap offsets (pad 0) and offsets of +1 / +2 (pad 2) are planned somewhere
    offs = {t.dy for (k, s, p) in NC.GEOMETRIES for _, taps in NC.plan(k, s, p, False) for t in taps}
    assert {-2, -1, 0, 1, 2} <= offs
    # stride 2, pad 0, even H: the last input row is read by no output
    assert any(c.k == 3 and c.s == 2 and c.p == 0 and c.H % 2 == 0 for c in NC.CASES)
    # joined data gradients on each of the four geometries the contract admits, on both tiles
    joined = {c[:3] + (NC.tile(c.Ci),) for c in NC.CASES if NC.has_joined(c)}
    assert joined == {g + (bn,) for g in ((1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1)) for bn in (64, 128)}
    # six reduction chunks per tap, three row tiles per tap of the weight gradient
    assert any(c.Ci == 192 and NC.has_wgrad(c) for c in NC.CASES) and any(c.Co == 192 for c in NC.CASES)


def test_weight_gradient_partitions_are_the_listed_ones():
    got = {}
    for c, want in NC.WGRAD_CASES.items():
        assert NC.has_wgrad(c)
        assert NC.variants(c)["wgrad"] == want, (c, NC.variants(c)["wgrad"])
        got[c] = want
    parts = list(got.values())
    assert any(per == 32 and last < 32 for per, n, last in parts)                      # fewer than 32 pixels
    assert (32, 1, 32) in parts
    assert any(n == 1 and last == 256 for per, n, last in parts)                       # M = 256: one part
    assert any(n == 2 and (n - 1) * per + last == 257 for per, n, last in parts)       # M = 257: two
    assert any(n > 1 and last == 1 for per, n, last in parts)
    assert any(n > 1 and last == per for per, n, last in parts)
    assert any(c.Ci == 192 for c in got) and any(c.k == 1 for c in got)
    # the step from one part to two lies where the table says, for every row-tile count of the table
    for (k, Ci) in ((3, 128), (1, 64), (3, 192), (3, 64), (1, 128)):
        assert NC.wgrad_partition(256, Ci, 128, k)[1] == 1 and NC.wgrad_partition(257, Ci, 128, k)[1] == 2


def test_restated_partition_equals_the_library_queries():
    q = _lib.query
    for c in ALL + NC.EMPTY_CASES:
        if not NC.has_wgrad(c):
            continue
        Ho, Wo = NC.out_size(c.H, c.k, c.s, c.p), NC.out_size(c.W, c.k, c.s, c.p)
        n = q("cova_conv_nhwc_wgrad_num_partials", c.B, Ho, Wo, c.Ci, c.Co, c.k)
        assert n == NC.variants(c)["wgrad"][1], c
        assert q("cova_conv_nhwc_wgrad_workspace_floats", c.B, Ho, Wo, c.Ci, c.Co, c.k) == NC.workspace_floats(c) \
            == n * c.k * c.k * c.Ci * c.Co, c
    L = NC.LARGE
    for (k, s, p) in L["geometries"]:
        Ho, Wo = NC.out_size(L["H"], k, s, p), NC.out_size(L["W"], k, s, p)
        per, n, last = NC.wgrad_partition(L["B"] * Ho * Wo, L["Ci"], L["Co"], k)
        assert q("cova_conv_nhwc_wgrad_num_partials", L["B"], Ho, Wo, L["Ci"], L["Co"], k) == n


def test_the_large_case_is_beyond_32_bit_offsets():
    L = NC.LARGE
    page = L["H"] * L["W"] * L["Ci"]
    assert 2 ** 31 < page and L["B"] * page > 2 ** 32                 # the second page starts beyond the 2^31st element
    assert 9 * 2 * L["wgrad_pixels"] < NC.EXACT_BELOW and 2 * L["wgrad_pixels"] <= 10 ** 5
    assert all(NC.joined_ok(k, s, p, L["H"], L["W"]) for (k, s, p) in L["geometries"])
    assert L["H"] % 2 == 0 and L["W"] % 2 == 1                         # parity classes of two sizes


@pytest.mark.parametrize("group", list(NC.GROUPS), ids=lambda g: "k%ds%dp%d-%dto%d" % g)
def test_probe_premises(group):
    """the bound of every case is below 2^24, the probes are integers in [-3, 3], no partial magnitude exceeds the bound,
    and torch's f32 CPU convolutions give the bits of their float64 forms"""
    cases = NC.GROUPS[group] + [c for c in NC.WGRAD_CASES if c[:5] == group]
    for c in cases:
        d = NC.probe(c)
        for t in d.values():
            assert t.dtype == torch.float32 and torch.equal(t, t.round()) and float(t.abs().max()) <= 3
        a = {k: v.abs() for k, v in d.items()}
        entries = [("fwd", NC.ref_fwd, {}), ("dgrad", NC.ref_dgrad, {}), ("dgrad", NC.ref_dgrad, dict(addend=True))]
        if NC.has_joined(c):
            entries.append(("dgrad", NC.ref_dgrad, dict(joined=True, addend=True)))
        if NC.has_wgrad(c):
            entries.append(("wgrad", NC.ref_wgrad, {}))
        for entry, ref, kw in entries:
            b = NC.bound(c, entry)
            assert b < NC.EXACT_BELOW, (c, entry, b)
            r64 = ref(c, d, **kw)
            assert torch.equal(r64, r64.round())
            assert float(ref(c, a, **kw).max()) <= b, (c, entry)      # the sum of magnitudes: every partial sum is below it
            assert torch.equal(ref(c, d, dtype=torch.float32, **kw), r64.float()), (c, entry)


def test_largest_bound_is_the_documented_one():
    worst = max(NC.bound(c, e) for c in ALL for e in ("fwd", "dgrad"))
    assert worst == 9 * 10 * 192 + 3 == 17283
    assert max(NC.bound(c, "wgrad") for c in ALL if NC.has_wgrad(c)) == 9 * 2049


@pytest.mark.parametrize("k,s,p", NC.GEOMETRIES)
def test_restated_planner_reproduces_conv2d_input(k, s, p):
    """the taps of plan() applied in plain torch to small maps give conv2d_input exactly; with a second source and an addend,
    the sum of the two data gradients and the addend.  This proves the restatement, not the kernel."""
    classes = NC.plan(k, s, p, False, Cs=128)
    assert [cl for cl, _ in classes] == [(y, x) for y in range(s) for x in range(s)]
    for m in [(1, 1, 1), (1, 1, 5), (2, 2, 2), (1, 3, 3), (2, 4, 7), (2, 5, 6), (1, 8, 9)]:
        if not NC.valid(k, s, p, m[1], m[2]):
            continue
        c = NC.Case(k, s, p, 64, 128, *m)
        d = NC.probe(c)
        shape = (c.B, c.Ci, c.H, c.W)
        got = NC.apply_plan(classes, s, [d["dy"]], [NC.dgrad_operand(d["w"])], shape)
        assert torch.equal(got, NC.ref_dgrad(c, d)), c
        if NC.has_joined(c):
            both = NC.plan(k, s, p, True, Cs=128)
            assert both[0][1][-1] == NC.Tap(1, 0, 0, 0) and [t for _, t in both[1:]] == [t for _, t in classes[1:]]
            got = NC.apply_plan(both, s, [d["dy"], d["dy2"]], [NC.dgrad_operand(d["w"]), NC.dgrad_operand(d["w1"])], shape,
                                d["add"])
            assert torch.equal(got, NC.ref_dgrad(c, d, joined=True, addend=True)), c
    # what the planner yields for the model's stride-2 convolution, written out: class (0, 0) reads the centre tap only
    assert NC.plan(3, 2, 1, False) == [((0, 0), [NC.Tap(0, 0, 0, 4)]),
                                       ((0, 1), [NC.Tap(0, 0, 1, 3), NC.Tap(0, 0, 0, 5)]),
                                       ((1, 0), [NC.Tap(0, 1, 0, 1), NC.Tap(0, 0, 0, 7)]),
                                       ((1, 1), [NC.Tap(0, 1, 1, 0), NC.Tap(0, 1, 0, 2), NC.Tap(0, 0, 1, 6), NC.Tap(0, 0, 0, 8)])]
    assert [len(t) for _, t in NC.plan(1, 2, 0, True)] == [2, 0, 0, 0]
    assert len(NC.plan(3, 1, 1, True)[0][1]) == NC.MAXTAP


def test_joined_geometries_are_the_four_with_the_same_output_grid():
    for (k, s, p) in NC.GEOMETRIES:
        got = {NC.joined_ok(k, s, p, H, W) for H in range(3, 12) for W in range(3, 12)}
        assert got == {(k, s, p) in ((1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1))}, (k, s, p)
    assert NC.out_size(2, 3, 2, 0) is None and NC.out_size(3, 3, 2, 0) == 1 and NC.out_size(1, 3, 1, 1) == 1


def test_integer_probes_see_one_wrong_tap():
    """what bit equality buys: a planner that drops one tap, reads it one pixel off, takes the neighbouring weight slice or
    applies one twice gives another integer somewhere, on the smallest maps too"""
    for (k, s, p) in NC.GEOMETRIES:
        for m in ((1, 3, 3), (2, 4, 7)):
            c = NC.Case(k, s, p, 64, 128, *m)
            d = NC.probe(c)
            shape, wd, ref = (c.B, c.Ci, c.H, c.W), NC.dgrad_operand(d["w"]), NC.ref_dgrad(c, d)
            good = NC.plan(k, s, p, False, Cs=128)
            ci = max(range(len(good)), key=lambda i: len(good[i][1]))
            cls, taps = good[ci]
            wrong = [taps[:-1], taps + taps[-1:], taps[:-1] + [taps[-1]._replace(dx=taps[-1].dx + 1)]]
            if k == 3:
                wrong.append(taps[:-1] + [taps[-1]._replace(wrow=(taps[-1].wrow + 128) % (9 * 128))])
            for bad in wrong:
                mutated = good[:ci] + [(cls, bad)] + good[ci + 1:]
                assert not torch.equal(NC.apply_plan(mutated, s, [d["dy"]], [wd], shape), ref), (c, bad)
