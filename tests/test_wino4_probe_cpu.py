"""The sparse probes of tests/wino4_probe.py are sensitive: on the CPU emulation of the F(4x4,3x3) split pipeline (round-to-
nearest bf16 pieces of V and of float32(U), six products accumulated in f32, the output transform in f32 in the epilogue's
order) the statistics the GPU test asserts stay at their floor for the complete split -- in the kernel's order of the piece
products and in reverse -- and exceed 1.5 x a gate for every single fault:

* each of the three small piece products (2,0), (0,2), (1,1) deleted at each ONE of the 36 transform positions, on a single
  launch of every form and shape, and on the tile rows of one parity only (one of the two weight images);
* each piece-1 and piece-2 slot (8 input channels) of V zeroed or swapped with its neighbour, per K-step, group and parity;
* each piece-1 and piece-2 slot of U zeroed or swapped, per K-step, group, 16-output-channel group and position half (the
  image of one wave), in both directions.

The gates are computed from the emulation's floor on the union of the GPU test's operand sets (3 x the worst q, 2.5 x the
worst RMS), not typed in.  This is the evidence that tests/test_wino4_probe_gpu.py would fail for a subtly wrong kernel; it
needs no GPU.

Stated limit: every (input channel, output channel) pair meets in ONE shift only, so a fault confined to a single (c, k)
element of the weight image is seen by the tiles of one launch -- 128 Winograd tiles at the all-shifts shape, of which a
one-position fault moves only a few beyond the gate.  That is below the guaranteed granularity (a whole 8-channel slot, or a
whole position across the channels); gross errors of that kind belong to the dense tests of tests/test_kernels_gpu.py."""
import functools

import pytest
import torch

import wino4_probe as wp

SMALL_TERMS = wp.TERMS[:3]
POSITIONS = [(i, j) for i in range(6) for j in range(6)]


@functools.lru_cache(maxsize=64)
def _case(form, shift):
    return wp.make_case(form, wp.SHAPE_ALL_SHIFTS, shift)


def _caught(c, fault):
    """the fault exceeds 1.5 x one of the two gates on this launch"""
    gate_max, gate_rms = wp.gates()
    q, r = wp.stats(wp.emulate(c, fault=fault), c)
    return q > 1.5 * gate_max or r > 1.5 * gate_rms, (q, r)


def test_operands_are_exact_and_every_piece_is_populated():
    """make_case asserts that V is an integer multiple of the channel's unit below 2^24 (an f32 number in any evaluation order,
    against the float64 transform); here: all three pieces of V and of U are there, the prologue's padding and ReLU cases
    exist, and the exact-arithmetic Winograd form of the probe's operands IS the float64 reference (transform matrices,
    tiling and scale are consistent)."""
    for form in wp.FORMS:
        c = wp.make_case(form, wp.SHAPE_RAGGED, 18)
        vp, up = wp.pieces(c.V32), wp.pieces(c.U32)
        live = c.V32 != 0
        # (V's third piece holds what lies below its 16th bit.  The median V has 20 bits -- 66 % of the third pieces are non-zero --
        # for the plain inputs, 19 (53 %) behind the affine prologue, 18 (34 %) behind its ReLU, which zeroes half the patch.)
        assert float((vp[1][live] != 0).double().mean()) > 0.98 and float((vp[2][live] != 0).double().mean()) > 0.3
        assert float((up[1] != 0).double().mean()) > 0.98 and float((up[2] != 0).double().mean()) > 0.9
        U = torch.einsum("ir,ort,jt->oij", wp.G, c.ker, wp.G)
        Y = torch.einsum("yi,bopqij,xj->bopqyx", wp.AT, c.V32.double()[:, c.cin_of] * U.view(1, 64, 1, 1, 6, 6), wp.AT)
        if c.out_scale is not None:
            Y = Y * c.out_scale.double().view(1, 64, 1, 1, 1, 1)
        assert float(wp.q_of(Y, c).max()) < 1e-6, form                     # float64 rounding only
    c = wp.make_case("pro_relu", wp.SHAPE_RAGGED, 9)
    assert bool((c.abc[2] > 0).any()) and bool((c.abc[2] < 0).any())         # relu(C) != 0: padding must not take it
    assert int((c.scale == 0).sum()) > 0                                     # a channel the ReLU switches off: exact zeros


def test_floor_gates_and_order_independence():
    floor_max, floor_rms = wp.floor()
    gate_max, gate_rms = wp.gates()
    print("emulator floor over %d operand sets: worst q %.3f, worst RMS %.3f; gates %.3f / %.3f" % (
        len(list(wp.launches())), floor_max, floor_rms, gate_max, gate_rms))
    assert gate_max == 3.0 * floor_max and gate_rms == 2.5 * floor_rms
    assert 0.5 < floor_max < 6.0 and 0.1 < floor_rms < floor_max          # a few units of 2^-24: the f32 class
    for form in wp.FORMS:
        for shape in wp.SHAPES:
            for t in (0, 27, 63):
                c = wp.make_case(form, shape, t)
                for terms in (wp.TERMS, tuple(reversed(wp.TERMS))):
                    y = wp.emulate(c, terms)
                    assert wp.describe(y, c, gate_max, gate_rms) is None, (form, shape, t, terms)


@pytest.mark.parametrize("form", wp.FORMS)
def test_every_small_term_deleted_at_one_position_fails(form):
    """... on ONE launch of every form and shape of the GPU test (the shift changes with the position), so a fault that only one
    kernel instantiation or one path has -- the prologue, the ragged edge, the weight ring wrapping into the next tile of a
    persistent block -- is seen there; at the all-shifts shape also when only one tile-row parity (one weight image) has it."""
    for shape in wp.SHAPES:
        cases = [wp.make_case(form, shape, t) for t in wp.SHIFTS8]
        for term in SMALL_TERMS:
            for n, pos in enumerate(POSITIONS):
                for parity in (None, 0, 1) if shape == wp.SHAPE_ALL_SHIFTS else (None,):
                    ok, got = _caught(cases[n % 8], wp.Fault("term", term=term, pos=pos, parity=parity))
                    assert ok, (form, shape, term, pos, parity, got, wp.gates())


@pytest.mark.parametrize("kind", ["zero", "swap"])
@pytest.mark.parametrize("piece", [1, 2])
def test_every_mis_staged_slot_of_v_fails(piece, kind):
    for slot in range(8):
        for parity in (0, 1):
            c = _case(("fwd", "dgrad")[slot % 2], 9 * slot)
            ok, got = _caught(c, wp.Fault(kind, operand="V", piece=piece, slot=slot, parity=parity))
            assert ok, (piece, kind, slot, parity, got, wp.gates())


@pytest.mark.parametrize("kind", ["zero", "swap"])
@pytest.mark.parametrize("piece", [1, 2])
def test_every_mis_staged_slot_of_u_fails(piece, kind):
    for form in ("fwd", "dgrad"):
        for slot in range(8):
            for cog in range(4):
                # a shift in which output channel 16 cog meets input channel 8 slot
                t = (8 * slot - 16 * cog) % 64 if form == "fwd" else (16 * cog - 8 * slot) % 64
                c = _case(form, t)
                assert int(c.cin_of[16 * cog]) == 8 * slot
                for half in (0, 1):
                    ok, got = _caught(c, wp.Fault(kind, operand="U", piece=piece, slot=slot, cog=cog, half=half))
                    assert ok, (form, piece, kind, slot, cog, half, got, wp.gates())


def test_the_eight_shifts_touch_every_slot_of_every_wave():
    """the forms and shapes that take the shifts 0, 9, ..., 63 only: every (16-output-channel group, 8-input-channel slot) pair
    and every element offset within a slot occurs, in both directions"""
    i64 = torch.arange(64)
    for sign in (1, -1):
        pairs, elems = set(), set()
        for t in wp.SHIFTS8:
            ci = (i64 + sign * t) % 64
            pairs |= set(zip((i64 // 16).tolist(), (ci // 8).tolist()))
            elems |= set(zip((ci // 8).tolist(), (ci % 8).tolist()))
        assert len(pairs) == 32 and len(elems) == 64


def test_failure_report_names_the_place():
    gate_max, gate_rms = wp.gates()
    c = _case("fwd", 9)
    f = wp.Fault("term", term=(0, 2), pos=(4, 1), wtile=11, parity=1)
    m = wp.describe(wp.emulate(c, fault=f), c, gate_max, gate_rms)
    assert m is not None, "a one-tile, one-position fault is not seen"
    for part in ("forward, shift 9", "tile-row parity 1 (-U image)", "Winograd tile 11 of it", "K-step", "16-channel group",
                 "position (4, 1) (half 1)", "third piece"):
        assert part in m, (part, m)
    c = _case("dgrad", 18)
    f = wp.Fault("zero", operand="V", piece=1, slot=5, parity=0)
    m = wp.describe(wp.emulate(c, fault=f), c, gate_max, gate_rms)
    assert "data gradient, shift 18" in m and "(K-step 1, 8-channel group 1," in m and "+U image" in m and "second piece" in m, m
    got = wp.emulate(c)
    got[1, 7, 2, 3, 1, 2] = float("nan")                     # an output nobody wrote
    assert wp.describe(got, c, gate_max, gate_rms) is not None
