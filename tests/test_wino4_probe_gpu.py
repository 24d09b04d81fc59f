"""The F(4x4,3x3) bf16-split main loop (csrc/conv_wino4_split.h) held piece by piece on the MI355X with the sparse probes of
tests/wino4_probe.py: one input channel per output channel, integer-lattice inputs (V = B^T d B exact in f32), generic f32
weights; the error of every output in units of 2^-24 |A^T| (|V| (.) |U|) |A| against the float64 sparse convolution.

Asserted per launch: worst q <= gate_max and worst RMS of q (per output channel, in-tile coordinate and tile-row parity)
<= gate_rms, the gates being 3 x / 2.5 x the floor of the CPU emulation of the complete split on the same operand sets
(wino4_probe.gates(); nothing typed in).  tests/test_wino4_probe_cpu.py shows that the emulation with any single piece
product deleted at one of the 36 positions, or with one mis-staged slot of one piece of V or of U, exceeds 1.5 x a gate.
Every out buffer is framed by guard rows that must stay untouched and starts as NaN (an output nobody wrote fails); every
launch runs twice and must be bit-equal.  The same probe on the f32 main loop (cova_set_option(9, 1)) is recorded beside
it as a control, not asserted.  The lines go to the file COVA_WRITE_W4_PROBE names (profiles/wino4_split_probe.txt)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import wino4_probe as wp  # noqa: E402
from cova_web_object_detection_amd._lib import call, query  # noqa: E402
from helpers import DEV  # noqa: E402

GUARD = 2 * 64          # guard rows (pixels of 64 channels) in front of and behind an out buffer
GUARD_VALUE = -12345.0


def framed_out(B, H, W):
    n = B * H * W
    buf = torch.full((n + 2 * GUARD, 64), GUARD_VALUE, device=DEV)
    out = buf[GUARD:GUARD + n].view(B, H, W, 64)
    out.fill_(float("nan"))
    return buf, out


def guards_untouched(buf):
    return bool((buf[:GUARD] == GUARD_VALUE).all()) and bool((buf[-GUARD:] == GUARD_VALUE).all())


def launch(c, with_part):
    """One launch of the case's form -> (frame, out [B, H, W, 64], statistics rows or None)"""
    B, H, W = c.B, c.H, c.W
    nu = query("cova_conv3x3_wino4_u_floats")
    uf, ud = torch.empty(nu, device=DEV), torch.empty(nu, device=DEV)
    call("cova_conv3x3_wino4_prep", c.w.to(DEV), uf, ud)
    u = ud if c.dgrad else uf
    x = c.x.to(DEV)
    buf, out = framed_out(B, H, W)
    part = torch.zeros(query("cova_conv3x3_wino4_num_partials", B, H, W), 2, 64, device=DEV) if with_part else None
    N = None
    if c.form in ("fwd", "dgrad"):
        call("cova_conv3x3_wino4", x, u, out, part, B, H, W)
    elif c.form in ("pro", "pro_relu"):
        call("cova_conv3x3_wino4_pro", x, c.abc.to(DEV), c.relu, u, out, part, B, H, W)
    elif c.form == "full":          # addend of zeros; mask fma(1, z, 0) > 0 with the sign pattern of the case
        one, zero = torch.ones(64, device=DEV), torch.zeros(64, device=DEV)
        call("cova_conv3x3_wino4_full", x, N, N, 0, u, torch.zeros_like(x), N, one, zero, c.z.to(DEV), zero, one, out, part, B, H, W)
    else:                           # bnact: power-of-two scale, zero shift, no ReLU
        call("cova_conv3x3_wino4_bnact", x, N, 0, u, N, c.out_scale.to(DEV), torch.zeros(64, device=DEV), 0, out, B, H, W)
    return buf, out, part


# which launches take statistics rows: the plain ones both ways, the prologue form with its ReLU, the masked gradient always
PARTS = {"fwd": (False, True), "dgrad": (False, True), "pro": (False,), "pro_relu": (True,), "full": (True,), "bnact": (False,)}


def probe(form, shape, f32):
    """Every shift of (form, shape) on one main loop -> (worst q, worst RMS, first failure description or None)"""
    gate_max, gate_rms = wp.gates()
    worst_q = worst_rms = 0.0
    failure = None
    query("cova_set_option", 9, f32)
    for t in wp.shifts_of(form, shape):
        c = wp.make_case(form, shape, t)
        for with_part in PARTS[form]:
            buf, out, part = launch(c, with_part)
            buf2, out2, part2 = launch(c, with_part)
            what = "%s %s shift %d part %d f32 %d" % (form, shape, t, with_part, f32)
            assert guards_untouched(buf) and guards_untouched(buf2), what + ": a guard row was written"
            assert torch.equal(buf, buf2) and (part is None or torch.equal(part, part2)), what + ": not bit-reproducible"
            got = out.cpu()
            if c.keep is not None:
                assert not bool(got[~c.keep].any()), what + ": a masked output is not an exact zero"
            tiles = wp.nhwc_to_tiles(got, c)
            q, r = wp.stats(tiles, c)
            worst_q, worst_rms = max(worst_q, q), max(worst_rms, r)
            if failure is None and not f32:
                failure = wp.describe(tiles, c, gate_max, gate_rms)
                if failure is not None:
                    failure = what + ": " + failure
    return worst_q, worst_rms, failure


@pytest.mark.parametrize("shape", wp.SHAPES, ids=lambda s: "%dx%dx%d_cap%d" % s)
@pytest.mark.parametrize("form", wp.FORMS)
def test_wino4_split_sparse_probe(form, shape):
    """forms: cova_conv3x3_wino4 with u_fwd / u_dgrad (with and without stat_part), cova_conv3x3_wino4_pro without / with
    ReLU (zero padding stays zero although relu(C) != 0), the data-gradient form of cova_conv3x3_wino4_full (masked outputs
    exact zeros), cova_conv3x3_wino4_bnact.  shapes: one tile row (+U image only), both parities (all 64 shifts for the plain
    launches), ragged with three tile rows, several tiles per persistent block (cova_set_option(2, 2))."""
    gate_max, gate_rms = wp.gates()
    floor_max, floor_rms = wp.floor()
    try:
        query("cova_set_option", 2, shape[3])
        q1, r1, _ = probe(form, shape, 1)
        q0, r0, failure = probe(form, shape, 0)
    finally:
        query("cova_set_option", 9, 0)
        query("cova_set_option", 2, 0)
    line = "%-8s %dx%dx%d cap %d  %2d shifts | split loop: worst q %6.2f  worst RMS %5.2f | f32 loop: %6.2f  %5.2f | floor %.2f %.2f  gates %.2f %.2f" % (
        form, shape[0], shape[1], shape[2], shape[3], len(wp.shifts_of(form, shape)), q0, r0, q1, r1, floor_max, floor_rms, gate_max, gate_rms)
    print(line)
    path = os.environ.get("COVA_WRITE_W4_PROBE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
    assert failure is None, failure
    assert q0 <= gate_max and r0 <= gate_rms, line
