"""The carried walk of the F(4x4,3x3) weight gradient (csrc/conv_wgrad4.hip) on small maps that put every path of it on a
handful of tiles: the straight-line interior body (with and without its turn at the side output), the general body of edge
patches, the segment change with its divisions and page bases, the rotating pair slots of the input role.

Per case, all six (activation prologue, gradient prologue) variants of ``cova_conv3x3_wgrad4_partial`` + ``_finish``:
  * the weight gradient against float64 at 5e-5 of the gradient's scale (the bound of
    ``test_kernels_gpu.py::test_conv3x3_winograd_f4x4_wgrad``);
  * the side output against the operand that test forms (1e-6, as it does: ``torch.addcmul`` rounds the products) and bit for
    bit against the operand formed with the kernel's two fused multiply-adds, every pixel written;
  * two launches bit for bit; the gradient with and without the side output bit for bit.

Shapes (B, H, W, grid cap): a map of one K-step (4 x 16); one tile row of three strips (4 x 48); strip remainders W = 20, 36;
partial last tile rows H = 10, 18, 122; 31 tile rows = two segments of 16 and 15 (more tile rows than a segment, and a segment
shorter than the others) against the single-segment maps; three pages with fewer walkers than segments, so that page and
segment changes fall inside a block's walk; grids that are a multiple of 16 (walker pairs 8 blocks apart) and grids that are not.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cova_web_object_detection_amd import _lib
from helpers import DEV, bits, close, relerr

call, query = _lib.call, _lib.query

BOUND = 5e-5
#        B, H,   W,  cap, grid a multiple of 16
CASES = [(1, 4, 16, 0, False),
         (1, 4, 48, 0, False),
         (2, 10, 20, 0, False),
         (3, 18, 36, 6, False),
         (3, 122, 36, 32, True),
         (3, 122, 36, 4, False)]
VARIANTS = [(pa, pd) for pa in (False, True) for pd in (0, 1, 2)]


@functools.lru_cache(maxsize=None)
def _case(B, H, W):
    """Inputs (NCHW float32 on the host), the prologue constants, and per variant the float64 operands' weight gradient.
    Computed once per map and shared by the tests; nothing modifies it."""
    g = torch.Generator().manual_seed(1009 * H + 17 * W + B)
    rnd = lambda *s: torch.randn(*s, generator=g)
    x, dy, z = rnd(B, 64, H, W), rnd(B, 64, H, W), rnd(B, 64, H, W)
    abc_a, abc_d = rnd(3, 64), rnd(3, 64)
    ch = lambda v: v.double().view(1, -1, 1, 1)
    acts = {False: x.double(), True: torch.relu(ch(abc_a[0]) * x.double() + ch(abc_a[2]))}
    grads = {0: dy.double(),
             1: ch(abc_d[0]) * dy.double() + ch(abc_d[2]),
             2: ch(abc_d[0]) * dy.double() + (ch(abc_d[1]) * z.double() + ch(abc_d[2]))}
    ref = {(pa, pd): torch.nn.grad.conv2d_weight(acts[pa], (64, 64, 3, 3), grads[pd], padding=1) for pa, pd in VARIANTS}
    return dict(x=x, dy=dy, z=z, abc_a=abc_a, abc_d=abc_d, acts=acts, grads=grads, ref=ref)


def _fma32(a, b, c):
    """float32(a * b + c) with ONE rounding: the product of two float32 is exact in float64"""
    return (a.double() * b.double() + c.double()).float()


def _side_operand(c, pd):
    """A*dy + (B*z + C) (pd = 2) or A*dy + C (pd = 1) as the kernel forms it: fused multiply-adds in float32, NHWC"""
    ch = lambda v: v.view(1, -1, 1, 1)
    inner = _fma32(ch(c["abc_d"][1]), c["z"], ch(c["abc_d"][2])) if pd == 2 else ch(c["abc_d"][2]).expand_as(c["dy"])
    return _fma32(ch(c["abc_d"][0]), c["dy"], inner).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("B,H,W", sorted({c[:3] for c in CASES}))
def test_float64_reference_is_well_inside_the_bound(B, H, W):
    """The float64 weight gradients the GPU test compares with, against the same sums taken tap by tap in another order:
    the reference's own error is ten orders of magnitude below the 5e-5 gate."""
    c = _case(B, H, W)
    for pa, pd in VARIANTS:
        a = F.pad(c["acts"][pa], (1, 1, 1, 1))
        g = c["grads"][pd]
        taps = torch.stack([torch.stack([torch.einsum("bohw,bihw->oi", g, a[:, :, r:r + H, t:t + W]) for t in range(3)], -1)
                            for r in range(3)], -2)
        err = relerr(c["ref"][(pa, pd)].numpy(), taps.numpy())
        print("float64 reference %s: %.3e" % ((pa, pd), err))
        assert err < 1e-6 * BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,cap,paired", CASES)
def test_wgrad4_carried_walk(B, H, W, cap, paired):
    c = _case(B, H, W)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)
    x, dy, z = nhwc(c["x"]), nhwc(c["dy"]), nhwc(c["z"])
    abc_a, abc_d = c["abc_a"].to(DEV), c["abc_d"].to(DEV)
    R = B * H * W
    dz_test = {1: torch.addcmul(abc_d[2].expand_as(dy), dy, abc_d[0]),                                        # A*dy + C
               2: torch.addcmul(torch.addcmul(abc_d[2].expand_as(dy), z, abc_d[1]), dy, abc_d[0])}           # A*dy + (B*z + C)
    query("cova_set_option", 2, cap)
    try:
        nblk = query("cova_conv3x3_wgrad4_num_partials", B, H, W)
        assert (nblk % 16 == 0) == paired, nblk
        ws = torch.empty(query("cova_conv3x3_wgrad4_workspace_floats", B, H, W), device=DEV)

        def launch(pa, pd, side):
            dzo = torch.full_like(dy, float("nan")) if side else None
            dw = torch.zeros(64, 64, 3, 3, device=DEV)
            ws.fill_(float("nan"))
            call("cova_conv3x3_wgrad4_partial", x, abc_a if pa else None, 1, dy, z if pd == 2 else None,
                 abc_d if pd else None, dzo, ws, B, H, W)
            call("cova_conv3x3_wgrad4_finish", ws, dw, None, None, None, None, None, None, B, H, W)
            return dw, dzo

        for pa, pd in VARIANTS:
            name = "F(4x4) wgrad %dx%dx%d cap %d, variant (%d, %d)" % (B, H, W, cap, pa, pd)
            dw, dzo = launch(pa, pd, pd != 0)
            close(dw, c["ref"][(pa, pd)], BOUND, name + " vs float64")
            dw2, dzo2 = launch(pa, pd, pd != 0)
            assert torch.equal(bits(dw), bits(dw2)), name + ": two launches differ"
            if pd:
                assert torch.isfinite(dzo).all(), name + ": side output has unwritten pixels"
                assert torch.equal(bits(dzo), bits(dzo2)), name + ": two launches' side outputs differ"
                close(dzo, dz_test[pd], 1e-6, name + " side output vs the materialised operand")
                assert torch.equal(bits(dzo), bits(_side_operand(c, pd))), name + ": side output is not the fused operand"
                dw3, _ = launch(pa, pd, False)
                assert torch.equal(bits(dw), bits(dw3)), name + ": the side output changes the gradient"
    finally:
        query("cova_set_option", 2, 0)
