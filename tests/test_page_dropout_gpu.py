"""GPU tests of the dropout of the page layers (CoVA(page_attention_dropout=, page_encoder_dropout=)):
the row kernels (cova_gelu_fwd_drop / cova_gelu_bwd_drop, cova_dropout_add_fwd / cova_dropout_regen_bwd) and the four
attention pairs with DROP through the C ABI on framed, guarded buffers against the float64 torch oracle
(tests/page_dropout_oracle.py: masks from the restated hash and stream rule as inputs, autograd, no code shared with the
kernels or engine.py), an all-dropped row, reproducibility, refusals and empty work, the composed engine layers, "off is
off", the modules and the whole model under autograd, and HotPathTrainer with the options on.

Bounds: the project's own for the page layers (tests/test_page_attention_gpu.py, tests/test_page_encoder_gpu.py): max-abs
error over max-abs float64 reference below 1e-5 for what a forward writes and below 1e-4 for gradients; cova_dropout_add_fwd
and cova_dropout_regen_bwd are bit-equal to the numpy float32 statement; lse is bit-equal to the plain forward's.  The whole
model on the cova_h64_n11 inputs keeps tests/test_model_gpu.py's LOGIT_TOL / LOSS_TOL / GRAD_TOL.

Measured on an MI355X (worst over all cases; bound in brackets): GELU with DROP forward 1.1e-7 [1e-5], backward 1.1e-7 [1e-4];
the attention pairs O 2.6e-7, lse 1.5e-7 [1e-5], dqkv 4.5e-7, d w 1.6e-7 [1e-4]; the composed layers out 3.9e-7 [1e-5], dh
6.1e-7, parameter gradients 1.2e-6 [1e-4]; the model with every dropout on: train logits 1.5e-6 [5e-5], loss 7.9e-7 [2e-5],
gradients on the 1 % floor 8.1e-6 [1e-4]; the trainer against the module 5.2e-6 [1e-4].  34 tests in 3.5 s."""
import functools
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import _lib, engine, weights  # noqa: E402
from cova_web_object_detection_amd.evaluation import evaluate_split  # noqa: E402
from cova_web_object_detection_amd.features import FeatureCache  # noqa: E402
from cova_web_object_detection_amd.models import CoVA, PageAttention, PageEncoder  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
from helpers import (bits_equal, compare_grads, DEV, framed, GRAD_TOL, GUARD, LOGIT_TOL,  # noqa: E402
                     LOSS_TOL, NAN, padded, profiled, relerr, routing_from_saved, starts, survived)
from oracle import cova_oracle as O  # noqa: E402
import attn_dropout_oracle as AD  # noqa: E402
import combined_cases as CC  # noqa: E402
import combined_oracle as CO  # noqa: E402
import page_attn_geo_oracle as PG  # noqa: E402
import page_dropout_oracle as PD  # noqa: E402
import page_encoder_oracle as PE  # noqa: E402
from config_cases import SPLIT_CFG as CFG  # noqa: E402
from gat_cases import device_gates  # noqa: E402
from trainer_cases import five_steps, page_set, seeded  # noqa: E402

GELU_FWD, GELU_BWD = "cova_gelu_fwd", "cova_gelu_bwd"
GELU_FWD_D, GELU_BWD_D = "cova_gelu_fwd_drop", "cova_gelu_bwd_drop"
ADD_FWD, REGEN_BWD = "cova_dropout_add_fwd", "cova_dropout_regen_bwd"
PA_FWD, PA_BWD = "cova_page_attn_fwd", "cova_page_attn_bwd"
PA_FWD_D, PA_BWD_D = "cova_page_attn_fwd_drop", "cova_page_attn_bwd_drop"
PA_FWD_G, PA_BWD_G = "cova_page_attn_fwd_geo", "cova_page_attn_bwd_geo"
PA_FWD_GD, PA_BWD_GD = "cova_page_attn_fwd_geo_drop", "cova_page_attn_bwd_geo_drop"
WSQ = "cova_page_attn_geo_workspace_floats"
NEW = (GELU_FWD_D, GELU_BWD_D, ADD_FWD, REGEN_BWD, PA_FWD_D, PA_BWD_D, PA_FWD_GD, PA_BWD_GD)
W, H = PG.PAGE_W, PG.PAGE_H
PAGE_SIZE = (H, W)
SEED = PD.page_dropout_seed(AD.dropout_base(123, 1), 0, 0)

f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
inv32 = lambda p: np.float32(1.0) / (np.float32(1.0) - np.float32(p))


# ---------------------------------------------------------------- 1. the row kernels through the C ABI
ROW_SHAPES = [(1, 4, 0), (5, 7, 3), (90, 256, 4), (33, 2048, 0)]


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("R,C,pad", ROW_SHAPES)
def test_row_kernels_match_their_statements_with_the_oracles_mask(R, C, pad, p):
    rs = np.random.RandomState(R + C)
    z = rs.uniform(-3, 3, (R, C)).astype(np.float32)          # (|z| < 3: gelu(z) and gelu'(z) are never exactly zero)
    z[z == 0] = 0.5
    g, x, y = (rs.standard_normal((R, C)).astype(np.float32) for _ in range(3))
    g[g == 0], y[y == 0] = 1.0, 1.0
    seed = SEED + R
    keep = PD.row_keep(p, seed, R, C)
    assert keep.shape == (R, C) and (R * C < 16 or not keep.all())
    ld = C + pad
    zd, gd, xd, yd = padded(z, ld), padded(g, ld), padded(x, ld), padded(y, ld)
    bufs = {k: framed(R, C, ld) for k in ("f", "dz", "out", "dy")}
    engine.call(GELU_FWD_D, zd, ld, R, C, bufs["f"][1], ld, p, seed)
    engine.call(GELU_BWD_D, gd, ld, zd, ld, R, C, bufs["dz"][1], ld, p, seed)
    engine.call(ADD_FWD, yd, ld, xd, ld, bufs["out"][1], ld, R, C, p, seed)
    engine.call(REGEN_BWD, gd, ld, bufs["dy"][1], ld, R, C, p, seed)
    torch.cuda.synchronize()
    got = {k: survived(b[0], R, C) for k, b in bufs.items()}
    inv = inv32(p)
    assert inv == np.float32(PD.inv_keep(p))
    assert bits_equal(got["out"], x + np.where(keep, y * inv, np.float32(0)))            # the numpy float32 statement
    assert bits_equal(got["dy"], np.where(keep, g * inv, np.float32(0)))
    scale = f64(keep) * PD.inv_keep(p)
    e_f = relerr(got["f"], (PE.gelu(f64(z)) * scale).numpy())
    e_b = relerr(got["dz"], (PE.gelu_grad(f64(z)) * f64(g) * scale).numpy())
    print("gelu drop (%d, %d, %d) p=%.1f: forward %.2e, backward %.2e" % (R, C, pad, p, e_f, e_b))
    assert e_f < 1e-5 and e_b < 1e-4
    assert np.array_equal(got["f"] == 0, ~keep) and np.array_equal(got["dz"] == 0, ~keep)
    assert not np.signbit(got["f"][~keep]).any() and not np.signbit(got["dz"][~keep]).any()   # a dropped element is +0
    # kept elements are the plain kernel's value times inv, one rounding
    plain_b, plain = framed(R, C, ld)
    engine.call(GELU_FWD, zd, ld, R, C, plain, ld)
    torch.cuda.synchronize()
    assert bits_equal(got["f"][keep], (survived(plain_b, R, C) * inv)[keep])


# ---------------------------------------------------------------- 2. the attention pairs through the C ABI
#            page sizes          E    Hh  pad  geo
ATT_SHAPES = {"ragged": ((37, 0, 1, 5, 0), 8, 2, 3, False),            # empty and one-box pages; unaligned rows
              "tiles": ((16, 17, 65), 32, 2, 4, False),                # either side of a sub-tile and of a 64-row tile
              "tiles-geo": ((16, 17, 65), 32, 2, 4, True),
              "head": ((90, 11), 128, 4, 0, False),
              "d128": ((33, 70), 128, 1, 4, False)}                    # dh = 128: the KT = 32 build


def build_att_case(name, sizes, E, heads, pad, geo, seed):
    rs = np.random.RandomState(seed)
    N = int(sum(sizes))
    return dict(name=name, sizes=tuple(sizes), N=N, B=len(sizes), E=E, heads=heads, pad=pad, geo=geo, ps=starts(sizes),
                qkv=rs.standard_normal((N, 3 * E)).astype(np.float32), g=rs.standard_normal((N, E)).astype(np.float32),
                w=(2.0 * rs.standard_normal((heads, 8))).astype(np.float32), boxes=PG.planted_boxes(sizes, seed + 1))


@functools.lru_cache(maxsize=None)
def att_case(name):
    return build_att_case(name, *ATT_SHAPES[name], seed=sum(map(ord, name)))


def att_oracle(case, p, seed):
    qkv = f64(case["qkv"]).requires_grad_(True)
    wl = f64(case["w"]).requires_grad_(True) if case["geo"] else None
    phi = PG.page_features(case["boxes"], case["ps"], W, H) if case["geo"] else None
    keeps = PD.attn_keeps(p, seed, case["ps"], case["heads"]) if p > 0 else None
    out, lse = PD.attend(qkv, case["ps"], case["heads"], keeps, p, wl, phi)
    (out * f64(case["g"])).sum().backward()
    return dict(out=out.detach().numpy(), lse=lse.detach().numpy(), dqkv=qkv.grad.numpy(),
                dw=wl.grad.numpy() if case["geo"] else None, keeps=keeps)


@functools.lru_cache(maxsize=None)
def att_ref(name, p, seed):
    return att_oracle(att_case(name), p, seed)


def launch_att(case, drop=None):
    """The forward and backward pair of the case (plain or GEO; ``drop`` = (p, seed): the _drop forms) on framed buffers
    -> dict of host arrays, guards checked.  Rows of empty pages stay unwritten."""
    N, B, E, heads, pad = case["N"], case["B"], case["E"], case["heads"], case["pad"]
    qkv, g, ps = dev(case["qkv"]), padded(case["g"], E + pad), dev(case["ps"])
    out_b, out = framed(N, E, E + pad)
    lse_b, lse = framed(N, heads, heads)
    d_b, d = framed(N, 3 * E, 3 * E + pad)
    tail = () if drop is None else (float(drop[0]), int(drop[1]))
    if not case["geo"]:
        engine.call(PA_FWD_D if tail else PA_FWD, qkv, 3 * E, ps, B, N, E, heads, out, E + pad, lse, *tail)
        engine.call(PA_BWD_D if tail else PA_BWD, g, E + pad, qkv, 3 * E, out, E + pad, lse, ps, B, N, E, heads, d,
                    3 * E + pad, *tail)
        torch.cuda.synchronize()
        return dict(out=survived(out_b, N, E), lse=survived(lse_b, N, heads), dqkv=survived(d_b, N, 3 * E))
    boxes, wd = dev(case["boxes"]), dev(case["w"])
    blocks = B * heads * ((N + 63) // 64)
    assert engine.query(WSQ, B, N, heads) == 8 * blocks
    ws_b, ws = framed(blocks, 8, 8)
    dw_b, dw = framed(heads, 8, 8)
    engine.call(PA_FWD_GD if tail else PA_FWD_G, qkv, 3 * E, ps, boxes, wd, float(W), float(H), B, N, E, heads, out, E + pad,
                lse, *tail)
    engine.call(PA_BWD_GD if tail else PA_BWD_G, g, E + pad, qkv, 3 * E, out, E + pad, lse, ps, boxes, wd, float(W),
                float(H), B, N, E, heads, d, 3 * E + pad, dw, ws, *tail)
    torch.cuda.synchronize()
    survived(ws_b, blocks, 8)
    return dict(out=survived(out_b, N, E), lse=survived(lse_b, N, heads), dqkv=survived(d_b, N, 3 * E),
                dw=survived(dw_b, heads, 8))


def check_att(got, ref, what):
    errs = {k: relerr(got[k], ref[k]) for k in ("out", "lse", "dqkv")}
    if ref["dw"] is not None:
        errs["dw"] = relerr(got["dw"], ref["dw"])
    print(what, {k: "%.2e" % v for k, v in errs.items()})
    for k, e in errs.items():
        assert e < (1e-4 if k in ("dqkv", "dw") else 1e-5), (what, k, e)


@pytest.mark.parametrize("name,p", [(n, 0.5) for n in ATT_SHAPES] + [("tiles", 0.1)])
def test_attention_pairs_match_the_float64_oracle_and_lse_is_the_plain_forwards(name, p):
    case = att_case(name)
    got, ref = launch_att(case, (p, SEED)), att_ref(name, p, SEED)
    check_att(got, ref, "%s p=%.1f" % (name, p))
    plain = launch_att(case)
    assert bits_equal(got["lse"], plain["lse"])               # the undropped lse, bit for bit
    assert not bits_equal(got["out"], plain["out"])
    kept = np.mean([k.mean() for k in ref["keeps"].values()])
    assert abs(kept - (1 - p)) < 0.1
    # the masks matter at these bounds: against the oracle without dropout O moves by far more than the bound
    assert relerr(att_ref(name, 0.0, 0)["out"], ref["out"]) > 1e-2
    if case["geo"]:
        assert float(np.abs(ref["dw"]).max()) > 0


# ---------------------------------------------------------------- 3. an all-dropped row
def test_a_row_whose_only_key_is_dropped_is_exactly_zero_and_passes_no_gradient():
    sizes, E, heads, p = (5, 1, 3), 8, 2, 0.6
    case = build_att_case("one-box", sizes, E, heads, 3, False, 31)
    i = int(case["ps"][1])
    seed = next(s for s in range(1, 10000)
                if all(PD.hash_uniform(s, PD.attn_index(i, a, i, heads)) < np.float32(p) for a in range(heads)))
    keeps = PD.attn_keeps(p, seed, case["ps"], heads)
    assert not keeps[(1, 0)].any() and not keeps[(1, 1)].any() and keeps[(0, 0)].any()
    got = launch_att(case, (p, seed))
    assert not got["out"][i].any() and not got["dqkv"][i].any()
    assert got["out"][:i].any() and got["dqkv"][:i].any()
    check_att(got, att_oracle(case, p, seed), "all-dropped row")


# ---------------------------------------------------------------- 4. reproducibility
@pytest.mark.parametrize("name", ["tiles", "tiles-geo"])
def test_one_seed_gives_the_same_bits_twice_another_seed_another_output(name):
    case = att_case(name)
    a, b, c = launch_att(case, (0.5, SEED)), launch_att(case, (0.5, SEED)), launch_att(case, (0.5, SEED + 1))
    for k in a:
        assert bits_equal(a[k], b[k]), k
    assert not bits_equal(a["out"], c["out"]) and bits_equal(a["lse"], c["lse"])


@pytest.mark.parametrize("geo", [False, True])
def test_a_page_depends_on_the_batch_rows_it_occupies_and_on_nothing_else(geo):
    n, E, heads, pad = 65, 32, 2, 4
    a = build_att_case("a", (4, n, 13), E, heads, pad, geo, 5)
    b = build_att_case("b", (1, 3, n, 6, 7), E, heads, pad, geo, 6)       # other pages around it, the same 65 rows
    for k in ("qkv", "g", "boxes"):
        b[k][4:4 + n] = a[k][4:4 + n]
    b["w"] = a["w"]
    ga, gb = launch_att(a, (0.5, SEED)), launch_att(b, (0.5, SEED))
    for k in ("out", "lse", "dqkv"):
        assert bits_equal(ga[k][4:4 + n], gb[k][4:4 + n]), k
    # the same page at other rows draws another mask
    c = build_att_case("c", (5, n, 12), E, heads, pad, geo, 5)
    for k in ("qkv", "g", "boxes"):
        c[k][5:5 + n] = a[k][4:4 + n]
    c["w"] = a["w"]
    gc = launch_att(c, (0.5, SEED))
    assert bits_equal(ga["lse"][4:4 + n], gc["lse"][5:5 + n]) and not bits_equal(ga["out"][4:4 + n], gc["out"][5:5 + n])


# ---------------------------------------------------------------- 5. refusals and empty work
BAD_P = (0.0, 1.0, -0.1, 1.5, NAN)


def test_row_entry_points_refuse_bad_arguments_and_skip_empty_work():
    R, C = 9, 24
    full = lambda *shape: torch.full(shape, GUARD, device=DEV)
    z, g, x, y = (torch.randn(R, C, device=DEV) for _ in range(4))
    f, dz, out, dy = full(R, C), full(R, C), full(R, C), full(R, C)
    good = {GELU_FWD_D: [z, C, R, C, f, C, 0.5, 7], GELU_BWD_D: [g, C, z, C, R, C, dz, C, 0.5, 7],
            ADD_FWD: [y, C, x, C, out, C, R, C, 0.5, 7], REGEN_BWD: [g, C, dy, C, R, C, 0.5, 7]}
    p_at = {GELU_FWD_D: 6, GELU_BWD_D: 8, ADD_FWD: 8, REGEN_BWD: 6}
    r_at = {GELU_FWD_D: 2, GELU_BWD_D: 4, ADD_FWD: 6, REGEN_BWD: 4}
    bad = {GELU_FWD_D: [{3: 0}, {2: -1}, {1: C - 1}, {5: C - 1}, {0: None}, {4: None}],
           GELU_BWD_D: [{5: 0}, {4: -1}, {1: C - 1}, {3: C - 1}, {7: C - 1}, {0: None}, {2: None}, {6: None}],
           ADD_FWD: [{7: 0}, {6: -1}, {1: C - 1}, {3: C - 1}, {5: C - 1}, {0: None}, {2: None}, {4: None}, {4: x}, {4: y}],
           REGEN_BWD: [{5: 0}, {4: -1}, {1: C - 1}, {3: C - 1}, {0: None}, {2: None}, {2: g}]}
    for name, changes in bad.items():
        for ch in changes + [{p_at[name]: v} for v in BAD_P]:
            args = list(good[name])
            for i, v in ch.items():
                args[i] = v
            with pytest.raises(_lib.CovaHipError, match="10001"):
                engine.call(name, *args)
    # R == 0 launches nothing and needs no pointer
    engine.call(GELU_FWD_D, None, C, 0, C, None, C, 0.5, 7)
    engine.call(GELU_BWD_D, None, C, None, C, 0, C, None, C, 0.5, 7)
    engine.call(ADD_FWD, None, C, None, C, None, C, 0, C, 0.5, 7)
    engine.call(REGEN_BWD, None, C, None, C, 0, C, 0.5, 7)
    for name in good:
        args = list(good[name])
        args[r_at[name]] = 0
        engine.call(name, *args)
    torch.cuda.synchronize()
    for t in (f, dz, out, dy):
        assert (t == GUARD).all()
    for name in good:                                         # and the good calls are good
        engine.call(name, *good[name])
    torch.cuda.synchronize()
    for t in (f, dz, out, dy):
        assert bool(torch.isfinite(t).all()) and (t != GUARD).all()


def test_attention_entry_points_refuse_bad_arguments_and_skip_empty_work():
    N, B, E, Hh = 8, 2, 16, 2
    full = lambda *shape: torch.full(shape, GUARD, device=DEV)
    ps = torch.tensor([0, 5, 8], dtype=torch.int64, device=DEV)
    qkv, g = torch.randn(N, 3 * E, device=DEV), torch.randn(N, E, device=DEV)
    boxes = dev(PG.planted_boxes((5, 3), 2))
    w = torch.randn(Hh, 8, device=DEV)
    out, lse, d, dw = full(N, E), full(N, Hh), full(N, 3 * E), full(Hh, 8)
    ws = full(engine.query(WSQ, B, N, Hh))
    good = {PA_FWD_D: [qkv, 3 * E, ps, B, N, E, Hh, out, E, lse, 0.5, 7],
            PA_BWD_D: [g, E, qkv, 3 * E, out, E, lse, ps, B, N, E, Hh, d, 3 * E, 0.5, 7],
            PA_FWD_GD: [qkv, 3 * E, ps, boxes, w, 96.0, 64.0, B, N, E, Hh, out, E, lse, 0.5, 7],
            PA_BWD_GD: [g, E, qkv, 3 * E, out, E, lse, ps, boxes, w, 96.0, 64.0, B, N, E, Hh, d, 3 * E, dw, ws, 0.5, 7]}
    p_at = {PA_FWD_D: 10, PA_BWD_D: 14, PA_FWD_GD: 14, PA_BWD_GD: 20}
    bn_at = {PA_FWD_D: (3, 4), PA_BWD_D: (8, 9), PA_FWD_GD: (7, 8), PA_BWD_GD: (12, 13)}
    bad = {PA_FWD_D: [{6: 3}, {6: 0}, {5: 0}, {1: 3 * E - 4}, {8: E - 1}, {0: None}, {2: None}, {7: None}, {9: None}],
           PA_BWD_D: [{11: 3}, {10: 0}, {1: E - 1}, {3: 3 * E - 4}, {5: E - 1}, {13: 3 * E - 1}, {0: None}, {2: None},
                      {4: None}, {6: None}, {7: None}, {12: None}],
           PA_FWD_GD: [{10: 3}, {9: 0}, {1: 3 * E - 4}, {12: E - 1}, {0: None}, {2: None}, {11: None}, {13: None},
                       {3: None}, {4: None}, {5: 0.0}, {6: -1.0}],
           PA_BWD_GD: [{15: 3}, {14: 0}, {1: E - 1}, {3: 3 * E - 4}, {5: E - 1}, {17: 3 * E - 1}, {0: None}, {2: None},
                       {4: None}, {6: None}, {7: None}, {16: None}, {8: None}, {9: None}, {18: None}, {19: None},
                       {10: 0.0}, {11: -1.0}]}
    for name, changes in bad.items():
        for ch in changes + [{p_at[name]: v} for v in BAD_P]:
            args = list(good[name])
            for i, v in ch.items():
                args[i] = v
            with pytest.raises(_lib.CovaHipError, match="10001"):
                engine.call(name, *args)
    # N == 0 or B == 0: nothing is launched, no pointer is needed
    for n, b in ((0, B), (N, 0), (0, 0)):
        for name in good:
            args = list(good[name])
            args[bn_at[name][0]], args[bn_at[name][1]] = b, n
            engine.call(name, *args)
            engine.call(name, *[None if torch.is_tensor(a) else a for a in args])
    torch.cuda.synchronize()
    for t in (out, lse, d, dw, ws):
        assert (t == GUARD).all()
    for name in good:                                         # and the good calls are good
        engine.call(name, *good[name])
    torch.cuda.synchronize()
    for t in (out, lse, d, dw, ws):
        assert bool(torch.isfinite(t).all()) and (t != GUARD).all()


# ---------------------------------------------------------------- 6. the composed layers
#                 pages            F    P   Hh   M   L  geometry
LAYER_CASES = {"small": ((37, 0, 1, 5, 0), 40, 8, 2, 16, 1, False),          # empty pages, a one-box page
               "geo": ((16, 17, 65), 100, 32, 2, 64, 3, True)}               # the attention's tile edges
BASE = AD.dropout_base(7, 1)
P_LAYER = 0.5


def build_layer_case(name, sizes, Fd, P, Hh, M, L, geometry, seed):
    rs = np.random.RandomState(seed)
    N = int(sum(sizes))

    def fill(spec):
        sd = {}
        for k, s in spec:
            if ".norm" in k:
                v = rs.uniform(0.5, 1.5, s) if k.endswith("weight") else 0.1 * rs.standard_normal(s)
            elif k.endswith("geometry.weight"):
                v = rs.uniform(-2, 2, s)
            elif len(s) == 2:
                v = rs.uniform(-1, 1, s) / np.sqrt(s[1])
            else:
                v = rs.uniform(-0.05, 0.05, s)
            sd[k] = v.astype(np.float32)
        return sd
    att = [("page_attention.qkv.weight", (3 * P, Fd))] + ([("page_attention.geometry.weight", (Hh, 8))] if geometry else [])
    return dict(name=name, sizes=tuple(sizes), N=N, F=Fd, P=P, Hh=Hh, M=M, L=L, geometry=geometry, ps=starts(sizes),
                sd=fill(weights.page_encoder_entries(Fd, P, Hh, L, M, geometry)), att_sd=fill(att),
                h=rs.standard_normal((N, Fd)).astype(np.float32), g=rs.standard_normal((N, P)).astype(np.float32),
                bboxes=PG.planted_boxes(sizes, seed + 1))


@functools.lru_cache(maxsize=None)
def layer_case(name):
    case = build_layer_case(name, *LAYER_CASES[name], seed=sum(map(ord, name)))
    phi = PG.page_features(case["bboxes"], case["ps"], W, H) if case["geometry"] else None
    for kind in ("enc", "att"):
        sd = {k: f64(v).requires_grad_(True) for k, v in case["sd" if kind == "enc" else "att_sd"].items()}
        h = f64(case["h"]).requires_grad_(True)
        if kind == "enc":
            masks = PD.encoder_masks(P_LAYER, BASE, case["ps"], case["Hh"], case["N"], case["P"], [case["M"]] * case["L"])
            case["masks"] = masks
            out = PD.page_encoder(h, sd, case["ps"], case["Hh"], masks, P_LAYER, phi)
        else:
            keeps = PD.attn_keeps(P_LAYER, PD.page_dropout_seed(BASE, PD.MAX_LAYERS, 0), case["ps"], case["Hh"])
            out = PD.page_attention(h, sd, case["ps"], case["Hh"], keeps, P_LAYER, phi)[0]
        (out * f64(case["g"])).sum().backward()
        case["ref_" + kind] = dict(out=out.detach().numpy(), dh=h.grad.numpy(), grads={k: v.grad.numpy() for k, v in sd.items()})
    return case


def run_layer(case, kind, **kw):
    """engine.page_encoder_fwd / _bwd (``kind`` "enc") or engine.page_attn_fwd / _bwd ("att") inside a [N, F + P + 1] feature
    matrix, as engine._head_fwd places them -> (dict(out, dh, grads) of host arrays, the saved dict)."""
    N, Fd, P = case["N"], case["F"], case["P"]
    T = Fd + P + 1
    sd = case["sd" if kind == "enc" else "att_sd"]
    params = {k: dev(v) for k, v in sd.items()}
    comb = torch.full((N, T), NAN, device=DEV)
    comb[:, :Fd] = dev(case["h"])
    if kind == "att":
        comb[:, Fd:Fd + P] = 0.0                             # (rows of empty pages are written by no attention kernel)
    ps = dev(case["ps"])
    bb = dev(case["bboxes"]) if case["geometry"] else None
    dcomb = torch.zeros((N, T), device=DEV)
    dcomb[:, Fd:Fd + P] = dev(case["g"])
    if kind == "enc":
        sv = engine.page_encoder_fwd(comb, T, N, Fd, ps, params, case["Hh"], case["L"], comb[:, Fd:], T, bboxes=bb,
                                     page_size=PAGE_SIZE, **kw)
        grads = engine.page_encoder_bwd(sv, dcomb[:, Fd:], T, params, dcomb, T)
    else:
        sv = engine.page_attn_fwd(comb, T, N, Fd, ps, params, case["Hh"], comb[:, Fd:], T, bboxes=bb, page_size=PAGE_SIZE,
                                  **kw)
        grads = engine.page_attn_bwd(sv, dcomb[:, Fd:], T, params, dcomb, T)
    torch.cuda.synchronize()
    assert set(grads) == set(sd)
    assert bool(torch.isnan(comb[:, Fd + P:]).all()) and not dcomb[:, Fd + P:].any()
    return dict(out=comb[:, Fd:Fd + P].cpu().numpy(), dh=dcomb[:, :Fd].cpu().numpy(),
                grads={k: v.cpu().numpy().reshape(sd[k].shape) for k, v in grads.items()}), sv


def same_bits(a, b):
    return (bits_equal(a["out"], b["out"]) and bits_equal(a["dh"], b["dh"])
            and all(bits_equal(a["grads"][k], b["grads"][k]) for k in a["grads"]))


@pytest.mark.parametrize("kind", ["att", "enc"])
@pytest.mark.parametrize("name", list(LAYER_CASES))
def test_composed_layers_with_dropout_match_the_oracle_and_reruns_are_bit_identical(name, kind):
    case = layer_case(name)
    on = dict(dropout=P_LAYER, seed_base=BASE, training=True)
    (got, sv), ref = run_layer(case, kind, **on), case["ref_" + kind]
    if kind == "enc":
        assert sv["drop"] == P_LAYER and sv["seed_base"] == BASE
        masks = case["masks"]
        if case["L"] == 3:                                    # every layer draws its own masks
            for a, b in ((0, 1), (1, 2), (0, 2)):
                assert all(not np.array_equal(masks[a][s], masks[b][s]) for s in (1, 2, 3))
                assert not np.array_equal(masks[a][0][(2, 0)], masks[b][0][(2, 0)])
    else:
        assert sv["drop"] == (P_LAYER, PD.page_dropout_seed(BASE, PD.MAX_LAYERS, 0))
        assert sv["drop"][1] == engine.page_dropout_seed(BASE, weights.PAGE_ENCODER_MAX_LAYERS, 0)
    e_out, e_dh = relerr(got["out"], ref["out"]), relerr(got["dh"], ref["dh"])
    errs = {k: relerr(got["grads"][k], ref["grads"][k]) for k in ref["grads"]}
    worst = max(errs, key=errs.get)
    print("%s %s: out %.2e, dh %.2e, worst parameter gradient %.2e (%s)" % (name, kind, e_out, e_dh, errs[worst], worst))
    assert e_out < 1e-5 and e_dh < 1e-4
    for k, e in errs.items():
        assert float(np.abs(ref["grads"][k]).max()) > 0, k
        assert e < 1e-4, (k, e)
    assert same_bits(got, run_layer(case, kind, **on)[0])
    other, _ = run_layer(case, kind, **dict(on, seed_base=AD.dropout_base(7, 2)))
    assert not bits_equal(got["out"], other["out"])


# ---------------------------------------------------------------- 7. off is off
@pytest.mark.parametrize("kind", ["att", "enc"])
def test_rate_zero_or_eval_mode_is_the_existing_path_bit_for_bit(kind):
    case = layer_case("geo")
    (ref, sv0), calls0 = profiled(lambda: run_layer(case, kind))
    assert not any(n in calls0 for n in NEW) and not sv0["drop"]
    key = engine.PAGE_ENC_DROP_KEY if kind == "enc" else engine.PAGE_ATTN_DROP_KEY
    for kw in (dict(dropout=0.0, seed_base=BASE), dict(dropout=0, seed_base=BASE, training=True),
               dict(dropout=0.5, seed_base=BASE, training=False), dict(dropout=0.5, seed_base=BASE, training={key: False})):
        (got, sv), calls = profiled(lambda: run_layer(case, kind, **kw))
        assert calls == calls0 and not sv["drop"], kw
        assert same_bits(got, ref), kw
    (got, sv), calls = profiled(lambda: run_layer(case, kind, dropout=0.5, seed_base=BASE, training={"decoder.0": False}))
    assert sv["drop"] and any(n in calls for n in NEW) and not same_bits(got, ref)
    L = case["L"]
    want = dict(calls0)
    if kind == "enc":
        for plain, drop, n in ((PA_FWD_G, PA_FWD_GD, L), (PA_BWD_G, PA_BWD_GD, L), (GELU_FWD, GELU_FWD_D, L),
                               (GELU_BWD, GELU_BWD_D, L)):
            assert want.pop(plain) == n
            want[drop] = n
        want[ADD_FWD] = want[REGEN_BWD] = 2 * L
    else:
        assert want.pop(PA_FWD_G) == 1 and want.pop(PA_BWD_G) == 1
        want[PA_FWD_GD] = want[PA_BWD_GD] = 1
    assert calls == want
    for bad in (1.0, -0.1, NAN):
        with pytest.raises(ValueError, match="page_encoder_dropout" if kind == "enc" else "page_attention_dropout"):
            run_layer(case, kind, dropout=bad)


# ---------------------------------------------------------------- 8. the modules under autograd
def module_run(layer, case, geometry):
    h = dev(case["h"]).requires_grad_(True)
    args = (dev(case["bboxes"]), PAGE_SIZE) if geometry else ()
    layer.zero_grad()
    out = layer(h, dev(case["ps"]), *args)
    (out * dev(case["g"])).sum().backward()
    return [out.detach(), h.grad] + [q.grad.clone() for q in layer.parameters()]


@pytest.mark.parametrize("kind", ["att", "enc"])
def test_modules_match_the_oracle_in_train_mode_and_are_the_plain_layers_in_eval_mode(kind):
    case = layer_case("geo")
    Fd, P, Hh, L, M = (case[k] for k in ("F", "P", "Hh", "L", "M"))
    if kind == "enc":
        layer, zero = PageEncoder(Fd, P, Hh, L, M, True, dropout=P_LAYER), PageEncoder(Fd, P, Hh, L, M, True)
        prefix, sd, name = "page_encoder.", case["sd"], "drop"
    else:
        layer, zero = PageAttention(Fd, P, Hh, geometry=True, dropout=P_LAYER), PageAttention(Fd, P, Hh, geometry=True)
        prefix, sd, name = "page_attention.", case["att_sd"], "attn_drop"
    state = {k[len(prefix):]: torch.from_numpy(v) for k, v in sd.items()}
    assert list(layer.state_dict()) == list(state) == list(zero.state_dict())
    layer.load_state_dict(state), zero.load_state_dict(state)
    layer, zero = layer.to(DEV).train(), zero.to(DEV).train()
    layer.seed_dropout(7)                                     # call 1 draws from BASE = dropout_base(7, 1)
    got, ref = module_run(layer, case, True), case["ref_" + kind]
    assert relerr(got[0].cpu(), ref["out"]) < 1e-5 and relerr(got[1].cpu(), ref["dh"]) < 1e-4
    for (k, q) in layer.named_parameters():
        assert relerr(q.grad.cpu(), ref["grads"][prefix + k]) < 1e-4, k
    second = module_run(layer, case, True)                    # call 2: the next stream
    assert not torch.equal(second[0], got[0])
    layer.seed_dropout(7)
    assert all(torch.equal(a, b) for a, b in zip(module_run(layer, case, True), got))
    plain = module_run(zero, case, True)
    assert not torch.equal(plain[0], got[0])
    assert all(torch.equal(a, b) for a, b in zip(module_run(layer.eval(), case, True), plain))
    layer.train()
    getattr(layer, name).eval()                               # the one submodule switches the layer's dropout off
    assert layer.training and all(torch.equal(a, b) for a, b in zip(module_run(layer, case, True), plain))


# ---------------------------------------------------------------- 9. the whole model
ENC = dict(page_encoder_dim=8, page_encoder_heads=2, page_encoder_layers=2)
RATES = dict(page_attention_dropout=0.5, page_encoder_dropout=0.1)


def model_inputs(**extra):
    cfg, ocfg, sd, b, ps, img_h = CC.all_on_inputs(True, drop_prob=0.2, **dict(ENC, **extra))
    return dict(cfg, **RATES), ocfg, sd, b, ps, img_h


def build_model(cfg, sd, img_h):
    kw = {k: cfg[k] for k in list(CC.ALL_ON) + list(ENC) + list(RATES) + ["attention_dropout"] if k in cfg}
    m = CoVA(cfg["roi_output_size"], img_h, cfg["n_classes"], cfg["use_context"], cfg["hidden_dim"], cfg["bbox_hidden_dim"],
             cfg["n_additional_feat"], cfg["drop_prob"], None, **kw)
    assert list(m.state_dict()) == list(sd)
    missing = m.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return m.to(DEV)


def test_model_with_every_dropout_on_matches_the_composed_oracle_on_the_reference_inputs():
    cfg, ocfg, sd, b, ps, img_h = model_inputs(attention_dropout=0.5)
    inputs = (b["images"], b["bboxes"], b["additional_feats"], b["context_indices"])
    sd64, inputs64 = {k: CC.f64(v) for k, v in sd.items()}, [CC.f64(t) for t in inputs]
    args = [t.to(DEV) for t in inputs]
    page = tuple(b["images"].shape[2:])
    N, K = b["context_indices"].shape
    m = build_model(cfg, sd, img_h).train()
    m.seed_dropout(5)
    logits = m(*args)
    sv = logits.grad_fn.sv
    base = AD.dropout_base(5, 1)
    assert sv["page_attn"]["drop"] == (0.5, PD.page_dropout_seed(base, PD.MAX_LAYERS, 0))
    assert sv["page_enc"]["drop"] == 0.1 and sv["page_enc"]["seed_base"] == base
    keeps = {}
    for l, layer in enumerate(sv["gat"]):
        for i, head in enumerate(layer["heads"]):
            stream = AD.attention_dropout_seed(base, l, i)
            assert head["drop"] == (0.5, stream)
            keeps[head["prefix"]] = AD.keep_mask(0.5, stream, N, K)
    oracle_masks = [sv["dec"][k].cpu().double() for k in ("m1", "m2")]          # the decoder's own masks, as generated
    assert all(0.0 < float(t.mean()) < 1.0 for t in oracle_masks)
    routing = routing_from_saved(dict(sv, gat=None))
    for layer in sv["gat"]:
        for head in layer["heads"]:
            routing["gate_" + head["prefix"] + "leaky"] = device_gates(head["Wh"], head["ctx"])
    routing[CO.RO_GATE] = (sv["readout"]["u"] > 0).cpu()
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(logits, b["labels"].to(DEV))
    loss.backward()
    hook = PD.patched(ps, b["bboxes"], page, base, heads=CC.ALL_ON["page_attention_heads"], p_attn=0.5,
                      encoder_heads=ENC["page_encoder_heads"], p_enc=0.1, keeps=keeps, attention_dropout=0.5)
    with CC.stated(*hook, any_dtype=True):
        loss_ref, logits_ref, grads_ref, _, _ = O.loss_and_grads(sd64, *inputs64, b["labels"], ocfg, oracle_masks, routing)
    assert logits_ref.dtype == torch.float64
    el, eo = relerr(logits.detach().cpu(), logits_ref), abs(loss.item() - float(loss_ref)) / abs(float(loss_ref))
    print("train logits %.2e, loss %.2e" % (el, eo))
    assert el < LOGIT_TOL and eo <= LOSS_TOL
    grads = {k: p.grad for k, p in m.named_parameters()}
    assert set(grads) == set(grads_ref)
    print("worst gradient on the 1 % floor:", compare_grads(grads, grads_ref, rtol=GRAD_TOL, outlier_frac=0.0))
    # the page masks are live: the oracle without them is another model
    plain = PE.patched(ps, b["bboxes"], page, heads=2, keeps=keeps, attention_dropout=0.5, encoder_heads=2)
    with CC.stated(*plain, any_dtype=True):
        _, logits_plain, _, _, _ = O.loss_and_grads(sd64, *inputs64, b["labels"], ocfg, oracle_masks, routing)
    assert relerr(logits_plain.detach(), logits_ref.detach()) > 1e-3
    # eval mode: the model without the options, bit for bit
    off = {k: v for k, v in cfg.items() if k not in RATES}
    with torch.no_grad():
        assert torch.equal(m.eval()(*args), build_model(off, m.state_dict(), img_h).eval()(*args))


# ---------------------------------------------------------------- 10. the trainer
def test_trainer_gradients_agree_with_the_module_under_the_same_seeds():
    cfg, _, sd, b, ps, img_h = model_inputs()
    batch = {k: v.to(DEV) for k, v in b.items() if torch.is_tensor(v)}
    tr = HotPathTrainer(cfg, sd, DEV, dropout_seed=5)
    assert tr.cfg["page_attention_dropout"] == 0.5 and tr.cfg["page_encoder_dropout"] == 0.1
    loss, _ = tr.forward_backward(batch)
    m = build_model(cfg, sd, img_h).train()
    m.seed_dropout(5)
    logits = m(batch["images"], batch["bboxes"], batch["additional_feats"], batch["context_indices"])
    mloss = torch.nn.CrossEntropyLoss(reduction="sum")(logits, batch["labels"])
    mloss.backward()
    assert abs(float(loss) - float(mloss.detach())) <= LOSS_TOL * abs(float(mloss.detach()))
    ref = {k: q.grad.detach().cpu() for k, q in m.named_parameters()}
    print("worst gradient:", compare_grads({k: v.clone() for k, v in tr.grads.items()}, ref, rtol=GRAD_TOL, outlier_frac=0.0))
    other = HotPathTrainer(cfg, sd, DEV, dropout_seed=6)
    other.forward_backward(batch)
    for k in ("page_attention.qkv.weight", "page_encoder.layers.1.ffn2.weight"):
        assert not torch.equal(other.grads[k], tr.grads[k]), k


PCFG = dict(CFG, page_attention_dim=16, page_attention_heads=2, **ENC)        # the page layers on, no dropout in them
DCFG = dict(PCFG, **RATES)


def test_five_steps_follow_the_seed_and_a_checkpoint_carries_the_options():
    u8, rows = page_set()
    ds = DeviceDataset(u8, rows, 2, DEV, spatial_k=6)
    sd = seeded(PCFG)
    a, b, c = (HotPathTrainer(DCFG, sd, DEV, dropout_seed=s) for s in (5, 5, 6))
    la, sa = five_steps(a, ds)
    lb, sb = five_steps(b, ds)
    lc, sc = five_steps(c, ds)
    assert la == lb and list(sa) == list(sb) and set(sa) == set(sd)          # no new state_dict keys
    for key in sa:
        assert torch.equal(sa[key], sb[key]), key
    assert la != lc and not torch.equal(sa["page_encoder.input.weight"], sc["page_encoder.input.weight"])
    plain = HotPathTrainer(PCFG, sd, DEV, dropout_seed=5)
    assert five_steps(plain, ds)[0] != la
    # a checkpoint: the cfg carries the options, a trainer rebuilt from it steps as the original
    blob = io.BytesIO()
    torch.save(dict(cfg=a.cfg, model=a.state_dict(), optimizer=a.optimizer_state_dict()), blob)
    blob.seek(0)
    ckpt = torch.load(blob, map_location="cpu", weights_only=False)
    assert {k: ckpt["cfg"][k] for k in RATES} == RATES
    d = HotPathTrainer(ckpt["cfg"], ckpt["model"], DEV, dropout_seed=5)
    d.load_optimizer_state_dict(ckpt["optimizer"])
    assert d.step_count == a.step_count == 5 and d.cfg == a.cfg
    batch = next(iter(ds.batches(3, prefetch=False)))
    assert float(a.train_step(batch)[0]) == float(d.train_step(batch)[0]) and torch.equal(a.pbucket.flat, d.pbucket.flat)
    for bad in (dict(PCFG, page_encoder_dropout=1.0), dict(CFG, page_encoder_dropout=0.1),
                dict(CFG, page_attention_dropout=0.1)):
        with pytest.raises(ValueError, match="dropout"):
            HotPathTrainer(bad, seeded({k: v for k, v in bad.items() if k not in RATES}), DEV)


def test_predict_evaluate_split_cached_steps_and_averaged_weights_with_the_options_on():
    u8, rows = page_set(P=9, seed=4)
    v8, vrows = page_set(P=11, seed=9)
    train, val = DeviceDataset(u8, rows, 2, DEV, spatial_k=6), DeviceDataset(v8, vrows, 2, DEV, spatial_k=6)
    kw = dict(frozen=("convnet.",), bn_eval=("convnet.",), dropout_seed=8, average="ema", average_decay=0.5)
    sd = seeded(PCFG)
    a, b = HotPathTrainer(DCFG, sd, DEV, **kw), HotPathTrainer(DCFG, sd, DEV, **kw)
    plain = HotPathTrainer(PCFG, sd, DEV, **kw)
    full = next(iter(val.batches(11, prefetch=False)))
    (logits, _), calls = profiled(lambda: a.predict(full))
    assert not any(n in calls for n in NEW) and torch.equal(logits, plain.predict(full)[0])
    assert torch.equal(a.loss(full), plain.loss(full))
    ra, rp = evaluate_split(a, val, with_loss=True), evaluate_split(plain, val, with_loss=True)
    assert np.array_equal(ra.ranks, rp.ranks) and ra.loss == rp.loss
    cache = FeatureCache.build(a, train)
    for fb, cb in zip(train.batches(3, prefetch=False), train.batches(3, features=cache)):
        assert "images" not in cb
        _, calls = profiled(lambda: (a.train_step(fb), b.train_step(cb)))
        assert calls[PA_FWD_D] == 2 * 3 and calls[ADD_FWD] == 2 * 4 and PA_FWD not in calls and GELU_FWD not in calls
        assert torch.equal(a.gbucket.flat, b.gbucket.flat) and torch.equal(a.pbucket.flat, b.pbucket.flat)
    ref = HotPathTrainer(PCFG, a.averaged_state_dict(), DEV)
    with a.averaged_weights():                                # evaluation on the averaged model: the plain path again
        (logits, _), calls = profiled(lambda: a.predict(full))
        assert not any(n in calls for n in NEW) and torch.equal(logits, ref.predict(full)[0])


def test_default_step_issues_none_of_the_new_launches_and_the_options_add_exactly_their_own():
    u8, rows = page_set(P=3)
    batch = next(iter(DeviceDataset(u8, rows, 2, DEV, spatial_k=6).batches(3, prefetch=False)))
    _, default = profiled(lambda: HotPathTrainer(CFG, seeded(CFG), DEV).train_step(batch))
    _, plain = profiled(lambda: HotPathTrainer(PCFG, seeded(PCFG), DEV).train_step(batch))
    assert not any(n in default for n in NEW) and not any(n in plain for n in NEW)
    off = dict(PCFG, page_attention_dropout=0.0, page_encoder_dropout=0)
    _, again = profiled(lambda: HotPathTrainer(off, seeded(PCFG), DEV).train_step(batch))
    assert again == plain
    L = ENC["page_encoder_layers"]
    delta = lambda calls: {k: calls.get(k, 0) - plain.get(k, 0) for k in set(calls) | set(plain)
                           if calls.get(k, 0) != plain.get(k, 0)}
    _, att = profiled(lambda: HotPathTrainer(dict(PCFG, page_attention_dropout=0.5), seeded(PCFG), DEV).train_step(batch))
    assert delta(att) == {PA_FWD_D: 1, PA_BWD_D: 1, PA_FWD: -1, PA_BWD: -1}, delta(att)
    _, enc = profiled(lambda: HotPathTrainer(dict(PCFG, page_encoder_dropout=0.1), seeded(PCFG), DEV).train_step(batch))
    assert delta(enc) == {PA_FWD_D: L, PA_BWD_D: L, PA_FWD: -L, PA_BWD: -L, GELU_FWD_D: L, GELU_BWD_D: L, GELU_FWD: -L,
                          GELU_BWD: -L, ADD_FWD: 2 * L, REGEN_BWD: 2 * L}, delta(enc)
    _, both = profiled(lambda: HotPathTrainer(DCFG, seeded(PCFG), DEV).train_step(batch))
    assert delta(both) == {PA_FWD_D: L + 1, PA_BWD_D: L + 1, PA_FWD: -L - 1, PA_BWD: -L - 1, GELU_FWD_D: L, GELU_BWD_D: L,
                           GELU_FWD: -L, GELU_BWD: -L, ADD_FWD: 2 * L, REGEN_BWD: 2 * L}, delta(both)
