"""GPU tests of the page encoder (CoVA(page_encoder_dim=P, ...)): cova_layernorm_fwd / _bwd and
cova_gelu_fwd / _bwd through the C ABI on framed, guarded buffers against the float64 torch oracle
(tests/page_encoder_oracle.py: autograd, no code shared with the kernels), refusals and empty work, the composed layer
(engine.page_encoder_fwd / page_encoder_bwd), the whole model under autograd through the oracle's hook, and HotPathTrainer
with the option on.

Bounds: the project's own for the page layers (tests/test_page_attention_gpu.py, tests/test_page_readout_gpu.py): max-abs
error over max-abs float64 reference below 1e-5 for what a forward writes and below 1e-4 for gradients.  The float32 oracle
sits at 2e-7 to 6e-7 at (P, L) = (8, 1), (128, 2) and (512, 3), so depth needs no wider bound.  The rows of 30 + N(0, 1)
separate the two-pass variance (about 1e-6) from a one-pass E[x^2] - mean^2 (about 1e-4) by a factor of ten on either
side of 1e-5.  The whole model on the cova_h64_n11 inputs keeps tests/test_model_gpu.py's LOGIT_TOL / LOSS_TOL / GRAD_TOL.

Measured on an MI355X (worst over all cases; bound in brackets): LayerNorm out 1.6e-7, mean 1.2e-7, rstd 1.1e-7 [1e-5], dx
2.0e-7, dweight 1.8e-7, dbias 1.7e-7 [1e-4]; rows of 30 + N(0, 1): out 1.1e-6, rstd 8e-8 [1e-5]; GELU 7.5e-8 [1e-5] and
1.1e-7 [1e-4]; the composed layer: out 4.7e-7 [1e-5], dh 4.0e-7, parameter gradients 9.0e-7 [1e-4]; the model: eval logits
1.5e-7, train logits 4.3e-6 [5e-5], loss 2.5e-6 [2e-5], gradients on the 1 % floor 1.7e-5, the encoder's tensors on their own
scale 1.9e-5 [1e-4].  44 tests in 3.4 s."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import _lib, engine, weights  # noqa: E402
from cova_web_object_detection_amd.evaluation import evaluate_split  # noqa: E402
from cova_web_object_detection_amd.features import FeatureCache  # noqa: E402
from cova_web_object_detection_amd.models import CoVA, PageEncoder  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
from helpers import (bits_equal, compare_grads, DEV, framed, GRAD_TOL, GUARD, LOGIT_TOL,  # noqa: E402
                     LOSS_TOL, NAN, padded, profiled, relerr, routing_from_saved, starts, survived)
from oracle import cova_oracle as O  # noqa: E402
import combined_cases as CC  # noqa: E402
import combined_oracle as CO  # noqa: E402
import page_attn_geo_oracle as PG  # noqa: E402
import page_encoder_oracle as PE  # noqa: E402
from config_cases import SPLIT_CFG as CFG  # noqa: E402
from gat_cases import device_gates  # noqa: E402
from trainer_cases import five_steps, page_set, seeded  # noqa: E402

LN_FWD, LN_BWD, LN_WSQ = "cova_layernorm_fwd", "cova_layernorm_bwd", "cova_layernorm_workspace_floats"
GELU_FWD, GELU_BWD = "cova_gelu_fwd", "cova_gelu_bwd"
EPS = 1e-5
LN_BWD_ROWS = 32           # csrc/page_encoder.hip's header: "block b owns the rows [b * LN_BWD_ROWS, ...), LN_BWD_ROWS = 32"

f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------- 1. LayerNorm through the C ABI
#             R     C   pad  (pad: extra floats per row; odd = unaligned rows = the scalar form)
LN_SHAPES = {"one": (1, 4, 0),                               # one row, one chunk
             "scalar": (5, 7, 3),                            # the scalar path, unaligned rows
             "partial": (65, 36, 4),                         # lanes filled in part
             "below": (LN_BWD_ROWS - 1, 128, 4),             # the partial-block boundary of the backward
             "at": (LN_BWD_ROWS, 128, 4),
             "above": (LN_BWD_ROWS + 1, 128, 4),
             "second": (300, 260, 4),                        # a lane's second chunk filled in part
             "limit": (70, 512, 0),                          # the channel limit
             "fold": (1100, 128, 4)}                         # many blocks in the fold


def ln_oracle(case):
    x, w, b = (f64(case[k]).requires_grad_(True) for k in ("x", "w", "b"))
    out, mean, rstd = PE.layer_norm(x, w, b, EPS, return_stats=True)
    (out * f64(case["g"])).sum().backward()
    return dict(out=out.detach().numpy(), mean=mean.detach().numpy(), rstd=rstd.detach().numpy(), dx=x.grad.numpy(),
                dw=w.grad.numpy(), db=b.grad.numpy())


def build_ln_case(R, C, pad, seed, offset=0.0):
    rs = np.random.RandomState(seed)
    return dict(R=R, C=C, pad=pad, x=(offset + rs.standard_normal((R, C))).astype(np.float32),
                w=rs.uniform(0.5, 1.5, C).astype(np.float32), b=(0.1 * rs.standard_normal(C)).astype(np.float32),
                g=rs.standard_normal((R, C)).astype(np.float32), res=rs.standard_normal((R, C)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def ln_case(name):
    case = build_ln_case(*LN_SHAPES[name], seed=sum(map(ord, name)))
    case["ref"] = ln_oracle(case)
    return case


def launch_ln(case, with_res=False, rows=None, in_place=False):
    """cova_layernorm_fwd + cova_layernorm_bwd over the first ``rows`` rows (all of them by default) on framed buffers
    -> dict of host arrays (guards checked).  ``in_place``: res IS dx."""
    R, C, pad = rows or case["R"], case["C"], case["pad"]
    ld = C + pad
    x, g = padded(case["x"][:R], ld), padded(case["g"][:R], ld)
    w, b = dev(case["w"]), dev(case["b"])
    out_b, out = framed(R, C, ld)
    mean_b, mean = framed(R, 1, 1)
    rstd_b, rstd = framed(R, 1, 1)
    dx_b, dx = framed(R, C, ld)
    dw_b, dw = framed(1, C, C)
    db_b, db = framed(1, C, C)
    res = None
    if with_res:
        res = padded(case["res"][:R], ld)
        if in_place:
            dx[:, :C] = res[:, :C]
            res = dx
    nws = engine.query(LN_WSQ, R, C)
    assert nws == -(-R // LN_BWD_ROWS) * 2 * C
    ws = torch.full((nws + 16,), NAN, device=DEV)
    ws[nws:] = GUARD
    engine.call(LN_FWD, x, ld, R, C, w, b, EPS, out, ld, mean, rstd)
    engine.call(LN_BWD, g, ld, x, ld, mean, rstd, w, R, C, res, ld if with_res else 0, dx, ld, dw, db, ws)
    torch.cuda.synchronize()
    assert (ws[nws:] == GUARD).all() and bool(torch.isfinite(ws[:nws]).all())
    return dict(out=survived(out_b, R, C), mean=survived(mean_b, R, 1).reshape(-1), rstd=survived(rstd_b, R, 1).reshape(-1),
                dx=survived(dx_b, R, C), dw=survived(dw_b, 1, C).reshape(-1), db=survived(db_b, 1, C).reshape(-1))


def check_ln(got, ref, what, res=None):
    want_dx = ref["dx"] if res is None else ref["dx"] + res.astype(np.float64)
    errs = {k: relerr(got[k], ref[k]) for k in ("out", "mean", "rstd", "dw", "db")}
    errs["dx"] = relerr(got["dx"], want_dx)
    print(what, {k: "%.2e" % v for k, v in errs.items()})
    for k, e in errs.items():
        assert e < (1e-5 if k in ("out", "mean", "rstd") else 1e-4), (what, k, e)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("name", list(LN_SHAPES))
def test_layernorm_forward_and_backward_match_the_float64_oracle(name, with_res):
    case = ln_case(name)
    got = launch_ln(case, with_res)
    check_ln(got, case["ref"], "%s res=%s" % (name, with_res), case["res"] if with_res else None)
    again = launch_ln(case, with_res)
    for k in got:                                             # two launches are bit-equal
        assert bits_equal(got[k], again[k]), k
    if with_res:                                              # the stream gradient updated in place: the same bits
        inp = launch_ln(case, True, in_place=True)
        for k in got:
            assert bits_equal(got[k], inp[k]), k


@pytest.mark.parametrize("with_res", [False, True])
def test_a_row_does_not_depend_on_the_rows_around_it(with_res):
    case = ln_case("partial")
    assert case["R"] == 65
    few, many = launch_ln(case, with_res, rows=5), launch_ln(case, with_res)
    for k in ("out", "mean", "rstd", "dx"):
        assert bits_equal(few[k], many[k][:5]), k
    assert not bits_equal(few["dw"], many["dw"])              # (sums over rows: other rows, other sums)


# ---------------------------------------------------------------- 2. two numerical corners
@pytest.mark.parametrize("C,pad", [(36, 4), (7, 3), (512, 0)])
def test_a_constant_row_gives_the_bias_exactly_and_a_finite_gradient(C, pad):
    """2.5 * C and -0.75 * C are exact in float32, so the mean is the constant, every centred value is +0 and the variance
    is 0: rstd = 1 / sqrt(eps), out = fma(0, weight, bias) = bias."""
    case = build_ln_case(6, C, pad, seed=C)
    case["x"][1], case["x"][4] = np.float32(2.5), np.float32(-0.75)
    got = launch_ln(case)
    for r, c in ((1, 2.5), (4, -0.75)):
        assert got["mean"][r] == np.float32(c) and bits_equal(got["out"][r], case["b"])
        assert abs(got["rstd"][r] - 1 / np.sqrt(EPS)) < 1e-5 / np.sqrt(EPS)
    assert np.isfinite(got["dx"]).all() and np.isfinite(got["dw"]).all()
    check_ln(got, ln_oracle(case), "constant rows C=%d" % C)


@pytest.mark.parametrize("C", [36, 128, 512])
def test_rows_far_from_zero_hold_the_forward_bound(C):
    """Rows of 30 + N(0, 1): a two-pass float32 variance errs by about 1e-6 here, a one-pass E[x^2] - mean^2 by about 1e-4."""
    case = build_ln_case(40, C, 4, seed=C + 1, offset=30.0)
    got, ref = launch_ln(case), ln_oracle(case)
    check_ln(got, ref, "offset rows C=%d" % C)
    x = case["x"].astype(np.float32)
    one_pass = (x * x).mean(1, dtype=np.float32) - x.mean(1, dtype=np.float32) ** 2          # what the kernel must not do
    assert relerr(1 / np.sqrt(one_pass + np.float32(EPS)), ref["rstd"]) > 1e-5


# ---------------------------------------------------------------- 3. GELU
GELU_SHAPES = [(1, 4, 0), (5, 7, 3), (90, 256, 4), (33, 2048, 0)]


@pytest.mark.parametrize("R,C,pad", GELU_SHAPES)
def test_gelu_forward_and_backward_match_the_float64_oracle(R, C, pad):
    rs = np.random.RandomState(R + C)
    z = rs.uniform(-6, 6, (R, C)).astype(np.float32)
    z[0, 0] = 0.0
    if C > 4:
        z[-1, 1:4] = [-6.0, 6.0, -0.0]
    g = rs.standard_normal((R, C)).astype(np.float32)
    ld = C + pad
    zd, gd = padded(z, ld), padded(g, ld)
    out_b, out = framed(R, C, ld)
    dz_b, dz = framed(R, C, ld)
    engine.call(GELU_FWD, zd, ld, R, C, out, ld)
    engine.call(GELU_BWD, gd, ld, zd, ld, R, C, dz, ld)
    torch.cuda.synchronize()
    got_out, got_dz = survived(out_b, R, C), survived(dz_b, R, C)
    e_f = relerr(got_out, PE.gelu(f64(z)).numpy())
    e_b = relerr(got_dz, (PE.gelu_grad(f64(z)) * f64(g)).numpy())
    print("gelu (%d, %d, %d): forward %.2e, backward %.2e" % (R, C, pad, e_f, e_b))
    assert e_f < 1e-5 and e_b < 1e-4
    zero = z == 0
    assert zero.any() and (got_out[zero] == 0).all() and bits_equal(got_dz[zero], np.float32(0.5) * g[zero])
    out2_b, out2 = framed(R, C, ld)
    engine.call(GELU_FWD, zd, ld, R, C, out2, ld)
    torch.cuda.synchronize()
    assert bits_equal(survived(out2_b, R, C), got_out)


# ---------------------------------------------------------------- 4. refusals and empty work
def test_entry_points_refuse_bad_arguments_and_skip_empty_work():
    R, C, M = 9, 16, 24
    full = lambda *shape: torch.full(shape, GUARD, device=DEV)
    x, g, w, b = (torch.randn(s, device=DEV) for s in ((R, C), (R, C), (C,), (C,)))
    out, mean, rstd, dx, dw, db = full(R, C), full(R), full(R), full(R, C), full(C), full(C)
    ws = torch.zeros(engine.query(LN_WSQ, R, C), device=DEV)
    z, gz, go, dz = torch.randn(R, M, device=DEV), torch.randn(R, M, device=DEV), full(R, M), full(R, M)
    good = {LN_FWD: [x, C, R, C, w, b, EPS, out, C, mean, rstd],
            LN_BWD: [g, C, x, C, mean, rstd, w, R, C, None, 0, dx, C, dw, db, ws],
            GELU_FWD: [z, M, R, M, go, M], GELU_BWD: [gz, M, z, M, R, M, dz, M]}
    bad = {LN_FWD: [{3: 0}, {3: 513}, {3: -4}, {2: -1}, {1: C - 1}, {8: C - 1}, {6: -1.0}, {0: None}, {4: None}, {5: None},
                    {7: None}, {9: None}, {10: None}],
           LN_BWD: [{8: 0}, {8: 513}, {7: -1}, {1: C - 1}, {3: C - 1}, {12: C - 1}, {9: dx, 10: C - 1}, {0: None}, {2: None},
                    {4: None}, {5: None}, {6: None}, {11: None}, {13: None}, {14: None}, {15: None}],
           GELU_FWD: [{3: 0}, {3: -8}, {2: -1}, {1: M - 1}, {5: M - 1}, {0: None}, {4: None}],
           GELU_BWD: [{5: 0}, {4: -1}, {1: M - 1}, {3: M - 1}, {7: M - 1}, {0: None}, {2: None}, {6: None}]}
    for name, changes in bad.items():
        for ch in changes:
            args = list(good[name])
            for i, v in ch.items():
                args[i] = v
            with pytest.raises(_lib.CovaHipError):
                engine.call(name, *args)
    # R == 0 launches nothing and needs no pointer
    engine.call(LN_FWD, None, C, 0, C, None, None, EPS, None, C, None, None)
    engine.call(LN_BWD, None, C, None, C, None, None, None, 0, C, None, 0, None, C, None, None, None)
    engine.call(GELU_FWD, None, M, 0, M, None, M)
    engine.call(GELU_BWD, None, M, None, M, 0, M, None, M)
    for name in good:
        args = list(good[name])
        args[{LN_FWD: 2, LN_BWD: 7, GELU_FWD: 2, GELU_BWD: 4}[name]] = 0
        engine.call(name, *args)
    torch.cuda.synchronize()
    for t in (out, mean, rstd, dx, dw, db, go, dz):
        assert (t == GUARD).all()
    q = lambda r, c: engine.query(LN_WSQ, r, c)
    assert q(1, 1) == 2 and q(32, 128) == 256 and q(33, 128) == 512 and q(1100, 512) == 35 * 1024
    assert q(0, 16) == 0 and q(-3, 16) == 0 and q(4, 0) == 0 and q(4, 513) == 0
    for name in good:                                         # and the good calls are good
        engine.call(name, *good[name])
    torch.cuda.synchronize()
    for t in (out, mean, rstd, dx, dw, db, go, dz):
        assert bool(torch.isfinite(t).all()) and (t != GUARD).all()


# ---------------------------------------------------------------- 5. the composed layer
#                 pages            F    P   Hh   M   L  geometry
LAYER_CASES = {"small": ((37, 0, 1, 5, 0), 40, 8, 2, 16, 1, False),          # empty pages, a one-box page
               "head": ((90, 11), 608, 128, 4, 256, 2, False),               # the configs[1] head
               "geo": ((16, 17, 65), 100, 32, 2, 64, 3, True)}               # the attention's tile edges
PAGE_SIZE = (PG.PAGE_H, PG.PAGE_W)


def build_layer_case(name, sizes, Fd, P, Hh, M, L, geometry, seed):
    rs = np.random.RandomState(seed)
    N = int(sum(sizes))
    sd = {}
    for k, s in weights.page_encoder_entries(Fd, P, Hh, L, M, geometry):
        if ".norm" in k:
            v = rs.uniform(0.5, 1.5, s) if k.endswith("weight") else 0.1 * rs.standard_normal(s)
        elif k.endswith("geometry.weight"):
            v = rs.uniform(-2, 2, s)
        elif len(s) == 2:
            v = rs.uniform(-1, 1, s) / np.sqrt(s[1])
        else:
            v = rs.uniform(-0.05, 0.05, s)
        sd[k] = v.astype(np.float32)
    return dict(name=name, sizes=tuple(sizes), N=N, F=Fd, P=P, Hh=Hh, M=M, L=L, geometry=geometry, ps=starts(sizes), sd=sd,
                h=rs.standard_normal((N, Fd)).astype(np.float32), g=rs.standard_normal((N, P)).astype(np.float32),
                bboxes=PG.planted_boxes(sizes, seed + 1))


def layer_oracle(case):
    sd = {k: f64(v).requires_grad_(True) for k, v in case["sd"].items()}
    h = f64(case["h"]).requires_grad_(True)
    phi = PG.page_features(case["bboxes"], case["ps"], PG.PAGE_W, PG.PAGE_H) if case["geometry"] else None
    out = PE.page_encoder(h, sd, case["ps"], case["Hh"], phi)
    (out * f64(case["g"])).sum().backward()
    return dict(out=out.detach().numpy(), dh=h.grad.numpy(), grads={k: v.grad.numpy() for k, v in sd.items()})


@functools.lru_cache(maxsize=None)
def layer_case(name):
    case = build_layer_case(name, *LAYER_CASES[name], seed=sum(map(ord, name)))
    case["ref"] = layer_oracle(case)
    return case


def run_layer(case, sd=None):
    """engine.page_encoder_fwd / page_encoder_bwd inside a [N, F + P + 1] feature matrix, as engine._head_fwd places them
    (for "small" and "geo" no row of it is 16-byte aligned) -> dict(out, dh, grads) of host arrays."""
    N, Fd, P = case["N"], case["F"], case["P"]
    T = Fd + P + (0 if case["name"] == "head" else 1)
    sd = case["sd"] if sd is None else sd
    params = {k: dev(v) for k, v in sd.items()}
    geo = any(k.endswith("geometry.weight") for k in sd)
    comb = torch.full((N, T), NAN, device=DEV)
    comb[:, :Fd] = dev(case["h"])
    ps = dev(case["ps"])
    sv = engine.page_encoder_fwd(comb, T, N, Fd, ps, params, case["Hh"], case["L"], comb[:, Fd:], T,
                                 bboxes=dev(case["bboxes"]) if geo else None, page_size=PAGE_SIZE)
    assert len(sv["blocks"]) == case["L"] and all(k in sv["blocks"][0] for k in ("x1", "x2", "mean1", "rstd1", "mean2", "rstd2",
                                                                                "qkv", "lse", "O", "z", "f"))
    dcomb = torch.zeros((N, T), device=DEV)
    dcomb[:, Fd:Fd + P] = dev(case["g"])
    grads = engine.page_encoder_bwd(sv, dcomb[:, Fd:], T, params, dcomb, T)
    torch.cuda.synchronize()
    assert set(grads) == set(sd)
    if T > Fd + P:
        assert bool(torch.isnan(comb[:, Fd + P:]).all()) and not dcomb[:, Fd + P:].any()
    return dict(out=comb[:, Fd:Fd + P].cpu().numpy(), dh=dcomb[:, :Fd].cpu().numpy(),
                grads={k: v.cpu().numpy().reshape(sd[k].shape) for k, v in grads.items()})


@pytest.mark.parametrize("name", list(LAYER_CASES))
def test_composed_layer_matches_the_float64_oracle_and_reruns_are_bit_identical(name):
    case = layer_case(name)
    got, ref = run_layer(case), case["ref"]
    e_out, e_dh = relerr(got["out"], ref["out"]), relerr(got["dh"], ref["dh"])
    errs = {k: relerr(got["grads"][k], ref["grads"][k]) for k in ref["grads"]}
    worst = max(errs, key=errs.get)
    print("%s: out %.2e, dh %.2e, worst parameter gradient %.2e (%s)" % (name, e_out, e_dh, errs[worst], worst))
    assert e_out < 1e-5 and e_dh < 1e-4
    for k, e in errs.items():
        assert float(np.abs(ref["grads"][k]).max()) > 0, k
        assert e < 1e-4, (k, e)
    assert any(k.endswith("geometry.weight") for k in errs) == case["geometry"]
    again = run_layer(case)
    assert bits_equal(got["out"], again["out"]) and bits_equal(got["dh"], again["dh"])
    for k in got["grads"]:
        assert bits_equal(got["grads"][k], again["grads"][k]), k


@pytest.mark.parametrize("name", list(LAYER_CASES))
def test_a_page_keeps_its_bits_alone_or_second_in_a_batch(name):
    case = layer_case(name)
    p = max(i for i, n in enumerate(case["sizes"]) if n > 0 and i > 0)
    lo, hi = int(case["ps"][p]), int(case["ps"][p + 1])
    alone = dict(case, sizes=(hi - lo,), N=hi - lo, ps=starts((hi - lo,)), h=case["h"][lo:hi], g=case["g"][lo:hi],
                 bboxes=case["bboxes"][lo:hi])
    a, b = run_layer(alone), run_layer(case)
    assert bits_equal(a["out"], b["out"][lo:hi]) and bits_equal(a["dh"], b["dh"][lo:hi])


def test_zero_geometry_weights_give_the_plain_paths_bits():
    case = layer_case("geo")
    zero = {k: (np.zeros_like(v) if k.endswith("geometry.weight") else v) for k, v in case["sd"].items()}
    plain = {k: v for k, v in case["sd"].items() if not k.endswith("geometry.weight")}
    a, b = run_layer(case, zero), run_layer(case, plain)
    assert bits_equal(a["out"], b["out"]) and bits_equal(a["dh"], b["dh"])
    for k in plain:
        assert bits_equal(a["grads"][k], b["grads"][k]), k
    assert not bits_equal(a["out"], run_layer(case)["out"])   # (the seeded geometry weights are live)


def test_page_encoder_module_under_autograd_matches_the_oracle():
    case = layer_case("small")
    layer = PageEncoder(case["F"], case["P"], case["Hh"], case["L"], case["M"])
    assert ["page_encoder." + k for k in layer.state_dict()] == list(case["sd"])
    layer.load_state_dict({k[len("page_encoder."):]: torch.from_numpy(v) for k, v in case["sd"].items()})
    layer = layer.to(DEV)
    h = dev(case["h"]).requires_grad_(True)
    out = layer(h, dev(case["ps"]))
    (out * dev(case["g"])).sum().backward()
    ref = case["ref"]
    assert relerr(out.detach().cpu(), ref["out"]) < 1e-5 and relerr(h.grad.cpu(), ref["dh"]) < 1e-4
    for k, p in layer.named_parameters():
        assert relerr(p.grad.cpu(), ref["grads"]["page_encoder." + k]) < 1e-4, k
    assert layer(h.detach()[:0], torch.zeros(1, dtype=torch.int64, device=DEV)).shape == (0, case["P"])


# ---------------------------------------------------------------- 6. the model
ENC = dict(page_encoder_dim=8, page_encoder_heads=2, page_encoder_layers=2)


def model_inputs(everything):
    """-> (cfg, ocfg, sd, batch, page_start, img_h, the page attention's heads) on the doubled cova_h64_n11 page: the encoder
    alone (no GAT, no other page layer) or with GAT + readout + page attention + geometry all on (combined_cases.ALL_ON)."""
    if everything:
        return CC.all_on_inputs(True, **ENC) + (CC.ALL_ON["page_attention_heads"],)
    fx, cfg, b = CC.doubled_page()
    cfg = dict(cfg, use_context=False, **ENC)
    sd = weights.seeded_state_dict(int(fx["meta/seed"]), logit_gain=float(fx["meta/logit_gain"]),
                                   **{k: v for k, v in cfg.items() if k != "drop_prob"})
    ps = torch.searchsorted(b["bboxes"][:, 0].contiguous(), torch.arange(3, dtype=torch.float32))
    return cfg, dict(cfg, use_context=True), sd, b, ps, int(fx["meta/img_h"]), 1


def build_model(cfg, sd, img_h):
    kw = {k: cfg[k] for k in list(CC.ALL_ON) + list(ENC) if k in cfg}
    m = CoVA(cfg["roi_output_size"], img_h, cfg["n_classes"], cfg["use_context"], cfg["hidden_dim"], cfg["bbox_hidden_dim"],
             cfg["n_additional_feat"], cfg["drop_prob"], None, **kw)
    assert list(m.state_dict()) == list(sd)
    missing = m.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return m.to(DEV)


@pytest.mark.parametrize("everything", [False, True], ids=["alone", "everything-on"])
def test_model_with_the_encoder_matches_the_oracle_on_the_reference_inputs(everything):
    """The whole model against O.loss_and_grads in float64 through page_encoder_oracle.patched.  With everything on the
    encoder is the FOURTH producer that accumulates into dcomb[:, :F] (after the GAT, the readout and the page attention):
    the gradients of bbox_feat_encoder.* and of the conv stack see the sum of all four."""
    cfg, ocfg, sd, b, ps, img_h, pa_heads = model_inputs(everything)
    enc_keys = [k for k in sd if k.startswith("page_encoder.")]
    assert len(enc_keys) == 1 + 2 * 11 + 2
    inputs = (b["images"], b["bboxes"], b["additional_feats"], b["context_indices"])
    sd64, inputs64 = {k: CC.f64(v) for k, v in sd.items()}, [CC.f64(t) for t in inputs]
    args = [t.to(DEV) for t in inputs]
    page = tuple(b["images"].shape[2:])
    hook = lambda: PE.patched(ps, b["bboxes"], page, heads=pa_heads, encoder_heads=ENC["page_encoder_heads"])
    with torch.no_grad():
        logits = build_model(cfg, sd, img_h).eval()(*args)
    with CC.stated(*hook(), any_dtype=True):
        ref = O.forward(O.clone_state_dict(sd64), *inputs64, ocfg, False)
    e = relerr(logits.cpu(), ref)
    print("eval logits %.2e" % e)
    assert e < LOGIT_TOL
    m = build_model(cfg, sd, img_h).train()
    m.seed_dropout(5)
    logits = m(*args)
    sv = logits.grad_fn.sv
    G, E = (16, 8) if everything else (0, 0)
    assert sv["P"] == 8 and sv["T"] == sv["F"] + sv["D"] + G + E + 8 and torch.equal(sv["page_start"].cpu(), ps)
    assert sv["page_enc"]["layers"] == 2 and ("readout" in sv) == ("page_attn" in sv) == ("gat" in sv) == everything
    routing = routing_from_saved(dict(sv, gat=None))
    for layer in sv.get("gat") or []:
        for head in layer["heads"]:
            routing["gate_" + head["prefix"] + "leaky"] = device_gates(head["Wh"], head["ctx"])
    if everything:
        routing[CO.RO_GATE] = (sv["readout"]["u"] > 0).cpu()
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(logits, b["labels"].to(DEV))
    loss.backward()
    with CC.stated(*hook(), any_dtype=True):
        loss_ref, logits_ref, grads_ref, _, _ = O.loss_and_grads(sd64, *inputs64, b["labels"], ocfg, None, routing)
    assert logits_ref.dtype == torch.float64
    el, eo = relerr(logits.detach().cpu(), logits_ref), abs(loss.item() - float(loss_ref)) / abs(float(loss_ref))
    print("train logits %.2e, loss %.2e" % (el, eo))
    assert el < LOGIT_TOL and eo <= LOSS_TOL
    grads = {k: p.grad for k, p in m.named_parameters()}
    assert set(grads) == set(grads_ref)
    print("worst gradient on the 1 % floor:", compare_grads(grads, grads_ref, rtol=GRAD_TOL, outlier_frac=0.0))
    worst = ("", 0.0)
    for k in enc_keys:                                        # (compare_grads floors the scale at 1 % of the largest gradient)
        # page_encoder.norm.bias is a bias in front of the decoder's Linear + train-mode BatchNorm: its gradient is the column
        # sum of dz W, and the rows of a BatchNorm's dz sum to zero, so it is analytically zero, a sum of cancelling terms.
        # tests/combined_cases.py's rule for such a bias: the larger of its own scale and its weight's, the scale of the terms.
        cancels = k == "page_encoder.norm.bias"
        scale = max(float(grads_ref[k].abs().max()), float(grads_ref["page_encoder.norm.weight"].abs().max())) if cancels else None
        assert cancels or float(grads_ref[k].abs().max()) > 0, k
        e = relerr(grads[k].cpu(), grads_ref[k], scale)
        worst = max(worst, (k, e), key=lambda x: x[1])
        assert e < 1e-4, (k, e)
    print("worst encoder tensor on its own scale:", worst)


ECFG = dict(CFG, **ENC)


def test_five_steps_with_the_encoder_are_reproducible_learn_and_survive_a_checkpoint():
    u8, rows = page_set()
    ds = DeviceDataset(u8, rows, 2, DEV, spatial_k=6)
    sd = seeded(ECFG)
    a, b = HotPathTrainer(ECFG, sd, DEV), HotPathTrainer(ECFG, sd, DEV)
    assert a.cfg["page_encoder_ffn_dim"] == 16 and a.params["page_encoder.layers.1.ffn1.weight"].shape == (16, 8)
    head = a._head_offset()                                   # the encoder's gradients sit in the head range of the bucket
    assert all(a.gbucket.offsets[k][0] >= head for k in a.params if k.startswith("page_encoder."))
    la, sa = five_steps(a, ds)
    lb, sb = five_steps(b, ds)
    assert la == lb and list(sa) == list(sb)
    for key in sa:
        assert torch.equal(sa[key], sb[key]), key
    for k in a.params:
        if k.startswith("page_encoder."):
            assert bool(torch.isfinite(sa[k]).all()) and not torch.equal(sa[k].cpu(), sd[k]), k
    la2, _ = five_steps(a, ds)                                # the same five batches again: the loss falls
    print("losses, first pass %s, second pass %s" % (la, la2))
    assert sum(la2) < sum(la)
    # checkpoint round trip: parameters, moments and step count into a fresh trainer, then one more identical step
    c = HotPathTrainer(ECFG, sd, DEV)
    c.load_state_dict(a.state_dict())
    c.load_optimizer_state_dict(a.optimizer_state_dict())
    assert torch.equal(a.pbucket.flat, c.pbucket.flat)
    batch = next(iter(ds.batches(3, prefetch=False)))
    assert float(a.train_step(batch)[0]) == float(c.train_step(batch)[0])
    assert torch.equal(a.pbucket.flat, c.pbucket.flat)
    with pytest.raises(ValueError, match="page_encoder_dim"):                     # a checkpoint without the encoder
        c.load_state_dict(seeded(CFG))
    with pytest.raises(ValueError, match="page_encoder_dim"):                     # and the reverse
        HotPathTrainer(CFG, seeded(CFG), DEV).load_state_dict(a.state_dict())
    with pytest.raises(ValueError, match="page_encoder_layers"):
        c.load_state_dict(seeded(dict(ECFG, page_encoder_layers=1)))


def test_cached_feature_steps_equal_the_recomputing_path_and_evaluate_split_runs():
    u8, rows = page_set(P=9, seed=4)
    v8, vrows = page_set(P=11, seed=9)
    train, val = DeviceDataset(u8, rows, 2, DEV, spatial_k=6), DeviceDataset(v8, vrows, 2, DEV, spatial_k=6)
    kw = dict(track_metrics=True, frozen=("convnet.",), bn_eval=("convnet.",))
    a, b = HotPathTrainer(ECFG, seeded(ECFG), DEV, **kw), HotPathTrainer(ECFG, seeded(ECFG), DEV, **kw)
    rep = evaluate_split(a, val, with_loss=True)
    assert rep.evaluated.all() and rep.ranks.shape == (11, 3) and np.isfinite(rep.loss)
    tcache, vcache = FeatureCache.build(a, train), FeatureCache.build(a, val)
    cached, full = next(iter(val.batches(11, features=vcache))), next(iter(val.batches(11, prefetch=False)))
    assert cached.get("images") is None and cached.get("page_start") is not None
    assert torch.equal(a.predict(cached)[0], a.predict(full)[0])
    plain = HotPathTrainer(CFG, seeded(CFG), DEV)
    assert not torch.equal(a.predict(full)[0], plain.predict(full)[0])
    stripped = {k: v for k, v in cached.items() if k not in ("images", "page_start")}
    with pytest.raises(ValueError, match="page_encoder_dim.*page_start"):
        a.predict(stripped)
    la = [float(a.train_step(batch)[0]) for batch in train.batches(3, features=tcache)]
    lb = [float(b.train_step(batch)[0]) for batch in train.batches(3, prefetch=False)]
    assert len(la) == 3 and la == lb and torch.equal(a.pbucket.flat, b.pbucket.flat)


def test_default_step_issues_none_of_the_new_launches_and_the_option_adds_exactly_its_own():
    u8, rows = page_set(P=3)
    batch = next(iter(DeviceDataset(u8, rows, 2, DEV, spatial_k=6).batches(3, prefetch=False)))
    _, plain = profiled(lambda: HotPathTrainer(CFG, seeded(CFG), DEV).train_step(batch))
    new = (LN_FWD, LN_BWD, LN_WSQ, GELU_FWD, GELU_BWD)
    assert not any(n in plain for n in new)
    off = dict(CFG, page_encoder_dim=0, page_encoder_heads=3, page_encoder_layers=4)       # off, said in so many words
    _, again = profiled(lambda: HotPathTrainer(off, seeded(CFG), DEV).train_step(batch))
    assert again == plain
    _, enc = profiled(lambda: HotPathTrainer(ECFG, seeded(ECFG), DEV).train_step(batch))
    L = ENC["page_encoder_layers"]
    added = {k: enc.get(k, 0) - plain.get(k, 0) for k in set(enc) | set(plain) if enc.get(k, 0) != plain.get(k, 0)}
    assert added == {LN_FWD: 2 * L + 1, LN_BWD: 2 * L + 1, GELU_FWD: L, GELU_BWD: L, "cova_page_attn_fwd": L,
                     "cova_page_attn_bwd": L, "cova_sgemm": (1 + 4 * L) + (8 * L + 2), "cova_colsum": 3 * L}, added
