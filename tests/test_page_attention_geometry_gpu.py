"""GPU tests of the box-geometry bias of the page self-attention (CoVA(page_attention_geometry=True)):
cova_page_attn_fwd_geo / cova_page_attn_bwd_geo through the C ABI against the float64 torch oracle
(tests/page_attn_geo_oracle.py: numpy-f32 features from tests/edge_oracle.py, autograd, no code shared with the kernels),
against the plain entry points at zero weights, refusals and empty work, models.PageAttention(geometry=True) and the whole
model under autograd, and HotPathTrainer with the option on.

Bounds: the project's own for this layer and for d_edge_w (tests/test_page_attention_gpu.py, tests/test_edge_gpu.py):
max-abs error over max-abs reference below 1e-5 for O, lse and A (recomputed on the host from the kernel's lse, the f32
qkv and the oracle's features), below 1e-4 for dqkv and d_geo_w.  The whole model on the cova_h64_n11 inputs keeps
tests/test_model_gpu.py's LOGIT_TOL / LOSS_TOL / GRAD_TOL.  That an exchange of the query and key roles is visible at
these bounds is shown on the CPU (tests/test_page_attention_geometry_cpu.py)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import _lib, engine, weights  # noqa: E402
from cova_web_object_detection_amd.evaluation import evaluate_split, fit, predict_split  # noqa: E402
from cova_web_object_detection_amd.features import FeatureCache  # noqa: E402
from cova_web_object_detection_amd.models import CoVA, PageAttention  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
from helpers import (bits_equal, compare_grads, DEV, framed, GRAD_TOL, GUARD, load_case, LOGIT_TOL,  # noqa: E402
                     LOSS_TOL, padded, profiled, relerr, routing_from_saved, starts, survived)
from oracle import cova_oracle as O  # noqa: E402
import page_attn_geo_oracle as PG  # noqa: E402
import page_attn_oracle as PA  # noqa: E402
from config_cases import SPLIT_CFG as CFG  # noqa: E402
from trainer_cases import five_steps, page_set, seeded  # noqa: E402

FWD, BWD = "cova_page_attn_fwd", "cova_page_attn_bwd"
FWDG, BWDG, WSQ = "cova_page_attn_fwd_geo", "cova_page_attn_bwd_geo", "cova_page_attn_geo_workspace_floats"
KEY, GEO_KEY = "page_attention.qkv.weight", "page_attention.geometry.weight"
W, H = PG.PAGE_W, PG.PAGE_H


# ---------------------------------------------------------------- 1. the kernels through the C ABI
#        page sizes                E   Hh  pad   (pad: extra floats per row of out / g / dqkv; odd = unaligned rows = scalar stores)
SHAPES = {"one": ((1,), 4, 1, 0),                          # a single row, dh 4
          "ragged": ((37, 0, 1, 5, 0), 8, 2, 3),           # empty pages; unaligned out / g / dqkv rows
          "tiles": ((16, 17, 15, 64, 65), 32, 2, 4),       # either side of a 16-row sub-tile and a 64-row tile; 65 rows = two
                                                           # own tiles: two partial blocks per head in the fold
          "clip": ((70, 2), 80, 4, 4),                     # dh 20; DOM offsets beyond +-64; four heads, different weights
          "d64": ((70, 3), 128, 2, 0),                     # the other three instantiations
          "d96": ((70, 3), 192, 2, 4),
          "d128": ((70, 3), 256, 2, 8)}                    # KT = 32: three tiles


def build_case(name, sizes, E, heads, pad, seed):
    rs = np.random.RandomState(seed)
    N = int(sum(sizes))
    return dict(name=name, sizes=tuple(sizes), N=N, B=len(sizes), E=E, heads=heads, pad=pad, ps=starts(sizes),
                qkv=rs.standard_normal((N, 3 * E)).astype(np.float32), g=rs.standard_normal((N, E)).astype(np.float32),
                w=(2.0 * rs.standard_normal((heads, 8))).astype(np.float32), boxes=PG.planted_boxes(sizes, seed + 1))


@functools.lru_cache(maxsize=None)
def geo_case(name):
    sizes, E, heads, pad = SHAPES[name]
    case = build_case(name, sizes, E, heads, pad, sum(map(ord, name)))
    case["ref"] = oracle64(case)
    return case


def oracle64(case, w=None):
    f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    qkv = f64(case["qkv"]).requires_grad_(True)
    wl = f64(case["w"] if w is None else w).requires_grad_(True)
    phi = PG.page_features(case["boxes"], case["ps"], W, H)
    out, A, lse = PG.attend(qkv, case["ps"], case["heads"], wl, phi)
    (out * f64(case["g"])).sum().backward()
    return dict(out=out.detach().numpy(), lse=lse.detach().numpy(), dqkv=qkv.grad.numpy(), dw=wl.grad.numpy(),
                A={k: v.detach().numpy() for k, v in A.items()}, phi=phi)


def host_probabilities(case, lse, phi, w=None):
    """A recomputed from the kernel's lse, the f32 qkv and weights and the oracle's features (float64 scores):
    exp(s_ij - lse_i) per page and head."""
    E, heads, ps = case["E"], case["heads"], case["ps"]
    dh = E // heads
    qkv, w = case["qkv"].astype(np.float64), (case["w"] if w is None else w).astype(np.float64)
    A = {}
    for p, n in enumerate(case["sizes"]):
        lo, hi = ps[p], ps[p + 1]
        for a in range(heads if n else 0):
            s = qkv[lo:hi, a * dh:(a + 1) * dh] @ qkv[lo:hi, E + a * dh:E + (a + 1) * dh].T / np.sqrt(dh)
            s = s + phi[p].astype(np.float64) @ w[a]
            A[(p, a)] = np.exp(s - lse[lo:hi, a:a + 1].astype(np.float64))
    return A


def launch(case, w=None, plain=False):
    """cova_page_attn_fwd_geo + cova_page_attn_bwd_geo (``plain``: the pair without the bias) on framed buffers -> dict
    of host arrays (guards checked: every output and the workspace)."""
    N, B, E, heads, pad = case["N"], case["B"], case["E"], case["heads"], case["pad"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    qkv, g, ps = dev(case["qkv"]), padded(case["g"], E + pad), dev(case["ps"])
    boxes, wd = dev(case["boxes"]), dev(case["w"] if w is None else w)
    out_b, out = framed(N, E, E + pad)
    lse_b, lse = framed(N, heads, heads)
    d_b, d = framed(N, 3 * E, 3 * E + pad)
    if plain:
        engine.call(FWD, qkv, 3 * E, ps, B, N, E, heads, out, E + pad, lse)
        engine.call(BWD, g, E + pad, qkv, 3 * E, out, E + pad, lse, ps, B, N, E, heads, d, 3 * E + pad)
        torch.cuda.synchronize()
        return dict(out=survived(out_b, N, E), lse=survived(lse_b, N, heads), dqkv=survived(d_b, N, 3 * E))
    nws = engine.query(WSQ, B, N, heads)
    blocks = B * heads * ((N + 63) // 64)
    assert nws == 8 * blocks
    ws_b, ws = framed(blocks, 8, 8)
    dw_b, dw = framed(heads, 8, 8)
    engine.call(FWDG, qkv, 3 * E, ps, boxes, wd, float(W), float(H), B, N, E, heads, out, E + pad, lse)
    engine.call(BWDG, g, E + pad, qkv, 3 * E, out, E + pad, lse, ps, boxes, wd, float(W), float(H), B, N, E, heads, d,
                3 * E + pad, dw, ws)
    torch.cuda.synchronize()
    assert torch.equal(qkv.cpu(), torch.from_numpy(case["qkv"])) and torch.equal(boxes.cpu(), torch.from_numpy(case["boxes"]))
    return dict(out=survived(out_b, N, E), lse=survived(lse_b, N, heads), dqkv=survived(d_b, N, 3 * E),
                dw=survived(dw_b, heads, 8), ws=survived(ws_b, blocks, 8))


def errors(got, ref, case, w=None):
    errs = {k: relerr(got[k], ref[k]) for k in ("out", "lse", "dqkv", "dw")}
    A = host_probabilities(case, got["lse"], ref["phi"], w)
    errs["A"] = max(relerr(A[k], ref["A"][k]) for k in A)
    return errs


def check_against(got, ref, case, what, w=None):
    errs = errors(got, ref, case, w)
    print(what, {k: "%.2e" % v for k, v in errs.items()})
    for k, e in errs.items():
        assert e < (1e-4 if k in ("dqkv", "dw") else 1e-5), (what, k, e)


@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_and_backward_match_the_float64_oracle(name):
    case = geo_case(name)
    got, ref = launch(case), case["ref"]
    check_against(got, ref, case, name)
    # the weights matter: against the plain oracle A moves by more than the bound's hundredfold
    _, A0, _ = PA.attend(torch.from_numpy(case["qkv"].astype(np.float64)), case["ps"], case["heads"])
    if max(case["sizes"]) > 1:
        assert max(float(np.abs(ref["A"][k] - A0[k].numpy()).max()) for k in A0) > 1e-3
        assert float(np.abs(ref["dw"]).max()) > 0
    # the workspace: the fold's terms are the blocks' sums, a block behind its page's end holds zeros
    N, B, heads = case["N"], case["B"], case["heads"]
    tiles = (N + 63) // 64
    ws = got["ws"].reshape(B, heads, tiles, 8)
    for p, n in enumerate(case["sizes"]):
        assert not ws[p, :, (n + 63) // 64:].any()
    assert relerr(ws.astype(np.float64).sum(axis=(0, 2)), ref["dw"]) < 1e-4
    ps, E = case["ps"], case["E"]
    for p, n in enumerate(case["sizes"]):
        if n == 1:                                   # one box: O = V exactly, dV = g, no gradient to Q or K
            i = ps[p]
            assert np.array_equal(got["out"][i], case["qkv"][i, 2 * E:])
            assert not got["dqkv"][i, :2 * E].any()
            assert relerr(got["dqkv"][i, 2 * E:], case["g"][i]) < 1e-6


@pytest.mark.parametrize("name", ["ragged", "tiles", "clip", "d128"])
def test_zero_weights_give_the_plain_entry_points_bits(name):
    case = geo_case(name)
    zero = np.zeros_like(case["w"])
    got, plain = launch(case, w=zero), launch(case, plain=True)
    for k in ("out", "lse", "dqkv"):
        assert bits_equal(got[k], plain[k]), k
    ref = oracle64(case, w=zero)
    assert float(np.abs(ref["dw"]).max()) > 0 and got["dw"].any()          # the gradient of a zero weight is not zero
    check_against(got, ref, case, name + " (w = 0)", w=zero)


@pytest.mark.parametrize("name", ["ragged", "tiles", "clip", "d128"])
def test_reruns_are_bit_identical(name):
    case = geo_case(name)
    a, b = launch(case), launch(case)
    for k in a:
        assert bits_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", ["ragged", "tiles", "clip"])
def test_a_page_keeps_its_bits_inside_a_larger_batch(name):
    """The first page alone, and again with three pages in front of it and three behind: O, lse and dqkv of its rows have
    the same bits (d_geo_w is a sum over all pages and is left out)."""
    full = geo_case(name)
    n, E, heads = full["sizes"][0], full["E"], full["heads"]
    small = build_case(name + "[0]", (n,), E, heads, full["pad"], 1)
    before, after = (4, 0, 70), (2, 13, 1)
    nb = sum(before)
    big = build_case(name + "+6", before + (n,) + after, E, heads, full["pad"], 5)
    for k in ("qkv", "g", "boxes"):
        small[k] = full[k][:n].copy()
        big[k][nb:nb + n] = small[k]
    small["w"] = big["w"] = full["w"]
    a, b = launch(small), launch(big)
    for k in ("out", "lse", "dqkv"):
        assert bits_equal(a[k], b[k][nb:nb + n]), k
    check_against(b, oracle64(big), big, name + " inside a larger batch")


def test_entry_points_refuse_bad_arguments_and_skip_empty_work():
    N, B, E, Hh = 8, 2, 16, 2
    full = lambda *shape: torch.full(shape, GUARD, device=DEV)
    ps = torch.tensor([0, 5, 8], dtype=torch.int64, device=DEV)
    qkv, g = torch.randn(N + 1, 3 * E, device=DEV), torch.randn(N, E, device=DEV)
    boxes = torch.from_numpy(PG.planted_boxes((5, 3), 2)).to(DEV)
    w = torch.randn(Hh, 8, device=DEV)
    out, lse, d, dw = full(N, E), full(N, Hh), full(N, 3 * E), full(Hh, 8)
    assert engine.query(WSQ, B, N, Hh) == 8 * B * Hh and engine.query(WSQ, B, 65, Hh) == 8 * B * Hh * 2
    assert [engine.query(WSQ, *a) for a in ((0, N, Hh), (B, 0, Hh), (B, N, 0), (-1, N, Hh), (1 << 20, 1 << 20, 64))] == [0] * 5
    ws = full(engine.query(WSQ, B, N, Hh))
    good_f = [qkv, 3 * E, ps, boxes, w, 96.0, 64.0, B, N, E, Hh, out, E, lse]
    good_b = [g, E, qkv, 3 * E, out, E, lse, ps, boxes, w, 96.0, 64.0, B, N, E, Hh, d, 3 * E, dw, ws]
    off = qkv.view(-1)[1:]                                    # 4 bytes past a 16-byte boundary; N rows still fit

    def bad(args, **changes):
        a = list(args)
        for i, v in changes.items():
            a[int(i[1:])] = v
        return a
    for ch in (dict(_10=3), dict(_10=0), dict(_10=-2), dict(_9=24, _10=4), dict(_9=8, _10=4), dict(_9=516, _10=6),
               dict(_9=0), dict(_9=-16), dict(_9=512, _10=2),                 # the plain pair's shape refusals
               dict(_0=off), dict(_1=3 * E + 2), dict(_1=3 * E - 4), dict(_12=E - 1), dict(_8=-1), dict(_7=-1),
               dict(_0=None), dict(_2=None), dict(_11=None), dict(_13=None),
               dict(_3=None), dict(_4=None),                                  # and the new operands
               dict(_5=0.0), dict(_5=-96.0), dict(_6=0.0), dict(_6=-1.0), dict(_5=float("nan"))):
        with pytest.raises(_lib.CovaHipError, match="10001"):
            engine.call(FWDG, *bad(good_f, **ch))
    for ch in (dict(_15=3), dict(_15=0), dict(_14=24, _15=4), dict(_14=516, _15=6), dict(_14=512, _15=2), dict(_14=0),
               dict(_2=off), dict(_3=3 * E + 2), dict(_3=3 * E - 4), dict(_1=E - 1), dict(_5=E - 1), dict(_17=3 * E - 1),
               dict(_13=-1), dict(_12=-1),
               dict(_0=None), dict(_2=None), dict(_4=None), dict(_6=None), dict(_7=None), dict(_16=None),
               dict(_8=None), dict(_9=None), dict(_18=None), dict(_19=None),
               dict(_10=0.0), dict(_10=-96.0), dict(_11=0.0), dict(_11=-1.0)):
        with pytest.raises(_lib.CovaHipError, match="10001"):
            engine.call(BWDG, *bad(good_b, **ch))
    # N == 0 or B == 0: nothing is launched, no pointer is needed
    for n, b in ((0, B), (N, 0), (0, 0)):
        engine.call(FWDG, None, 3 * E, None, None, None, 96.0, 64.0, b, n, E, Hh, None, E, None)
        engine.call(BWDG, None, E, None, 3 * E, None, E, None, None, None, None, 96.0, 64.0, b, n, E, Hh, None, 3 * E, None,
                    None)
        engine.call(FWDG, *bad(good_f, _7=b, _8=n))
        engine.call(BWDG, *bad(good_b, _12=b, _13=n))
    torch.cuda.synchronize()
    for t in (out, lse, d, dw, ws):
        assert (t == GUARD).all()
    engine.call(FWDG, *good_f)                                  # and the good calls are good
    engine.call(BWDG, *good_b)
    torch.cuda.synchronize()
    for t in (out, lse, d, dw, ws):
        assert bool(torch.isfinite(t).all()) and (t != GUARD).all()


# ---------------------------------------------------------------- 2. the module
def test_page_attention_with_geometry_under_autograd_matches_the_oracle():
    rs = np.random.RandomState(13)
    sizes, Fd, E, Hh = (40, 0, 61, 30), 24, 8, 2
    N, ps = sum(sizes), starts(sizes)
    torch.manual_seed(11)
    layer = PageAttention(Fd, E, Hh, geometry=True)
    assert not layer.geometry.weight.detach().any()
    with torch.no_grad():
        layer.geometry.weight.copy_(torch.from_numpy((2.0 * rs.standard_normal((Hh, 8))).astype(np.float32)))
    sd = {"page_attention." + k: v.detach().clone().double().requires_grad_(True) for k, v in layer.state_dict().items()}
    assert list(sd) == [KEY, GEO_KEY] and sd[GEO_KEY].shape == (Hh, 8)
    h_host = torch.from_numpy(rs.standard_normal((N, Fd)).astype(np.float32))
    g_host = torch.from_numpy(rs.standard_normal((N, E)).astype(np.float32))
    boxes = PG.planted_boxes(sizes, 3)
    phi = PG.page_features(boxes, ps, W, H)
    layer = layer.to(DEV)
    h = h_host.to(DEV).requires_grad_(True)
    bx, psd = torch.from_numpy(boxes).to(DEV), torch.from_numpy(ps).to(DEV)
    out, lse = layer(h, psd, bx, (H, W), return_lse=True)
    assert out.shape == (N, E) and lse.shape == (N, Hh) and not lse.requires_grad
    (out * g_host.to(DEV)).sum().backward()
    h_ref = h_host.double().requires_grad_(True)
    out_ref, _, lse_ref, _ = PG.page_attention(h_ref, sd, ps, Hh, phi, return_all=True)
    (out_ref * g_host.double()).sum().backward()
    assert relerr(out.detach().cpu(), out_ref.detach()) < 1e-5
    assert relerr(lse.cpu(), lse_ref.detach()) < 1e-5
    assert relerr(h.grad.cpu(), h_ref.grad) < 1e-4
    assert relerr(layer.qkv.weight.grad.cpu(), sd[KEY].grad) < 1e-4
    assert float(sd[GEO_KEY].grad.abs().max()) > 0
    assert relerr(layer.geometry.weight.grad.cpu(), sd[GEO_KEY].grad) < 1e-4
    plain_ref = PA.page_attention(h_host.double(), sd, ps, Hh).detach()
    assert relerr(plain_ref, out_ref.detach()) > 1e-3                       # the bias is live
    with pytest.raises(ValueError, match="bboxes"):
        layer(h.detach(), psd)
    with pytest.raises(ValueError, match="bboxes"):
        layer(h.detach(), psd, bx)
    with pytest.raises(ValueError, match="page_size"):
        layer(h.detach(), psd, bx, (0, W))
    assert layer(h.detach()[:0], torch.zeros(1, dtype=torch.int64, device=DEV), bx[:0], (H, W)).shape == (0, E)


# ---------------------------------------------------------------- 3. the whole model
@pytest.mark.parametrize("context", [True, False])
def test_model_with_the_geometry_bias_matches_the_oracle_on_the_reference_inputs(monkeypatch, context):
    """The cova_h64_n11 inputs as tests/test_page_attention_gpu.py uses them: the one page given twice, the last five
    boxes moved to the copy.  The geometry weights are seeded and non-zero."""
    fx, cfg, _, b = load_case("cova_h64_n11")
    b = dict(b, images=b["images"].repeat(2, 1, 1, 1).contiguous(), bboxes=b["bboxes"].clone())
    b["bboxes"][6:, 0] = 1.0
    E, Hh = 8, 2
    cfg = dict(cfg, use_context=context, page_attention_dim=E, page_attention_heads=Hh, page_attention_geometry=True)
    ocfg = {k: v for k, v in dict(cfg, use_context=True).items() if not k.startswith("page_attention")}
    wcfg = {k: v for k, v in cfg.items() if k != "drop_prob"}
    seed, gain = int(fx["meta/seed"]), float(fx["meta/logit_gain"])
    sd = weights.seeded_state_dict(seed, logit_gain=gain, **wcfg)
    assert list(sd).index(GEO_KEY) == list(sd).index(KEY) + 1 and not sd[GEO_KEY].any()
    zero_sd = {k: v.clone() for k, v in sd.items()}
    sd[GEO_KEY] = torch.from_numpy((2.0 * np.random.RandomState(seed + 1).standard_normal((Hh, 8))).astype(np.float32))
    img_h, page_size = int(fx["meta/img_h"]), tuple(b["images"].shape[2:])
    ps = torch.searchsorted(b["bboxes"][:, 0].contiguous(), torch.arange(3, dtype=torch.float32))
    assert ps.tolist() == [0, 6, 11]
    inputs = (b["images"], b["bboxes"], b["additional_feats"], b["context_indices"])
    monkeypatch.setattr(O, "gat_stack", PG.patched_gat_stack(ps, Hh, b["bboxes"], page_size))
    zero_ref = O.forward(O.clone_state_dict(zero_sd), *inputs, ocfg, False)
    args = [t.to(DEV) for t in inputs]

    def build():
        m = CoVA(cfg["roi_output_size"], img_h, cfg["n_classes"], context, cfg["hidden_dim"], cfg["bbox_hidden_dim"],
                 cfg["n_additional_feat"], cfg["drop_prob"], None, page_attention_dim=E, page_attention_heads=Hh,
                 page_attention_geometry=True)
        assert [k for k in m.state_dict()] == list(sd)
        missing = m.load_state_dict(sd, strict=True)
        assert not missing.missing_keys and not missing.unexpected_keys
        return m.to(DEV)

    m = build().eval()
    with torch.no_grad():
        logits = m(*args)
    ref = O.forward(O.clone_state_dict(sd), *inputs, ocfg, False)
    assert relerr(logits.cpu(), ref) < LOGIT_TOL
    assert relerr(zero_ref, ref) > 1e-3                        # the bias is live
    m = build().train()
    logits = m(*args)
    sv = logits.grad_fn.sv
    assert "bboxes" in sv["page_attn"] and (sv["page_attn"]["img_h"], sv["page_attn"]["img_w"]) == page_size
    routing = routing_from_saved(sv)
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(logits, b["labels"].to(DEV))
    loss.backward()
    loss_ref, logits_ref, grads_ref, _, _ = O.loss_and_grads(sd, *inputs, b["labels"], ocfg, None, routing)
    assert relerr(logits.detach().cpu(), logits_ref) < LOGIT_TOL
    assert abs(loss.item() - float(loss_ref)) <= LOSS_TOL * abs(float(loss_ref))
    grads = {k: p.grad for k, p in m.named_parameters()}
    assert GEO_KEY in grads and GEO_KEY in grads_ref
    compare_grads(grads, grads_ref, rtol=GRAD_TOL, outlier_frac=0.0)
    for k in (KEY, GEO_KEY):                                   # (compare_grads floors the scale at 1 % of the largest gradient)
        assert float(grads_ref[k].abs().max()) > 0
        assert relerr(grads[k].cpu(), grads_ref[k]) < 1e-4, k


# ---------------------------------------------------------------- 4. the trainer
ACFG = dict(CFG, page_attention_dim=16, page_attention_heads=2)
GCFG = dict(ACFG, page_attention_geometry=True)


def test_five_steps_move_the_geometry_weight_off_zero_and_are_reproducible():
    u8, rows = page_set()
    ds = DeviceDataset(u8, rows, 2, DEV, spatial_k=6)
    sd = seeded(GCFG)
    assert sd[GEO_KEY].shape == (2, 8) and not sd[GEO_KEY].any()
    a, b = HotPathTrainer(GCFG, sd, DEV), HotPathTrainer(GCFG, sd, DEV)
    assert a.params[GEO_KEY].shape == (2, 8) and a.grads[GEO_KEY].shape == (2, 8)
    assert sum(v.numel() for v in a.params.values()) == sum(v.numel() for v in HotPathTrainer(ACFG, seeded(ACFG), DEV).params.values()) + 16
    la, sa = five_steps(a, ds)
    lb, sb = five_steps(b, ds)
    assert la == lb and list(sa) == list(sb)
    for key in sa:
        assert torch.equal(sa[key], sb[key]), key
    assert bool(torch.isfinite(sa[GEO_KEY]).all())
    assert bool((sa[GEO_KEY] != 0).all())                                       # every feature of every head has moved
    c = HotPathTrainer(GCFG, sd, DEV)                                           # checkpoint round trip, one more equal step
    c.load_state_dict(a.state_dict())
    c.load_optimizer_state_dict(a.optimizer_state_dict())
    batch = next(iter(ds.batches(3, prefetch=False)))
    assert float(a.train_step(batch)[0]) == float(c.train_step(batch)[0])
    assert torch.equal(a.pbucket.flat, c.pbucket.flat)
    with pytest.raises(ValueError, match="page_attention_geometry"):            # a checkpoint without the weight
        c.load_state_dict(seeded(ACFG))
    with pytest.raises(ValueError, match="page_attention_geometry"):            # and the reverse
        HotPathTrainer(ACFG, seeded(ACFG), DEV).load_state_dict(a.state_dict())


def test_a_fresh_frozen_geometry_weight_trains_like_the_plain_page_attention_bit_for_bit():
    u8, rows = page_set()
    ds = DeviceDataset(u8, rows, 2, DEV, spatial_k=6)
    g = HotPathTrainer(GCFG, seeded(GCFG), DEV, frozen=("page_attention.geometry.",))
    p = HotPathTrainer(ACFG, seeded(ACFG), DEV)
    lg, sg = five_steps(g, ds)
    lp, sp = five_steps(p, ds)
    assert lg == lp and [k for k in sg if k != GEO_KEY] == list(sp)
    for key in sp:
        assert torch.equal(sg[key], sp[key]), key
    assert not sg[GEO_KEY].any()


def test_only_the_option_issues_the_new_launches():
    u8, rows = page_set(P=3)
    batch = next(iter(DeviceDataset(u8, rows, 2, DEV, spatial_k=6).batches(3, prefetch=False)))
    _, plain = profiled(lambda: HotPathTrainer(CFG, seeded(CFG), DEV).train_step(batch))
    _, pa = profiled(lambda: HotPathTrainer(ACFG, seeded(ACFG), DEV).train_step(batch))
    off = dict(ACFG, page_attention_geometry=False)
    _, pa_off = profiled(lambda: HotPathTrainer(off, seeded(ACFG), DEV).train_step(batch))
    assert not any(n in plain for n in (FWDG, BWDG)) and not any(n in pa for n in (FWDG, BWDG)) and pa_off == pa
    assert pa[FWD] == 1 and pa[BWD] == 1
    _, geo = profiled(lambda: HotPathTrainer(GCFG, seeded(GCFG), DEV).train_step(batch))
    assert geo[FWDG] == 1 and geo[BWDG] == 1 and FWD not in geo and BWD not in geo
    swap = lambda d: {{FWDG: FWD, BWDG: BWD}.get(k, k): v for k, v in d.items()}
    assert swap(geo) == pa                                                         # the same step otherwise


def test_evaluate_split_cached_predict_split_and_fit_with_the_option_on():
    u8, rows = page_set(P=9, seed=4)
    v8, vrows = page_set(P=11, seed=9)
    train, val = DeviceDataset(u8, rows, 2, DEV, spatial_k=6), DeviceDataset(v8, vrows, 2, DEV, spatial_k=6)
    sd = seeded(GCFG)
    sd[GEO_KEY] = torch.from_numpy(np.random.RandomState(8).standard_normal((2, 8)).astype(np.float32))
    tr = HotPathTrainer(GCFG, sd, DEV, track_metrics=True, frozen=("convnet.",), bn_eval=("convnet.",))
    rep = evaluate_split(tr, val, with_loss=True)
    assert rep.evaluated.all() and rep.ranks.shape == (11, 3) and np.isfinite(rep.loss)
    tcache, vcache = FeatureCache.build(tr, train), FeatureCache.build(tr, val)
    cached, full = next(iter(val.batches(11, features=vcache))), next(iter(val.batches(11, prefetch=False)))
    assert cached.get("images") is None and cached.get("page_size") is not None
    assert torch.equal(tr.predict(cached)[0], tr.predict(full)[0])
    plain = HotPathTrainer(ACFG, {k: v for k, v in sd.items() if k != GEO_KEY}, DEV)
    assert not torch.equal(tr.predict(full)[0], plain.predict(full)[0])            # the bias is live
    stripped = {k: v for k, v in cached.items() if k not in ("images", "page_size")}
    with pytest.raises(ValueError, match="page_attention_geometry.*page_size"):
        tr.predict(stripped)
    rep_c = evaluate_split(tr, val, with_loss=True, features=vcache)
    assert np.array_equal(rep_c.ranks, rep.ranks)
    boxes, _ = predict_split(tr, val)
    assert tuple(boxes.shape) == (11, 3) and int(boxes.min()) >= 0
    before = tr.params[GEO_KEY].clone()
    loss = float(tr.train_step(next(iter(train.batches(3, features=tcache))))[0])       # a FeatureCache-fed step
    assert np.isfinite(loss) and not torch.equal(tr.params[GEO_KEY], before)
    out = fit(tr, train, val, 2, 3, sampling_fraction=0.9, seed=12, eval_interval=1, train_features=tcache,
              val_features=vcache)
    assert len(out.history) == 2 and out.history[-1]["eval_acc"] is not None
