"""GPU tests of the page readout (CoVA(page_context_dim=G)): cova_page_readout_fwd / cova_page_readout_bwd through the C
ABI against the float64 torch oracle (tests/readout_oracle.py: autograd, no code shared with the hand-written backward),
refusals and empty work, models.PageReadout and the whole model under autograd, and HotPathTrainer with the option on.

Bounds: the project's own for this layer (tests/test_gatv2_gpu.py, tests/test_edge_gpu.py): max-abs error over max-abs
reference below 1e-5 for out, r and beta, below 1e-4 for dP and d_att_w; d_att_b = sum du is a sum of terms that cancel
within a page up to the LeakyReLU slopes (every page's de sums to zero) and is held on the larger of its own and d_att_w's
scale.  The kernel tests feed P: the float64 oracle sees the same f32 values.  The whole model on the cova_h64_n11 inputs
keeps tests/test_model_gpu.py's LOGIT_TOL / LOSS_TOL / GRAD_TOL."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import _lib, engine, weights  # noqa: E402
from cova_web_object_detection_amd.evaluation import evaluate_split, fit  # noqa: E402
from cova_web_object_detection_amd.features import FeatureCache  # noqa: E402
from cova_web_object_detection_amd.models import CoVA, PageReadout  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
from helpers import (bits_equal, compare_grads, DEV, framed, GRAD_TOL, GUARD, load_case, LOGIT_TOL,  # noqa: E402
                     LOSS_TOL, NAN, padded, profiled, relerr, routing_from_saved, SGEMM_TOL, starts, survived)
from oracle import cova_oracle as O  # noqa: E402
import gatv2_oracle as G2  # noqa: E402
import readout_oracle as RO  # noqa: E402
from config_cases import SPLIT_CFG as CFG  # noqa: E402
from gat_cases import device_gates  # noqa: E402
from trainer_cases import five_steps, n_params, page_set, seeded  # noqa: E402

FWD, BWD, WSQ = "cova_page_readout_fwd", "cova_page_readout_bwd", "cova_page_readout_workspace_floats"
KEYS = ["page_readout.W.weight", "page_readout.attention_layer.weight", "page_readout.attention_layer.bias"]
AW = KEYS[1]


# ---------------------------------------------------------------- 1. the kernels through the C ABI
#        page sizes           G  pad   (pad: extra floats per row of P / out / g / dP; odd = unaligned rows = the scalar form)
SHAPES = {"one": ((1,), 6, 0),                        # one box; fewer channels than lanes
          "scalar": ((37, 0, 1, 5, 0), 6, 3),         # G % 4 != 0; empty pages in the middle and at the end
          "vec4": ((90, 11), 64, 4),                  # the float4 form
          "unaligned": ((90, 11), 64, 1),             # G % 4 == 0 but odd leading dimensions: the scalar form at 64 channels
          "wide": ((300, 2, 130), 384, 8),            # more rows than a block has threads; the second float4 chunk part-filled
          "long": ((1100, 3), 128, 4),                # a page longer than any per-block staging
          "limit": ((70,), 512, 0)}                   # the channel limit


def build_case(name, sizes, G, pad, seed):
    rs = np.random.RandomState(seed)
    N = int(sum(sizes))
    return dict(name=name, sizes=tuple(sizes), N=N, B=len(sizes), G=G, pad=pad, ps=starts(sizes),
                P=rs.standard_normal((N, G)).astype(np.float32),
                aw=(rs.standard_normal(G) / np.sqrt(G)).astype(np.float32), ab=rs.standard_normal(1).astype(np.float32),
                g=rs.standard_normal((N, G)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def ro_case(name):
    sizes, G, pad = SHAPES[name]
    case = build_case(name, sizes, G, pad, sum(map(ord, name)))
    case["ref"] = oracle64(case)
    return case


def oracle64(case, gate=None):
    f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    P, aw, ab = (f64(case[k]).requires_grad_(True) for k in ("P", "aw", "ab"))
    rows, beta, r, u = RO.pool(P, aw, ab, case["ps"], 0.2, gate)
    (rows * f64(case["g"])).sum().backward()
    return dict(out=rows.detach().numpy(), beta=beta.detach().numpy(), r=r.detach().numpy(), u=u.detach().numpy(),
                dP=P.grad.numpy(), daw=aw.grad.numpy(), dab=ab.grad.numpy())


def launch(case):
    """cova_page_readout_fwd + cova_page_readout_bwd on framed buffers -> dict of host arrays (guards checked)."""
    N, B, G, pad = case["N"], case["B"], case["G"], case["pad"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    P, g = padded(case["P"], G + pad), padded(case["g"], G + pad)
    aw, ab, ps = dev(case["aw"]), dev(case["ab"]), dev(case["ps"])
    u_b, u = framed(N, 1, 1)
    beta_b, beta = framed(N, 1, 1)
    r_b, r = framed(B, G, G)
    out_b, out = framed(N, G, G + pad)
    dP_b, dP = framed(N, G, G + pad)
    daw_b, daw = framed(1, G, G)
    dab_b, dab = framed(1, 1, 1)
    nws = engine.query(WSQ, B, G)
    assert nws == B * (G + 1)
    ws = torch.full((nws + 16,), NAN, device=DEV)
    ws[nws:] = GUARD
    engine.call(FWD, P, G + pad, aw, ab, ps, B, N, G, 0.2, u, beta, r, out, G + pad)
    engine.call(BWD, g, G + pad, P, G + pad, u, beta, r, aw, ps, B, N, G, 0.2, dP, G + pad, daw, dab, ws)
    torch.cuda.synchronize()
    assert (ws[nws:] == GUARD).all() and bool(torch.isfinite(ws[:nws]).all())
    empty = [p for p, n in enumerate(case["sizes"]) if n == 0]
    return dict(u=survived(u_b, N, 1).reshape(-1), beta=survived(beta_b, N, 1).reshape(-1),
                r=survived(r_b, B, G, unwritten=empty), out=survived(out_b, N, G), dP=survived(dP_b, N, G),
                daw=survived(daw_b, 1, G).reshape(-1), dab=survived(dab_b, 1, 1).reshape(-1))


def errors(got, ref, case):
    live = [p for p, n in enumerate(case["sizes"]) if n > 0]
    errs = {k: relerr(got[k], ref[k]) for k in ("out", "beta", "dP", "daw")}
    errs["r"] = relerr(got["r"][live], ref["r"][live])
    errs["dab"] = relerr(got["dab"], ref["dab"], scale=max(np.abs(ref["daw"]).max(), np.abs(ref["dab"]).max()))
    return errs


def check_against(got, ref, case, what):
    errs = errors(got, ref, case)
    print(what, {k: "%.2e" % v for k, v in errs.items()})
    for k, e in errs.items():
        assert e < (1e-5 if k in ("out", "r", "beta") else 1e-4), (what, k, e)


@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_and_backward_match_the_float64_oracle(name):
    case = ro_case(name)
    got, ref = launch(case), case["ref"]
    check_against(got, ref, case, name)
    assert relerr(got["u"], ref["u"]) < 1e-5
    ps = case["ps"]
    for p, n in enumerate(case["sizes"]):
        if n == 0:
            continue
        rows = got["out"][ps[p]:ps[p + 1]]
        assert bits_equal(rows, np.broadcast_to(got["r"][p], rows.shape))          # every box gets its page's vector
        assert abs(float(got["beta"][ps[p]:ps[p + 1]].astype(np.float64).sum()) - 1.0) < 1e-5
        if n == 1:                                                                # one box: beta = 1, r = P_i, dP = g
            i = ps[p]
            assert got["beta"][i] == 1.0 and np.array_equal(got["r"][p], case["P"][i])
            assert relerr(got["dP"][i], case["g"][i]) < 1e-6
    assert float(np.abs(ref["daw"]).max()) > 0 or case["N"] == 1


def planted_zero_case(name):
    """Rows A and B of a page get u = +0.0 and u = -0.0 exactly: b = -0.0, P[A] = +0 everywhere (a has a positive entry: the
    products hold a +0), P[B, c] = -0 where a[c] > 0 and +0 where a[c] < 0 (every product is -0)."""
    base = ro_case(name)
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items() if k != "ref"}
    p = max(i for i, n in enumerate(case["sizes"]) if n >= 2)
    A, Bz = int(case["ps"][p]), int(case["ps"][p]) + 1
    assert (case["aw"] > 0).any() and (case["aw"] != 0).all()
    case["ab"] = np.asarray([-0.0], np.float32)
    case["P"][A] = 0.0
    case["P"][Bz] = np.where(case["aw"] > 0, np.float32(-0.0), np.float32(0.0))
    return case, A, Bz


@pytest.mark.parametrize("name", ["scalar", "vec4", "unaligned", "wide"])
def test_signed_zero_scores_take_the_slope_branch(name):
    case, A, Bz = planted_zero_case(name)
    got = launch(case)
    assert got["u"][A] == 0 and not np.signbit(got["u"][A])
    assert got["u"][Bz] == 0 and np.signbit(got["u"][Bz])
    ref = oracle64(case)                                                          # u > 0: both rows on the alpha branch
    assert not ref["u"][[A, Bz]].any()
    wrong = oracle64(case, gate=torch.from_numpy(ref["u"] >= 0))
    check_against(got, ref, case, name + " (+-0)")
    scale = np.abs(ref["dP"]).max()
    for i in (A, Bz):
        assert np.abs(got["dP"][i] - ref["dP"][i]).max() < 1e-4 * scale
        assert np.abs(wrong["dP"][i] - ref["dP"][i]).max() > 1e-3 * scale
    assert relerr(got["beta"], wrong["beta"]) < 1e-5                              # (the value is the same on either branch)


@pytest.mark.parametrize("name", ["scalar", "vec4", "long"])
def test_scores_spread_by_two_hundred_stay_finite(name):
    """a is scaled until the scores of a page span +-200, and one row of each page is scaled to a score of 250: exp() of
    the shifted scores underflows for most rows, beta stays finite, sums to 1 and sits on the largest row."""
    base = ro_case(name)
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items() if k != "ref"}
    case["ab"] = np.zeros(1, np.float32)
    u0 = case["P"].astype(np.float64) @ case["aw"].astype(np.float64)
    case["aw"] = (case["aw"] * (200.0 / np.abs(u0).max())).astype(np.float32)
    u0 = case["P"].astype(np.float64) @ case["aw"].astype(np.float64)
    tops = []
    for p, n in enumerate(case["sizes"]):
        if n >= 2:
            t = int(case["ps"][p]) + int(np.argmax(np.abs(u0[case["ps"][p]:case["ps"][p + 1]])))
            case["P"][t] *= np.float32(250.0 / u0[t])
            tops.append((p, t))
    got = launch(case)
    assert abs(float(got["u"].max()) - 250.0) < 0.01 and float(got["u"].min()) < -100.0
    for k in ("beta", "out", "dP", "daw", "dab"):
        assert np.isfinite(got[k]).all(), k
    for p, t in tops:
        lo, hi = case["ps"][p], case["ps"][p + 1]
        assert abs(float(got["beta"][lo:hi].astype(np.float64).sum()) - 1.0) < 1e-5
        assert got["beta"][t] > 1.0 - 1e-5 and int(np.argmax(got["beta"][lo:hi])) == t - lo
        assert relerr(got["r"][p], case["P"][t]) < 1e-5


@pytest.mark.parametrize("name", ["scalar", "vec4", "wide", "long"])
def test_reruns_are_bit_identical(name):
    case = ro_case(name)
    a, b = launch(case), launch(case)
    live = [p for p, n in enumerate(case["sizes"]) if n > 0]
    for k in a:
        x, y = (a[k][live], b[k][live]) if k == "r" else (a[k], b[k])
        assert bits_equal(x, y), k


@pytest.mark.parametrize("name", ["scalar", "vec4", "unaligned"])
def test_a_page_keeps_its_bits_inside_a_larger_batch(name):
    """The same pages with three more pages in front of them and three behind: u, beta, r, out and dP of their rows have
    the same bits.  d_att_w and d_att_b are sums over all pages and are left out."""
    small = ro_case(name)
    before, after = (4, 0, 9), (2, 13, 1)
    rs = np.random.RandomState(3)
    nb, na, G = sum(before), sum(after), small["G"]
    big = build_case(name + "+6", before + small["sizes"] + after, G, small["pad"], 5)
    big["aw"], big["ab"] = small["aw"], small["ab"]
    for k in ("P", "g"):
        big[k] = np.concatenate([rs.standard_normal((nb, G)).astype(np.float32), small[k],
                                 rs.standard_normal((na, G)).astype(np.float32)])
    a, b = launch(small), launch(big)
    N = small["N"]
    for k in ("u", "beta", "out", "dP"):
        assert bits_equal(a[k], b[k][nb:nb + N]), k
    live = [p for p, n in enumerate(small["sizes"]) if n > 0]
    assert bits_equal(a["r"][live], b["r"][[len(before) + p for p in live]])
    check_against(b, oracle64(big), big, name + " inside a larger batch")


def test_entry_points_refuse_bad_arguments_and_skip_empty_work():
    N, B, G = 8, 2, 16
    z = lambda *shape: torch.zeros(shape, device=DEV)
    full = lambda *shape: torch.full(shape, GUARD, device=DEV)
    ps = torch.tensor([0, 5, 8], dtype=torch.int64, device=DEV)
    P, aw, ab, g = torch.randn(N, G, device=DEV), torch.randn(G, device=DEV), z(1), torch.randn(N, G, device=DEV)
    u, beta, r, out = full(N), full(N), full(B, G), full(N, G)
    dP, daw, dab, ws = full(N, G), full(G), full(1), z(engine.query(WSQ, B, G))
    good_f = [P, G, aw, ab, ps, B, N, G, 0.2, u, beta, r, out, G]
    good_b = [g, G, P, G, u, beta, r, aw, ps, B, N, G, 0.2, dP, G, daw, dab, ws]

    def bad(args, **changes):
        a = list(args)
        for i, v in changes.items():
            a[int(i[1:])] = v
        return a
    for ch in (dict(_7=0), dict(_7=513), dict(_7=-4), dict(_6=-1), dict(_5=-1), dict(_1=G - 1), dict(_13=G - 1),
               dict(_0=None), dict(_2=None), dict(_3=None), dict(_4=None), dict(_9=None), dict(_10=None), dict(_11=None),
               dict(_12=None)):
        with pytest.raises(_lib.CovaHipError):
            engine.call(FWD, *bad(good_f, **ch))
    for ch in (dict(_11=0), dict(_11=513), dict(_10=-1), dict(_9=-1), dict(_1=G - 1), dict(_3=G - 1), dict(_14=G - 1),
               dict(_0=None), dict(_2=None), dict(_4=None), dict(_5=None), dict(_6=None), dict(_7=None), dict(_8=None),
               dict(_13=None), dict(_15=None), dict(_16=None), dict(_17=None)):
        with pytest.raises(_lib.CovaHipError):
            engine.call(BWD, *bad(good_b, **ch))
    # N == 0 or B == 0: nothing is launched, no pointer is needed
    for n, b in ((0, B), (N, 0), (0, 0)):
        engine.call(FWD, None, G, None, None, None, b, n, G, 0.2, None, None, None, None, G)
        engine.call(BWD, None, G, None, G, None, None, None, None, None, b, n, G, 0.2, None, G, None, None, None)
        engine.call(FWD, *bad(good_f, _5=b, _6=n))
        engine.call(BWD, *bad(good_b, _9=b, _10=n))
    torch.cuda.synchronize()
    for t in (u, beta, r, out, dP, daw, dab):
        assert (t == GUARD).all()
    assert engine.query(WSQ, 5, 384) == 5 * 385 and engine.query(WSQ, 1, 1) == 2
    assert engine.query(WSQ, 0, 16) == 0 and engine.query(WSQ, 4, 0) == 0 and engine.query(WSQ, 4, 513) == 0
    engine.call(FWD, *good_f)                                   # and the good calls are good
    engine.call(BWD, *good_b)
    torch.cuda.synchronize()
    for t in (u, beta, r, out, dP, daw, dab):
        assert bool(torch.isfinite(t).all()) and (t != GUARD).all()


# ---------------------------------------------------------------- 2. the module
def bias_scale(grads, prefix="page_readout."):
    return max(float(grads[prefix + "attention_layer.weight"].abs().max()),
               float(grads[prefix + "attention_layer.bias"].abs().max()))


def test_page_readout_under_autograd_matches_the_oracle():
    rs = np.random.RandomState(13)
    sizes, Fd, G = (40, 0, 61, 30), 24, 8
    N, ps = sum(sizes), starts(sizes)
    torch.manual_seed(11)
    layer = PageReadout(Fd, G)
    sd = {"page_readout." + k: v.detach().clone().double().requires_grad_(True) for k, v in layer.state_dict().items()}
    assert list(sd) == KEYS
    h_host = torch.from_numpy(rs.standard_normal((N, Fd)).astype(np.float32))
    g_host = torch.from_numpy(rs.standard_normal((N, G)).astype(np.float32))
    layer = layer.to(DEV)
    h = h_host.to(DEV).requires_grad_(True)
    out, beta = layer(h, torch.from_numpy(ps).to(DEV), return_attn_wts=True)
    assert out.shape == (N, G) and beta.shape == (N,) and not beta.requires_grad
    sv = out.grad_fn.sv
    (out * g_host.to(DEV)).sum().backward()
    h_ref = h_host.double().requires_grad_(True)
    rows_ref, beta_ref, _, _, P_ref = RO.readout(h_ref, sd, ps, gate=(sv["u"] > 0).cpu(), return_all=True)
    assert relerr(sv["P"].cpu(), P_ref.detach()) < SGEMM_TOL   # a wrong projection cannot hide behind the forced gates
    (rows_ref * g_host.double()).sum().backward()
    assert relerr(out.detach().cpu(), rows_ref.detach()) < 1e-5
    assert relerr(beta.cpu(), beta_ref.detach()) < 1e-5
    assert relerr(h.grad.cpu(), h_ref.grad) < 1e-4
    ref_grads = {k: v.grad for k, v in sd.items()}
    for key, p in layer.named_parameters():
        k = "page_readout." + key
        assert float(ref_grads[KEYS[0]].abs().max()) > 0
        assert relerr(p.grad.cpu(), ref_grads[k], bias_scale(ref_grads) if k == KEYS[2] else None) < 1e-4, key
    assert layer(h.detach(), torch.from_numpy(ps).to(DEV)).shape == (N, G)
    assert layer(h.detach()[:0], torch.zeros(1, dtype=torch.int64, device=DEV)).shape == (0, G)


# ---------------------------------------------------------------- 3. the whole model
@pytest.mark.parametrize("context", [True, False])
def test_model_with_the_readout_matches_the_oracle_on_the_reference_inputs(monkeypatch, context):
    """The cova_h64_n11 inputs hold ONE page.  Its boxes then all receive the same vector, which the decoder's train-mode
    BatchNorm removes again: the readout's gradients are analytically zero there.  So the page is given twice and the
    last five boxes are moved to the copy: the same image, boxes, neighbours and labels as two pages (6 + 5 boxes)."""
    fx, cfg, _, b = load_case("cova_h64_n11")
    assert b["images"].shape[0] == 1 and b["bboxes"].shape[0] == 11
    b = dict(b, images=b["images"].repeat(2, 1, 1, 1).contiguous(), bboxes=b["bboxes"].clone())
    b["bboxes"][6:, 0] = 1.0
    G = 16
    ext = dict(n_heads=2, n_gat_layers=2, attention="gatv2") if context else {}
    cfg = dict(cfg, use_context=context, page_context_dim=G, **ext)
    # the oracle reaches its gat_stack hook under use_context=True only; without heads in the state dict the patched
    # stack states [own | r_page], which is the use_context=False head
    ocfg = dict(cfg, use_context=True)
    wcfg = {k: v for k, v in cfg.items() if k != "drop_prob"}
    seed, gain = int(fx["meta/seed"]), float(fx["meta/logit_gain"])
    sd = weights.seeded_state_dict(seed, logit_gain=gain, **wcfg)
    assert [k for k in sd if k.startswith("page_readout.")] == KEYS and any(k.startswith("gat.") for k in sd) == context
    img_h = int(fx["meta/img_h"])
    n_pages = int(b["images"].shape[0])
    ps = torch.searchsorted(b["bboxes"][:, 0].contiguous(), torch.arange(n_pages + 1, dtype=torch.float32))
    assert ps.tolist() == [0, 6, 11]
    monkeypatch.setattr(O, "gat", G2.patched_gat(b["bboxes"], tuple(b["images"].shape[2:])))
    inputs = (b["images"], b["bboxes"], b["additional_feats"], b["context_indices"])
    # the same seed's model without the option (its own state dict: the decoder is narrower)
    pcfg = {k: v for k, v in cfg.items() if k != "page_context_dim"}
    plain_sd = weights.seeded_state_dict(seed, logit_gain=gain, **{k: v for k, v in pcfg.items() if k != "drop_prob"})
    plain_ref = O.forward(O.clone_state_dict(plain_sd), *inputs, pcfg, False)
    monkeypatch.setattr(O, "gat_stack", RO.patched_gat_stack(ps))
    args = [t.to(DEV) for t in inputs]

    def build():
        m = CoVA(cfg["roi_output_size"], img_h, cfg["n_classes"], context, cfg["hidden_dim"], cfg["bbox_hidden_dim"],
                 cfg["n_additional_feat"], cfg["drop_prob"], None, page_context_dim=G, **ext)
        assert [k for k in m.state_dict()] == list(sd)
        missing = m.load_state_dict(sd, strict=True)
        assert not missing.missing_keys and not missing.unexpected_keys
        return m.to(DEV)

    m = build().eval()
    with torch.no_grad():
        logits = m(*args)
    ref = O.forward(O.clone_state_dict(sd), *inputs, ocfg, False)
    assert relerr(logits.cpu(), ref) < LOGIT_TOL
    assert relerr(plain_ref, ref) > 1e-3                       # the option is live
    m = build().train()
    logits = m(*args)
    sv = logits.grad_fn.sv
    assert sv["T"] == sv["F"] + sv["D"] + G and sv["D"] == (cfg["hidden_dim"] if context else 0)
    assert torch.equal(sv["page_start"].cpu(), ps)             # derived on the device from the page column
    routing = routing_from_saved(dict(sv, gat=None))           # conv, RoI and decoder decisions; the head's gates below
    heads = [head for layer in sv.get("gat") or [] for head in layer["heads"]]
    assert len(heads) == (4 if context else 0)
    for head in heads:
        routing["gate_" + head["prefix"] + "leaky"] = device_gates(head["Wh"], head["ctx"])
    routing["gate_page_readout.leaky"] = (sv["readout"]["u"] > 0).cpu()
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(logits, b["labels"].to(DEV))
    loss.backward()
    loss_ref, logits_ref, grads_ref, _, inter = O.loss_and_grads(sd, *inputs, b["labels"], ocfg, None, routing)
    e = relerr(sv["readout"]["P"].cpu(), inter["own"].double() @ sd[KEYS[0]].double().T)
    print("P against the oracle's projection: %.2e" % e)
    assert e < SGEMM_TOL
    assert relerr(logits.detach().cpu(), logits_ref) < LOGIT_TOL
    assert abs(loss.item() - float(loss_ref)) <= LOSS_TOL * abs(float(loss_ref))
    grads = {k: p.grad for k, p in m.named_parameters()}
    compare_grads(grads, grads_ref, rtol=GRAD_TOL, outlier_frac=0.0)
    for k in KEYS:                                             # (compare_grads floors the scale at 1 % of the largest gradient)
        assert float(grads_ref[k].abs().max()) > 0, k
        assert relerr(grads[k].cpu(), grads_ref[k], bias_scale(grads_ref) if k == KEYS[2] else None) < 1e-4, k


# ---------------------------------------------------------------- 4. the trainer
RCFG = dict(CFG, page_context_dim=16)


@pytest.mark.parametrize("kw", [dict(), dict(optimizer="adamw", max_grad_norm=1.0,
                                             param_groups=[dict(params="page_readout.", lr=5e-3, weight_decay=0.0)]),
                                dict(optimizer="sgd", momentum=0.9, lr=1e-3)])
def test_five_steps_with_the_readout_move_its_attention_vector_and_are_reproducible(kw):
    u8, rows = page_set()
    ds = DeviceDataset(u8, rows, 2, DEV, spatial_k=6)
    sd = seeded(RCFG)
    assert sd[AW].shape == (1, 16)
    a, b = HotPathTrainer(RCFG, sd, DEV, **kw), HotPathTrainer(RCFG, sd, DEV, **kw)
    assert a.params[AW].shape == (1, 16) and a.grads[KEYS[0]].shape == (16, 64 * 9 + 8)
    T = 584 + 32                                            # the readout's 16 * 584 + 17 and a decoder 16 columns wider
    assert sum(v.numel() for v in a.params.values()) == n_params(RCFG) == n_params(CFG) + 16 * 584 + 17 + 16 * (2 * T + 16) + 7 * 16
    assert a.pbucket.flat.numel() >= n_params(RCFG) and a.gbucket.flat.numel() == a.pbucket.flat.numel()
    la, sa = five_steps(a, ds)
    lb, sb = five_steps(b, ds)
    assert la == lb and list(sa) == list(sb)
    for key in sa:
        assert torch.equal(sa[key], sb[key]), key
    assert bool(torch.isfinite(sa[AW]).all())
    assert bool((sa[AW].cpu() != sd[AW]).all())                                 # every channel has moved
    assert not torch.equal(sa[KEYS[0]].cpu(), sd[KEYS[0]])
    # checkpoint round trip: parameters, moments and step count into a fresh trainer, then one more identical step
    c = HotPathTrainer(RCFG, sd, DEV, **kw)
    c.load_state_dict(a.state_dict())
    c.load_optimizer_state_dict(a.optimizer_state_dict())
    batch = next(iter(ds.batches(3, prefetch=False)))
    assert float(a.train_step(batch)[0]) == float(c.train_step(batch)[0])
    assert torch.equal(a.pbucket.flat, c.pbucket.flat)
    with pytest.raises(ValueError, match="page_context_dim"):                   # a checkpoint without the readout
        c.load_state_dict(seeded(CFG))
    with pytest.raises(ValueError, match="page_context_dim"):                   # and the reverse
        HotPathTrainer(CFG, seeded(CFG), DEV).load_state_dict(a.state_dict())


def test_default_step_issues_none_of_the_new_launches_and_the_option_adds_exactly_its_own():
    u8, rows = page_set(P=3)
    batch = next(iter(DeviceDataset(u8, rows, 2, DEV, spatial_k=6).batches(3, prefetch=False)))
    _, plain = profiled(lambda: HotPathTrainer(CFG, seeded(CFG), DEV).train_step(batch))
    assert not any(n in plain for n in (FWD, BWD, WSQ))
    _, again = profiled(lambda: HotPathTrainer(dict(CFG, page_context_dim=0), seeded(CFG), DEV).train_step(batch))
    assert again == plain
    _, ro = profiled(lambda: HotPathTrainer(RCFG, seeded(RCFG), DEV).train_step(batch))
    assert ro[FWD] == 1 and ro[BWD] == 1
    added = {k: ro.get(k, 0) - plain.get(k, 0) for k in set(ro) | set(plain) if ro.get(k, 0) != plain.get(k, 0)}
    assert added == {FWD: 1, BWD: 1, "cova_sgemm": 3}, added
    ncfg = dict(RCFG, use_context=False)                                          # independent of use_context
    _, nro = profiled(lambda: HotPathTrainer(ncfg, seeded(ncfg), DEV).train_step(batch))
    assert nro[FWD] == 1 and nro[BWD] == 1 and not any(n.startswith("cova_gat") for n in nro)


def test_evaluate_split_cached_predict_and_fit_with_the_option_on():
    u8, rows = page_set(P=9, seed=4)
    v8, vrows = page_set(P=11, seed=9)
    train, val = DeviceDataset(u8, rows, 2, DEV, spatial_k=6), DeviceDataset(v8, vrows, 2, DEV, spatial_k=6)
    tr = HotPathTrainer(RCFG, seeded(RCFG), DEV, track_metrics=True, frozen=("convnet.",), bn_eval=("convnet.",))
    rep = evaluate_split(tr, val, with_loss=True)
    assert rep.evaluated.all() and rep.ranks.shape == (11, 3) and np.isfinite(rep.loss)
    tcache, vcache = FeatureCache.build(tr, train), FeatureCache.build(tr, val)
    cached, full = next(iter(val.batches(11, features=vcache))), next(iter(val.batches(11, prefetch=False)))
    assert cached.get("images") is None and cached.get("page_start") is not None
    assert torch.equal(tr.predict(cached)[0], tr.predict(full)[0])
    # the batch's table and the one derived from the page column are the same pages
    derived = dict(full)
    derived.pop("page_start")
    assert torch.equal(tr.predict(derived)[0], tr.predict(full)[0])
    plain = HotPathTrainer(CFG, seeded(CFG), DEV)
    assert not torch.equal(tr.predict(full)[0], plain.predict(full)[0])
    stripped = {k: v for k, v in cached.items() if k not in ("images", "page_start")}
    with pytest.raises(ValueError, match="page_start"):
        tr.predict(stripped)
    before = tr.params[AW].clone()
    out = fit(tr, train, val, 1, 3, sampling_fraction=0.9, seed=12, eval_interval=1, train_features=tcache,
              val_features=vcache)
    assert len(out.history) == 1 and out.history[0]["eval_acc"] is not None and tr.step_count == 3
    assert not torch.equal(tr.params[AW], before)


@pytest.mark.parametrize("kw", [dict(accumulate_steps=2), dict(average="ema")])
def test_accumulation_and_averaging_complete_two_steps_with_the_option(kw):
    u8, rows = page_set(P=6)
    ds = DeviceDataset(u8, rows, 2, DEV, spatial_k=6)
    tr = HotPathTrainer(RCFG, seeded(RCFG), DEV, **kw)
    n = n_params(RCFG)
    second = tr.accbucket if "accumulate_steps" in kw else tr.abucket
    assert sum(v.numel() for v in tr.params.values()) == n and KEYS[0] in second.views       # (a bucket pads its entries)
    assert tr.pbucket.flat.numel() >= n and tr.gbucket.flat.numel() == second.flat.numel() == tr.pbucket.flat.numel()
    before = tr.params[AW].clone()
    losses = [float(tr.train_step(batch)[0]) for batch in ds.batches(3, prefetch=False)]
    assert len(losses) == 2 and all(np.isfinite(x) for x in losses)
    assert bool(torch.isfinite(tr.pbucket.flat).all()) and bool(torch.isfinite(second.flat).all())
    assert not torch.equal(tr.params[AW], before)
    if "average" in kw:
        assert bool(torch.isfinite(tr.averaged_state_dict()[AW]).all())
