"""GPU tests of the head with SEVERAL of its opt-in layers on at once (edge_geometry, attention="gatv2", attention_dropout,
page_context_dim, page_attention_dim, page_attention_geometry), against the composed oracle (tests/combined_oracle.py).
Each layer has its own tests with the others off; what is new here is where they meet, engine._head_fwd / engine.model_bwd:
the page attention's columns behind a readout's (comb[:, F + D + G:], an offset no other test uses; with the "odd" widths
no offset is a multiple of 4 and T is odd), three producers accumulating into dcomb[:, :F] in turn (observed through the
gradients of bbox_feat_encoder.* and bn_additional_feat.*), decoder masks over the G + E columns, and the trainer's path.

a. The head alone through the cached-feature path (the visual columns are given) against the float64 oracle, train mode
   with forced decoder masks at drop_prob 0.5 and eval mode, over {static, gatv2} x {edge off, on} x {readout, page
   attention, both, both + geometry} with a GAT and the four page-layer sets without one, at two width sets: 40 cases.
   Bounds, inputs and comparator: tests/combined_cases.py (1e-5 forward, 1e-4 per gradient tensor on its own scale, 2e-5 for
   the saved projections).  That the comparator rejects an overwriting producer and a page attention that reads the
   readout's columns is shown on the CPU (tests/test_combined_head_cpu.py).
b. The whole model through CoVA on the doubled cova_h64_n11 page with everything on, with and without context: eval and
   train logits, loss and every gradient against O.loss_and_grads run in float64 (tests/test_model_gpu.py's LOGIT_TOL /
   LOSS_TOL / GRAD_TOL, outlier_frac 0, and 1e-4 per tensor on its own scale for every key the options add); once with
   forced decoder masks of width T at drop_prob 0.5; once with attention_dropout 0.5, the oracle's keep masks from
   attn_dropout_oracle.keep_mask.
c. HotPathTrainer.forward_backward against the module under the same seed, everything on; predict on cached features.
d. Fresh (zero) edge and geometry weights in company give the bits of the model built without the two options.
e. The launches the all-on step adds are the sum of what each option adds alone.

Measured on an MI355X (worst over all cases of a section; bound in brackets):
   a. 40 cases x (train, eval): logits, loss, beta, lse, attention rows 6.3e-7 [1e-5]; saved projections P, qkv 3.4e-7
      [2e-5]; gradients on their own scale 2.0e-6 [1e-4] (a GAT head's attention_layer.bias)
   b. eval logits 5.0e-7, train logits 5.4e-6 [5e-5]; loss 7.1e-7 [2e-5]; projections 1.0e-6 [2e-5]; gradients on the 1 %
      floor 1.6e-5 [1e-4]; the options' tensors on their own scale, per run: plain 2.1e-5, decoder masks 9.1e-5, attention
      dropout 3.3e-5, no context 1.7e-5 and 5.4e-6 [1e-4].  The 9.1e-5 is gat.layers.1.heads.1.edge_layer.weight under the
      p = 0.5 masks: a second-layer gradient that is a small sum of cancelling terms on these eleven boxes (the float32
      CPU oracle is 3.3e-5 from float64 there, and the head's own kernels reach 2e-6 on given inputs in section a); it is
      the float32 conditioning of that tensor on these inputs, with little room.  The GAT's other keys, not held on their
      own scale in the whole model, reach 2.8e-3 (layer 1's attention_layer.weight under the masks).
   c. loss equal to all printed digits [2e-5], gradients on the 1 % floor 1.3e-5 [1e-4]"""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import engine, weights  # noqa: E402
from cova_web_object_detection_amd.features import FeatureCache  # noqa: E402
from cova_web_object_detection_amd.models import CoVA  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
from helpers import compare_grads, DEV, GRAD_TOL, LOGIT_TOL, LOSS_TOL, profiled, routing_from_saved, SGEMM_TOL  # noqa: E402
from oracle import cova_oracle as O  # noqa: E402
import attn_dropout_oracle as AD  # noqa: E402
import combined_cases as CC  # noqa: E402
import combined_oracle as CO  # noqa: E402
from config_cases import SPLIT_CFG as CFG  # noqa: E402
from gat_cases import device_gates  # noqa: E402
from trainer_cases import page_set  # noqa: E402

NEW_PREFIXES = ("gat.", "page_readout.", "page_attention.")
relerr = CC.relerr


def option_key(k):
    """The keys the six options add, held per tensor on their own scale in the whole model as each option's own test holds
    its keys.  The GAT's W_i / W_j / attention_layer.* are the reference model's keys: on the whole model's inputs their
    gradients are small sums of cancelling terms on which any float32 computation (the float32 oracle too: up to 1.2e-3,
    tests/test_combined_head_cpu.py) is far from the float64 one, so the whole model holds them through compare_grads and
    section a holds them on their own scale."""
    return k.endswith(CO.EDGE) or k.startswith(("page_readout.", "page_attention."))


def leaky_gates(head, params):
    """The LeakyReLU decisions the device took in one attention head: GATv2 per channel from the saved projections, the
    static score from the saved s and t (tests/helpers.py) with the edge term where the head has one (tests/test_edge_gpu.py)."""
    if head.get("attention") == "gatv2":
        return device_gates(head["Wh"], head["ctx"])
    ctx = head["ctx"]
    t = torch.cat((head["t"], head["t"].new_zeros(1))).double()
    u = head["s"].double().view(-1, 1) + t[ctx.clamp(min=-1)]
    if head.get("phi") is not None:
        w = params[head["prefix"] + "edge_layer.weight"].double().view(-1)
        u = u.float().double() + (head["phi"].double() * w).sum(-1)
    return (u > 0).cpu()


def head_routing(sv, params):
    """Every discrete decision of the head, as the device took it (no conv stack in front: nothing else to force)."""
    n_vis, hd = sv["n_vis"], sv["Hd"]
    r = {"gate_bbox": (sv["comb"][:, n_vis:n_vis + hd] > 0).cpu(), "gate_dec": (sv["dec"]["y"] > 0).cpu()}
    for layer in sv.get("gat") or []:
        for head in layer["heads"]:
            r["gate_" + head["prefix"] + "leaky"] = leaky_gates(head, params)
    if "readout" in sv:
        r[CO.RO_GATE] = (sv["readout"]["u"] > 0).cpu()
    return r


def saved_intermediates(sv):
    inter = {"attn/" + head["prefix"]: head["attn"].cpu() for layer in sv.get("gat") or [] for head in layer["heads"]}
    if "readout" in sv:
        inter["readout/beta"], inter["readout/P"] = sv["readout"]["beta"].cpu(), sv["readout"]["P"].cpu()
    if "page_attn" in sv:
        inter["page_attn/lse"], inter["page_attn/qkv"] = sv["page_attn"]["lse"].cpu(), sv["page_attn"]["qkv"].cpu()
    return inter


# ---------------------------------------------------------------- a. the head alone, against float64
def run_head(case, training):
    """engine.model_fwd on the case's feature table (+ ce_sum and engine.model_bwd in train mode) -> (what the comparator
    reads, the saved state, the parameters)."""
    sd, cfg = case["sd"], case["cfg"]
    params = {k: sd[k].to(DEV) for k in O.param_keys(sd)}
    buffers = {k: v.clone().to(DEV) for k, v in sd.items() if k not in params}
    plan = engine.grad_plan([k for k in params if not k.startswith("convnet.")])
    assert "convstack" not in plan and {"bbox", "addl"} <= plan
    table, ids = case["table"].to(DEV), case["row_ids"].to(DEV)
    logits, sv = engine.model_fwd(cfg, params, buffers, None, case["bboxes"].to(DEV), case["additional"].to(DEV),
                                  case["ctx"].to(DEV), training, (0, 0), [m.to(DEV) for m in case["masks"]] if training else None,
                                  True, plan, visual_feats=(table, ids), page_size=CC.PAGE_SIZE,
                                  page_start=case["page_start"].to(DEV))
    assert (sv["F"], sv["D"], sv["G"], sv["E"], sv["T"]) == tuple(case[k] for k in "FDGET")
    assert torch.equal(sv["comb"][:, :CC.N_VIS].cpu(), case["visual"])               # the given columns, as given
    got = dict(logits=logits.cpu(), loss=None, grads={}, inter=saved_intermediates(sv))
    if training:
        assert sv["dec"]["drop"] and sv["dec"]["drop1"] and tuple(sv["dec"]["m1"].shape) == (case["N"], case["T"])
        loss, dl, _ = engine.ce_sum(logits, case["labels"].to(DEV))
        grads = engine.model_bwd(sv, dl, params, plan=plan)
        torch.cuda.synchronize()
        got.update(loss=float(loss), grads={k: g.cpu() for k, g in grads.items()})
    return got, sv, params


@pytest.mark.parametrize("width", list(CC.WIDTHS))
@pytest.mark.parametrize("row", CC.matrix(), ids=CC.case_id)
def test_head_on_given_features_matches_the_float64_oracle(row, width):
    case = CC.build_case(width, row)
    context, attention, edge, page = row
    got, sv, params = run_head(case, True)
    assert ("gat" in sv) == context and ("readout" in sv) == (case["G"] > 0) and ("page_attn" in sv) == (case["E"] > 0)
    if case["E"]:
        assert ("bboxes" in sv["page_attn"]) == CC.PAGE_LAYERS[page][2]
        assert sv["page_attn"]["out"].data_ptr() == sv["comb"].data_ptr() + 4 * (case["F"] + case["D"] + case["G"])
    ref = CC.reference(case, True, head_routing(sv, params))
    assert set(got["grads"]) == set(ref["grads"])                                   # every gradient model_bwd returns
    errs = CC.check_head(got, ref, "%s %s train" % (width, CC.case_id(row)))
    got_eval, _, _ = run_head(case, False)
    errs_eval = CC.check_head(got_eval, CC.reference(case, False), "%s %s eval" % (width, CC.case_id(row)))
    assert relerr(got_eval["logits"], got["logits"]) > 1e-3                         # (two modes, two results)
    assert set(errs) > set(errs_eval)


# ---------------------------------------------------------------- b. the whole model
def build_model(cfg, sd, img_h):
    kw = {k: cfg[k] for k in list(CC.ALL_ON) + ["attention_dropout"] if k in cfg}
    m = CoVA(cfg["roi_output_size"], img_h, cfg["n_classes"], cfg["use_context"], cfg["hidden_dim"], cfg["bbox_hidden_dim"],
             cfg["n_additional_feat"], cfg["drop_prob"], None, **kw)
    assert list(m.state_dict()) == list(sd)
    missing = m.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return m.to(DEV)


def model_routing(sv):
    """The conv stack's, the RoI op's and the decoder's decisions (tests/helpers.py) and the head's (GATv2 heads here)."""
    routing = routing_from_saved(dict(sv, gat=None))
    for layer in sv.get("gat") or []:
        for head in layer["heads"]:
            routing["gate_" + head["prefix"] + "leaky"] = device_gates(head["Wh"], head["ctx"])
    routing[CO.RO_GATE] = (sv["readout"]["u"] > 0).cpu()
    return routing


@pytest.mark.parametrize("context,variant", [(True, "plain"), (True, "decoder-masks"), (True, "attention-dropout"),
                                             (False, "plain"), (False, "decoder-masks")])
def test_model_with_everything_on_matches_the_composed_oracle(context, variant):
    extra = {"decoder-masks": dict(drop_prob=CC.P_DROP), "attention-dropout": dict(attention_dropout=0.5)}.get(variant, {})
    cfg, ocfg, sd, b, ps, img_h = CC.all_on_inputs(context, **extra)
    inputs = (b["images"], b["bboxes"], b["additional_feats"], b["context_indices"])
    # the reference is the oracle in FLOAT64 through the whole model: on these inputs the float32 oracle is itself a third
    # of the per-tensor bound away from it (tests/test_combined_head_cpu.py), and by another amount on another CPU
    sd64, inputs64 = {k: CC.f64(v) for k, v in sd.items()}, [CC.f64(t) for t in inputs]
    args = [t.to(DEV) for t in inputs]
    page = tuple(b["images"].shape[2:])
    N, K = b["context_indices"].shape
    if variant == "plain":
        with torch.no_grad():
            logits = build_model(cfg, sd, img_h).eval()(*args)
        with CC.stated(*CO.patched(ps, b["bboxes"], page, heads=2), any_dtype=True):
            ref = O.forward(O.clone_state_dict(sd64), *inputs64, ocfg, False)
        e = relerr(logits.cpu(), ref)
        print("eval logits %.2e" % e)
        assert e < LOGIT_TOL
    m = build_model(cfg, sd, img_h).train()
    masks = oracle_masks = None
    if variant == "decoder-masks":
        T = m.n_total_feat
        D = cfg["hidden_dim"] if context else 0
        assert T == sd["decoder.1.weight"].shape[0] == 64 * 9 + cfg["bbox_hidden_dim"] + D + 16 + 8
        rs = np.random.RandomState(2)
        masks = [torch.from_numpy((rs.uniform(size=(N, T)) > CC.P_DROP).astype(np.uint8)) for _ in range(2)]
        m._forced_masks = [t.to(DEV) for t in masks]
        oracle_masks = [t.double() for t in masks]
        assert not all(bool(t[:, T - 24:].all()) for t in masks)                    # the G + E columns lose entries
    m.seed_dropout(5)
    logits = m(*args)
    sv = logits.grad_fn.sv
    assert sv["T"] == sv["F"] + sv["D"] + 16 + 8 and torch.equal(sv["page_start"].cpu(), ps)
    heads = [(l, i, head) for l, layer in enumerate(sv.get("gat") or []) for i, head in enumerate(layer["heads"])]
    assert len(heads) == (4 if context else 0) and "bboxes" in sv["page_attn"]
    keeps = {}
    if variant == "attention-dropout":
        base = AD.dropout_base(5, 1)
        for l, i, head in heads:
            stream = AD.attention_dropout_seed(base, l, i)
            assert head["drop"] == (0.5, stream)                                   # the streams the saved heads report
            keeps[head["prefix"]] = AD.keep_mask(0.5, stream, N, K)
        assert not all(k.all() for k in keeps.values())
    else:
        assert all(head["drop"] is None for _, _, head in heads)
    routing = model_routing(sv)
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(logits, b["labels"].to(DEV))
    loss.backward()
    with CC.stated(*CO.patched(ps, b["bboxes"], page, heads=2, keeps=keeps, attention_dropout=0.5 if keeps else 0.0),
                   any_dtype=True):
        loss_ref, logits_ref, grads_ref, _, inter = O.loss_and_grads(sd64, *inputs64, b["labels"], ocfg, oracle_masks, routing)
    assert logits_ref.dtype == torch.float64
    e = relerr(sv["readout"]["P"].cpu(), inter["own"].double() @ sd[CO.RO_KEY].double().T)
    q = relerr(sv["page_attn"]["qkv"].cpu(), inter["own"].double() @ sd["page_attention.qkv.weight"].double().T)
    print("projections against the oracle's: P %.2e, qkv %.2e" % (e, q))
    assert e < SGEMM_TOL and q < SGEMM_TOL
    el, eo = relerr(logits.detach().cpu(), logits_ref), abs(loss.item() - float(loss_ref)) / abs(float(loss_ref))
    print("train logits %.2e, loss %.2e" % (el, eo))
    assert el < LOGIT_TOL and eo <= LOSS_TOL
    grads = {k: p.grad for k, p in m.named_parameters()}
    assert set(grads) == set(grads_ref)
    print("worst gradient on the 1 % floor:", compare_grads(grads, grads_ref, rtol=GRAD_TOL, outlier_frac=0.0))
    worst, other = ("", 0.0), ("", 0.0)
    for k in grads_ref:                                        # (compare_grads floors the scale at 1 % of the largest gradient)
        e = relerr(grads[k].cpu(), grads_ref[k], CC.grad_scale(k, grads_ref))
        if option_key(k):
            assert float(grads_ref[k].abs().max()) > 0, k
            worst = max(worst, (k, e), key=lambda x: x[1])
            assert e < 1e-4, (k, e)
        elif k.startswith("gat."):
            other = max(other, (k, e), key=lambda x: x[1])
    assert sum(map(option_key, grads_ref)) == (4 if context else 0) + 3 + 2
    print("worst option tensor on its own scale:", worst, "(not held: the GAT's other keys,", other, ")")


# ---------------------------------------------------------------- c. the trainer
def test_trainer_gradients_agree_with_the_module_with_everything_on():
    """tests/test_attn_dropout_gpu.py::test_trainer_gradients_agree_with_the_module_under_the_same_seeds with the page layers
    on as well: same weights, same seed, so the decoder's and every head's masks come from the same streams.  The trainer
    projects with one GEMM per head where the module issues two: GRAD_TOL, not bit for bit."""
    cfg, _, sd, b, ps, img_h = CC.all_on_inputs(True, drop_prob=0.2, attention_dropout=0.5)
    batch = {k: v.to(DEV) for k, v in b.items() if torch.is_tensor(v)}
    tr = HotPathTrainer(cfg, sd, DEV, dropout_seed=5)
    loss, _ = tr.forward_backward(batch)
    m = build_model(cfg, sd, img_h).train()
    m.seed_dropout(5)
    logits = m(batch["images"], batch["bboxes"], batch["additional_feats"], batch["context_indices"])
    sv = logits.grad_fn.sv
    base = engine.dropout_base(5, 1)
    assert [h["drop"] for layer in sv["gat"] for h in layer["heads"]] == [(0.5, engine.attention_dropout_seed(base, l, i))
                                                                         for l in range(2) for i in range(2)]
    assert "readout" in sv and "bboxes" in sv["page_attn"] and sv["dec"]["drop"]
    mloss = torch.nn.CrossEntropyLoss(reduction="sum")(logits, batch["labels"])
    mloss.backward()
    mloss = mloss.detach()
    print("loss: trainer %.6f, module %.6f" % (float(loss), float(mloss)))
    assert abs(float(loss) - float(mloss)) <= 2e-5 * abs(float(mloss))
    ref = {k: q.grad.detach().cpu() for k, q in m.named_parameters()}
    assert set(ref) == set(tr.grads)
    assert all(float(ref[k].abs().max()) > 0 for k in ref
               if k.startswith(NEW_PREFIXES) and not (k.startswith("gat.") and k.endswith("attention_layer.bias")))
    worst = compare_grads({k: v.clone() for k, v in tr.grads.items()}, ref, rtol=GRAD_TOL, outlier_frac=0.0)
    print("worst gradient:", worst)


ON = dict(edge_geometry=True, attention="gatv2", attention_dropout=0.5, page_context_dim=16, page_attention_dim=16,
          page_attention_heads=2, page_attention_geometry=True)


def seeded(cfg, live=True):
    """seeded weights of a trainer configuration; ``live``: the two zero-initialised weights get seeded non-zero values"""
    wcfg = {k: v for k, v in cfg.items() if k not in ("drop_prob", "attention_dropout")}
    sd = weights.seeded_state_dict(77, logit_gain=2.0, **wcfg)
    rs = np.random.RandomState(8)
    for k in sd:
        if live and (k.endswith(CO.EDGE) or k == CO.GEO_KEY):
            sd[k] = torch.from_numpy(rs.standard_normal(tuple(sd[k].shape)).astype(np.float32))
    return sd


def test_predict_on_cached_features_equals_the_full_batch_with_everything_on():
    cfg = dict(CFG, **ON)
    v8, vrows = page_set(P=11, seed=9)
    val = DeviceDataset(v8, vrows, 2, DEV, spatial_k=6)
    tr = HotPathTrainer(cfg, seeded(cfg), DEV, frozen=("convnet.",), bn_eval=("convnet.",))
    vcache = FeatureCache.build(tr, val)
    cached, full = next(iter(val.batches(11, features=vcache))), next(iter(val.batches(11, prefetch=False)))
    assert cached.get("images") is None and cached.get("page_start") is not None and cached.get("page_size") is not None
    (a, _), calls = profiled(lambda: tr.predict(cached))
    assert calls["cova_page_readout_fwd"] == 1 and calls["cova_page_attn_fwd_geo"] == 1 and calls["cova_gat2_fwd"] == 1
    assert calls["cova_edge_geometry"] == 1 and "cova_gat2_fwd_drop" not in calls
    assert torch.equal(a, tr.predict(full)[0])
    plain = HotPathTrainer(CFG, seeded(CFG), DEV)
    assert not torch.equal(a, plain.predict(full)[0])


# ---------------------------------------------------------------- d. inert options stay inert in company
def test_fresh_edge_and_geometry_weights_in_company_give_the_bits_of_the_model_without_them():
    extra = dict(drop_prob=0.2, attention_dropout=0.5)
    cfg, _, sd, b, _, img_h = CC.all_on_inputs(True, fresh=True, **extra)
    zero = [k for k in sd if k.endswith(CO.EDGE) or k == CO.GEO_KEY]
    assert len(zero) == 5 and not any(sd[k].any() for k in zero)
    pcfg, _, psd, _, _, _ = CC.all_on_inputs(True, edge_geometry=False, page_attention_geometry=False, **extra)
    assert [k for k in sd if k not in zero] == list(psd) and all(torch.equal(sd[k], psd[k]) for k in psd)
    args = [b[k].to(DEV) for k in ("images", "bboxes", "additional_feats", "context_indices")]
    out = []
    for c, s in ((cfg, sd), (pcfg, psd)):
        m = build_model(c, s, img_h).train()
        m.seed_dropout(5)
        logits = m(*args)
        sv = logits.grad_fn.sv
        assert ("bboxes" in sv["page_attn"]) == (c is cfg) and (sv["gat"][0]["heads"][0]["phi"] is not None) == (c is cfg)
        assert sv["gat"][1]["heads"][1]["drop"] is not None and sv["dec"]["drop"]
        torch.nn.CrossEntropyLoss(reduction="sum")(logits, b["labels"].to(DEV)).backward()
        out.append((logits.detach(), {k: p.grad for k, p in m.named_parameters()}))
    (la, ga), (lb, gb) = out
    assert torch.equal(la, lb)
    assert set(ga) == set(gb) | set(zero)
    for k in gb:
        assert torch.equal(ga[k], gb[k]), k
    assert all(bool(ga[k].any()) for k in zero)                                     # inert in value, not in gradient


# ---------------------------------------------------------------- e. launch bookkeeping
FAMILY = [(re.compile(r"^cova_gat2?_(fwd|bwd)(_edge|_drop)?$"), r"cova_gat_\1"),
          (re.compile(r"^cova_page_attn_(fwd|bwd)(_geo)?$"), r"cova_page_attn_\1")]


def launches(cfg, batch):
    """{entry point: calls} of one train step, (the exact names, the names with every variant of the GAT pair and of the
    page-attention pair under one family name and the host-side size queries left out)"""
    _, calls = profiled(lambda: HotPathTrainer(cfg, seeded(cfg), DEV).train_step(batch))
    fam = {}
    for name, n in calls.items():
        if name.endswith(("_floats", "_ints")):
            continue
        for rx, to in FAMILY:
            name = rx.sub(to, name)
        fam[name] = fam.get(name, 0) + n
    return calls, fam


def added(a, b):
    return {k: a.get(k, 0) - b.get(k, 0) for k in set(a) | set(b) if a.get(k, 0) != b.get(k, 0)}


def plus(a, b):
    out = {k: a.get(k, 0) + b.get(k, 0) for k in set(a) | set(b)}
    return {k: v for k, v in out.items() if v}


def test_the_all_on_step_adds_the_sum_of_what_each_option_adds_alone():
    u8, rows = page_set(P=3)
    batch = next(iter(DeviceDataset(u8, rows, 2, DEV, spatial_k=6).batches(3, prefetch=False)))
    _, plain = launches(CFG, batch)
    attn = dict(CFG, page_attention_dim=16, page_attention_heads=2)
    alone = {"edge_geometry": (dict(CFG, edge_geometry=True), plain), "gatv2": (dict(CFG, attention="gatv2"), plain),
             "attention_dropout": (dict(CFG, attention_dropout=0.5), plain),
             "page_context_dim": (dict(CFG, page_context_dim=16), plain), "page_attention_dim": (attn, plain)}
    total = {}
    for option, (cfg, base) in alone.items():
        d = added(launches(cfg, batch)[1], base)
        print(option, "adds", d)
        total = plus(total, d)
    _, attn_fam = launches(attn, batch)
    d = added(launches(dict(attn, page_attention_geometry=True), batch)[1], attn_fam)       # (the bias needs its layer)
    print("page_attention_geometry adds", d)
    total = plus(total, d)
    exact, fam = launches(dict(CFG, **ON), batch)
    print("everything adds", added(fam, plain))
    assert added(fam, plain) == total
    assert total == {"cova_edge_geometry": 1, "cova_page_readout_fwd": 1, "cova_page_readout_bwd": 1, "cova_page_attn_fwd": 1,
                     "cova_page_attn_bwd": 1, "cova_sgemm": 6}
    # and the variants the all-on step takes: one GATv2 pair with dropout, one page-attention pair with the bias
    for name, n in (("cova_gat2_fwd_drop", 1), ("cova_gat2_bwd_drop", 1), ("cova_page_attn_fwd_geo", 1),
                    ("cova_page_attn_bwd_geo", 1)):
        assert exact.get(name, 0) == n, name
    for name in ("cova_gat_fwd", "cova_gat_bwd", "cova_gat_fwd_edge", "cova_gat_bwd_edge", "cova_gat_fwd_drop",
                 "cova_gat_bwd_drop", "cova_gat2_fwd", "cova_gat2_bwd", "cova_page_attn_fwd", "cova_page_attn_bwd"):
        assert name not in exact, name
