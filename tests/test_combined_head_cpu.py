"""The composed oracle (tests/combined_oracle.py) has to be trustworthy before the kernels are held to it
(tests/test_combined_head_gpu.py): with one option on it IS that option's own oracle, bit for bit in float64, outputs and
autograd gradients; it passes gradcheck with everything on; its columns are [GAT D | readout G | page attention E]; on the
inputs of the GPU tests every option is live and every new parameter has a gradient; and the comparator of the GPU test
rejects the two mistakes that test exists for (a producer that overwrites dcomb[:, :F], a page attention that takes its
gradient from the readout's columns), planted in the oracle, while the reference alone is inside every bound."""
import warnings

import numpy as np
import pytest
import torch

from cova_web_object_detection_amd import weights
from cova_web_object_detection_amd.models import CoVA
from oracle import cova_oracle as O
import attn_dropout_oracle as AD
import combined_cases as CC
import combined_oracle as CO
import edge_oracle as EO
import gatv2_oracle as G2
import page_attn_geo_oracle as PG
import page_attn_oracle as PA
import readout_oracle as RO

SIZES, FD, KN = (4, 1, 3), 6, 3
PS = [0, 4, 5, 8]
PAGE = (PG.PAGE_H, PG.PAGE_W)
ALL_ON, all_on_inputs = CC.ALL_ON, CC.all_on_inputs


def tiny(seed=0, context=True, attention="gat", edge=False, G=0, E=0, heads=2, geo=False, D=4):
    """3 pages of 4, 1 and 3 boxes, 6 own features -> (h, ctx, boxes, sd), float64 leaves."""
    rs = np.random.RandomState(seed)
    N = sum(SIZES)
    rnd = lambda *s: torch.from_numpy(rs.standard_normal(s)).requires_grad_(True)
    sd = {}
    if context:
        for l, prefixes in enumerate(weights.gat_prefixes(2, 2)):
            fin, dh = (FD if l == 0 else D), D // 2
            for p in prefixes:
                sd[p + "W_i.weight"], sd[p + "W_j.weight"] = rnd(dh, fin), rnd(dh, fin)
                sd[p + "attention_layer.weight"] = rnd(1, dh if attention == "gatv2" else 2 * dh)
                sd[p + "attention_layer.bias"] = rnd(1)
                if edge:
                    sd[p + "edge_layer.weight"] = rnd(1, 8)
    if G:
        sd["page_readout.W.weight"], sd["page_readout.attention_layer.weight"] = rnd(G, FD), rnd(1, G)
        sd["page_readout.attention_layer.bias"] = rnd(1)
    if E:
        sd[PA.KEY] = rnd(3 * E, FD)
        if geo:
            sd[PG.GEO_KEY] = rnd(heads, 8)
    ctx = torch.from_numpy(CC.context_table(rs, SIZES, KN))
    return rnd(N, FD), ctx, torch.from_numpy(PG.planted_boxes(SIZES, seed + 1)), sd


def outputs_and_grads(fn, h, sd, seed=5):
    """fn() -> columns; -> (columns, d h, {key: d sd[key]}) under one fixed cotangent"""
    for v in [h] + list(sd.values()):
        v.grad = None
    cols = fn()
    g = torch.from_numpy(np.random.RandomState(seed).standard_normal(tuple(cols.shape)))
    (cols * g).sum().backward()
    return cols.detach().clone(), h.grad.clone(), {k: (None if v.grad is None else v.grad.clone()) for k, v in sd.items()}


def assert_same(a, b):
    assert torch.equal(a[0], b[0]) and a[0].dtype == torch.float64 and a[0].shape[1] > 0
    assert torch.equal(a[1], b[1])
    assert list(a[2]) == list(b[2])
    for k in a[2]:
        assert a[2][k] is not None and torch.equal(a[2][k], b[2][k]), k


def sibling_stack(monkeypatch, gat=None, gat_stack=None):
    """the per-feature hooks as the single-feature tests install them -> the resulting O.gat_stack"""
    if gat is not None:
        monkeypatch.setattr(O, "gat", gat)
    if gat_stack is not None:
        monkeypatch.setattr(O, "gat_stack", gat_stack)
    return O.gat_stack


# ---------------------------------------------------------------- 1. one option on: the option's own oracle
def test_no_option_is_the_plain_stack(monkeypatch):
    h, ctx, boxes, sd = tiny()
    batch = CO.Batch()
    assert_same(outputs_and_grads(lambda: CO.head(batch, h, ctx, sd)[0], h, sd),
                outputs_and_grads(lambda: O.gat_stack(h, ctx, sd)[0], h, sd))


def test_edge_geometry_alone_is_the_edge_oracle(monkeypatch):
    h, ctx, boxes, sd = tiny(edge=True)
    routing = {"gate_gat.layers.0.heads.1.leaky": torch.from_numpy(np.random.RandomState(1).uniform(size=(8, KN)) > 0.5)}
    batch = CO.Batch(bboxes=boxes, page_size=PAGE)
    mine = outputs_and_grads(lambda: CO.head(batch, h, ctx, sd, routing=routing)[0], h, sd)
    stack = sibling_stack(monkeypatch, gat=EO.patched_gat(boxes, PAGE))
    assert_same(mine, outputs_and_grads(lambda: stack(h, ctx, sd, routing=routing)[0], h, sd))


@pytest.mark.parametrize("edge", [False, True])
def test_gatv2_alone_is_the_gatv2_oracle(monkeypatch, edge):
    h, ctx, boxes, sd = tiny(attention="gatv2", edge=edge)
    routing = {"gate_gat.layers.1.heads.0.leaky": torch.from_numpy(np.random.RandomState(1).uniform(size=(8, KN, 2)) > 0.5)}
    batch = CO.Batch(bboxes=boxes, page_size=PAGE)
    mine = outputs_and_grads(lambda: CO.head(batch, h, ctx, sd, routing=routing)[0], h, sd)
    stack = sibling_stack(monkeypatch, gat=G2.patched_gat(boxes, PAGE))
    assert_same(mine, outputs_and_grads(lambda: stack(h, ctx, sd, routing=routing)[0], h, sd))


@pytest.mark.parametrize("attention", ["gat", "gatv2"])
def test_attention_dropout_alone_is_the_dropout_oracle(attention):
    h, ctx, boxes, sd = tiny(attention=attention)
    p = 0.5
    keeps = {pre: AD.keep_mask(p, AD.attention_dropout_seed(AD.dropout_base(5, 1), l, i), 8, KN)
             for l, prefixes in enumerate(weights.gat_prefixes(2, 2)) for i, pre in enumerate(prefixes)}
    assert not all(k.all() for k in keeps.values())
    batch = CO.Batch(keeps=keeps, attention_dropout=p)

    def sibling():
        x = h
        for prefixes in weights.gat_prefixes(2, 2):
            x = torch.cat([AD.head(attention, x, ctx, sd, pre, keeps[pre], p)[0] for pre in prefixes], 1)
        return x
    assert_same(outputs_and_grads(lambda: CO.head(batch, h, ctx, sd)[0], h, sd), outputs_and_grads(sibling, h, sd))


@pytest.mark.parametrize("context", [True, False])
def test_readout_alone_is_the_readout_oracle(monkeypatch, context):
    h, ctx, boxes, sd = tiny(context=context, G=5)
    routing = {CO.RO_GATE: torch.from_numpy(np.random.RandomState(1).uniform(size=8) > 0.5)}
    batch = CO.Batch(PS)
    mine = outputs_and_grads(lambda: CO.head(batch, h, ctx, sd, routing=routing)[0], h, sd)
    assert mine[0].shape[1] == (4 if context else 0) + 5
    stack = sibling_stack(monkeypatch, gat_stack=RO.patched_gat_stack(PS))
    assert_same(mine, outputs_and_grads(lambda: stack(h, ctx, sd, routing=routing)[0], h, sd))


@pytest.mark.parametrize("context", [True, False])
@pytest.mark.parametrize("geo", [False, True])
def test_page_attention_alone_is_its_oracle(monkeypatch, context, geo):
    h, ctx, boxes, sd = tiny(context=context, E=8, geo=geo)
    batch = CO.Batch(PS, boxes, PAGE, heads=2)
    mine = outputs_and_grads(lambda: CO.head(batch, h, ctx, sd)[0], h, sd)
    assert mine[0].shape[1] == (4 if context else 0) + 8
    hook = PG.patched_gat_stack(PS, 2, boxes, PAGE) if geo else PA.patched_gat_stack(PS, 2)
    stack = sibling_stack(monkeypatch, gat_stack=hook)
    assert_same(mine, outputs_and_grads(lambda: stack(h, ctx, sd)[0], h, sd))


def test_patched_returns_both_replacements_and_the_single_head_form():
    """patched()'s gat is the composed head for one prefix; its gat_stack does not go through O.gat at all"""
    h, ctx, boxes, sd = tiny(attention="gatv2", edge=True, G=5, E=8, geo=True)
    gat, stack = CO.patched(PS, boxes, PAGE, heads=2)
    batch = CO.Batch(PS, boxes, PAGE, heads=2)
    cols, attn0 = stack(h, ctx, sd)
    ref, ref_attn = CO.head(batch, h, ctx, sd)
    assert torch.equal(cols, ref) and torch.equal(attn0, ref_attn) and cols.shape == (8, 4 + 5 + 8)
    p = "gat.layers.0.heads.1."
    assert torch.equal(gat(h, ctx, sd, prefix=p), CO.gat_head(batch, h, ctx, sd, prefix=p)[0])
    o, a = gat(h, ctx, sd, return_attn_wts=True, prefix=p)
    assert o.shape == (8, 2) and a.shape == (8, KN)


# ---------------------------------------------------------------- 2. differentiable
def test_gradcheck_with_every_option_on():
    h, ctx, boxes, sd = tiny(attention="gatv2", edge=True, G=3, E=8, geo=True)
    keeps = {pre: AD.keep_mask(0.5, 11 + i, 8, KN) for i, pre in enumerate(p for l in weights.gat_prefixes(2, 2) for p in l)}
    batch = CO.Batch(PS, boxes, PAGE, heads=2, keeps=keeps, attention_dropout=0.5)
    keys = list(sd)

    def fn(hh, *vals):
        return CO.head(batch, hh, ctx, dict(zip(keys, vals)))[0]
    assert fn(h, *sd.values()).shape == (8, 4 + 3 + 8)
    assert torch.autograd.gradcheck(fn, (h,) + tuple(sd.values()), eps=1e-6, atol=1e-6, rtol=1e-5)
    h, ctx, boxes, sd = tiny(seed=1, attention="gat", edge=True, G=3, E=8, geo=True)          # the static score
    keys = list(sd)
    assert torch.autograd.gradcheck(fn, (h,) + tuple(sd.values()), eps=1e-6, atol=1e-6, rtol=1e-5)


# ---------------------------------------------------------------- 3. column order and widths
@pytest.mark.parametrize("context", [True, False])
def test_each_layer_moves_its_own_columns_only(context):
    h, ctx, boxes, sd = tiny(context=context, attention="gatv2", edge=True, G=5, E=8, geo=True)
    D, G, E = (4 if context else 0), 5, 8
    batch = CO.Batch(PS, boxes, PAGE, heads=2)
    with torch.no_grad():
        base = CO.head(batch, h, ctx, sd)[0]
        assert base.shape == (8, D + G + E)

        def moved(prefix):
            other = {k: (v + 0.25 if k.startswith(prefix) else v) for k, v in sd.items()}
            assert any(k.startswith(prefix) for k in sd)
            return (CO.head(batch, h, ctx, other)[0] != base).any(0)
        ro, pa = moved("page_readout."), moved("page_attention.")
        assert ro[D:D + G].all() and not ro[:D].any() and not ro[D + G:].any()
        assert pa[D + G:].all() and not pa[:D + G].any()
        if context:
            gat = moved("gat.")
            assert gat[:D].all() and not gat[D:].any()


# ---------------------------------------------------------------- 4. the preconditions of the GPU tests
def static_twin(context, **extra):
    """all_on_inputs with the static score: the same seed's model (tests/test_gatv2_gpu.py's form of "GATv2 is live")"""
    cfg, ocfg, sd, b, ps, img_h = all_on_inputs(context, **extra)
    assert cfg["attention"] == "gatv2"
    return all_on_inputs(context, **dict(extra, attention="gat"))


def inputs_of(b):
    return (b["images"], b["bboxes"], b["additional_feats"], b["context_indices"])


def switched_off(sd, option):
    """The state dict of the same model with one option made inert, every other weight kept."""
    off = {k: v.clone() for k, v in sd.items()}
    for k in sd:
        if option == "edge_geometry" and k.endswith(CO.EDGE) or option == "page_attention_geometry" and k == CO.GEO_KEY:
            off[k].zero_()
        if option == "page_context_dim" and k == CO.RO_KEY:                       # P = 0: r = 0, the columns are zero
            off[k].zero_()
        if option == "page_attention_dim" and k == PA.KEY:                        # V = 0: O = 0
            off[k][2 * off[k].shape[0] // 3:].zero_()
    return off


@pytest.mark.parametrize("context", [True, False])
def test_every_option_is_live_and_every_new_parameter_has_a_gradient_on_the_gpu_tests_inputs(context):
    cfg, ocfg, sd, b, ps, _ = all_on_inputs(context)
    N, Kc = b["context_indices"].shape
    page = tuple(b["images"].shape[2:])
    with CC.stated(*CO.patched(ps, b["bboxes"], page, heads=2)):
        ref = O.forward(O.clone_state_dict(sd), *inputs_of(b), ocfg, False)
        options = ["page_context_dim", "page_attention_dim", "page_attention_geometry"]
        options += ["edge_geometry", "gatv2"] if context else []
        for option in options:
            off = static_twin(context)[2] if option == "gatv2" else switched_off(sd, option)
            off = O.forward(O.clone_state_dict(off), *inputs_of(b), ocfg, False)
            e = CC.relerr(off, ref)
            print("%s off moves the logits by %.2e" % (option, e))
            assert e > 1e-3, option
        _, _, grads, _, _ = O.loss_and_grads(sd, *inputs_of(b), b["labels"], ocfg, None, None)
    new = [k for k in sd if k.startswith(("gat.", "page_readout.", "page_attention.")) and k in grads]
    assert len(new) == (4 * 5 if context else 0) + 3 + 2
    for k in new:
        if k.startswith("gat.") and k.endswith("attention_layer.bias"):       # outside the LeakyReLU: softmax removes it
            assert float(grads[k].abs().max()) < 1e-6 * max(float(g.abs().max()) for g in grads.values()), k
        else:
            assert float(grads[k].abs().max()) > 0, k
    if context:                                                                   # attention dropout: the masks drop something
        keeps = {p: AD.keep_mask(0.5, AD.attention_dropout_seed(AD.dropout_base(5, 1), l, i), N, Kc)
                 for l, prefixes in enumerate(weights.gat_prefixes(2, 2)) for i, p in enumerate(prefixes)}
        with CC.stated(*CO.patched(ps, b["bboxes"], page, heads=2, keeps=keeps, attention_dropout=0.5)):
            dropped = O.forward(O.clone_state_dict(sd), *inputs_of(b), ocfg, True)
        with CC.stated(*CO.patched(ps, b["bboxes"], page, heads=2)):
            kept = O.forward(O.clone_state_dict(sd), *inputs_of(b), ocfg, True)
        e = CC.relerr(dropped, kept)
        print("attention_dropout off moves the train-mode logits by %.2e" % e)
        assert e > 1e-3


def test_the_float32_oracle_alone_misses_the_per_tensor_bound_so_the_whole_model_reference_runs_in_float64():
    """The whole-model GPU test holds every gradient tensor of the options on its OWN scale to 1e-4.  The float32 CPU oracle
    cannot carry that bound: its own distance from the same oracle run in float64 (same ReLU / LeakyReLU / max-pool / RoIPool
    decisions) is about a third of the bound on the keys the options add and reaches 1e-3 on the GAT's W_i / W_j /
    attention_layer.weight, small sums of cancelling terms on these inputs (and the float32 sums differ from one CPU to the
    next).  So that test states the whole model in float64 (combined_oracle.roi_pool_in_dtype): shown to work here."""
    cfg, ocfg, sd, b, ps, _ = all_on_inputs(True)
    page = tuple(b["images"].shape[2:])
    tap = {}
    with CC.stated(*CO.patched(ps, b["bboxes"], page, heads=2)):
        _, logits32, g32, _, inter = O.loss_and_grads(sd, *inputs_of(b), b["labels"], ocfg, None, {"_tap": tap})
        _, arg = O.roi_pool_argmax(inter["feat"], b["bboxes"], cfg["roi_output_size"], O.feature_map_size(b["images"].shape[2]) / b["images"].shape[2])
    routing = {k: v > 0 for k, v in tap.items() if k != "pool_in"}
    routing["roi_argmax"] = arg.reshape(arg.shape[0], -1)
    with CC.stated(*CO.patched(ps, b["bboxes"], page, heads=2), any_dtype=True):
        _, logits64, g64, _, _ = O.loss_and_grads({k: CC.f64(v) for k, v in sd.items()}, *[CC.f64(t) for t in inputs_of(b)],
                                                  b["labels"], ocfg, None, routing)
    assert logits64.dtype == torch.float64 and all(g.dtype == torch.float64 for g in g64.values())
    assert CC.relerr(logits32, logits64) < 5e-5                                # (LOGIT_TOL: the two runs state one model)
    errs = {k: CC.relerr(g32[k], g64[k], CC.grad_scale(k, g64)) for k in g64}
    added = [k for k in g64 if k.endswith(CO.EDGE) or k.startswith(("page_readout.", "page_attention."))]
    assert len(added) == 4 + 3 + 2 and all(float(g64[k].abs().max()) > 0 for k in added)
    worst = max((errs[k], k) for k in g64 if k.startswith("gat."))
    print("float32 oracle against float64, own scale: keys the options add %.2e, the GAT's keys %.2e (%s)"
          % (max(errs[k] for k in added), *worst))
    assert worst[0] > 1e-4


@pytest.mark.parametrize("width", list(CC.WIDTHS))
def test_the_head_cases_are_live_aligned_as_claimed_and_clear_of_the_lse_spacing(width):
    case = CC.build_case(width, (True, "gatv2", True, "both+geo"))
    F, D, G, E, T = (case[k] for k in "FDGET")
    assert T == F + D + G + E and case["sd"]["decoder.1.weight"].shape == (T, T)
    offsets = [F, F + D, F + D + G, T]
    assert all(o % 4 for o in offsets) and T % 2 if width == "odd" else not any(o % 4 for o in offsets)
    ctx, N = case["ctx"], case["N"]
    assert (ctx == -1).any() and (ctx[:, 0] >= 0).all() and bool((ctx == torch.arange(N).view(-1, 1)).any())
    ref, base = CC.reference(case), CC.reference(case, training=False)
    for option in ("page_context_dim", "page_attention_dim", "page_attention_geometry", "edge_geometry"):
        off = CC.reference(case, training=False, sd=switched_off(case["sd"], option))
        assert CC.relerr(off["logits"], base["logits"]) > 1e-3, option
    static = CC.reference(CC.build_case(width, (True, "gat", True, "both+geo")), training=False)     # the same seed's static model
    assert CC.relerr(static["logits"], base["logits"]) > 1e-3
    for k, g in ref["grads"].items():
        if not k.endswith(CC.SUM_BIASES):
            assert float(g.abs().max()) > 0, k
    # an f32 lse near 100 is spaced 7.6e-6 apart; these stay far below
    assert float(ref["inter"]["page_attn/lse"].abs().max()) < 16


# ---------------------------------------------------------------- 5. the comparator of the GPU test
def as_float32(ref):
    """what a correct float32 implementation would hand the comparator: the reference rounded once"""
    r32 = lambda t: t.float().double()
    return dict(logits=r32(ref["logits"]), loss=float(np.float32(float(ref["loss"]))),
                grads={k: r32(v) for k, v in ref["grads"].items()}, inter={k: r32(v) for k, v in ref["inter"].items()})


@pytest.mark.parametrize("row", [(True, "gatv2", True, "both+geo"), (True, "gat", False, "both"), (False, "gat", False, "both")],
                         ids=CC.case_id)
def test_the_comparator_rejects_the_two_mistakes_and_accepts_the_reference(row):
    case = CC.build_case("odd", row)
    D, G, E = case["D"], case["G"], case["E"]
    ref = CC.reference(case)
    errs = CC.check_head(as_float32(ref), ref, "the reference, rounded to float32")
    assert max(errs.values()) < 1e-6                       # the reference alone is far inside every bound

    def overwriting(good):
        """the readout's data gradient OVERWRITES dcomb[:, :F]: what the GAT had added to it is lost"""
        def fn(h_i, ctx, sd, alpha=0.2, routing=None):
            cols, attn = good(h_i, ctx, sd, alpha, routing)
            lost, _ = good(h_i.detach(), ctx, sd, alpha, routing)
            return torch.cat((lost[:, :D], cols[:, D:]), dim=1), attn
        return fn

    def wrong_columns(good):
        """the page attention's backward takes its g from dcomb[:, F + D:] instead of dcomb[:, F + D + G:]"""
        def fn(h_i, ctx, sd, alpha=0.2, routing=None):
            cols, attn = good(h_i, ctx, sd, alpha, routing)
            out = cols[:, D + G:]
            carrier = torch.zeros_like(cols)
            carrier[:, D:D + E] = out - out.detach()          # zero in value; its gradient is the one of the wrong columns
            return torch.cat((cols[:, :D + G], out.detach()), dim=1) + carrier, attn
        return fn

    observers = [k for k in ref["grads"] if k.startswith(("bbox_feat_encoder.", "bn_additional_feat."))]
    assert len(observers) == 6
    for mistake in ([overwriting] if D else []) + [wrong_columns]:
        bad = CC.reference(case, gat_stack=mistake)
        assert CC.relerr(bad["logits"], ref["logits"]) < 1e-12                 # the forward is untouched
        with pytest.raises(AssertionError):
            CC.check_head(bad, ref, mistake.__name__)
        errs = CC.head_errors(bad, ref)
        seen = [k for k in observers if errs["grad/" + k] > 10 * CC.BWD_TOL]
        print(mistake.__name__, "seen by", seen)
        assert seen, mistake.__name__                         # the three-way sum's observers see it, far above the bound


# ---------------------------------------------------------------- 6. state-dict order
@pytest.mark.parametrize("context", [True, False])
def test_state_dict_order_with_every_option_on_equals_the_module(context):
    cfg, _, sd, _, _, img_h = all_on_inputs(context, attention_dropout=0.5)
    kw = {k: cfg[k] for k in list(ALL_ON) + ["attention_dropout"] if k in cfg}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = CoVA(cfg["roi_output_size"], img_h, cfg["n_classes"], context, cfg["hidden_dim"], cfg["bbox_hidden_dim"],
                 cfg["n_additional_feat"], cfg["drop_prob"], None, **kw)
    spec = weights.state_dict_spec(**{k: v for k, v in cfg.items() if k not in ("drop_prob", "attention_dropout")})
    assert list(m.state_dict()) == [k for k, _ in spec] == list(sd)
    assert [tuple(v.shape) for v in m.state_dict().values()] == [tuple(s) for _, s in spec]
    order = [k.split(".")[0] for k in sd]
    firsts = [order.index(p) for p in (["gat"] if context else []) + ["page_readout", "page_attention", "decoder"]]
    assert firsts == sorted(firsts)
