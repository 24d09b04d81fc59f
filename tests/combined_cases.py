"""The inputs, the float64 reference and the comparator that tests/test_combined_head_gpu.py holds the head with several
page layers on to, kept apart from it so that tests/test_combined_head_cpu.py can show without a GPU that the reference
alone is inside the bounds and that the comparator rejects the two mistakes the GPU test exists for.  No GPU is needed here.

The head alone: the visual columns are GIVEN (a table and row ids, the cached-feature path of engine.model_fwd), the
reference is oracle.cova_oracle.loss_and_grads in float64 on the same rows through combined_oracle.on_table / .patched.

Bounds (none new): max-abs error over max-abs reference below 1e-5 for everything the forward writes (logits, loss, beta,
lse, the GAT attention rows) and below 1e-4 for every gradient, the bounds of the per-layer kernel tests
(tests/test_page_readout_gpu.py, tests/test_page_attention_gpu.py, tests/test_gatv2_gpu.py); SGEMM_TOL = 2e-5 for the saved
projections P and qkv (tests/test_kernels_gpu.py).  Every gradient tensor is held against ITS OWN largest entry.  The one
exception is the rule tests/test_page_readout_gpu.py states for d_att_b: the bias of a Linear in front of a train-mode
BatchNorm or inside a softmax has a gradient that is a sum of terms which cancel (analytically zero for
bbox_feat_encoder.0.bias, decoder.1.bias and a GATv2 head's attention_layer.bias), so it is held on the larger of its own
scale and the scale of the weight gradient beside it, which is the scale of the terms."""
import contextlib

import numpy as np
import torch

import cova_amd  # noqa: F401
from cova_web_object_detection_amd import weights
from helpers import SGEMM_TOL, load_case, relerr  # noqa: F401  (the suites read SGEMM_TOL from here)
from oracle import cova_oracle as O
import combined_oracle as CO
import page_attn_geo_oracle as PG

FWD_TOL, BWD_TOL = 1e-5, 1e-4
N_VIS = 64                                  # resnet18, roi_output_size (1, 1)
PAGES = (37, 0, 1, 5, 67)                   # an empty page in the middle, a one-box page, a page longer than a 64-row block
K = 6
PAGE_SIZE = (PG.PAGE_H, PG.PAGE_W)          # (height, width): not square
P_DROP = 0.5
# F = 64 + bbox + additional.  "odd": F = 74, F + D = 86, F + D + G = 99, T = 107 (without context 74, 87, 95): no offset is a
# multiple of 4 and T is odd, so every row of comb / dcomb is unaligned.  "vec4": 76, 92, 108, 140 (76, 92, 124): all are.
WIDTHS = {"odd": dict(bbox_hidden_dim=7, n_additional_feat=3, hidden_dim=12, G=13, E=8, Hh=2),
          "vec4": dict(bbox_hidden_dim=8, n_additional_feat=4, hidden_dim=16, G=16, E=32, Hh=1)}
PAGE_LAYERS = {"readout": (True, False, False), "attention": (False, True, False), "both": (True, True, False),
               "both+geo": (True, True, True)}
SUM_BIASES = ("attention_layer.bias", "bbox_feat_encoder.0.bias", "decoder.1.bias")
HEAD_KEYS = ("bbox_feat_encoder.", "bn_additional_feat.", "gat.", "page_readout.", "page_attention.", "decoder.")


def matrix():
    """(context, attention, edge, page layers): {static, gatv2} x {edge off, on} x the four page-layer sets with a GAT, the
    four page-layer sets without one (no heads: neither a scoring mode nor an edge term exists there)."""
    rows = [(True, a, e, p) for a in ("gat", "gatv2") for e in (False, True) for p in PAGE_LAYERS]
    return rows + [(False, "gat", False, p) for p in PAGE_LAYERS]


def case_id(row):
    context, attention, edge, page = row
    return "%s-%s" % (("%s%s" % (attention, "+edge" if edge else "")) if context else "nocontext", page)


def context_table(rs, sizes, k=K):
    """int64 [N, k] batch-global ids inside the row's page, -1 pads behind them; every row has a neighbour, the first row
    of every page lists ITSELF, every third row has pads."""
    rows, lo = [], 0
    for n in sizes:
        for i in range(n):
            valid = k if i % 3 else int(rs.randint(1, k))
            ids = lo + rs.randint(0, n, valid)
            if i == 0:
                ids[0] = lo
            rows.append(np.concatenate([ids, np.full(k - valid, -1)]))
        lo += n
    return np.asarray(rows, np.int64).reshape(-1, k)


def boxes_with_area(sizes, seed):
    """page_attn_geo_oracle.planted_boxes (identical boxes, far corners) with its box of no area made one pixel square: the
    positional encoder divides a box's width by its height."""
    b = PG.planted_boxes(sizes, seed)
    flat = (b[:, 3] <= b[:, 1]) | (b[:, 4] <= b[:, 2])
    b[flat, 3:] = b[flat, 1:3] + 1.0
    assert (b[:, 3] > b[:, 1]).all() and (b[:, 4] > b[:, 2]).all()
    return b


def build_case(width, row, seed=3):
    """Everything of one configuration, on the host: cfg (the engine's), ocfg (the oracle's), sd (float32, seeded; the two
    zero-initialised weights get seeded non-zero values), the inputs and the forced decoder masks."""
    context, attention, edge, page = row
    w = WIDTHS[width]
    readout, attn, geo = PAGE_LAYERS[page]
    G, E = (w["G"] if readout else 0), (w["E"] if attn else 0)
    cfg = dict(roi_output_size=(1, 1), n_classes=4, use_context=context, hidden_dim=w["hidden_dim"],
               bbox_hidden_dim=w["bbox_hidden_dim"], n_additional_feat=w["n_additional_feat"], drop_prob=P_DROP,
               page_context_dim=G, page_attention_dim=E, page_attention_heads=w["Hh"] if attn else 1,
               page_attention_geometry=geo, page_size=PAGE_SIZE)
    if context:
        cfg.update(n_heads=2, n_gat_layers=2, attention=attention, edge_geometry=edge)
    sd = weights.seeded_state_dict(seed, logit_gain=2.0, **{k: v for k, v in cfg.items() if k not in ("drop_prob", "page_size")})
    rs = np.random.RandomState(seed + 1)
    for k in sd:
        if k.endswith(CO.EDGE) or k == CO.GEO_KEY:
            sd[k] = torch.from_numpy(rs.uniform(-2, 2, tuple(sd[k].shape)).astype(np.float32))
    N = sum(PAGES)
    F = N_VIS + cfg["bbox_hidden_dim"] + cfg["n_additional_feat"]
    D = cfg["hidden_dim"] if context else 0
    T = F + D + G + E
    table = rs.standard_normal((N + 3, N_VIS)).astype(np.float32)
    row_ids = ((np.arange(N) * 7 + 2) % (N + 3)).astype(np.int32)             # neither the identity nor a permutation of it
    masks = [(rs.uniform(size=(N, T)) > P_DROP).astype(np.uint8) for _ in range(2)]
    return dict(width=width, row=row, cfg=cfg, ocfg=dict(cfg, use_context=True), sd=sd, N=N, F=F, D=D, G=G, E=E, T=T,
                heads=cfg["page_attention_heads"], table=torch.from_numpy(table), row_ids=torch.from_numpy(row_ids),
                visual=torch.from_numpy(table[row_ids]), bboxes=torch.from_numpy(boxes_with_area(PAGES, seed + 2)),
                additional=torch.from_numpy(rs.standard_normal((N, cfg["n_additional_feat"])).astype(np.float32)),
                ctx=torch.from_numpy(context_table(rs, PAGES)), labels=torch.from_numpy(rs.randint(0, 4, N)),
                page_start=torch.from_numpy(np.concatenate([[0], np.cumsum(PAGES)]).astype(np.int64)),
                masks=[torch.from_numpy(m) for m in masks])


@contextlib.contextmanager
def stated(gat, gat_stack, visual=None, any_dtype=False):
    """oracle.cova_oracle with the composed head's replacements (and, with ``visual``, a given table in front of it; with
    ``any_dtype`` a RoIPool that a float64 run of the whole model can pass through)."""
    saved = {k: getattr(O, k) for k in ("gat", "gat_stack", "convnet", "roi_pool")}
    O.gat, O.gat_stack = gat, gat_stack
    if visual is not None:
        O.convnet, O.roi_pool = CO.on_table(visual)
    elif any_dtype:
        O.roi_pool = CO.roi_pool_in_dtype
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(O, k, v)


def f64(t):
    return t.double() if t.is_floating_point() else t


def reference(case, training=True, routing=None, sd=None, gat_stack=None):
    """The float64 statement of the head of ``case``: train mode with the case's decoder masks (loss and every gradient) or
    eval mode (forward only) -> dict(logits, loss, grads, inter).  ``gat_stack``(good) -> a replacement for the composed
    stack (the CPU test plants its mistakes there)."""
    sd = {k: f64(v) for k, v in (sd or case["sd"]).items()}
    tap = {}
    gat, stack = CO.patched(case["page_start"], case["bboxes"], PAGE_SIZE, case["heads"], tap=tap)
    if gat_stack is not None:
        stack = gat_stack(stack)
    images = torch.zeros((len(PAGES), 3) + PAGE_SIZE, dtype=torch.float64)          # read for their height only
    inputs = (images, case["bboxes"].double(), case["additional"].double(), case["ctx"])
    with stated(gat, stack, case["visual"].double()):
        if training:
            masks = [m.double() for m in case["masks"]]
            loss, logits, grads, _, _ = O.loss_and_grads(sd, *inputs, case["labels"], case["ocfg"], masks, routing)
            grads = {k: g for k, g in grads.items() if k.startswith(HEAD_KEYS)}
        else:
            logits, loss, grads = O.forward(O.clone_state_dict(sd), *inputs, case["ocfg"], False).detach(), None, {}
    inter = {"attn/" + p: a.detach() for p, a in tap["attn"].items()}
    if "readout" in tap:
        inter["readout/beta"], inter["readout/P"] = tap["readout"][0].detach(), tap["readout"][3].detach()
    if "page_attn" in tap:
        inter["page_attn/lse"], inter["page_attn/qkv"] = tap["page_attn"][1].detach(), tap["page_attn"][2].detach()
    return dict(logits=logits, loss=loss, grads=grads, inter=inter)


def grad_scale(key, grads_ref):
    """None (the tensor's own largest entry), or for a bias whose gradient is a sum of cancelling terms the larger of its
    own scale and its weight's (module docstring)."""
    if not key.endswith(SUM_BIASES):
        return None
    weight = key[:-len("bias")] + "weight"
    return max(float(grads_ref[key].abs().max()), float(grads_ref[weight].abs().max()))


def head_errors(got, ref):
    """{what: error} of everything ``ref`` holds; ``got`` must hold it all."""
    errs = {"logits": relerr(got["logits"], ref["logits"])}
    if ref["loss"] is not None:
        errs["loss"] = abs(float(got["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    for k, v in ref["inter"].items():
        errs[k] = relerr(got["inter"][k], v)
    assert set(got["grads"]) >= set(ref["grads"]), sorted(set(ref["grads"]) - set(got["grads"]))
    for k, g in ref["grads"].items():
        errs["grad/" + k] = relerr(got["grads"][k].reshape(g.shape), g, grad_scale(k, ref["grads"]))
    return errs


def bound(what):
    return BWD_TOL if what.startswith("grad/") else SGEMM_TOL if what.endswith(("/P", "/qkv")) else FWD_TOL


def check_head(got, ref, what):
    """Print the worst forward and backward error, then hold every entry to its bound."""
    errs = head_errors(got, ref)
    fwd = max((e, k) for k, e in errs.items() if not k.startswith("grad/"))
    bwd = max([(e, k) for k, e in errs.items() if k.startswith("grad/")] or [(0.0, "-")])
    print("%s: worst forward %.2e (%s), worst gradient %.2e (%s)" % (what, fwd[0], fwd[1], bwd[0], bwd[1]))
    for k, e in errs.items():
        assert e < bound(k), (what, k, e)
    return errs


# ---------------------------------------------------------------- the whole model (cova_h64_n11 inputs)
ALL_ON = dict(n_heads=2, n_gat_layers=2, attention="gatv2", edge_geometry=True, page_context_dim=16, page_attention_dim=8,
              page_attention_heads=2, page_attention_geometry=True)


def doubled_page():
    """The cova_h64_n11 inputs as tests/test_page_readout_gpu.py uses them: the one page given twice, the last five boxes
    moved to the copy."""
    fx, cfg, _, b = load_case("cova_h64_n11")
    b = dict(b, images=b["images"].repeat(2, 1, 1, 1).contiguous(), bboxes=b["bboxes"].clone())
    b["bboxes"][6:, 0] = 1.0
    return fx, cfg, b


def all_on_inputs(context, fresh=False, **extra):
    """-> (cfg, ocfg, sd with seeded non-zero edge / geometry weights (``fresh``: the zeros of a new model), batch,
    page_start, img_h)"""
    fx, cfg, b = doubled_page()
    on = dict(ALL_ON) if context else {k: v for k, v in ALL_ON.items() if k.startswith("page_")}
    cfg = dict(cfg, use_context=context, **dict(on, **extra))
    wcfg = {k: v for k, v in cfg.items() if k not in ("drop_prob", "attention_dropout")}
    seed = int(fx["meta/seed"])
    sd = weights.seeded_state_dict(seed, logit_gain=float(fx["meta/logit_gain"]), **wcfg)
    rs = np.random.RandomState(seed + 1)
    for k in sd:
        if k.endswith(CO.EDGE) or k == CO.GEO_KEY:
            assert not sd[k].any()
            if not fresh:
                sd[k] =torch.from_numpy(rs.uniform(-2, 2, tuple(sd[k].shape)).astype(np.float32))
    ps = torch.searchsorted(b["bboxes"][:, 0].contiguous(), torch.arange(3, dtype=torch.float32))
    assert ps.tolist() == [0, 6, 11]
    return cfg, dict(cfg, use_context=True), sd, b, ps, int(fx["meta/img_h"])
