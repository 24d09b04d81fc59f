"""GPU tests of the edge-geometry extension: cova_edge_geometry bit for bit against the numpy oracle (tests/edge_oracle.py),
cova_gat_fwd_edge / cova_gat_bwd_edge against the torch oracle in float64, the zero-weight identity with cova_gat_fwd / _bwd,
pads and reproducibility, the modules under autograd, and HotPathTrainer with the option on.

Bounds: the project's own for this layer (tests/test_model_gpu.py::test_gat_layer_matches_reference_fixture): max-abs error
over max-abs reference below 1e-5 for h' and attn, below 1e-4 for every gradient (d_edge_w included); the whole model on the
cova_h64_n11 inputs keeps tests/test_model_gpu.py's LOGIT_TOL / LOSS_TOL / GRAD_TOL."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import _lib, engine, weights  # noqa: E402
from cova_web_object_detection_amd.evaluation import evaluate_split, fit  # noqa: E402
from cova_web_object_detection_amd.features import FeatureCache  # noqa: E402
from cova_web_object_detection_amd.models import CoVA, GraphAttentionLayer, MultiHeadGraphAttention  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset, attention_rows  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
from helpers import (compare_grads, DEV, GRAD_TOL, GUARD, load_case,  # noqa: E402
                     LOGIT_TOL, LOSS_TOL, profiled, random_xyxy, relerr, routing_from_saved)
from oracle import cova_oracle as O  # noqa: E402
import edge_oracle as EO  # noqa: E402
import graph_oracle as GO  # noqa: E402
from config_cases import SPLIT_CFG as CFG  # noqa: E402
from gat_cases import EDGE_W  # noqa: E402
from trainer_cases import five_steps, page_set, seeded  # noqa: E402

NEW = ("cova_edge_geometry", "cova_gat_fwd_edge", "cova_gat_bwd_edge")
PAGE = (1280.0, 1280.0)                                   # (height, width) of the kernel tests' pages
random_boxes = functools.partial(random_xyxy, size=1280.0, max_wh=300)


def as_batch(pages):
    ps = np.concatenate([[0], np.cumsum([p.shape[0] for p in pages])]).astype(np.int64)
    bb = [np.concatenate([np.full((p.shape[0], 1), i, np.float32), p.reshape(-1, 4)], 1) for i, p in enumerate(pages)]
    return np.concatenate(bb, 0).astype(np.float32), ps


# ---------------------------------------------------------------- 1. phi through the C ABI
@functools.lru_cache(maxsize=None)
def phi_batch():
    """Pages of 0, 1, 2, 25, 0, 65 boxes: the 25-box page on half-pixel coordinates, the last page with identical boxes,
    points, segments and a pair of coincident points (uni == 0)."""
    rs = np.random.RandomState(31)
    pages = [random_boxes(rs, n) for n in (0, 1, 2, 25, 0, 65)]
    pages[3] = (np.round(pages[3] * 2) / 2).astype(np.float32)
    last = pages[5]
    last[4] = last[3]
    last[40] = last[3]                                    # identical boxes, near and far in DOM order
    last[10, 2:] = last[10, :2]                           # a point
    last[11] = last[10]                                   # ... twice
    last[20, 2] = last[20, 0]                             # a vertical segment
    return as_batch(pages)


def run_phi(bboxes, ctx, page=PAGE):
    """cova_edge_geometry into a buffer framed by guard rows; every value of phi must have been written."""
    N, K = ctx.shape
    bb = torch.from_numpy(np.ascontiguousarray(bboxes)).to(DEV)
    buf = torch.full((N + 4, K, 8), GUARD, dtype=torch.float32, device=DEV)
    engine.call("cova_edge_geometry", bb, torch.from_numpy(np.ascontiguousarray(ctx)).to(DEV), N, K, float(page[1]),
                float(page[0]), buf[2:])
    host = buf.cpu().numpy()
    assert (host[:2] == GUARD).all() and (host[N + 2:] == GUARD).all()
    return host[2:N + 2]


@functools.lru_cache(maxsize=None)
def phi_table(name):
    bb, ps = phi_batch()
    N = bb.shape[0]
    if name == "window12":
        ctx = GO.batch_graph(bb, ps, 12, 0)
    elif name == "spatial24":
        ctx = GO.batch_graph(bb, ps, 0, 24)
    else:                                                 # K = 100: arbitrary ids, an all-pad row, an id >= N
        rs = np.random.RandomState(8)
        ctx = rs.randint(-1, N, (N, 100)).astype(np.int64)
        ctx[6] = -1
        ctx[9, 5] = N
        ctx[9, 6] = N + 1000
        base = int(ps[5])
        ctx[base + 3, :3] = [base + 4, base + 40, base + 3]        # identical boxes (and the box itself)
        ctx[base + 10, :2] = [base + 11, base + 20]                # coincident points; a point and a segment
        ctx[0, 0], ctx[N - 1, 0] = N - 1, 0                         # |j - i| > 64
    return ctx, EO.edge_features(bb, ctx, PAGE[1], PAGE[0])


@pytest.mark.parametrize("name", ["window12", "spatial24", "k100"])
def test_phi_equals_the_oracle_bit_for_bit(name):
    bb, ps = phi_batch()
    ctx, ref = phi_table(name)
    got = run_phi(bb, ctx)
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.array_equal(got, ref) and np.array_equal(got.view(np.uint32) == 0x80000000, ref.view(np.uint32) == 0x80000000)
    assert np.isfinite(got).all() and (got != GUARD).all()
    if name == "k100":
        base = int(ps[5])
        assert not got[6].any() and not got[9, 5:7].any()                       # pads and ids >= N: eight zeros
        assert got[base + 3, 0, 6] == 1.0 and got[base + 3, 1, 6] == 1.0        # identical boxes: IoU 1
        assert got[base + 10, 0, 6] == 0.0                                      # uni == 0
        assert got[0, 0, 7] == 1.0 and got[-1, 0, 7] == -1.0
    assert np.array_equal(run_phi(bb, ctx), got)


def test_phi_entry_point_refuses_bad_arguments_and_skips_empty_work():
    bb = torch.zeros((4, 5), device=DEV)
    ctx = torch.zeros((4, 6), dtype=torch.int64, device=DEV)
    phi = torch.full((4, 6, 8), GUARD, device=DEV)
    for args in ((bb, ctx, 4, 6, 0.0, 10.0, phi), (bb, ctx, 4, 6, 10.0, -1.0, phi), (bb, None, 4, 6, 10.0, 10.0, phi),
                 (bb, ctx, 4, 2000, 10.0, 10.0, phi), (bb, ctx, 4, 6, 10.0, 10.0, phi.view(-1)[1:])):
        with pytest.raises(_lib.CovaHipError):
            engine.call("cova_edge_geometry", *args)
    engine.call("cova_edge_geometry", None, None, 0, 6, 10.0, 10.0, None)
    engine.call("cova_edge_geometry", None, None, 4, 0, 10.0, 10.0, None)
    torch.cuda.synchronize()
    assert (phi == GUARD).all()


# ---------------------------------------------------------------- 2. forward and backward through the C ABI
def launch(case, edge_w, edge=True):
    """cova_gat_fwd(_edge) + cova_gat_bwd(_edge) on the device copies of a case -> dict of device tensors."""
    N, D, K = case["N"], case["D"], case["K"]
    d = {k: torch.from_numpy(np.ascontiguousarray(case[k])).to(DEV) for k in ("Wh", "aw", "ab", "ctx", "phi", "g")}
    ew = None if edge_w is None else torch.from_numpy(np.asarray(edge_w, np.float32)).to(DEV)
    new = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    s, t, attn, hp = new(N), new(N), new(N, K), new(N, D)
    dWh, ds, dt, daw, dab, dew, du = new(N, 2 * D), new(N), new(N), new(2 * D), new(1), new(8), new(N, K)
    csr = torch.zeros((engine.query("cova_gat_transpose_ints", N, K),), dtype=torch.int32, device=DEV)
    engine.call("cova_gat_transpose", d["ctx"], N, K, csr)
    if edge:
        ws = new(engine.query("cova_gat_edge_workspace_floats", N, K))
        engine.call("cova_gat_fwd_edge", d["Wh"], 2 * D, d["aw"], d["ab"], d["ctx"], d["phi"], ew, N, K, D, 0.2, s, t,
                    attn, hp, D)
        engine.call("cova_gat_bwd_edge", d["g"], D, d["Wh"], 2 * D, s, t, attn, d["ctx"], d["aw"], d["phi"], ew, N, K, D,
                    0.2, dWh, 2 * D, ds, dt, daw, dab, dew, csr, du, ws)
    else:
        engine.call("cova_gat_fwd", d["Wh"], 2 * D, d["aw"], d["ab"], d["ctx"], N, K, D, 0.2, s, t, attn, hp, D)
        engine.call("cova_gat_bwd", d["g"], D, d["Wh"], 2 * D, s, t, attn, d["ctx"], d["aw"], N, K, D, 0.2, dWh, 2 * D,
                    ds, dt, daw, dab, csr, du)
    torch.cuda.synchronize()
    return dict(s=s, t=t, attn=attn, hp=hp, dWh=dWh, daw=daw, dab=dab, dew=dew, du=du)


def oracle64(case, edge_w):
    """tests/edge_oracle.gat in float64 on a random Wh: h = Wh [N, 2D], W_i = [I 0], W_j = [0 I] (exact projections)."""
    N, D = case["N"], case["D"]
    f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    eye = torch.eye(D, dtype=torch.float64)
    zero = torch.zeros((D, D), dtype=torch.float64)
    sd = {"gat.W_i.weight": torch.cat((eye, zero), 1), "gat.W_j.weight": torch.cat((zero, eye), 1),
          "gat.attention_layer.weight": f64(case["aw"]).view(1, 2 * D).requires_grad_(True),
          "gat.attention_layer.bias": f64(case["ab"]).requires_grad_(True),
          "gat.edge_layer.weight": f64(edge_w).view(1, 8).requires_grad_(True)}
    h = f64(case["Wh"]).requires_grad_(True)
    hp, attn = EO.gat(h, torch.from_numpy(case["ctx"]), sd, f64(case["phi"]), return_attn_wts=True)
    (hp * f64(case["g"])).sum().backward()
    return dict(hp=hp.detach().numpy(), attn=attn.detach().numpy(), dWh=h.grad.numpy(),
                daw=sd["gat.attention_layer.weight"].grad.numpy().reshape(-1),
                dab=sd["gat.attention_layer.bias"].grad.numpy(), dew=sd["gat.edge_layer.weight"].grad.numpy().reshape(-1))


@functools.lru_cache(maxsize=None)
def gat_case(name):
    rs = np.random.RandomState({"wide": 41, "general": 42, "hub": 43, "k2": 44}[name])
    if name == "k2":                 # `-cs 1` at hidden_dim 100 (the GAT of tests/golden/cova_roi5_odd at K = 2): ldw = 200,
        from cova_web_object_detection_amd import synthetic      # pages of 11, 70 and 2 boxes, the DOM-order window
        counts = [11, 70, 2]
        N, D, K = sum(counts), 100, 2
        bb, ps = as_batch([random_boxes(rs, n) for n in counts])
        ctx = synthetic.collate_context([synthetic.context_window_indices(n, 1) for n in counts])
        assert int((ctx[:, 1] == -1).sum()) == 2 * len(counts) and (ctx[:, 0] >= 0).all()
    elif name == "wide":              # K <= 64, D = 6 x 64: the wide kernels; a hybrid graph over two pages
        N, D, K = 130, 384, 24
        bb, ps = as_batch([random_boxes(rs, 65), random_boxes(rs, 65)])
        ctx = GO.batch_graph(bb, ps, 6, 12)
    elif name == "general":          # K = 100: the general kernels, two 64-lane passes; arbitrary ids, an all-pad row
        N, D, K = 70, 40, 100
        bb, ps = as_batch([random_boxes(rs, 70)])
        ctx = rs.randint(-1, N, (N, K)).astype(np.int64)
        ctx[17] = -1
    else:                            # one box in every other row: a transposed-index row of 63 edges
        N, D, K = 64, 96, 24
        bb, ps = as_batch([random_boxes(rs, 64)])
        ctx = np.stack([rs.permutation(np.delete(np.arange(N), [5, i] if i != 5 else [5]))[:K] for i in range(N)])
        ctx = ctx.astype(np.int64)
        ctx[:, 0] = 5
        ctx[5, 0] = -1
        assert int((ctx == 5).sum()) == 63
    assert ctx.shape == (N, K)
    case = dict(N=N, D=D, K=K, ctx=ctx, phi=EO.edge_features(bb, ctx, PAGE[1], PAGE[0]),
                Wh=rs.standard_normal((N, 2 * D)).astype(np.float32),
                aw=(rs.standard_normal(2 * D) / np.sqrt(D)).astype(np.float32),
                ab=rs.standard_normal(1).astype(np.float32), g=rs.standard_normal((N, D)).astype(np.float32))
    case["ref"] = oracle64(case, EDGE_W)
    return case


def check_against(got, ref, what):
    errs = {k: relerr(got[k].cpu().numpy().reshape(ref[k].shape), ref[k]) for k in ("hp", "attn", "dWh", "daw", "dab", "dew")}
    print(what, {k: "%.2e" % v for k, v in errs.items()})
    for k in ("hp", "attn"):
        assert errs[k] < 1e-5, (what, k, errs[k])
    for k in ("dWh", "daw", "dab", "dew"):
        assert errs[k] < 1e-4, (what, k, errs[k])


@pytest.mark.parametrize("name", ["wide", "general", "hub", "k2"])
def test_forward_and_backward_match_the_float64_oracle(name):
    case = gat_case(name)
    assert float(np.abs(case["ref"]["dew"]).min()) > 0
    check_against(launch(case, EDGE_W), case["ref"], name)
    # the term is live: without it the attention is another one, far outside the bound
    assert relerr(launch(case, None, edge=False)["attn"].cpu().numpy(), case["ref"]["attn"]) > 1e-3


@pytest.mark.parametrize("name", ["wide", "general", "hub", "k2"])
def test_zero_edge_weight_is_the_plain_layer_bit_for_bit(name):
    case = gat_case(name)
    zero = np.zeros(8, np.float32)
    e, p = launch(case, zero), launch(case, None, edge=False)
    for k in ("s", "t", "attn", "hp", "dWh", "daw", "dab", "du"):
        assert torch.equal(e[k], p[k]), k
    ref = oracle64(case, zero)
    assert float(e["dew"].abs().min()) > 0
    assert relerr(e["dew"].cpu().numpy(), ref["dew"]) < 1e-4


def test_pad_rows_and_reproducibility():
    case = gat_case("general")
    a, b = launch(case, EDGE_W), launch(case, EDGE_W)
    K = case["K"]
    assert np.allclose(a["attn"][17].cpu().numpy(), 1.0 / K) and float(a["hp"][17].abs().max()) == 0.0
    assert float(a["du"][17].abs().max()) == 0.0 and not case["phi"][17].any()      # nothing of the row reaches d_edge_w
    assert torch.equal(a["du"].cpu()[torch.from_numpy(case["ctx"]) < 0], torch.zeros(int((case["ctx"] < 0).sum())))
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for name in ("wide", "hub"):
        c = gat_case(name)
        assert torch.equal(launch(c, EDGE_W)["dew"], launch(c, EDGE_W)["dew"])
    # several blocks of partials (N * K > 4096 slots) against the same sum in float64
    du, phi = a["du"].cpu().numpy().astype(np.float64), case["phi"].astype(np.float64)
    assert case["N"] * K > 4096
    assert relerr(a["dew"].cpu().numpy(), np.einsum("nk,nke->e", du, phi)) < 1e-5


def test_edge_entry_points_refuse_bad_arguments():
    case = gat_case("hub")
    N, D, K = case["N"], case["D"], case["K"]
    z = lambda *shape: torch.zeros(shape, device=DEV)
    ctx = torch.from_numpy(case["ctx"]).to(DEV)
    with pytest.raises(_lib.CovaHipError):                                      # no phi
        engine.call("cova_gat_fwd_edge", z(N, 2 * D), 2 * D, z(2 * D), z(1), ctx, None, z(8), N, K, D, 0.2, z(N), z(N),
                    z(N, K), z(N, D), D)
    with pytest.raises(_lib.CovaHipError):                                      # the scatter form (no csr) is not extended
        engine.call("cova_gat_bwd_edge", z(N, D), D, z(N, 2 * D), 2 * D, z(N), z(N), z(N, K), ctx, z(2 * D), z(N, K, 8),
                    z(8), N, K, D, 0.2, z(N, 2 * D), 2 * D, z(N), z(N), z(2 * D), z(1), z(8), None, z(N, K), z(64))
    assert engine.query("cova_gat_edge_workspace_floats", 70, 100) == 16
    assert engine.query("cova_gat_edge_workspace_floats", 0, 24) == 0


# ---------------------------------------------------------------- 3. the modules
def test_edge_aware_layer_under_autograd_matches_the_oracle():
    rs = np.random.RandomState(13)
    N, Fd, D = 131, 24, 8
    bb = np.concatenate([np.zeros((N, 1), np.float32), GO.tie_grid()], 1)     # integer coordinates; box 130 covers the others
    ctx_np = GO.batch_graph(bb, [0, N], 2, 6)
    torch.manual_seed(11)
    layer = GraphAttentionLayer(Fd, D, edge_geometry=True)
    assert list(dict(layer.named_parameters())) == ["W_i.weight", "W_j.weight", "attention_layer.weight",
                                                    "attention_layer.bias", "edge_layer.weight"]
    assert not layer.edge_layer.weight.detach().any()                          # zero at construction
    with torch.no_grad():
        layer.edge_layer.weight.copy_(torch.from_numpy(EDGE_W).view(1, 8))
    sd = {"gat." + k: v.detach().clone().double().requires_grad_(True) for k, v in layer.state_dict().items()}
    h_host = torch.from_numpy(rs.standard_normal((N, Fd)).astype(np.float32))
    g_host = torch.from_numpy(rs.standard_normal((N, D)).astype(np.float32))
    layer = layer.to(DEV)
    h, ctx, boxes = h_host.to(DEV).requires_grad_(True), torch.from_numpy(ctx_np).to(DEV), torch.from_numpy(bb).to(DEV)
    with pytest.raises(ValueError, match="bboxes"):
        layer(h, ctx)
    with pytest.raises(ValueError, match="page_size"):
        layer(h, ctx, bboxes=boxes)
    hp, attn = layer(h, ctx, return_attn_wts=True, bboxes=boxes, page_size=(300, 500))
    (hp * g_host.to(DEV)).sum().backward()
    assert layer(h, ctx, bboxes=boxes, page_size=(300, 500)).shape == (N, D)
    phi = torch.from_numpy(EO.edge_features(bb, ctx_np, 500, 300)).double()
    h_ref = h_host.double().requires_grad_(True)
    hp_ref, attn_ref = EO.gat(h_ref, torch.from_numpy(ctx_np), sd, phi, return_attn_wts=True)
    (hp_ref * g_host.double()).sum().backward()
    assert relerr(hp.detach().cpu(), hp_ref.detach()) < 1e-5
    assert relerr(attn.cpu(), attn_ref.detach()) < 1e-5
    assert relerr(h.grad.cpu(), h_ref.grad) < 1e-4
    for key, p in layer.named_parameters():
        assert relerr(p.grad.cpu(), sd["gat." + key].grad) < 1e-4, key
    # a plain layer takes the defaulted keywords and ignores them; the multi-head module computes phi once
    plain = GraphAttentionLayer(Fd, D).to(DEV)
    assert torch.equal(plain(h, ctx), plain(h, ctx, False, bboxes=boxes, page_size=(300, 500)))
    multi = MultiHeadGraphAttention(Fd, D, 2, 2, edge_geometry=True).to(DEV)
    with pytest.raises(ValueError):
        multi(h, ctx)
    out, lens = profiled(lambda: multi(h, ctx, bboxes=boxes, page_size=(300, 500)))
    assert out.shape == (N, D) and lens["cova_edge_geometry"] == 1 and lens["cova_gat_fwd_edge"] == 4


def edge_gates(sv, routing):
    """routing_from_saved's LeakyReLU decisions, restated with the edge term the HIP forward added to u."""
    for layer in sv["gat"]:
        for head in layer["heads"]:
            ctx = head["ctx"]
            t = torch.cat((head["t"], head["t"].new_zeros(1))).double()
            u = head["s"].double().view(-1, 1) + t[ctx.clamp(min=-1)]
            w = sv["params"][head["prefix"] + "edge_layer.weight"].double().view(-1)
            u = u.float().double() + (head["phi"].double() * w).sum(-1)
            routing["gate_" + head["prefix"] + "leaky"] = (u > 0).cpu()
    return routing


def test_edge_aware_model_matches_the_oracle_on_the_reference_inputs(monkeypatch):
    fx, cfg, _, batch = load_case("cova_h64_n11")
    cfg = dict(cfg, n_heads=2, n_gat_layers=2, edge_geometry=True)
    wcfg = {k: v for k, v in cfg.items() if k != "drop_prob"}
    sd = weights.seeded_state_dict(int(fx["meta/seed"]), logit_gain=float(fx["meta/logit_gain"]), **wcfg)
    rs = np.random.RandomState(19)
    edge_keys = [k for k in sd if k.endswith("edge_layer.weight")]
    assert len(edge_keys) == 4
    for k in edge_keys:
        sd[k] = torch.from_numpy(rs.uniform(-2, 2, (1, 8)).astype(np.float32))
    img_h = int(fx["meta/img_h"])
    page = tuple(batch["images"].shape[2:])
    monkeypatch.setattr(O, "gat", EO.patched_gat(batch["bboxes"], page))
    b = batch
    args = [b[k].to(DEV) for k in ("images", "bboxes", "additional_feats", "context_indices")]

    def build():
        m = CoVA(cfg["roi_output_size"], img_h, cfg["n_classes"], cfg["use_context"], cfg["hidden_dim"],
                 cfg["bbox_hidden_dim"], cfg["n_additional_feat"], cfg["drop_prob"], None, n_heads=2, n_gat_layers=2,
                 edge_geometry=True)
        assert [k for k in m.state_dict()] == list(sd)
        assert all(not m.state_dict()[k].any() for k in edge_keys)            # zero at construction
        missing = m.load_state_dict(sd, strict=True)
        assert not missing.missing_keys and not missing.unexpected_keys
        return m.to(DEV)

    m = build().eval()
    with torch.no_grad():
        logits = m(*args)
    ref = O.forward(O.clone_state_dict(sd), b["images"], b["bboxes"], b["additional_feats"], b["context_indices"], cfg, False)
    assert relerr(logits.cpu(), ref) < LOGIT_TOL
    plain_sd = {k: v for k, v in sd.items() if k not in edge_keys}
    plain_ref = O.forward(O.clone_state_dict(plain_sd), b["images"], b["bboxes"], b["additional_feats"],
                          b["context_indices"], cfg, False)
    assert relerr(plain_ref, ref) > 1e-3                                      # the seeded edge weights change the logits
    m = build().train()
    logits = m(*args)
    sv = logits.grad_fn.sv
    sv["params"] = {k: p.detach() for k, p in m.named_parameters()}
    routing = edge_gates(sv, routing_from_saved(sv))
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(logits, b["labels"].to(DEV))
    loss.backward()
    loss_ref, logits_ref, grads_ref, _, _ = O.loss_and_grads(sd, b["images"], b["bboxes"], b["additional_feats"],
                                                             b["context_indices"], b["labels"], cfg, None, routing)
    assert relerr(logits.detach().cpu(), logits_ref) < LOGIT_TOL
    assert abs(loss.item() - float(loss_ref)) <= LOSS_TOL * abs(float(loss_ref))
    grads = {k: p.grad for k, p in m.named_parameters()}
    assert all(float(grads_ref[k].abs().max()) > 0 for k in edge_keys)
    compare_grads(grads, grads_ref, rtol=GRAD_TOL, outlier_frac=0.0)
    for k in edge_keys:                                  # (compare_grads floors the scale at 1 % of the largest gradient)
        assert relerr(grads[k].cpu(), grads_ref[k]) < 1e-4, k


# ---------------------------------------------------------------- 4. the trainer
ECFG = dict(CFG, edge_geometry=True)


@pytest.mark.parametrize("kw", [dict(), dict(optimizer="adamw", max_grad_norm=1.0,
                                             param_groups=[dict(params="gat.edge_layer.", lr=5e-2, weight_decay=0.0)]),
                                dict(optimizer="sgd", momentum=0.9, lr=1e-3)])
def test_five_steps_move_the_edge_weights_and_are_reproducible(kw):
    u8, rows = page_set()
    ds = DeviceDataset(u8, rows, 2, DEV, spatial_k=6)
    sd = seeded(ECFG)
    assert "gat.edge_layer.weight" in sd and not sd["gat.edge_layer.weight"].any()
    a, b = HotPathTrainer(ECFG, sd, DEV, **kw), HotPathTrainer(ECFG, sd, DEV, **kw)
    assert "gat.edge_layer.weight" in a.params and a.grads["gat.edge_layer.weight"].shape == (1, 8)
    assert engine._adjacent(a.params["gat.W_i.weight"], a.params["gat.W_j.weight"])
    la, sa = five_steps(a, ds)
    lb, sb = five_steps(b, ds)
    assert la == lb and list(sa) == list(sb)
    for key in sa:
        assert torch.equal(sa[key], sb[key]), key
    w = sa["gat.edge_layer.weight"]
    assert w.shape == (1, 8) and bool(torch.isfinite(w).all()) and float(w.abs().min()) > 0      # off zero, every feature
    # checkpoint round trip: parameters, moments and step count into a fresh trainer, then one more identical step
    c = HotPathTrainer(ECFG, sd, DEV, **kw)
    c.load_state_dict(a.state_dict())
    c.load_optimizer_state_dict(a.optimizer_state_dict())
    batch = next(iter(ds.batches(3, prefetch=False)))
    assert float(a.train_step(batch)[0]) == float(c.train_step(batch)[0])
    assert torch.equal(a.params["gat.edge_layer.weight"], c.params["gat.edge_layer.weight"])
    assert torch.equal(a.pbucket.flat, c.pbucket.flat)


def test_frozen_zero_edge_weights_train_like_the_plain_model_bit_for_bit():
    u8, rows = page_set()
    ds = DeviceDataset(u8, rows, 2, DEV, spatial_k=6)
    plain = HotPathTrainer(CFG, seeded(CFG), DEV)
    edge = HotPathTrainer(ECFG, seeded(ECFG), DEV, frozen=("gat.edge_layer.weight",))
    lp, sp = five_steps(plain, ds)
    le, se = five_steps(edge, ds)
    assert lp == le and [k for k in se if k not in sp] == ["gat.edge_layer.weight"]
    assert not se["gat.edge_layer.weight"].any()
    for key in sp:
        assert torch.equal(sp[key], se[key]), key
    assert not torch.equal(sp["gat.W_i.weight"], seeded(CFG)["gat.W_i.weight"].to(DEV))          # the steps did train
    assert float(edge.grads["gat.edge_layer.weight"].abs().max()) > 0          # the gradient is there, the optimizer skips it


def test_default_step_issues_none_of_the_new_launches():
    u8, rows = page_set(P=3)
    batch = next(iter(DeviceDataset(u8, rows, 2, DEV, spatial_k=6).batches(3, prefetch=False)))
    _, plain = profiled(lambda: HotPathTrainer(CFG, seeded(CFG), DEV).train_step(batch))
    assert not any(n in plain for n in NEW + ("cova_gat_edge_workspace_floats",))
    assert plain["cova_gat_fwd"] == 1 and plain["cova_gat_bwd"] == 1
    cfg = dict(ECFG, n_heads=2, n_gat_layers=2)
    _, edge = profiled(lambda: HotPathTrainer(cfg, seeded(cfg), DEV).train_step(batch))
    assert edge["cova_edge_geometry"] == 1 and edge["cova_gat_fwd_edge"] == 4 and edge["cova_gat_bwd_edge"] == 4
    assert "cova_gat_fwd" not in edge and "cova_gat_bwd" not in edge
    rest = lambda d: {k: v for k, v in d.items() if "gat_fwd" not in k and "gat_bwd" not in k and k != "cova_edge_geometry"
                      and k != "cova_sgemm"}
    _, plain22 = profiled(lambda: HotPathTrainer(dict(CFG, n_heads=2, n_gat_layers=2),
                                                 seeded(dict(CFG, n_heads=2, n_gat_layers=2)), DEV).train_step(batch))
    assert rest(edge) == rest(plain22) and edge["cova_sgemm"] == plain22["cova_sgemm"]


def test_evaluate_split_fit_from_a_feature_cache_and_attention_rows_with_the_option_on():
    u8, rows = page_set(P=9, seed=4)
    v8, vrows = page_set(P=11, seed=9)
    train, val = DeviceDataset(u8, rows, 2, DEV, spatial_k=6), DeviceDataset(v8, vrows, 2, DEV, spatial_k=6)
    sd = seeded(ECFG)
    sd["gat.edge_layer.weight"] = torch.from_numpy(EDGE_W).view(1, 8).clone()
    tr = HotPathTrainer(ECFG, sd, DEV, track_metrics=True, frozen=("convnet.",), bn_eval=("convnet.",))
    rep = evaluate_split(tr, val, with_loss=True)
    assert rep.evaluated.all() and rep.ranks.shape == (11, 3) and np.isfinite(rep.loss)
    tcache, vcache = FeatureCache.build(tr, train), FeatureCache.build(tr, val)
    cached, full = next(iter(val.batches(11, features=vcache))), next(iter(val.batches(11, prefetch=False)))
    assert "images" not in cached and cached["page_size"] == (96, 96) == tuple(full["images"].shape[2:])
    assert torch.equal(tr.predict(cached)[0], tr.predict(full)[0])             # the page size reaches phi without images
    zero = HotPathTrainer(ECFG, seeded(ECFG), DEV)
    assert not torch.equal(tr.predict(full)[0], zero.predict(full)[0])
    assert torch.equal(zero.predict(full)[0], HotPathTrainer(CFG, seeded(CFG), DEV).predict(full)[0])
    bad = dict(cached)
    del bad["page_size"]
    with pytest.raises(ValueError, match="page_size"):
        tr.predict(bad)
    before = tr.params["gat.edge_layer.weight"].clone()
    out = fit(tr, train, val, 1, 3, sampling_fraction=0.9, seed=12, eval_interval=1, train_features=tcache,
              val_features=vcache)
    assert len(out.history) == 1 and out.history[0]["eval_acc"] is not None and tr.step_count == 3
    assert not torch.equal(tr.params["gat.edge_layer.weight"], before)
    rows_out = attention_rows(tr, full)
    K = full["context_indices"].shape[1]
    assert rows_out.shape == (int((full["labels"] > 0).sum()), 5 + 5 * K) and bool(torch.isfinite(rows_out).all())
