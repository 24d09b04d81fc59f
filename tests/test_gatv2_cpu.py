"""Host side of the GATv2 scoring mode (no GPU): the parameter list with the option off and on, the torch oracle
(tests/gatv2_oracle.py) on the property the mode exists for -- two boxes ranking one neighbour set differently, which the
static score cannot do --, the oracle's gradients against torch.autograd.gradcheck, and the option / shape-mismatch errors
of the spec, the modules, the engine and the trainer."""
import warnings

import numpy as np
import pytest
import torch

import cova_amd  # noqa: F401
from cova_web_object_detection_amd import _lib, engine, weights
from cova_web_object_detection_amd.models import CoVA, GraphAttentionLayer, MultiHeadGraphAttention
from cova_web_object_detection_amd.trainer import HotPathTrainer

import gatv2_oracle as G2
from oracle import cova_oracle as O
from config_cases import SPLIT_CFG


# ---------------------------------------------------------------- the parameter list
def test_default_spec_is_unchanged_key_for_key():
    base = weights.state_dict_spec()
    assert len(base) == 50                                                       # the reference's state_dict
    assert weights.state_dict_spec(attention="gat") == base
    assert dict(base)["gat.attention_layer.weight"] == (1, 768)
    for kw in (dict(n_heads=2, n_gat_layers=2), dict(edge_geometry=True), dict(backbone="resnet50")):
        assert weights.state_dict_spec(attention="gat", **kw) == weights.state_dict_spec(**kw)


@pytest.mark.parametrize("kw", [dict(), dict(n_heads=2, n_gat_layers=2, edge_geometry=True), dict(hidden_dim=64, n_heads=4)])
def test_v2_spec_changes_the_attention_weight_shape_only(kw):
    base, v2 = weights.state_dict_spec(**kw), weights.state_dict_spec(attention="gatv2", **kw)
    assert [k for k, _ in v2] == [k for k, _ in base]                            # keys and their order
    changed = [(k, a, b) for (k, a), (_, b) in zip(base, v2) if a != b]
    heads = [p for layer in weights.gat_prefixes(kw.get("n_heads", 1), kw.get("n_gat_layers", 1)) for p in layer]
    dh = kw.get("hidden_dim", 384) // kw.get("n_heads", 1)
    assert changed == [(p + "attention_layer.weight", (1, 2 * dh), (1, dh)) for p in heads]
    sd = weights.seeded_state_dict(3, attention="gatv2", **kw)                   # no special case in the generator
    assert [tuple(sd[k].shape) for k, _ in v2] == [tuple(s) for _, s in v2]
    assert all(float(sd[p + "attention_layer.weight"].abs().min()) > 0 for p in heads)
    assert weights.state_dict_spec(use_context=False, attention="gatv2") == weights.state_dict_spec(use_context=False)


def test_unknown_attention_modes_are_refused():
    for bad in ("GATv2", "v2", None, True, 2):
        with pytest.raises(ValueError, match="attention"):
            weights.state_dict_spec(attention=bad)
    with pytest.raises(ValueError, match="attention"):
        GraphAttentionLayer(8, 4, attention="dynamic")
    with pytest.raises(ValueError, match="attention"):
        MultiHeadGraphAttention(8, 4, 2, 1, attention="dynamic")
    with pytest.raises(ValueError, match="attention"):
        CoVA((3, 3), 64, 4, True, 32, 8, 0, 0.2, None, attention="dynamic")
    assert weights.attention_of(torch.zeros(1, 8), 4) == "gat" and weights.attention_of(torch.zeros(1, 4), 4) == "gatv2"
    with pytest.raises(ValueError, match="attention"):
        weights.attention_of(torch.zeros(1, 5), 4)


def test_header_declares_the_v2_entry_points():
    protos = _lib.parse_header()
    assert len(protos["cova_gat2_fwd"]) == 15 and len(protos["cova_gat2_bwd"]) == 22       # (the stream included)
    assert len(protos["cova_gat2_workspace_floats"]) == 3


# ---------------------------------------------------------------- the oracle: what the mode is for
def ranking_case():
    """D = 2, identity projections: boxes 0 and 1 are the queries, both with the neighbour set (2, 3).
    score(q, n) = lrelu(q_x + n_x) + lrelu(q_y + n_y): box 0 = (-1, 0) scores n2 = (1, 0) with 0 and n3 = (0, 1) with 0.8;
    box 1 = (0, -1) scores n2 with 0.8 and n3 with 0."""
    h = torch.tensor([[-1.0, 0.0], [0.0, -1.0], [1.0, 0.0], [0.0, 1.0]], dtype=torch.float64)
    ctx = torch.tensor([[2, 3], [2, 3], [-1, -1], [-1, -1]], dtype=torch.int64)
    eye = torch.eye(2, dtype=torch.float64)
    return h, ctx, eye


def test_two_queries_rank_one_neighbour_set_differently_and_the_static_score_cannot():
    h, ctx, eye = ranking_case()
    sd = {"gat.W_i.weight": eye, "gat.W_j.weight": eye, "gat.attention_layer.weight": torch.ones(1, 2, dtype=torch.float64),
          "gat.attention_layer.bias": torch.zeros(1, dtype=torch.float64)}
    hp, attn = G2.gat_v2(h, ctx, sd, return_attn_wts=True)
    e = np.exp(0.8)
    assert torch.allclose(attn[0], torch.tensor([1.0, e], dtype=torch.float64) / (1 + e), rtol=1e-12, atol=0)
    assert torch.allclose(attn[1], torch.tensor([e, 1.0], dtype=torch.float64) / (1 + e), rtol=1e-12, atol=0)
    assert attn[0, 1] > attn[0, 0] and attn[1, 0] > attn[1, 1]                   # the winner depends on the query
    assert torch.allclose(attn[2:], torch.full((2, 2), 0.5, dtype=torch.float64)) and not hp[2:].any()      # all-pad rows
    assert torch.allclose(hp[0], attn[0, 0] * h[2] + attn[0, 1] * h[3])
    # the static score LeakyReLU(a_i . Wh_i + a_j . Wh_j + b) on the same inputs: whatever its weights, both queries order
    # the two neighbours alike (a_i . Wh_i is constant within a row, LeakyReLU is monotone)
    rs = np.random.RandomState(0)
    for _ in range(200):
        ssd = {"gat.W_i.weight": eye, "gat.W_j.weight": eye,
               "gat.attention_layer.weight": torch.from_numpy(rs.standard_normal((1, 4)) * 3),
               "gat.attention_layer.bias": torch.from_numpy(rs.standard_normal(1))}
        _, sattn = O.gat(h, ctx, ssd, return_attn_wts=True)
        d0, d1 = float(sattn[0, 0] - sattn[0, 1]), float(sattn[1, 0] - sattn[1, 1])
        assert d0 * d1 >= 0 and (d0 == 0) == (d1 == 0)


def gate_row(z, alpha=0.2):
    return torch.where(z > 0, torch.ones_like(z), alpha * torch.ones_like(z))


def test_signed_zero_takes_the_slope_branch_and_pads_and_out_of_range_ids_are_masked():
    wi = torch.tensor([[1.0, -2.0, 0.5], [-0.0, 0.0, 0.0]], dtype=torch.float64, requires_grad=True)
    wj = torch.tensor([[-1.0, 2.0, 1.0], [-0.0, 0.0, 3.0]], dtype=torch.float64)
    ctx = torch.tensor([[0, 1, -1, 2, 7]], dtype=torch.int64).expand(2, 5).contiguous()
    a = torch.ones(1, 3, dtype=torch.float64)
    _, attn = G2.attend(wi, wj, ctx, a, torch.zeros(1, dtype=torch.float64))
    assert float(attn[:, 2:].detach().abs().max()) == 0.0                               # -1, N and N + 5 are pads
    z = (wi.unsqueeze(1) + wj.unsqueeze(0)).detach()                              # [i, j, d]
    assert z[0, 0].tolist() == [0.0, 0.0, 1.5] and z[1, 1].tolist()[:2] == [0.0, 0.0]
    assert np.signbit(z[1, 1, 0].item()) and not np.signbit(z[1, 1, 1].item())   # -0.0 and +0.0
    # d attn[i,0] / d wi[i,d] = attn0 (1 - attn0) a[d] gate(z[i,0,d]) - attn0 attn1 a[d] gate(z[i,1,d]): the channels at
    # z == +-0 carry the slope 0.2
    for i in (0, 1):
        g = torch.autograd.grad(attn[i, 0], wi, retain_graph=True)[0][i]
        a0, a1 = attn[i, 0].detach(), attn[i, 1].detach()
        assert torch.allclose(g, a0 * (1 - a0) * gate_row(z[i, 0]) - a0 * a1 * gate_row(z[i, 1]), rtol=1e-12, atol=1e-15)
    assert gate_row(z[0, 0]).tolist() == [0.2, 0.2, 1.0] and gate_row(z[1, 1]).tolist() == [0.2, 0.2, 1.0]


def test_oracle_gradients_pass_gradcheck_with_and_without_the_edge_term_and_forced_gates():
    rs = np.random.RandomState(2)
    N, K, D = 7, 5, 4
    f = lambda *s: torch.from_numpy(rs.standard_normal(s)).requires_grad_(True)
    ctx = torch.from_numpy(rs.randint(-1, N, (N, K)).astype(np.int64))
    ctx[3] = -1
    ctx[4, :2] = 4                                                                # a self-loop, twice
    ctx[5, 0] = N + 2
    wi, wj, a, b, ew = f(N, D), f(N, D), f(1, D), f(1), f(1, 8)
    phi = torch.from_numpy(rs.standard_normal((N, K, 8)))
    plain = lambda wi, wj, a, b: G2.attend(wi, wj, ctx, a, b)[0]
    assert torch.autograd.gradcheck(plain, (wi, wj, a, b), eps=1e-6, atol=1e-6)
    edge = lambda wi, wj, a, b, ew: G2.attend(wi, wj, ctx, a, b, 0.2, ew, phi)[0]
    assert torch.autograd.gradcheck(edge, (wi, wj, a, b, ew), eps=1e-6, atol=1e-6)
    attn_of = lambda wi, wj, a, b, ew: G2.attend(wi, wj, ctx, a, b, 0.2, ew, phi)[1]
    assert torch.autograd.gradcheck(attn_of, (wi, wj, a, b, ew), eps=1e-6, atol=1e-6)
    gate = torch.from_numpy(rs.rand(N, K, D) > 0.5)                               # forced decisions: still a smooth function
    forced = lambda wi, wj, a, b: G2.attend(wi, wj, ctx, a, b, gate=gate)[0]
    assert torch.autograd.gradcheck(forced, (wi, wj, a, b), eps=1e-6, atol=1e-6)
    own = (wi.unsqueeze(1) + torch.cat((wj, torch.zeros(1, D, dtype=wj.dtype)))[ctx.clamp(min=-1, max=N).where(
        (ctx >= 0) & (ctx < N), torch.full_like(ctx, N))]) > 0
    assert torch.equal(G2.attend(wi, wj, ctx, a, b, gate=own)[0], G2.attend(wi, wj, ctx, a, b)[0])
    # a zero edge weight is the plain head; through the state_dict interface too
    zero = torch.zeros(1, 8, dtype=torch.float64)
    assert torch.equal(G2.attend(wi, wj, ctx, a, b, 0.2, zero, phi)[1], G2.attend(wi, wj, ctx, a, b)[1])
    h = torch.from_numpy(rs.standard_normal((N, 6)))
    sd = {"gat.W_i.weight": torch.from_numpy(rs.standard_normal((D, 6))), "gat.W_j.weight":
          torch.from_numpy(rs.standard_normal((D, 6))), "gat.attention_layer.weight": a.detach(),
          "gat.attention_layer.bias": b.detach()}
    assert G2.is_v2(sd, "gat.")
    ref = G2.attend(h @ sd["gat.W_i.weight"].T, h @ sd["gat.W_j.weight"].T, ctx, a.detach(), b.detach())[0]
    assert torch.equal(G2.gat_v2(h, ctx, sd), ref)
    assert torch.equal(G2.patched_gat()(h, ctx, sd), ref)                         # the dispatch on the weight's width


# ---------------------------------------------------------------- modules, engine, trainer: shapes and mismatches
CFG = dict(SPLIT_CFG, n_heads=2, n_gat_layers=2)
V2CFG = dict(CFG, attention="gatv2")
seeded = lambda cfg: weights.seeded_state_dict(5, **{k: v for k, v in cfg.items() if k != "drop_prob"})


def build(attention, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return CoVA((3, 3), 64, 4, True, 32, 8, 0, 0.2, None, attention=attention, **kw)


def test_modules_take_a_defaulted_trailing_attention_argument():
    layer = GraphAttentionLayer(12, 8, attention="gatv2")
    assert layer.attention_layer.weight.shape == (1, 8) and layer.attention_layer.bias.shape == (1,)
    assert list(dict(layer.named_parameters())) == ["W_i.weight", "W_j.weight", "attention_layer.weight",
                                                    "attention_layer.bias"]
    assert GraphAttentionLayer(12, 8).attention_layer.weight.shape == (1, 16) and GraphAttentionLayer(12, 8).attention == "gat"
    multi = MultiHeadGraphAttention(12, 8, 2, 2, True, "gatv2")
    assert all(h.attention == "gatv2" and h.edge_geometry and h.attention_layer.weight.shape == (1, 4)
               for l in multi.layers for h in l.heads)
    ref = build("gat")                                                            # the reference's nine-argument call
    assert ref._cfg["attention"] == "gat"
    assert [(k, tuple(v.shape)) for k, v in ref.state_dict().items()] == [(k, tuple(s)) for k, s in
                                                                          weights.state_dict_spec(hidden_dim=32, bbox_hidden_dim=8)]
    m = build("gatv2", n_heads=2, n_gat_layers=2)
    assert m._cfg["attention"] == "gatv2"
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [
        (k, tuple(s)) for k, s in weights.state_dict_spec(**{k: v for k, v in V2CFG.items() if k != "drop_prob"})]
    m.load_state_dict(seeded(V2CFG), strict=True)


def test_checkpoints_of_the_other_mode_are_refused_by_name():
    static_sd, v2_sd = seeded(CFG), seeded(V2CFG)
    with pytest.raises(RuntimeError, match=r"attention='gatv2'.*belongs to attention='gat'"):
        build("gatv2", n_heads=2, n_gat_layers=2).load_state_dict(static_sd)
    with pytest.raises(RuntimeError, match=r"attention='gat'.*belongs to attention='gatv2'"):
        build("gat", n_heads=2, n_gat_layers=2).load_state_dict(v2_sd)
    with pytest.raises(ValueError, match=r"attention='gatv2'.*attention='gat'"):
        HotPathTrainer(V2CFG, static_sd, "cpu")
    with pytest.raises(ValueError, match=r"attention='gat'.*attention='gatv2'"):
        HotPathTrainer(CFG, v2_sd, "cpu")
    tr = HotPathTrainer(V2CFG, v2_sd, "cpu")
    key = "gat.layers.1.heads.0.attention_layer.weight"
    assert tr.params[key].shape == (1, 16) and tr.grads[key].shape == (1, 16)
    for p in ("gat.layers.0.heads.0.", "gat.layers.1.heads.1."):                 # one-GEMM projections kept
        assert engine._adjacent(tr.params[p + "W_i.weight"], tr.params[p + "W_j.weight"])
        assert engine._adjacent(tr.grads[p + "W_i.weight"], tr.grads[p + "W_j.weight"])
    before = tr.state_dict()
    with pytest.raises(ValueError, match=r"attention='gatv2'.*attention='gat'"):
        tr.load_state_dict(static_sd)
    assert all(torch.equal(before[k], v) for k, v in tr.state_dict().items())    # nothing was copied
    tr.load_state_dict(v2_sd)
    with pytest.raises(ValueError):                                               # moments of a static trainer do not fit
        tr.load_optimizer_state_dict(HotPathTrainer(CFG, static_sd, "cpu").optimizer_state_dict())


def test_engine_names_both_sides_of_a_mode_and_weight_mismatch():
    with pytest.raises(ValueError, match=r"attention='gatv2'.*gat\.attention_layer\.weight.*\(1, 16\).*attention='gat'"):
        engine.check_attention_weight("gat.", torch.zeros(1, 16), 8, "gatv2")
    with pytest.raises(ValueError, match=r"attention='gat'.*\(1, 8\).*attention='gatv2'"):
        engine.check_attention_weight("gat.", torch.zeros(1, 8), 8, "gat")
    with pytest.raises(ValueError, match="attention"):
        engine.check_attention_weight("gat.", torch.zeros(1, 8), 8, "other")
    engine.check_attention_weight("gat.", torch.zeros(1, 8), 8, "gatv2")
    engine.check_attention_weight("gat.", torch.zeros(1, 16), 8, "gat")
