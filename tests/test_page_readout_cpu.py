"""CPU tests of the page readout (CoVA(page_context_dim=G)): the torch oracle's autograd against the closed-form backward
the kernels implement (include/cova_hip.h, cova_page_readout_bwd), the operator's behaviour on small pages, the state_dict
contract of weights.state_dict_spec / models.CoVA with and without the option, and the refusals that need no device."""
import warnings

import numpy as np
import pytest
import torch

from cova_web_object_detection_amd import weights
from cova_web_object_detection_amd.models import CoVA, PageReadout
from cova_web_object_detection_amd.trainer import HotPathTrainer
import readout_oracle as RO
from config_cases import PAGE_SPEC as BASE

KEYS = ["page_readout.W.weight", "page_readout.attention_layer.weight", "page_readout.attention_layer.bias"]


def case(sizes, G, seed=0, scale=1.0):
    rs = np.random.RandomState(seed)
    N = int(sum(sizes))
    ps = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    P = torch.from_numpy(rs.standard_normal((N, G)))
    a = torch.from_numpy(scale * rs.standard_normal(G) / np.sqrt(G))
    b = torch.from_numpy(rs.standard_normal(1))
    g = torch.from_numpy(rs.standard_normal((N, G)))
    return P, a, b, ps, g


# ---------------------------------------------------------------- the oracle against the closed form
@pytest.mark.parametrize("sizes,G", [((1,), 6), ((37, 0, 1, 5, 0), 6), ((90, 11), 64), ((300, 2, 130), 12)])
@pytest.mark.parametrize("forced", [False, True])
def test_autograd_of_the_oracle_matches_the_closed_form_backward(sizes, G, forced):
    P, a, b, ps, g = case(sizes, G, seed=len(sizes) + G, scale=3.0)
    gate = None
    if forced:                                               # forced gates: some against the sign of u
        gate = torch.from_numpy(np.random.RandomState(5).rand(P.shape[0]) > 0.5)
    Pl, al, bl = (t.clone().requires_grad_(True) for t in (P, a, b))
    rows, beta, r, u = RO.pool(Pl, al, bl, ps, gate=gate)
    (rows * g).sum().backward()
    dP, da, db = RO.closed_form_bwd(g, P, a, b, ps, gate=gate)
    assert P.dtype == torch.float64 and rows.dtype == torch.float64
    scale = float(Pl.grad.abs().max())
    assert float((dP - Pl.grad).abs().max()) < 1e-12 * max(scale, 1.0)
    assert float((da - al.grad).abs().max()) < 1e-11 * max(float(al.grad.abs().max()), 1.0)
    assert float((db - bl.grad).abs().max()) < 1e-11 * max(float(al.grad.abs().max()), 1.0)
    if not forced and len(sizes) > 1:
        assert float(al.grad.abs().max()) > 0


# ---------------------------------------------------------------- behaviour
def test_a_one_box_page_returns_its_row_with_beta_one_and_no_score_gradient():
    P, a, b, ps, g = case((1, 4), 6, seed=3)
    rows, beta, r, u = RO.pool(P, a, b, ps)
    assert torch.equal(rows[0], P[0]) and float(beta[0]) == 1.0 and torch.equal(r[0], P[0])
    # du of the single box is zero: dP of that row is g itself and the row adds nothing to d_att_w / d_att_b
    dP, da, db = RO.closed_form_bwd(g, P, a, b, ps)
    assert torch.allclose(dP[0], g[0], rtol=0, atol=1e-15)
    dP4, da4, db4 = RO.closed_form_bwd(g[1:], P[1:], a, b, [0, 4])
    assert torch.allclose(da, da4, rtol=0, atol=1e-14) and torch.allclose(db, db4, rtol=0, atol=1e-14)


def test_equal_scores_give_the_mean_and_beta_sums_to_one_per_page():
    P, a, b, ps, _ = case((7, 0, 12), 5, seed=4)
    rows, beta, r, u = RO.pool(P, torch.zeros(5, dtype=torch.float64), b, ps)        # a = 0: every score is b
    assert torch.allclose(r[0], P[:7].mean(0), rtol=0, atol=1e-14) and torch.allclose(r[2], P[7:].mean(0), rtol=0, atol=1e-14)
    assert not r[1].any()                                    # the empty page: zeros in the oracle, nothing on the device
    assert torch.allclose(beta[:7], torch.full((7,), 1 / 7, dtype=torch.float64))
    rows, beta, r, u = RO.pool(P, a, b, ps)
    assert abs(float(beta[:7].sum()) - 1) < 1e-14 and abs(float(beta[7:].sum()) - 1) < 1e-14
    assert rows.shape == P.shape and torch.equal(rows[0], rows[6]) and torch.equal(rows[7], rows[18])
    assert not torch.equal(rows[0], rows[7])
    assert torch.allclose(rows[3], (beta[:7].unsqueeze(1) * P[:7]).sum(0), rtol=0, atol=1e-14)


def test_shifting_the_bias_keeps_beta_only_while_all_gates_agree():
    P, a, b, ps, _ = case((9,), 4, seed=6)
    u = RO.pool(P, a, torch.zeros(1, dtype=torch.float64), ps)[3]
    assert float(u.min()) < 0 < float(u.max())
    up = torch.tensor([float(-u.min()) + 1.0])               # every score positive, and more so
    beta1 = RO.pool(P, a, up.double(), ps)[1]
    beta2 = RO.pool(P, a, up.double() + 5.0, ps)[1]
    assert torch.allclose(beta1, beta2, rtol=0, atol=1e-14)  # one branch: softmax is shift-invariant
    down = torch.tensor([float(-u.max()) - 1.0]).double()    # every score negative: the alpha branch, also one branch
    assert torch.allclose(RO.pool(P, a, down, ps)[1], RO.pool(P, a, down - 5.0, ps)[1], rtol=0, atol=1e-14)
    mixed = RO.pool(P, a, torch.zeros(1, dtype=torch.float64), ps)[1]
    assert float((mixed - beta1).abs().max()) > 1e-3         # gates disagree: the shift changes the distribution
    # u == +-0 takes the alpha branch: the value is the same on either branch, the gradient is not
    zero = torch.zeros(1, dtype=torch.float64)
    Z = P[:3].clone()
    Z[0], Z[1] = 0.0, -0.0
    g = torch.from_numpy(np.random.RandomState(8).standard_normal((3, 4)))
    uz = RO.pool(Z, a, zero, [0, 3])[3]
    assert not uz[:2].any() and float(uz[2]) != 0
    third = bool(uz[2] > 0)
    dflt = RO.closed_form_bwd(g, Z, a, zero, [0, 3])
    slope = RO.closed_form_bwd(g, Z, a, zero, [0, 3], gate=torch.tensor([False, False, third]))
    ident = RO.closed_form_bwd(g, Z, a, zero, [0, 3], gate=torch.tensor([True, True, third]))
    assert all(torch.equal(x, y) for x, y in zip(dflt, slope))
    assert float((dflt[0][:2] - ident[0][:2]).abs().max()) > 1e-3 * float(dflt[0].abs().max())


# ---------------------------------------------------------------- spec and module keys
@pytest.mark.parametrize("extra", [dict(), dict(use_context=False), dict(n_heads=2, n_gat_layers=2, attention="gatv2"),
                                   dict(backbone_layers=2), dict(edge_geometry=True)])
def test_spec_keys_order_shapes_and_decoder_widths(extra):
    G = 16
    cfg = dict(BASE, **extra)
    plain = weights.state_dict_spec(**cfg)
    assert weights.state_dict_spec(page_context_dim=0, **cfg) == plain
    spec = weights.state_dict_spec(page_context_dim=G, **cfg)
    keys, pkeys = [k for k, _ in spec], [k for k, _ in plain]
    assert [k for k in keys if k not in KEYS] == pkeys
    i = keys.index(KEYS[0])
    assert keys[i:i + 3] == KEYS and keys[i + 3] == "decoder.1.weight"
    assert keys[i - 1].startswith("gat." if cfg["use_context"] else "bn_additional_feat.")
    n_feat = (128 if cfg.get("backbone_layers") == 2 else 64) * 9 + 8 + 2
    shapes = dict(spec)
    assert shapes[KEYS[0]] == (G, n_feat) and shapes[KEYS[1]] == (1, G) and shapes[KEYS[2]] == (1,)
    T = n_feat + (32 if cfg["use_context"] else 0) + G
    assert shapes["decoder.1.weight"] == (T, T) and shapes["decoder.1.bias"] == (T,)
    assert shapes["decoder.2.running_mean"] == (T,) and shapes["decoder.5.weight"] == (4, T)
    assert dict(plain)["decoder.1.weight"] == (T - G, T - G)
    for k, s in plain:                                       # nothing in front of the decoder changes
        if not k.startswith("decoder."):
            assert shapes[k] == s
    sd = weights.seeded_state_dict(7, page_context_dim=G, **cfg)
    assert list(sd) == keys and all(tuple(sd[k].shape) == s for k, s in spec)
    bound = 1.0 / np.sqrt(n_feat)                             # drawn like any Linear
    w = sd[KEYS[0]]
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.5 * bound and float(sd[KEYS[2]].abs()) <= 0.05
    # the entries in front of the readout draw the same numbers with and without it
    sd0 = weights.seeded_state_dict(7, **cfg)
    for k in pkeys[:pkeys.index("decoder.1.weight")]:
        assert torch.equal(sd[k], sd0[k]), k


@pytest.mark.parametrize("extra", [dict(), dict(use_context=False), dict(n_heads=2, n_gat_layers=2, attention="gatv2"),
                                   dict(backbone_layers=2)])
def test_module_state_dict_equals_the_spec(extra):
    cfg = dict(BASE, **extra)
    kw = {k: v for k, v in extra.items() if k != "use_context"}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        build = lambda **more: CoVA((3, 3), 64, 4, cfg["use_context"], 32, 8, 2, 0.2, None, **kw, **more)
        m, m0, mz = build(page_context_dim=16), build(), build(page_context_dim=0)
    spec = weights.state_dict_spec(page_context_dim=16, **cfg)
    assert list(m.state_dict()) == [k for k, _ in spec]
    assert all(tuple(m.state_dict()[k].shape) == s for k, s in spec)
    assert isinstance(m.page_readout, PageReadout) and m._cfg["page_context_dim"] == 16
    names = [n for n, _ in m.named_children()]
    assert names.index("page_readout") == names.index("decoder") - 1
    if cfg["use_context"]:
        assert names.index("gat") == names.index("page_readout") - 1
    # the default is today's model exactly
    assert list(m0.state_dict()) == [k for k, _ in weights.state_dict_spec(**cfg)]
    assert [n for n, _ in m0.named_modules()] == [n for n, _ in mz.named_modules()]
    assert not any("page_readout" in n for n, _ in m0.named_modules()) and m0._cfg["page_context_dim"] == 0
    assert [n for n, _ in m.named_modules() if "page_readout" not in n] == [n for n, _ in m0.named_modules()]


def test_page_readout_module_parameters():
    r = PageReadout(24, 8)
    assert {k: tuple(v.shape) for k, v in r.state_dict().items()} == {
        "W.weight": (8, 24), "attention_layer.weight": (1, 8), "attention_layer.bias": (1,)}
    with pytest.raises(ValueError):
        PageReadout(24, 8, alpha=0.1)
    with pytest.raises(ValueError):
        PageReadout(24, 0)
    with pytest.raises(RuntimeError, match="MI355X"):        # no CPU fallback
        r(torch.zeros(3, 24), torch.tensor([0, 3]))


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("bad", [-1, 513, 1.5, True, None, "16"])
def test_check_page_context_dim_refuses(bad):
    with pytest.raises(ValueError, match="page_context_dim"):
        weights.check_page_context_dim(bad)
    with pytest.raises(ValueError, match="page_context_dim"):
        weights.state_dict_spec(page_context_dim=bad)


def test_check_page_context_dim_accepts_the_range():
    assert [weights.check_page_context_dim(g) for g in (0, 1, 512, np.int64(7))] == [0, 1, 512, 7]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="page_context_dim"):
            CoVA((3, 3), 64, 4, page_context_dim=513)


def test_trainer_names_the_option_on_a_checkpoint_of_the_other_kind():
    """Both mismatches are found from the keys, before the trainer touches a device."""
    cfg = dict(BASE, drop_prob=0.2)
    with_sd = weights.seeded_state_dict(3, page_context_dim=16, **BASE)
    without_sd = weights.seeded_state_dict(3, **BASE)
    nowhere = "cuda:63"                                      # never reached
    with pytest.raises(ValueError, match=r"page_context_dim=16.*lacks.*page_readout\.W\.weight"):
        HotPathTrainer(dict(cfg, page_context_dim=16), without_sd, nowhere)
    with pytest.raises(ValueError, match=r"page_context_dim=0.*page_readout\.W\.weight"):
        HotPathTrainer(cfg, with_sd, nowhere)
    with pytest.raises(ValueError, match=r"page_context_dim=8.*\(16, 586\)"):
        HotPathTrainer(dict(cfg, page_context_dim=8), with_sd, nowhere)
    with pytest.raises(ValueError, match="page_context_dim"):
        HotPathTrainer(dict(cfg, page_context_dim=1.5), with_sd, nowhere)
