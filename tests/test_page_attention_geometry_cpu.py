"""CPU tests of the box-geometry bias of the page self-attention (CoVA(page_attention_geometry=True)): the oracle
(tests/page_attn_geo_oracle.py) against the plain one and against the weight gradient written out by hand, the proof that
an exchange of the query and key roles is visible at the GPU tests' bounds, the state_dict contract of
weights.state_dict_spec / models.CoVA with the option, the zero init and the refusals that need no device."""
import warnings

import numpy as np
import pytest
import torch

from cova_web_object_detection_amd import weights
from cova_web_object_detection_amd.models import CoVA, PageAttention
from cova_web_object_detection_amd.trainer import HotPathTrainer
import page_attn_geo_oracle as PG
import page_attn_oracle as PA
from config_cases import PAGE_SPEC as BASE

KEY, GEO_KEY = "page_attention.qkv.weight", "page_attention.geometry.weight"
SIZES, E, HEADS = (37, 0, 1, 5, 0), 8, 2


def case(seed=0, std=2.0):
    rs = np.random.RandomState(seed)
    N = int(sum(SIZES))
    ps = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    boxes = PG.planted_boxes(SIZES, seed + 1)
    phi = PG.page_features(boxes, ps, PG.PAGE_W, PG.PAGE_H)
    return (torch.from_numpy(rs.standard_normal((N, 3 * E))), ps, torch.from_numpy(rs.standard_normal((N, E))),
            torch.from_numpy(std * rs.standard_normal((HEADS, 8))), boxes, phi)


# ---------------------------------------------------------------- the oracle
def test_features_are_the_edge_oracles_on_the_dense_page_table():
    _, ps, _, _, boxes, phi = case()
    assert sorted(phi) == [0, 2, 3] and phi[0].shape == (37, 37, 8) and phi[0].dtype == np.float32
    f = phi[0]
    assert np.array_equal(f[:, :, 7], np.clip(np.arange(37)[None, :] - np.arange(37)[:, None], -64, 64) / np.float32(64))
    for e in (0, 1, 2, 3, 7):                                   # the five antisymmetric features
        assert np.array_equal(f[:, :, e], -f[:, :, e].T), e
    for e in (4, 5, 6):                                         # the three symmetric ones
        assert np.array_equal(f[:, :, e], f[:, :, e].T), e
    diag = f[np.arange(37), np.arange(37)]
    assert diag[2, 6] == 0 and (np.delete(diag[:, 6], 2) == 1).all()          # IoU 1 on the diagonal; 0 without area
    assert np.array_equal(f[0], f[1] + np.asarray([0, 0, 0, 0, 0, 0, 0, 1 / 64], np.float32))   # two identical boxes
    assert f[3, 4, 4] > 0.9 and f[3, 4, 5] > 0.9               # the far-apart pair: gaps of most of the page


def test_zero_weights_give_the_plain_oracle():
    qkv, ps, _, w, _, phi = case(1)
    out, A, lse = PG.attend(qkv, ps, HEADS, torch.zeros_like(w), phi)
    out0, A0, lse0 = PA.attend(qkv, ps, HEADS)
    assert torch.equal(out, out0) and torch.equal(lse, lse0) and all(torch.equal(A[k], A0[k]) for k in A0)
    out1, A1, _ = PG.attend(qkv, ps, HEADS, w, phi)
    assert max(float((A1[k] - A0[k]).abs().max()) for k in A0) > 1e-3


def test_autograd_weight_gradient_is_the_hand_written_einsum():
    qkv, ps, g, w, _, phi = case(2)
    leaf, wl = qkv.clone().requires_grad_(True), w.clone().requires_grad_(True)
    out, A, lse = PG.attend(leaf, ps, HEADS, wl, phi)
    (out * g).sum().backward()
    dh = E // HEADS
    dw = np.zeros((HEADS, 8))
    for (p, a), att in A.items():
        lo, hi = int(ps[p]), int(ps[p + 1])
        att = att.detach().numpy()
        gh = g[lo:hi, a * dh:(a + 1) * dh].numpy()
        v = qkv[lo:hi, 2 * E + a * dh:2 * E + (a + 1) * dh].numpy()
        delta = (gh * (att @ v)).sum(1, keepdims=True)
        ds = att * (gh @ v.T - delta)
        dw[a] += np.einsum("ij,ije->e", ds, phi[p].astype(np.float64))
    assert float(wl.grad.abs().max()) > 0
    assert np.abs(dw - wl.grad.numpy()).max() < 1e-12 * float(wl.grad.abs().max())


def test_exchanged_query_and_key_roles_move_A_beyond_the_gpu_bound():
    qkv, ps, _, w, _, phi = case(3)
    _, A, _ = PG.attend(qkv, ps, HEADS, w, phi)
    _, As, _ = PG.attend(qkv, ps, HEADS, w, PG.swapped(phi))
    for k in A:
        if A[k].shape[0] > 1:
            assert float((A[k] - As[k]).abs().max()) > 1e-3, k


# ---------------------------------------------------------------- spec and module keys
@pytest.mark.parametrize("extra", [dict(), dict(use_context=False),
                                   dict(page_context_dim=16, n_heads=2, n_gat_layers=2, edge_geometry=True)])
def test_spec_keys_order_and_shapes(extra):
    cfg = dict(BASE, page_attention_dim=16, **extra)
    for Hh in (1, 2, 4):
        plain = weights.state_dict_spec(page_attention_heads=Hh, **cfg)
        assert weights.state_dict_spec(page_attention_heads=Hh, page_attention_geometry=False, **cfg) == plain
        spec = weights.state_dict_spec(page_attention_heads=Hh, page_attention_geometry=True, **cfg)
        keys = [k for k, _ in spec]
        assert [(k, s) for k, s in spec if k != GEO_KEY] == plain           # nothing else changes, the decoder included
        i = keys.index(GEO_KEY)
        assert keys[i - 1] == KEY and keys[i + 1] == "decoder.1.weight" and dict(spec)[GEO_KEY] == (Hh, 8)
    sd = weights.seeded_state_dict(7, page_attention_heads=2, page_attention_geometry=True, **cfg)
    sd0 = weights.seeded_state_dict(7, page_attention_heads=2, **cfg)
    assert list(sd) == [k for k, _ in weights.state_dict_spec(page_attention_heads=2, page_attention_geometry=True, **cfg)]
    assert sd[GEO_KEY].shape == (2, 8) and not sd[GEO_KEY].any()             # zero, and drawn from no stream:
    for k in sd0:
        assert torch.equal(sd[k], sd0[k]), k


@pytest.mark.parametrize("extra", [dict(), dict(use_context=False), dict(page_context_dim=16)])
def test_module_state_dict_equals_the_spec_and_starts_at_zero(extra):
    cfg = dict(BASE, **extra)
    kw = {k: v for k, v in extra.items() if k != "use_context"}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        build = lambda **more: CoVA((3, 3), 64, 4, cfg["use_context"], 32, 8, 2, 0.2, None, **kw, **more)
        m = build(page_attention_dim=16, page_attention_heads=2, page_attention_geometry=True)
        m0 = build(page_attention_dim=16, page_attention_heads=2)
    spec = weights.state_dict_spec(page_attention_dim=16, page_attention_heads=2, page_attention_geometry=True, **cfg)
    assert list(m.state_dict()) == [k for k, _ in spec]
    assert all(tuple(m.state_dict()[k].shape) == s for k, s in spec)
    assert m._cfg["page_attention_geometry"] is True and m0._cfg["page_attention_geometry"] is False
    w = m.page_attention.geometry.weight
    assert isinstance(m.page_attention.geometry, torch.nn.Linear) and m.page_attention.geometry.bias is None
    assert w.shape == (2, 8) and w.requires_grad and not w.detach().any()
    assert list(m0.state_dict()) == [k for k, _ in spec if k != GEO_KEY]     # the default is today's model exactly
    assert [n for n, _ in m.named_modules() if n != "page_attention.geometry"] == [n for n, _ in m0.named_modules()]
    missing = m.load_state_dict(weights.seeded_state_dict(5, page_attention_dim=16, page_attention_heads=2,
                                                          page_attention_geometry=True, **cfg), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys


def test_page_attention_module_parameters():
    layer = PageAttention(24, 8, 2, geometry=True)
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == {"qkv.weight": (24, 24), "geometry.weight": (2, 8)}
    assert not layer.geometry.weight.detach().any()
    assert list(PageAttention(24, 8, 2).state_dict()) == list(PageAttention(24, 8, 2, geometry=False).state_dict()) == ["qkv.weight"]
    with pytest.raises(RuntimeError, match="MI355X"):        # no CPU fallback
        layer(torch.zeros(3, 24), torch.tensor([0, 3]), torch.zeros(3, 5), (64, 96))


# ---------------------------------------------------------------- refusals
def test_the_option_needs_the_layer():
    with pytest.raises(ValueError, match="page_attention_geometry.*page_attention_dim"):
        weights.state_dict_spec(page_attention_geometry=True)
    with pytest.raises(ValueError, match="page_attention_geometry.*page_attention_dim"):
        weights.state_dict_spec(page_attention_dim=0, page_attention_heads=2, page_attention_geometry=True)
    with pytest.raises(ValueError, match="page_attention_geometry"):
        weights.state_dict_spec(page_attention_dim=16, page_attention_geometry=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="page_attention_geometry.*page_attention_dim"):
            CoVA((3, 3), 64, 4, page_attention_geometry=True)
    with pytest.raises(ValueError, match="page_attention_geometry.*page_attention_dim"):
        HotPathTrainer(dict(BASE, drop_prob=0.2, page_attention_geometry=True), weights.seeded_state_dict(3, **BASE), "cuda:63")


def test_trainer_names_the_option_on_a_checkpoint_of_the_other_kind():
    """Both mismatches are found from the keys, before the trainer touches a device."""
    acfg = dict(BASE, page_attention_dim=16, page_attention_heads=2)
    cfg = dict(acfg, drop_prob=0.2)
    with_sd = weights.seeded_state_dict(3, page_attention_geometry=True, **acfg)
    without_sd = weights.seeded_state_dict(3, **acfg)
    nowhere = "cuda:63"                                      # never reached
    with pytest.raises(ValueError, match=r"page_attention_geometry=True.*lacks.*page_attention\.geometry\.weight"):
        HotPathTrainer(dict(cfg, page_attention_geometry=True), without_sd, nowhere)
    with pytest.raises(ValueError, match=r"page_attention_geometry=False.*page_attention\.geometry\.weight"):
        HotPathTrainer(cfg, with_sd, nowhere)
    with pytest.raises(ValueError, match=r"page_attention_geometry=False.*page_attention\.geometry\.weight"):
        HotPathTrainer(dict(cfg, page_attention_geometry=False), with_sd, nowhere)
    other = dict(with_sd)
    other[GEO_KEY] = torch.zeros(4, 8)
    with pytest.raises(ValueError, match=r"page_attention_heads=2.*\(4, 8\)"):
        HotPathTrainer(dict(cfg, page_attention_geometry=True), other, nowhere)
