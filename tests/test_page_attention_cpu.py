"""CPU tests of the page self-attention (CoVA(page_attention_dim=E, page_attention_heads=Hh)): the torch oracle's autograd
against the closed-form backward the kernels implement (include/cova_hip.h, cova_page_attn_bwd) written out in numpy, the
operator's behaviour on small pages, the state_dict contract of weights.state_dict_spec / models.CoVA with and without the
option, and the refusals that need no device."""
import warnings

import numpy as np
import pytest
import torch

from cova_web_object_detection_amd import weights
from cova_web_object_detection_amd.models import CoVA, PageAttention
from cova_web_object_detection_amd.trainer import HotPathTrainer
import page_attn_oracle as PA
from config_cases import PAGE_SPEC as BASE

KEY = "page_attention.qkv.weight"
RKEYS = ["page_readout.W.weight", "page_readout.attention_layer.weight", "page_readout.attention_layer.bias"]


def case(sizes, E, seed=0, scale=1.0):
    rs = np.random.RandomState(seed)
    N = int(sum(sizes))
    ps = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    qkv = rs.standard_normal((N, 3 * E))
    qkv[:, :E] *= scale
    return torch.from_numpy(qkv), ps, torch.from_numpy(rs.standard_normal((N, E)))


def closed_form_bwd(g, qkv, ps, heads):
    """The hand-derived backward in numpy: delta_i = g_i . O_i, dA_ij = g_i . V_j, ds_ij = A_ij (dA_ij - delta_i),
    dQ = ds K / sqrt(dh), dK = ds^T Q / sqrt(dh), dV = A^T g."""
    g, qkv = np.asarray(g, np.float64), np.asarray(qkv, np.float64)
    E = qkv.shape[1] // 3
    dh = E // heads
    d = np.zeros_like(qkv)
    for p in range(len(ps) - 1):
        lo, hi = int(ps[p]), int(ps[p + 1])
        for a in range(heads if hi > lo else 0):
            c = slice(a * dh, (a + 1) * dh)
            q, k, v = qkv[lo:hi, c], qkv[lo:hi, E:][:, c], qkv[lo:hi, 2 * E:][:, c]
            s = q @ k.T / np.sqrt(dh)
            A = np.exp(s - s.max(1, keepdims=True))
            A /= A.sum(1, keepdims=True)
            gh = g[lo:hi, c]
            delta = (gh * (A @ v)).sum(1, keepdims=True)
            ds = A * (gh @ v.T - delta)
            d[lo:hi, c] = ds @ k / np.sqrt(dh)
            d[lo:hi, E:][:, c] = ds.T @ q / np.sqrt(dh)
            d[lo:hi, 2 * E:][:, c] = A.T @ gh
    return d


# ---------------------------------------------------------------- the oracle against the closed form
@pytest.mark.parametrize("sizes,E,heads", [((1,), 4, 1), ((37, 0, 1, 5, 0), 8, 2), ((90, 11), 16, 4)])
def test_autograd_of_the_oracle_matches_the_closed_form_backward(sizes, E, heads):
    qkv, ps, g = case(sizes, E, seed=len(sizes) + E, scale=3.0)
    leaf = qkv.clone().requires_grad_(True)
    out, A, lse = PA.attend(leaf, ps, heads)
    assert out.dtype == torch.float64 and out.shape == (qkv.shape[0], E) and lse.shape == (qkv.shape[0], heads)
    (out * g).sum().backward()
    d = closed_form_bwd(g, qkv, ps, heads)
    assert np.abs(d - leaf.grad.numpy()).max() < 1e-12 * max(float(leaf.grad.abs().max()), 1.0)
    if sum(sizes) > 1:
        assert float(leaf.grad[:, :E].abs().max()) > 0


# ---------------------------------------------------------------- behaviour
@pytest.mark.parametrize("sizes,E,heads", [((1,), 4, 1), ((37, 0, 1, 5, 0), 8, 2), ((90, 11), 16, 4)])
def test_rows_of_A_sum_to_one_per_page_and_head(sizes, E, heads):
    qkv, ps, _ = case(sizes, E, seed=2)
    _, A, lse = PA.attend(qkv, ps, heads)
    live = [p for p, n in enumerate(sizes) if n > 0]
    assert sorted(A) == [(p, a) for p in live for a in range(heads)]
    for (p, a), att in A.items():
        assert att.shape == (sizes[p], sizes[p])
        assert float((att.sum(1) - 1).abs().max()) < 1e-14
        dh = E // heads
        lo, hi = ps[p], ps[p + 1]
        s = qkv[lo:hi, a * dh:(a + 1) * dh] @ qkv[lo:hi, E + a * dh:E + (a + 1) * dh].t() / np.sqrt(dh)
        assert torch.allclose(torch.exp(s - lse[lo:hi, a:a + 1]), att, rtol=0, atol=1e-14)


def test_a_one_box_page_returns_its_V_row_and_sends_no_gradient_to_Q_or_K():
    qkv, ps, g = case((1, 4), 8, seed=3)
    leaf = qkv.clone().requires_grad_(True)
    out, A, _ = PA.attend(leaf, ps, 2)
    assert torch.equal(out[0], qkv[0, 16:]) and float(A[(0, 0)].detach()) == 1.0 and float(A[(0, 1)].detach()) == 1.0
    (out * g).sum().backward()
    assert not leaf.grad[0, :16].any()
    assert torch.allclose(leaf.grad[0, 16:], g[0], rtol=0, atol=1e-15)
    assert float(leaf.grad[1:, :16].abs().max()) > 0


def test_equal_keys_give_the_page_mean_of_V():
    qkv, ps, _ = case((7, 0, 12), 8, seed=4)
    qkv[:7, 8:16] = qkv[0, 8:16]
    qkv[7:, 8:16] = qkv[7, 8:16]
    out, A, _ = PA.attend(qkv, ps, 2)
    assert torch.allclose(out[:7], qkv[:7, 16:].mean(0).expand(7, 8), rtol=0, atol=1e-14)
    assert torch.allclose(out[7:], qkv[7:, 16:].mean(0).expand(12, 8), rtol=0, atol=1e-14)
    assert torch.allclose(A[(2, 1)], torch.full((12, 12), 1 / 12, dtype=torch.float64), rtol=0, atol=1e-15)


def test_a_constant_added_to_every_K_row_of_a_page_leaves_A_unchanged():
    qkv, ps, _ = case((9, 5), 8, seed=6)
    _, A, _ = PA.attend(qkv, ps, 2)
    shifted = qkv.clone()
    shifted[:9, 8:16] += torch.from_numpy(np.random.RandomState(1).standard_normal(8))
    out2, A2, _ = PA.attend(shifted, ps, 2)
    for key in A:
        assert torch.allclose(A[key], A2[key], rtol=0, atol=1e-13), key
    # (a constant per row of the scores; a change of one key does move A)
    shifted[0, 8:16] += 1.0
    assert float((PA.attend(shifted, ps, 2)[1][(0, 0)] - A[(0, 0)]).abs().max()) > 1e-3


# ---------------------------------------------------------------- spec and module keys
@pytest.mark.parametrize("extra", [dict(), dict(use_context=False),
                                   dict(page_context_dim=16, n_heads=2, n_gat_layers=2, attention="gatv2")])
def test_spec_keys_order_shapes_and_decoder_widths(extra):
    E, Hh = 16, 2
    cfg = dict(BASE, **extra)
    plain = weights.state_dict_spec(**cfg)
    assert weights.state_dict_spec(page_attention_dim=0, **cfg) == plain
    assert weights.state_dict_spec(page_attention_dim=0, page_attention_heads=3, **cfg) == plain
    spec = weights.state_dict_spec(page_attention_dim=E, page_attention_heads=Hh, **cfg)
    assert spec == weights.state_dict_spec(page_attention_dim=E, page_attention_heads=4, **cfg)    # heads add no weights
    keys, pkeys = [k for k, _ in spec], [k for k, _ in plain]
    assert [k for k in keys if k != KEY] == pkeys
    i = keys.index(KEY)
    assert keys[i + 1] == "decoder.1.weight"
    if cfg.get("page_context_dim"):
        assert keys[i - 3:i] == RKEYS
    else:
        assert keys[i - 1].startswith("gat." if cfg["use_context"] else "bn_additional_feat.")
    n_feat = 64 * 9 + 8 + 2
    shapes = dict(spec)
    assert shapes[KEY] == (3 * E, n_feat)
    T = n_feat + (32 if cfg["use_context"] else 0) + cfg.get("page_context_dim", 0) + E
    assert shapes["decoder.1.weight"] == (T, T) and shapes["decoder.1.bias"] == (T,)
    assert shapes["decoder.2.running_mean"] == (T,) and shapes["decoder.5.weight"] == (4, T)
    assert dict(plain)["decoder.1.weight"] == (T - E, T - E)
    for k, s in plain:                                       # nothing in front of the decoder changes
        if not k.startswith("decoder."):
            assert shapes[k] == s
    sd = weights.seeded_state_dict(7, page_attention_dim=E, page_attention_heads=Hh, **cfg)
    assert list(sd) == keys and all(tuple(sd[k].shape) == s for k, s in spec)
    bound = 1.0 / np.sqrt(n_feat)                             # drawn like any Linear
    assert 0.5 * bound < float(sd[KEY].abs().max()) <= bound
    sd0 = weights.seeded_state_dict(7, **cfg)
    for k in pkeys[:pkeys.index("decoder.1.weight")]:
        assert torch.equal(sd[k], sd0[k]), k


@pytest.mark.parametrize("extra", [dict(), dict(use_context=False),
                                   dict(page_context_dim=16, n_heads=2, n_gat_layers=2, attention="gatv2")])
def test_module_state_dict_equals_the_spec(extra):
    cfg = dict(BASE, **extra)
    kw = {k: v for k, v in extra.items() if k != "use_context"}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        build = lambda **more: CoVA((3, 3), 64, 4, cfg["use_context"], 32, 8, 2, 0.2, None, **kw, **more)
        m, m0, mz = build(page_attention_dim=16, page_attention_heads=2), build(), build(page_attention_dim=0)
    spec = weights.state_dict_spec(page_attention_dim=16, page_attention_heads=2, **cfg)
    assert list(m.state_dict()) == [k for k, _ in spec]
    assert all(tuple(m.state_dict()[k].shape) == s for k, s in spec)
    assert isinstance(m.page_attention, PageAttention)
    assert m._cfg["page_attention_dim"] == 16 and m._cfg["page_attention_heads"] == 2
    names = [n for n, _ in m.named_children()]
    assert names.index("page_attention") == names.index("decoder") - 1
    if cfg.get("page_context_dim"):
        assert names.index("page_readout") == names.index("page_attention") - 1
    # the default is today's model exactly
    assert list(m0.state_dict()) == [k for k, _ in weights.state_dict_spec(**cfg)]
    assert [n for n, _ in m0.named_modules()] == [n for n, _ in mz.named_modules()]
    assert not any("page_attention" in n for n, _ in m0.named_modules()) and m0._cfg["page_attention_dim"] == 0
    assert [n for n, _ in m.named_modules() if "page_attention" not in n] == [n for n, _ in m0.named_modules()]


def test_page_attention_module_parameters():
    layer = PageAttention(24, 8, 2)
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == {"qkv.weight": (24, 24)}
    assert (layer.dim, layer.heads) == (8, 2)
    with pytest.raises(ValueError):
        PageAttention(24, 0)
    with pytest.raises(ValueError, match="page_attention"):
        PageAttention(24, 8, 3)
    with pytest.raises(RuntimeError, match="MI355X"):        # no CPU fallback
        layer(torch.zeros(3, 24), torch.tensor([0, 3]))


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("bad", [(-4, 1), (516, 1), (1.5, 1), (True, 1), (None, 1), ("16", 1), (16, 1.0), (16, True),
                                 (16, None), (16, 0), (16, -2), (16, 3), (24, 4), (6, 1), (8, 4), (2, 1), (512, 2),
                                 (260, 2)])
def test_check_page_attention_refuses(bad):
    with pytest.raises(ValueError, match="page_attention"):
        weights.check_page_attention(*bad)
    with pytest.raises(ValueError, match="page_attention"):
        weights.state_dict_spec(page_attention_dim=bad[0], page_attention_heads=bad[1])


def test_check_page_attention_accepts_the_range():
    ok = [(0, 1), (0, 7), (4, 1), (8, 2), (128, 1), (128, 4), (512, 4), (512, 128), (384, 4), (np.int64(24), np.int32(2))]
    assert [weights.check_page_attention(*a) for a in ok] == [(int(e), int(h)) for e, h in ok]
    assert weights.check_page_attention(16) == (16, 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="page_attention"):
            CoVA((3, 3), 64, 4, page_attention_dim=516)
        with pytest.raises(ValueError, match="page_attention"):
            CoVA((3, 3), 64, 4, page_attention_dim=16, page_attention_heads=3)


def test_trainer_names_the_option_on_a_checkpoint_of_the_other_kind():
    """Both mismatches are found from the keys, before the trainer touches a device."""
    cfg = dict(BASE, drop_prob=0.2)
    with_sd = weights.seeded_state_dict(3, page_attention_dim=16, page_attention_heads=2, **BASE)
    without_sd = weights.seeded_state_dict(3, **BASE)
    nowhere = "cuda:63"                                      # never reached
    with pytest.raises(ValueError, match=r"page_attention_dim=16.*lacks.*page_attention\.qkv\.weight"):
        HotPathTrainer(dict(cfg, page_attention_dim=16, page_attention_heads=2), without_sd, nowhere)
    with pytest.raises(ValueError, match=r"page_attention_dim=0.*page_attention\.qkv\.weight"):
        HotPathTrainer(cfg, with_sd, nowhere)
    with pytest.raises(ValueError, match=r"page_attention_dim=8.*\(48, 586\)"):
        HotPathTrainer(dict(cfg, page_attention_dim=8), with_sd, nowhere)
    with pytest.raises(ValueError, match="page_attention"):
        HotPathTrainer(dict(cfg, page_attention_dim=1.5), with_sd, nowhere)
    with pytest.raises(ValueError, match="page_attention"):
        HotPathTrainer(dict(cfg, page_attention_dim=16, page_attention_heads=3), with_sd, nowhere)
