"""Host side of the attention dropout (no GPU): the numpy restatement of the counter hash against words computed by hand
(plain Python integers), the kept share of the masks, the per-head seed derivation against every decoder stream, the
option's validation in the constructors and the trainer's cfg, and what a default model keeps: module list, mode dict,
state_dict.  The float64 oracle's own gradients are held to torch.autograd.gradcheck."""
import math
import warnings

import numpy as np
import pytest
import torch
from torch import nn

import cova_amd  # noqa: F401
from cova_web_object_detection_amd import _lib, engine, weights
from cova_web_object_detection_amd.models import CoVA, GraphAttentionLayer, MultiHeadGraphAttention, _layer_modes
from cova_web_object_detection_amd.trainer import HotPathTrainer

import attn_dropout_oracle as AD
from config_cases import SPLIT_CFG as CFG

M64 = (1 << 64) - 1


def mix_by_hand(seed, idx):
    """csrc/common.h hash_mix64 in unbounded Python integers, reduced modulo 2**64 after every product"""
    z = (seed + 0x9E3779B97F4A7C15 * (idx + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


# (seed, idx, word, uniform): the first is the first output of splitmix64 seeded with 0 (Steele, Lea, Flood 2014)
WORDS = [(0, 0, 0xE220A8397B1DCDAF, 0.8833107948303223),
         (0, 1, 0x6E789E6AA1B965F4, 0.4315279722213745),
         (123, 0, 0xB4DC9BD462DE412B, 0.7064911723136902),
         (0x5EED, 7, 0x1289A69805C125B1, 0.07241284847259521),
         ((2 << 56) | (1 << 48) | 12345, 13000, 0xDBAEE0C0F45297B7, 0.8581371307373047),
         (M64, (1 << 40) + 3, 0x57236B271759DE0B, 0.34038418531417847)]


def test_hash_restatement_matches_hand_computed_words():
    for seed, idx, word, uni in WORDS:
        assert mix_by_hand(seed, idx) == word
        assert int(AD.hash_mix64(seed, np.asarray([idx]))[0]) == word
        u = AD.hash_uniform(seed, np.asarray([idx]))
        assert u.dtype == np.float32 and float(u[0]) == uni == (word >> 40) / 16777216.0
    assert WORDS[4][0] == engine.attention_dropout_seed(12345, 1, 0)            # the stream of layer 1, head 0 at base 12345
    idx = np.arange(1000, dtype=np.uint64)
    assert [int(v) for v in AD.hash_mix64(99, idx)] == [mix_by_hand(99, i) for i in range(1000)]
    # the compare is >= in float32: a uniform equal to p is kept, p = 0 keeps everything
    u = AD.hash_uniform(5, idx)
    assert AD.keep_mask(0.0, 5, 10, 100).all()
    assert AD.keep_mask(float(u[17]), 5, 10, 100).reshape(-1)[17]
    assert not AD.keep_mask(float(np.nextafter(u[17], np.float32(2))), 5, 10, 100).reshape(-1)[17]
    assert AD.inv_keep(0.5) == 2.0 and AD.inv_keep(0.6) == float(np.float32(1) / (np.float32(1) - np.float32(0.6)))


@pytest.mark.parametrize("p", [0.1, 0.5, 0.6])
def test_kept_share_lies_within_five_binomial_deviations(p):
    n = 13000
    sd = math.sqrt(p * (1 - p) / n)
    for seed in (0, 123, engine.attention_dropout_seed(engine.dropout_base(123, 1), 0, 0),
                 engine.attention_dropout_seed(engine.dropout_base(7, 40), 1, 1)):
        share = float(AD.keep_mask(p, seed, 130, 100).mean())
        print(p, hex(seed), share)
        assert abs(share - (1 - p)) < 5 * sd, (p, seed, share)
    # two streams of one step are unrelated: they agree on about (1-p)^2 + p^2 of the slots
    a = AD.keep_mask(p, engine.attention_dropout_seed(1000, 0, 0), 130, 100)
    b = AD.keep_mask(p, engine.attention_dropout_seed(1000, 0, 1), 130, 100)
    q = (1 - p) ** 2 + p ** 2
    assert abs(float((a == b).mean()) - q) < 5 * math.sqrt(q * (1 - q) / n)


def test_attention_streams_never_meet_a_decoder_stream_or_each_other():
    for seed in (0x5EED, 123, 0, (1 << 48) - 1):
        decoder, attention = set(), set()
        for step in range(1000):
            base = engine.dropout_base(seed, step)
            assert base == AD.dropout_base(seed, step) == (seed * 0x9E3779B1 + 2 * step) & ((1 << 48) - 1)
            decoder.update((base, base + 1))
            for layer in range(2):
                for head in range(2):
                    s = engine.attention_dropout_seed(base, layer, head)
                    assert s == AD.attention_dropout_seed(base, layer, head) and 0 <= s < 1 << 63
                    assert s & ((1 << 48) - 1) == base and s >> 48 == ((layer + 1) << 8 | (head + 1))
                    attention.add(s)
        assert len(attention) == 4000 and not (attention & decoder)
        assert max(decoder) <= 1 << 48 < min(attention)          # for every step and seed, not only these
    # the trainer's and the module's bases are the same rule (base of step s under seed d)
    assert engine.dropout_base(123, 1) == (123 * 0x9E3779B1 + 2) & 0xFFFFFFFFFFFF
    for bad in ((-1, 0, 0), (1 << 48, 0, 0), (0, 127, 0), (0, 0, 255), (0, -1, 0)):
        with pytest.raises(ValueError, match="attention_dropout_seed"):
            engine.attention_dropout_seed(*bad)


seeded = lambda cfg: weights.seeded_state_dict(5, **{k: v for k, v in cfg.items() if k not in ("drop_prob", "attention_dropout")})


def build(use_context=True, **kw):
    """the reference's nine positional arguments, extensions by keyword"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return CoVA((3, 3), 64, 4, use_context, 32, 8, 0, 0.2, None, **kw)


@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, float("nan"), float("inf"), "0.5x", None, True])
def test_rates_outside_the_half_open_unit_interval_are_refused(bad):
    with pytest.raises(ValueError, match="attention_dropout"):
        weights.check_attention_dropout(bad)
    with pytest.raises(ValueError, match="attention_dropout"):
        GraphAttentionLayer(8, 4, attention_dropout=bad)
    with pytest.raises(ValueError, match="attention_dropout"):
        MultiHeadGraphAttention(8, 4, 2, 1, attention_dropout=bad)
    with pytest.raises(ValueError, match="attention_dropout"):
        build(attention_dropout=bad)
    with pytest.raises(ValueError, match="attention_dropout"):
        HotPathTrainer(dict(CFG, attention_dropout=bad), seeded(CFG), "cpu")
    with pytest.raises(ValueError, match="attention_dropout"):
        engine.check_gat_drop((bad, 1))


def test_good_rates_are_taken_by_every_layer_and_the_header_declares_the_entry_points():
    assert weights.check_attention_dropout(0) == 0.0 and weights.check_attention_dropout(np.float32(0.5)) == 0.5
    assert engine.check_gat_drop(None) is None and engine.check_gat_drop((0.0, 9)) is None
    assert engine.check_gat_drop((0.25, 9)) == (0.25, 9)
    with pytest.raises(ValueError, match="seed"):
        engine.check_gat_drop((0.25, 1 << 64))
    tr = HotPathTrainer(dict(CFG, attention_dropout=0.6), seeded(CFG), "cpu")
    assert tr.cfg["attention_dropout"] == 0.6
    assert "attention_dropout" not in HotPathTrainer(CFG, seeded(CFG), "cpu").cfg
    assert list(tr.state_dict()) == list(HotPathTrainer(CFG, seeded(CFG), "cpu").state_dict())
    protos = _lib.parse_header()
    assert len(protos["cova_gat_fwd_drop"]) == len(protos["cova_gat_fwd_edge"]) + 2
    assert len(protos["cova_gat_bwd_drop"]) == len(protos["cova_gat_bwd_edge"]) + 2
    assert len(protos["cova_gat2_fwd_drop"]) == len(protos["cova_gat2_fwd"]) + 2
    assert len(protos["cova_gat2_bwd_drop"]) == len(protos["cova_gat2_bwd"]) + 2
    import ctypes
    for name, at in (("cova_gat_fwd_drop", 11), ("cova_gat_bwd_drop", 15), ("cova_gat2_fwd_drop", 11), ("cova_gat2_bwd_drop", 13)):
        assert protos[name][at:at + 2] == [ctypes.c_float, ctypes.c_ulonglong], name


def test_a_default_model_keeps_its_module_list_mode_dict_and_state_dict():
    ref = build()
    assert ref._cfg["attention_dropout"] == 0.0
    names = [n for n, _ in ref.named_modules()]
    assert names == [n for n, _ in build(attention_dropout=0.0).named_modules()]
    assert not any("attn_drop" in n for n in names)
    assert [n for n, m in ref.named_modules() if isinstance(m, nn.Dropout)] == ["decoder.0", "decoder.4"]
    assert _layer_modes(ref) is True and _layer_modes(ref.eval()) is False
    ref.train()
    ref.convnet.eval()
    modes = _layer_modes(ref)
    assert set(modes) == {n + "." for n, m in ref.named_modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)} | {
        "decoder.0", "decoder.4"}
    # with the option on: one weightless Dropout per head, named by the head's prefix; the state_dict does not change
    on = build(attention_dropout=0.5)
    assert on._cfg["attention_dropout"] == 0.5 and on.gat.attn_drop.p == 0.5
    assert [n for n in (n for n, _ in on.named_modules()) if n not in names] == ["gat." + engine.ATTN_DROP_KEY]
    assert list(on.state_dict()) == list(ref.state_dict())
    assert _layer_modes(on) is True
    on.gat.eval()
    assert _layer_modes(on)["gat.attn_drop"] is False and _layer_modes(on)["decoder.0"] is True
    assert not engine.is_train(_layer_modes(on), "gat." + engine.ATTN_DROP_KEY)
    on22 = build(attention_dropout=0.5, n_heads=2, n_gat_layers=2)
    prefixes = [p for layer in weights.gat_prefixes(2, 2) for p in layer]
    assert [n for n, m in on22.named_modules() if isinstance(m, nn.Dropout) and n.startswith("gat.")] == [
        p + engine.ATTN_DROP_KEY for p in prefixes]
    assert list(on22.state_dict()) == list(build(n_heads=2, n_gat_layers=2).state_dict())
    assert build(use_context=False, attention_dropout=0.5)._cfg["attention_dropout"] == 0.0      # (no GAT: nothing to drop)
    layer = GraphAttentionLayer(8, 4)
    assert layer.attention_dropout == 0.0 and [n for n, _ in layer.named_modules()] == [
        "", "W_i", "W_j", "attention_layer", "leakyrelu"]
    assert [n for n, _ in GraphAttentionLayer(8, 4, attention_dropout=0.1).named_modules()][-1] == "attn_drop"


def test_oracle_with_a_mask_passes_gradcheck_in_both_modes_and_a_dropped_slot_still_gets_the_softmax_term():
    rs = np.random.RandomState(4)
    N, K, D = 7, 5, 4
    f = lambda *s: torch.from_numpy(rs.standard_normal(s)).requires_grad_(True)
    ctx = torch.from_numpy(rs.randint(-1, N, (N, K)).astype(np.int64))
    ctx[3] = -1
    ctx[5, 0] = N + 2
    ctx[1] = torch.tensor([0, 2, 4, 6, 5])
    keep = AD.keep_mask(0.5, engine.attention_dropout_seed(engine.dropout_base(77, 1), 0, 0), N, K)
    keep[1] = [True, False, True, False, True]
    keep[2] = False                                                              # a row with every slot dropped
    wi, wj, b = f(N, D), f(N, D), f(1)
    for mode, a in (("gat", f(1, 2 * D)), ("gatv2", f(1, D))):
        fn = lambda wi, wj, a, b: AD.attend(mode, wi, wj, ctx, a, b, keep, 0.5)[0]
        assert torch.autograd.gradcheck(fn, (wi, wj, a, b), eps=1e-6, atol=1e-6)
        hp, attn, _ = AD.attend(mode, wi, wj, ctx, a, b, keep, 0.5)
        plain_hp, plain_attn, _ = AD.attend(mode, wi, wj, ctx, a, b)
        assert torch.equal(attn, plain_attn) and torch.allclose(attn.sum(1), torch.ones(N, dtype=torch.float64))
        assert not hp[2].any() and not hp[3].any() and bool(plain_hp[2].any())
        # row 1: h' = 2 * (attn0 Wh_0 + attn2 Wh_4 + attn4 Wh_5)
        want = 2.0 * (attn[1, 0] * wj[0] + attn[1, 2] * wj[4] + attn[1, 4] * wj[5])
        assert torch.allclose(hp[1], want, rtol=1e-12, atol=1e-15)
        if mode == "gat":
            # de of the DROPPED slot 1 of row 1 is -alpha_1 * dot: not zero
            e, _, _, _ = AD.static_scores(wi, wj, ctx, a, b)
            e = e.detach().requires_grad_(True)
            at = torch.softmax(e, dim=1)
            w = at * torch.from_numpy(keep).double() * 2.0
            rows = wj.detach()[ctx[1]]
            ((w[1].unsqueeze(-1) * rows).sum(0)).sum().backward()
            dalpha = torch.from_numpy(keep[1]).double() * 2.0 * rows.sum(1)
            dot = (at[1] * dalpha).sum()
            assert torch.allclose(e.grad[1], (at[1] * (dalpha - dot)).detach(), rtol=1e-10, atol=1e-14)
            assert float(e.grad[1, 1].abs()) > 1e-6 and dalpha[1] == 0
