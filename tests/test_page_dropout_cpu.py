"""CPU tests of the dropout of the page layers (CoVA(page_attention_dropout=, page_encoder_dropout=)):
the stream rule engine.page_dropout_seed against every other dropout stream of a step, the float64 oracle
(tests/page_dropout_oracle.py) without dropout against the oracles it builds on, its placement of the four sites against
torch's own nn.TransformerEncoderLayer with mask-multiplying modules in place of its Dropouts, the kept share of the hash
on the two index forms, and the option checks of weights."""
import math
import warnings

import numpy as np
import pytest
import torch

from cova_web_object_detection_amd import engine, weights
from cova_web_object_detection_amd.models import CoVA, PageAttention, PageEncoder
import attn_dropout_oracle as AD
import page_attn_geo_oracle as PG
import page_attn_oracle as PA
import page_dropout_oracle as PD
import page_encoder_oracle as PE

SEED_CALLS = [(seed, call) for seed in (0, 1, 5, 123, 0x5EED, 2 ** 31 - 1, 2 ** 40 + 7) for call in (1, 2, 3, 1000)]
BASES = [engine.dropout_base(seed, call) for seed, call in SEED_CALLS]


def random_sd(F_in, P, M, L, heads=1, geometry=False, seed=0):
    rs = np.random.RandomState(seed)
    spec = weights.page_encoder_entries(F_in, P, heads, L, M, geometry)
    return {k: torch.from_numpy(rs.standard_normal(s) * (1.0 if len(s) == 1 else 1.0 / np.sqrt(s[-1]))) for k, s in spec}


# ---------------------------------------------------------------- the stream rule
def test_page_streams_are_pairwise_distinct_and_equal_no_other_stream_of_any_step():
    L = weights.PAGE_ENCODER_MAX_LAYERS
    assert L == PD.MAX_LAYERS and engine.PAGE_DROP_SITES == PD.SITES == 4
    attention = set()
    assert BASES == [AD.dropout_base(seed, call) for seed, call in SEED_CALLS]
    for base in BASES:
        assert 0 <= base < 1 << 48
        for layer in (0, 1, 7, 126):
            for head in (0, 1, 254):
                attention.add(engine.attention_dropout_seed(base, layer, head))
    decoder = set(BASES) | set(b + 1 for b in BASES)
    for base in BASES:
        streams = [engine.page_dropout_seed(base, l, s) for l in range(L + 1) for s in range(4)]
        assert streams == [PD.page_dropout_seed(base, l, s) for l in range(L + 1) for s in range(4)]
        assert len(set(streams)) == 9 * 4
        assert all(s >> 63 == 1 and s < 1 << 64 and s & ((1 << 48) - 1) == base for s in streams)
        assert not set(streams) & decoder and not set(streams) & attention
    assert all(s >> 63 == 0 for s in decoder | attention)
    # two bases: the streams differ wherever (base, layer, site) does
    a, b = BASES[0], BASES[5]
    assert not {engine.page_dropout_seed(a, l, s) for l in range(L + 1) for s in range(4)} & \
        {engine.page_dropout_seed(b, l, s) for l in range(L + 1) for s in range(4)}
    assert engine.page_dropout_seed(0, 0, 0) == (1 << 63) | (1 << 56) | (1 << 48)
    assert engine.page_dropout_seed(5, L, 0) == (1 << 63) | ((L + 1) << 56) | (1 << 48) | 5
    for bad in ((-1, 0, 0), (1 << 48, 0, 0), (0, -1, 0), (0, L + 1, 0), (0, 0, -1), (0, 0, 4)):
        with pytest.raises(ValueError, match="page_dropout_seed"):
            engine.page_dropout_seed(*bad)


# ---------------------------------------------------------------- no dropout is the old oracle
@pytest.mark.parametrize("geometry", [False, True])
def test_all_keep_masks_at_rate_zero_are_the_oracles_it_builds_on_exactly(geometry):
    sizes, Fd, P, Hh, M, L = (7, 0, 1, 12), 6, 8, 2, 16, 2
    ps = np.concatenate([[0], np.cumsum(sizes)])
    N = int(ps[-1])
    sd = random_sd(Fd, P, M, L, Hh, geometry, seed=3)
    rs = np.random.RandomState(4)
    h = torch.from_numpy(rs.standard_normal((N, Fd)))
    phi = PG.page_features(PG.planted_boxes(sizes, 5), ps, PG.PAGE_W, PG.PAGE_H) if geometry else None
    assert PD.inv_keep(0.0) == 1.0
    want = PE.page_encoder(h, sd, ps, Hh, phi)
    masks = PD.all_keep_masks(ps, Hh, N, P, PD.ffn_widths(sd))
    assert torch.equal(PD.page_encoder(h, sd, ps, Hh, masks, 0.0, phi), want)
    assert torch.equal(PD.page_encoder(h, sd, ps, Hh, None, 0.0, phi), want)
    qkv = torch.from_numpy(rs.standard_normal((N, 3 * P)))
    gw = torch.from_numpy(rs.standard_normal((Hh, 8))) if geometry else None
    ref = PG.attend(qkv, ps, Hh, gw, phi) if geometry else PA.attend(qkv, ps, Hh)
    for keeps in (PD.all_keep_attn(ps, Hh), None):
        out, lse = PD.attend(qkv, ps, Hh, keeps, 0.0, gw, phi)
        assert torch.equal(out, ref[0]) and torch.equal(lse, ref[2])
    # and a real mask changes O, never lse
    keeps = PD.attn_keeps(0.5, 77, ps, Hh)
    out, lse = PD.attend(qkv, ps, Hh, keeps, 0.5, gw, phi)
    assert torch.equal(lse, ref[2]) and not torch.equal(out, ref[0])


# ---------------------------------------------------------------- placement against torch
class MaskMul(torch.nn.Module):
    """stands in for an nn.Dropout: multiplies by a given keep mask times inv"""

    def __init__(self, keep, p):
        super().__init__()
        self.scale = torch.from_numpy(np.asarray(keep, np.float64)) * PD.inv_keep(p)

    def forward(self, x):
        return x * self.scale


@pytest.mark.parametrize("n,P,Hh,M,p", [(1, 8, 2, 16, 0.5), (23, 32, 4, 64, 0.1), (90, 128, 4, 256, 0.5)])
def test_block_of_the_oracle_places_its_three_row_masks_where_torchs_encoder_layer_has_its_dropouts(n, P, Hh, M, p):
    sd = random_sd(5, P, M, 1, seed=n)
    pre = PE.layer_prefix(0)
    ref = torch.nn.TransformerEncoderLayer(P, Hh, M, dropout=0.0, activation="gelu", batch_first=True, norm_first=True,
                                           dtype=torch.float64)
    with torch.no_grad():
        ref.self_attn.in_proj_weight.copy_(sd[pre + "qkv.weight"])
        ref.self_attn.in_proj_bias.zero_()
        ref.self_attn.out_proj.weight.copy_(sd[pre + "out.weight"])
        ref.self_attn.out_proj.bias.copy_(sd[pre + "out.bias"])
        for mine, theirs in (("norm1", ref.norm1), ("norm2", ref.norm2), ("ffn1", ref.linear1), ("ffn2", ref.linear2)):
            theirs.weight.copy_(sd[pre + mine + ".weight"])
            theirs.bias.copy_(sd[pre + mine + ".bias"])
    k1, kh, k2 = PD.row_keep(p, 11, n, P), PD.row_keep(p, 12, n, M), PD.row_keep(p, 13, n, P)
    assert not (k1.all() and kh.all() and k2.all())
    ref.dropout1, ref.dropout, ref.dropout2 = MaskMul(k1, p), MaskMul(kh, p), MaskMul(k2, p)
    ref.train()                                               # (eval mode may take a fused path)
    x = torch.from_numpy(np.random.RandomState(3).standard_normal((n, P)))
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    got = PD.block(xa, sd, pre, [0, n], Hh, (None, k1, kh, k2), p)           # (no attention mask: site 0 off)
    want = ref(xb.unsqueeze(0)).squeeze(0)
    assert got.dtype == torch.float64
    assert float((got - want).detach().abs().max()) < 1e-12 * max(float(want.detach().abs().max()), 1.0)
    g = torch.from_numpy(np.random.RandomState(4).standard_normal((n, P)))
    (got * g).sum().backward()
    (want * g).sum().backward()
    assert float((xa.grad - xb.grad).abs().max()) < 1e-12 * max(float(xb.grad.abs().max()), 1.0)
    plain = PE.block(x, sd, pre, [0, n], Hh)
    assert float((plain - got.detach()).abs().max()) > 1e-3   # the masks are live


# ---------------------------------------------------------------- the kept share
def share_ok(keep, p):
    n = keep.size
    sigma = math.sqrt(p * (1 - p) / n)
    return abs(float(keep.mean()) - (1 - p)) < 5 * sigma


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_kept_share_of_2_to_the_20_consecutive_indices_is_within_five_sigma(p):
    n = 1 << 20
    streams = [PD.page_dropout_seed(engine.dropout_base(123, 1), l, s) for l in (0, 3, 8) for s in range(4) if l < 8 or s == 0]
    assert len(streams) == 9
    for seed in streams:
        # the attention index of a 90-box page, two heads: rows 100 .. 189 of the batch, consecutive (i, a, j) triples
        t = np.arange(n, dtype=np.uint64)
        j, a, i = t % np.uint64(90), (t // np.uint64(90)) % np.uint64(2), t // np.uint64(180)
        idx = ((((np.uint64(100) + i) * np.uint64(2) + a) << np.uint64(32)) | (np.uint64(100) + j))
        assert idx[0] == PD.attn_index(100, 0, 100, 2) and idx[91] == PD.attn_index(100, 1, 101, 2)
        assert share_ok(PD.hash_uniform(seed, idx) >= np.float32(p), p), ("attention", hex(seed))
        assert share_ok(PD.row_keep(p, seed, 1 << 10, 1 << 10), p), ("rows", hex(seed))


# ---------------------------------------------------------------- the options
def test_option_checks_raise_as_specified():
    for opt in ("page_attention_dropout", "page_encoder_dropout"):
        assert weights.check_page_dropout(0, opt) == 0.0 and weights.check_page_dropout(0.25, opt) == 0.25
        assert isinstance(weights.check_page_dropout(np.float32(0.5), opt), float)
        for bad in (1.0, -0.1, float("nan"), True, "p", None, 2):
            with pytest.raises(ValueError, match=opt):
                weights.check_page_dropout(bad, opt)
    base = dict(page_attention_dim=8, page_attention_heads=2, page_encoder_dim=8, page_encoder_heads=2)
    got = weights.page_options(dict(base, page_attention_dropout=0.1, page_encoder_dropout=0.5))
    assert got["page_attention_dropout"] == 0.1 and got["page_encoder_dropout"] == 0.5
    assert weights.page_options(got) == got
    off = weights.page_options({})
    assert off["page_attention_dropout"] == 0.0 and off["page_encoder_dropout"] == 0.0
    with pytest.raises(ValueError, match="page_attention_dropout.*page_attention_dim"):
        weights.page_options(dict(page_encoder_dim=8, page_attention_dropout=0.1))
    with pytest.raises(ValueError, match="page_encoder_dropout.*page_encoder_dim"):
        weights.page_options(dict(page_attention_dim=8, page_encoder_dropout=0.1))
    weights.page_options(dict(page_attention_dropout=0.0, page_encoder_dropout=0))          # rate 0 needs no layer
    # no new state_dict keys, and state_dict_spec does not take the rates
    assert "page_attention_dropout" not in weights.SPEC_OPTIONS and "page_encoder_dropout" not in weights.SPEC_OPTIONS


def test_modules_create_the_dropout_submodule_only_when_the_rate_is_positive():
    a0, a1 = PageAttention(6, 8, 2), PageAttention(6, 8, 2, dropout=0.1)
    e0, e1 = PageEncoder(6, 8, 2, 2), PageEncoder(6, 8, 2, 2, dropout=0.1)
    assert not hasattr(a0, "attn_drop") and isinstance(a1.attn_drop, torch.nn.Dropout) and a1.attn_drop.p == 0.1
    assert not hasattr(e0, "drop") and isinstance(e1.drop, torch.nn.Dropout) and e1.drop.p == 0.1
    assert list(a0.state_dict()) == list(a1.state_dict()) and list(e0.state_dict()) == list(e1.state_dict())
    for bad in (1.0, -0.5):
        with pytest.raises(ValueError, match="page_attention_dropout"):
            PageAttention(6, 8, 2, dropout=bad)
        with pytest.raises(ValueError, match="page_encoder_dropout"):
            PageEncoder(6, 8, 2, dropout=bad)
    kw = dict(page_attention_dim=8, page_attention_heads=2, page_encoder_dim=8, page_encoder_heads=2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = CoVA((1, 1), 64, 4, False, 8, 4, 0, 0.2, None, **kw)
        m = CoVA((1, 1), 64, 4, False, 8, 4, 0, 0.2, None, page_attention_dropout=0.1, page_encoder_dropout=0.3, **kw)
        with pytest.raises(ValueError, match="page_encoder_dropout"):
            CoVA((1, 1), 64, 4, False, 8, 4, 0, 0.2, None, page_encoder_dropout=0.3)
    assert list(m.state_dict()) == list(plain.state_dict())
    assert m.page_attention.attn_drop.p == 0.1 and m.page_encoder.drop.p == 0.3
    assert m._cfg["page_attention_dropout"] == 0.1 and m._cfg["page_encoder_dropout"] == 0.3
    assert plain._cfg["page_attention_dropout"] == 0.0 and not hasattr(plain.page_encoder, "drop")
    names = [n for n, mod in m.named_modules() if isinstance(mod, torch.nn.Dropout)]
    assert engine.PAGE_ATTN_DROP_KEY in names and engine.PAGE_ENC_DROP_KEY in names
