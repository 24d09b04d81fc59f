"""CPU tests of the page encoder (CoVA(page_encoder_dim=P, ...)): the float64 oracle (tests/page_encoder_oracle.py) against
torch's own nn.TransformerEncoderLayer(norm_first=True, activation="gelu", dropout=0) and F.layer_norm, the state_dict
contract of weights.state_dict_spec / weights.seeded_state_dict / models.CoVA with and without the option, every ValueError
of the option table, and the trainer's checkpoint messages (found from the keys, before any device work)."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cova_web_object_detection_amd import weights
from cova_web_object_detection_amd.models import CoVA, PageEncoder
from cova_web_object_detection_amd.trainer import HotPathTrainer
import page_encoder_oracle as PE
from config_cases import make_cfg, ORACLE_CASES, PAGE_SPEC as BASE

N_FEAT = 64 * 9 + 8 + 2
LAYER_KEYS = ["norm1.weight", "norm1.bias", "qkv.weight", "geometry.weight", "out.weight", "out.bias", "norm2.weight",
              "norm2.bias", "ffn1.weight", "ffn1.bias", "ffn2.weight", "ffn2.bias"]


def encoder_keys(L, geometry):
    keys = ["page_encoder.input.weight"]
    for l in range(L):
        keys += ["page_encoder.layers.%d.%s" % (l, k) for k in LAYER_KEYS if geometry or k != "geometry.weight"]
    return keys + ["page_encoder.norm.weight", "page_encoder.norm.bias"]


def random_sd(F_in, P, M, L, heads=1, geometry=False, seed=0):
    rs = np.random.RandomState(seed)
    spec = weights.page_encoder_entries(F_in, P, heads, L, M, geometry)
    return {k: torch.from_numpy(rs.standard_normal(s) * (1.0 if len(s) == 1 else 1.0 / np.sqrt(s[-1]))) for k, s in spec}


# ---------------------------------------------------------------- the oracle against torch's own modules
@pytest.mark.parametrize("n,P,Hh,M", [(1, 8, 2, 16), (23, 32, 4, 64), (90, 128, 4, 256)])
def test_block_of_the_oracle_is_torchs_pre_ln_encoder_layer_on_one_page(n, P, Hh, M):
    sd = random_sd(5, P, M, 1, seed=n)
    p = PE.layer_prefix(0)
    ref = torch.nn.TransformerEncoderLayer(P, Hh, M, dropout=0.0, activation="gelu", batch_first=True, norm_first=True,
                                           dtype=torch.float64)
    with torch.no_grad():
        ref.self_attn.in_proj_weight.copy_(sd[p + "qkv.weight"])
        ref.self_attn.in_proj_bias.zero_()
        ref.self_attn.out_proj.weight.copy_(sd[p + "out.weight"])
        ref.self_attn.out_proj.bias.copy_(sd[p + "out.bias"])
        for mine, theirs in (("norm1", ref.norm1), ("norm2", ref.norm2), ("ffn1", ref.linear1), ("ffn2", ref.linear2)):
            theirs.weight.copy_(sd[p + mine + ".weight"])
            theirs.bias.copy_(sd[p + mine + ".bias"])
    ref.train()                                               # (eval mode may take a fused path; dropout is 0)
    x = torch.from_numpy(np.random.RandomState(3).standard_normal((n, P)))
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    got = PE.block(xa, sd, p, [0, n], Hh)
    want = ref(xb.unsqueeze(0)).squeeze(0)
    assert got.requires_grad and want.requires_grad
    assert got.dtype == torch.float64
    assert float((got - want).detach().abs().max()) < 1e-12 * max(float(want.detach().abs().max()), 1.0)
    g = torch.from_numpy(np.random.RandomState(4).standard_normal((n, P)))
    (got * g).sum().backward()
    (want * g).sum().backward()
    assert float((xa.grad - xb.grad).abs().max()) < 1e-12 * max(float(xb.grad.abs().max()), 1.0)


def test_pages_do_not_see_each_other_and_the_depth_is_read_off_the_keys():
    sd = random_sd(6, 8, 16, 3, seed=2)
    assert PE.n_layers(sd) == 3
    h = torch.from_numpy(np.random.RandomState(5).standard_normal((12, 6)))
    both = PE.page_encoder(h, sd, [0, 7, 7, 12], 2)
    assert torch.equal(both[:7], PE.page_encoder(h[:7], sd, [0, 7], 2))
    assert torch.equal(both[7:], PE.page_encoder(h[7:], sd, [0, 5], 2))
    assert float((both - PE.page_encoder(h, sd, [0, 12], 2)).abs().max()) > 1e-3


@pytest.mark.parametrize("C", [1, 7, 36, 512])
def test_layer_norm_and_gelu_of_the_oracle_are_torchs(C):
    rs = np.random.RandomState(C)
    x = torch.from_numpy(30 + rs.standard_normal((9, C)))
    w, b = torch.from_numpy(rs.standard_normal(C)), torch.from_numpy(rs.standard_normal(C))
    out, mean, rstd = PE.layer_norm(x, w, b, return_stats=True)
    want = F.layer_norm(x, (C,), w, b, 1e-5)
    assert float((out - want).abs().max()) < 1e-12 * max(float(want.abs().max()), 1.0)
    assert torch.allclose(mean, x.mean(1), rtol=0, atol=1e-13)
    assert torch.allclose(rstd, 1 / torch.sqrt(x.var(1, unbiased=False) + 1e-5), rtol=1e-13, atol=0)
    z = torch.from_numpy(np.linspace(-6, 6, 241)).requires_grad_(True)
    assert torch.allclose(PE.gelu(z), F.gelu(z), rtol=0, atol=1e-15)
    PE.gelu(z).sum().backward()
    assert torch.allclose(PE.gelu_grad(z.detach()), z.grad, rtol=0, atol=1e-14)
    assert float(PE.gelu(torch.zeros(1, dtype=torch.float64))) == 0.0 and float(PE.gelu_grad(torch.zeros(1))) == 0.5


# ---------------------------------------------------------------- spec, seeded weights and module keys
@pytest.mark.parametrize("geometry", [False, True])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("P", [0, 8, 128])
def test_spec_key_order_shapes_and_decoder_width(P, L, geometry):
    if P == 0 and geometry:
        with pytest.raises(ValueError, match="page_encoder_geometry"):
            weights.state_dict_spec(page_encoder_dim=0, page_encoder_geometry=True, **BASE)
        return
    Hh = 2
    cfg = dict(BASE, page_context_dim=16, page_attention_dim=8)
    plain = weights.state_dict_spec(**cfg)
    spec = weights.state_dict_spec(page_encoder_dim=P, page_encoder_heads=Hh, page_encoder_layers=L,
                                   page_encoder_geometry=geometry, **cfg)
    if P == 0:
        assert spec == plain
        return
    keys, pkeys = [k for k, _ in spec], [k for k, _ in plain]
    enc = encoder_keys(L, geometry)
    assert [k for k in keys if not k.startswith("page_encoder.")] == pkeys
    i = keys.index(enc[0])
    assert keys[i:i + len(enc)] == enc and keys[i - 1] == "page_attention.qkv.weight"
    assert keys[i + len(enc)] == "decoder.1.weight"
    shapes, M = dict(spec), 2 * P
    assert shapes[enc[0]] == (P, N_FEAT)
    for l in range(L):
        p = "page_encoder.layers.%d." % l
        want = {"norm1.weight": (P,), "norm1.bias": (P,), "qkv.weight": (3 * P, P), "out.weight": (P, P), "out.bias": (P,),
                "norm2.weight": (P,), "norm2.bias": (P,), "ffn1.weight": (M, P), "ffn1.bias": (M,), "ffn2.weight": (P, M),
                "ffn2.bias": (P,)}
        if geometry:
            want["geometry.weight"] = (Hh, 8)
        assert {k[len(p):]: s for k, s in spec if k.startswith(p)} == want
    assert shapes["page_encoder.norm.weight"] == shapes["page_encoder.norm.bias"] == (P,)
    T = N_FEAT + 32 + 16 + 8 + P                              # T = F + D + G + E + P
    assert shapes["decoder.1.weight"] == (T, T) and shapes["decoder.5.weight"] == (4, T)
    assert dict(plain)["decoder.1.weight"] == (T - P, T - P)
    wide = dict(weights.state_dict_spec(page_encoder_dim=P, page_encoder_heads=Hh, page_encoder_ffn_dim=12, **cfg))
    assert wide["page_encoder.layers.0.ffn1.weight"] == (12, P) and wide["page_encoder.layers.0.ffn2.weight"] == (P, 12)


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_with_the_option_off_spec_and_seeded_weights_are_unchanged(name):
    roi, _, _, _, hidden, bbox_hidden, seed = ORACLE_CASES[name]
    for context in (True, False):
        cfg = {k: v for k, v in make_cfg(roi, hidden, bbox_hidden, use_context=context).items() if k != "drop_prob"}
        off = dict(page_encoder_dim=0, page_encoder_heads=3, page_encoder_layers=5, page_encoder_ffn_dim=64)
        assert weights.state_dict_spec(**cfg, **off) == weights.state_dict_spec(**cfg)
        a, b = weights.seeded_state_dict(seed, **cfg), weights.seeded_state_dict(seed, **cfg, **off)
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
        # and with it on, everything in front of the encoder keeps its bits (the stream is drawn in state_dict order)
        on = weights.seeded_state_dict(seed, page_encoder_dim=8, page_encoder_heads=2, **cfg)
        for k in list(a)[:list(a).index("decoder.1.weight")]:
            assert torch.equal(a[k], on[k]), k


def test_seeded_weights_follow_the_linear_and_affine_rules_and_geometry_draws_nothing():
    kw = dict(page_encoder_dim=8, page_encoder_heads=2, page_encoder_layers=2, **BASE)
    sd, geo = weights.seeded_state_dict(5, **kw), weights.seeded_state_dict(5, page_encoder_geometry=True, **kw)
    assert [k for k in sd if k.startswith("page_encoder.")] == encoder_keys(2, False)
    assert [k for k in geo if k.startswith("page_encoder.")] == encoder_keys(2, True)
    for k, v in geo.items():
        if k.endswith("geometry.weight"):
            assert tuple(v.shape) == (2, 8) and not v.any()
        else:
            assert torch.equal(v, sd[k]), k                   # zero without drawing from the stream
    for k in encoder_keys(2, False):
        v = sd[k]
        if ".norm" in k and k.endswith("weight"):
            assert float(v.min()) >= 0.5 and float(v.max()) <= 1.5 and float((v - 1).abs().min()) > 0
        elif ".norm" in k:
            assert float(v.abs().max()) < 1.0 and float(v.abs().min()) > 0
        elif v.dim() == 2:
            bound = 1.0 / np.sqrt(v.shape[1])
            assert 0.5 * bound < float(v.abs().max()) <= bound
        else:
            assert float(v.abs().max()) <= 0.05


@pytest.mark.parametrize("geometry", [False, True])
def test_module_state_dict_equals_the_spec(geometry):
    kw = dict(page_encoder_dim=8, page_encoder_heads=2, page_encoder_layers=2, page_encoder_ffn_dim=12,
              page_encoder_geometry=geometry)
    extra = dict(page_context_dim=16, page_attention_dim=8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        build = lambda **more: CoVA((3, 3), 64, 4, True, 32, 8, 2, 0.2, None, **extra, **more)
        m, m0, mz = build(**kw), build(), build(page_encoder_dim=0, page_encoder_layers=4)
    spec = weights.state_dict_spec(**BASE, **extra, **kw)
    assert list(m.state_dict()) == [k for k, _ in spec]
    assert all(tuple(m.state_dict()[k].shape) == s for k, s in spec)
    assert isinstance(m.page_encoder, PageEncoder) and m._cfg["page_encoder_dim"] == 8 and m._cfg["page_encoder_ffn_dim"] == 12
    names = [n for n, _ in m.named_children()]
    assert names.index("page_encoder") == names.index("decoder") - 1 == names.index("page_attention") + 1
    if geometry:
        assert not m.state_dict()["page_encoder.layers.1.geometry.weight"].any()
    assert list(m0.state_dict()) == [k for k, _ in weights.state_dict_spec(**BASE, **extra)]
    assert [n for n, _ in m0.named_modules()] == [n for n, _ in mz.named_modules()]
    assert not any("page_encoder" in n for n, _ in m0.named_modules()) and m0._cfg["page_encoder_dim"] == 0
    assert [n for n, _ in m.named_modules() if "page_encoder" not in n] == [n for n, _ in m0.named_modules()]


def test_page_encoder_module_parameters_and_no_cpu_fallback():
    layer = PageEncoder(24, 8, 2, layers=2)
    assert list(layer.state_dict()) == [k[len("page_encoder."):] for k in encoder_keys(2, False)]
    assert (layer.dim, layer.heads, layer.n_layers, layer.ffn_dim) == (8, 2, 2, 16)
    with pytest.raises(ValueError):
        PageEncoder(24, 0)
    with pytest.raises(ValueError, match="page_encoder"):
        PageEncoder(24, 8, 3)
    with pytest.raises(RuntimeError, match="MI355X"):
        layer(torch.zeros(3, 24), torch.tensor([0, 3]))


# ---------------------------------------------------------------- refusals
BAD = [dict(page_encoder_dim=-4), dict(page_encoder_dim=516), dict(page_encoder_dim=1.5), dict(page_encoder_dim=True),
       dict(page_encoder_dim=None), dict(page_encoder_dim="16"),
       dict(page_encoder_dim=16, page_encoder_heads=0), dict(page_encoder_dim=16, page_encoder_heads=3),
       dict(page_encoder_dim=16, page_encoder_heads=True), dict(page_encoder_dim=16, page_encoder_heads=1.0),
       dict(page_encoder_dim=24, page_encoder_heads=4), dict(page_encoder_dim=6), dict(page_encoder_dim=8, page_encoder_heads=4),
       dict(page_encoder_dim=512, page_encoder_heads=2), dict(page_encoder_dim=2),
       dict(page_encoder_dim=16, page_encoder_layers=0), dict(page_encoder_dim=16, page_encoder_layers=9),
       dict(page_encoder_dim=16, page_encoder_layers=2.0), dict(page_encoder_dim=16, page_encoder_layers=True),
       dict(page_encoder_dim=0, page_encoder_layers=0), dict(page_encoder_dim=0, page_encoder_layers=9),
       dict(page_encoder_dim=16, page_encoder_ffn_dim=0), dict(page_encoder_dim=16, page_encoder_ffn_dim=6),
       dict(page_encoder_dim=16, page_encoder_ffn_dim=2052), dict(page_encoder_dim=16, page_encoder_ffn_dim=32.0),
       dict(page_encoder_dim=16, page_encoder_ffn_dim=True), dict(page_encoder_dim=0, page_encoder_ffn_dim=6),
       dict(page_encoder_dim=16, page_encoder_geometry=1), dict(page_encoder_dim=16, page_encoder_geometry=None),
       dict(page_encoder_dim=0, page_encoder_geometry=True), dict(page_encoder_geometry=True)]


@pytest.mark.parametrize("bad", BAD, ids=[str(sorted(b.items())) for b in BAD])
def test_every_value_error_of_the_option_table(bad):
    with pytest.raises(ValueError, match="page_encoder"):
        weights.state_dict_spec(**bad)
    with pytest.raises(ValueError, match="page_encoder"):
        weights.seeded_state_dict(1, **bad)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="page_encoder"):
            CoVA((3, 3), 64, 4, **bad)
    with pytest.raises(ValueError, match="page_encoder"):
        HotPathTrainer(dict(BASE, drop_prob=0.2, **bad), {}, "cuda:63")


def test_the_accepted_range():
    ok = [((0,), (0, 1, 1, 0, False)), ((0, 7, 8), (0, 7, 8, 0, False)), ((4,), (4, 1, 1, 8, False)),
          ((128, 4, 2), (128, 4, 2, 256, False)), ((512, 4, 8, 2048, True), (512, 4, 8, 2048, True)),
          ((np.int64(24), np.int32(2), np.int64(3), np.int64(4), np.bool_(True)), (24, 2, 3, 4, True))]
    for args, want in ok:
        assert weights.check_page_encoder(*args) == want
        assert weights.check_page_encoder(*want) == want      # a checked tuple passes again (the trainer stores it in its cfg)
    assert weights.state_dict_spec(page_encoder_dim=0, page_encoder_ffn_dim=0, **BASE) == weights.state_dict_spec(**BASE)
    # the head-width rule is the page attention's own, not a copy: one function states both
    for e, h in ((16, 3), (24, 4), (6, 1), (512, 2)):
        with pytest.raises(ValueError) as a:
            weights.check_page_attention(e, h)
        with pytest.raises(ValueError) as b:
            weights.check_page_encoder(e, h)
        assert str(a.value).replace("page_attention", "page_encoder") == str(b.value)


def test_trainer_names_the_option_on_a_checkpoint_of_another_kind():
    """Every mismatch is found from the keys and shapes, before the trainer touches a device."""
    cfg = dict(BASE, drop_prob=0.2)
    on = dict(page_encoder_dim=16, page_encoder_heads=2, page_encoder_layers=2)
    with_sd = weights.seeded_state_dict(3, **BASE, **on)
    without_sd = weights.seeded_state_dict(3, **BASE)
    geo_sd = weights.seeded_state_dict(3, page_encoder_geometry=True, **BASE, **on)
    nowhere = "cuda:63"                                      # never reached
    with pytest.raises(ValueError, match=r"page_encoder_dim=16.*lacks.*page_encoder\.input\.weight"):
        HotPathTrainer(dict(cfg, **on), without_sd, nowhere)
    with pytest.raises(ValueError, match=r"page_encoder_dim=0.*holds.*page_encoder\.input\.weight"):
        HotPathTrainer(cfg, with_sd, nowhere)
    with pytest.raises(ValueError, match=r"page_encoder_dim=8.*\(16, 586\).*page_encoder_dim=16"):
        HotPathTrainer(dict(cfg, **dict(on, page_encoder_dim=8)), with_sd, nowhere)
    with pytest.raises(ValueError, match=r"page_encoder_layers=3.*holds 2 layer.*page_encoder_layers=2"):
        HotPathTrainer(dict(cfg, **dict(on, page_encoder_layers=3)), with_sd, nowhere)
    with pytest.raises(ValueError, match=r"page_encoder_layers=1.*holds 2 layer"):
        HotPathTrainer(dict(cfg, **dict(on, page_encoder_layers=1)), with_sd, nowhere)
    with pytest.raises(ValueError, match=r"page_encoder_ffn_dim=64.*\(32, 16\).*page_encoder_ffn_dim=32"):
        HotPathTrainer(dict(cfg, page_encoder_ffn_dim=64, **on), with_sd, nowhere)
    with pytest.raises(ValueError, match=r"page_encoder_geometry=True.*lacks.*layers\.0\.geometry\.weight"):
        HotPathTrainer(dict(cfg, page_encoder_geometry=True, **on), with_sd, nowhere)
    with pytest.raises(ValueError, match=r"page_encoder_geometry=False.*holds.*layers\.0\.geometry\.weight"):
        HotPathTrainer(dict(cfg, **on), geo_sd, nowhere)
    with pytest.raises(ValueError, match=r"page_encoder_heads=4.*\(2, 8\)"):
        HotPathTrainer(dict(cfg, page_encoder_geometry=True, **dict(on, page_encoder_heads=4)), geo_sd, nowhere)
