"""state_dict contract of the hot path and a platform-stable seeded weight generator.

The reference builds its parameters from ``torchvision.models.resnet18(pretrained=True)``
truncated to ``children()[:-5]`` (reference models.py:49-51) plus the modules created in
``CoVA.__init__`` (models.py:65-90) and ``GraphAttentionLayer.__init__`` (models.py:156-165).
ImageNet weights are not available offline, so parity work and the benchmark use weights
drawn from a fixed numpy ``RandomState`` stream (legacy MT19937 => identical on every box),
shaped exactly like the reference's 50 ``state_dict`` entries.
"""
import inspect
from collections import OrderedDict, namedtuple

import numpy as np
import torch

BACKBONE_CHANNELS = 64  # ResNet-18 conv1/layer1 width (models.py:49-51 keeps conv1..layer1)
BACKBONE_STRIDE = 4     # conv1 stride 2 * maxpool stride 2
EDGE_FEATURES = 8       # relative-geometry features per edge (include/cova_hip.h, cova_edge_geometry)
ATTENTION_MODES = ("gat", "gatv2")   # the reference's static score | a . LeakyReLU(Wh_i + Wh_j) + b (cova_gat2_fwd)


def check_attention(attention):
    if attention not in ATTENTION_MODES:
        raise ValueError("attention must be one of %s, got %r" % (ATTENTION_MODES, attention))
    return attention


def check_attention_dropout(p):
    """Rate of the dropout on the attention coefficients (cova_gat_fwd_drop): a real number in [0, 1) -> float."""
    try:
        ok = not isinstance(p, bool) and 0.0 <= float(p) < 1.0          # (NaN fails both comparisons)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("attention_dropout must be a number in [0, 1), got %r" % (p,))
    return float(p)


PAGE_CONTEXT_MAX = 512               # channels of the page readout's vector (RO_MAX_G of csrc/readout.hip)
PAGE_READOUT_KEYS = ("page_readout.W.weight", "page_readout.attention_layer.weight", "page_readout.attention_layer.bias")


def check_page_context_dim(g):
    """Width of the page readout's vector (cova_page_readout_fwd): an int in [0, 512], 0 = no readout -> int."""
    if isinstance(g, bool) or not isinstance(g, (int, np.integer)) or not 0 <= g <= PAGE_CONTEXT_MAX:
        raise ValueError("page_context_dim must be an integer in [0, %d] (0: no page readout), got %r"
                         % (PAGE_CONTEXT_MAX, g))
    return int(g)


PAGE_ATTENTION_MAX = 512             # channels of the page attention's output (PA_MAX_E of csrc/page_attn.hip)
PAGE_ATTENTION_MAX_HEAD = 128        # columns of one head (PA_MAX_DH)
PAGE_ATTENTION_KEY = "page_attention.qkv.weight"


def _check_width_and_heads(e, heads, dim_name, heads_name, off):
    """The rule the page attention kernels set for a width and its head count (cova_page_attn_fwd), shared by every layer
    that runs them: E an int in [0, 512] (0 = off), Hh an int >= 1 that divides E, E / Hh a multiple of 4 in [4, 128]."""
    for name, v in ((dim_name, e), (heads_name, heads)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s must be an integer, got %r" % (name, v))
    e, heads = int(e), int(heads)
    if not 0 <= e <= PAGE_ATTENTION_MAX:
        raise ValueError("%s must be an integer in [0, %d] (0: %s), got %r" % (dim_name, PAGE_ATTENTION_MAX, off, e))
    if heads < 1:
        raise ValueError("%s must be at least 1, got %r" % (heads_name, heads))
    if e > 0:
        if e % heads:
            raise ValueError("%s=%d does not divide %s=%d" % (heads_name, heads, dim_name, e))
        dh = e // heads
        if dh % 4 or not 4 <= dh <= PAGE_ATTENTION_MAX_HEAD:
            raise ValueError("%s / %s = %d: the head width must be a multiple of 4 in "
                             "[4, %d]" % (dim_name, heads_name, dh, PAGE_ATTENTION_MAX_HEAD))
    return e, heads


def check_page_attention(e, heads=1):
    """Width and head count of the page self-attention (cova_page_attn_fwd): E an int in [0, 512] (0 = off), Hh an int >= 1
    that divides E, the head width E / Hh a multiple of 4 in [4, 128] -> (E, Hh)."""
    return _check_width_and_heads(e, heads, "page_attention_dim", "page_attention_heads", "no page attention")


PAGE_ATTENTION_GEO_KEY = "page_attention.geometry.weight"


def check_page_attention_geometry(geometry, e):
    """``page_attention_geometry`` (cova_page_attn_fwd_geo) against the layer's width: the option needs the layer -> bool."""
    if not isinstance(geometry, (bool, np.bool_)):
        raise ValueError("page_attention_geometry must be a bool, got %r" % (geometry,))
    if geometry and e <= 0:
        raise ValueError("page_attention_geometry=True needs page_attention_dim > 0 (the bias belongs to the page "
                         "attention's scores), got page_attention_dim=%r" % (e,))
    return bool(geometry)


PAGE_ENCODER_MAX_LAYERS = 8
PAGE_ENCODER_MAX_FFN = 2048          # columns of the feed-forward part (a multiple of 4: the float4 rows of cova_gelu_fwd)
PAGE_ENCODER_EPS = 1e-5              # nn.LayerNorm's default
PAGE_ENCODER_INPUT_KEY = "page_encoder.input.weight"
PAGE_ENCODER_NORM_KEYS = ("page_encoder.norm.weight", "page_encoder.norm.bias")


def check_page_encoder(dim, heads=1, layers=1, ffn_dim=None, geometry=False):
    """The page encoder's options -> (P, Hh, L, M, geometry).  P and Hh follow the page attention's rule
    (its kernels run every layer); L an int in [1, 8], validated with P = 0 too; M (None: 2 P) a multiple of 4 in [4, 2048];
    ``geometry`` a bool that needs P > 0."""
    dim, heads = _check_width_and_heads(dim, heads, "page_encoder_dim", "page_encoder_heads", "no page encoder")
    if isinstance(layers, bool) or not isinstance(layers, (int, np.integer)) or not 1 <= layers <= PAGE_ENCODER_MAX_LAYERS:
        raise ValueError("page_encoder_layers must be an integer in [1, %d], got %r" % (PAGE_ENCODER_MAX_LAYERS, layers))
    if ffn_dim is None or (dim == 0 and not isinstance(ffn_dim, bool) and isinstance(ffn_dim, (int, np.integer)) and ffn_dim == 0):
        ffn_dim = 2 * dim                  # (0 with P = 0 is this function's own result: a checked tuple passes again)
    elif (isinstance(ffn_dim, bool) or not isinstance(ffn_dim, (int, np.integer)) or ffn_dim % 4
          or not 4 <= ffn_dim <= PAGE_ENCODER_MAX_FFN):
        raise ValueError("page_encoder_ffn_dim must be a multiple of 4 in [4, %d] (None: 2 * page_encoder_dim), got %r"
                         % (PAGE_ENCODER_MAX_FFN, ffn_dim))
    if not isinstance(geometry, (bool, np.bool_)):
        raise ValueError("page_encoder_geometry must be a bool, got %r" % (geometry,))
    if geometry and dim <= 0:
        raise ValueError("page_encoder_geometry=True needs page_encoder_dim > 0 (the bias belongs to the encoder's "
                         "attention scores), got page_encoder_dim=%r" % (dim,))
    return dim, heads, int(layers), int(ffn_dim), bool(geometry)


PAGE_ATTENTION_DROPOUT_OPTION = "page_attention_dropout"
PAGE_ENCODER_DROPOUT_OPTION = "page_encoder_dropout"


def check_page_dropout(p, option, width=None):
    """Rate of a page layer's dropout (``page_attention_dropout`` on the page attention's probabilities,
    cova_page_attn_fwd_drop; ``page_encoder_dropout``, torch's ``dropout=`` of nn.TransformerEncoderLayer, on the four
    sites of every encoder block): check_attention_dropout's rule, a real number in [0, 1) -> float.  ``option`` names the
    cfg entry in the error.  With ``width`` (the layer's page_attention_dim / page_encoder_dim) a rate > 0 needs the layer."""
    try:
        ok = not isinstance(p, bool) and 0.0 <= float(p) < 1.0          # (NaN fails both comparisons)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s must be a number in [0, 1), got %r" % (option, p))
    if width is not None and float(p) > 0.0 and width <= 0:
        layer = option[:-len("dropout")] + "dim"
        raise ValueError("%s=%r needs %s > 0 (the dropout belongs to that layer), got %s=%r" % (option, p, layer, layer, width))
    return float(p)


# The page layers' dropout rates: no weights, so not arguments of state_dict_spec (as ``attention_dropout``).
PAGE_DROPOUT_DEFAULTS = ((PAGE_ATTENTION_DROPOUT_OPTION, 0.0), (PAGE_ENCODER_DROPOUT_OPTION, 0.0))

# Every page option that shapes the state_dict with its default, in the order of CoVA's and state_dict_spec's arguments.
PAGE_OPTION_DEFAULTS = (("page_context_dim", 0), ("page_attention_dim", 0), ("page_attention_heads", 1),
                        ("page_attention_geometry", False), ("page_encoder_dim", 0), ("page_encoder_heads", 1),
                        ("page_encoder_layers", 1), ("page_encoder_ffn_dim", None), ("page_encoder_geometry", False))
PAGE_ENCODER_OPTIONS = tuple(k for k, _ in PAGE_OPTION_DEFAULTS if k.startswith("page_encoder_"))   # check_page_encoder's order


def page_options(cfg):
    """The page options of a cfg-like mapping (missing ones at their defaults), each through its check_* function -> a
    dict of all nine and the two dropout rates (PAGE_DROPOUT_DEFAULTS), normalised.  A normalised dict passes again
    unchanged."""
    v = {k: cfg.get(k, default) for k, default in PAGE_OPTION_DEFAULTS}
    out = {"page_context_dim": check_page_context_dim(v["page_context_dim"])}
    out["page_attention_dim"], out["page_attention_heads"] = check_page_attention(v["page_attention_dim"],
                                                                                  v["page_attention_heads"])
    out["page_attention_geometry"] = check_page_attention_geometry(v["page_attention_geometry"], out["page_attention_dim"])
    out.update(zip(PAGE_ENCODER_OPTIONS, check_page_encoder(*(v[k] for k in PAGE_ENCODER_OPTIONS))))
    for (k, default), width in zip(PAGE_DROPOUT_DEFAULTS, ("page_attention_dim", "page_encoder_dim")):
        out[k] = check_page_dropout(cfg.get(k, default), k, out[width])
    return out


# The head's context layers: what stands behind the F own features of a box in the decoder's input, in COLUMN order, which
# is also the order of their state_dict entries (between the additional-feature BatchNorm and the decoder) and the order
# in which engine.model_bwd runs their backwards.  That last order is part of the result: every layer ACCUMULATES its data
# gradient into dcomb[:, :F], float sums do not commute, so the GAT adds first, then the readout, the page attention and
# the encoder.  It is stated here and nowhere else; a new layer goes at the end.
#   key: the layer's entry of engine.model_fwd's saved dict;  letter: its width's entry there;  option: the cfg entry that
#   sets the width;  prefix: of its state_dict keys;  paged: reads the batch's page table;  width: cfg -> columns (0: off)
ContextLayer = namedtuple("ContextLayer", "key letter option prefix paged width")
CONTEXT_LAYERS = (
    ContextLayer("gat", "D", "hidden_dim", "gat.", False, lambda cfg: cfg["hidden_dim"] if cfg["use_context"] else 0),
    ContextLayer("readout", "G", "page_context_dim", "page_readout.", True, lambda cfg: cfg.get("page_context_dim", 0)),
    ContextLayer("page_attn", "E", "page_attention_dim", "page_attention.", True,
                 lambda cfg: cfg.get("page_attention_dim", 0)),
    ContextLayer("page_enc", "P", "page_encoder_dim", "page_encoder.", True, lambda cfg: cfg.get("page_encoder_dim", 0)),
)
HeadLayout = namedtuple("HeadLayout", "n_vis Hd A F layers T page_option")


def head_layout(cfg, n_vis):
    """Columns of the decoder's input for ``cfg`` over ``n_vis`` visual columns: [visual | bbox Hd | additional A] = the F
    own features, then the context layers.  ``layers`` = ((key, offset, width), ...) in CONTEXT_LAYERS order, width 0 for
    a layer that is off; ``T`` the total width; ``page_option`` the option of the first layer on that reads the page table
    (None: the batch needs none).  The one place that adds the widths up."""
    Hd, A = cfg["bbox_hidden_dim"], cfg["n_additional_feat"]
    T = F = n_vis + Hd + A
    layers, page_option = [], None
    for layer in CONTEXT_LAYERS:
        width = layer.width(cfg)
        layers.append((layer.key, T, width))
        T += width
        if width > 0 and layer.paged and page_option is None:
            page_option = layer.option
    return HeadLayout(n_vis, Hd, A, F, tuple(layers), T, page_option)


def page_encoder_layer_prefix(l):
    return "page_encoder.layers.%d." % l


def page_encoder_entries(n_feat, dim, heads, layers, ffn_dim, geometry):
    """Ordered (key, shape) list of the page encoder: the input projection, per layer norm1, qkv, (geometry,) out, norm2,
    ffn1, ffn2, then the final norm."""
    spec = [(PAGE_ENCODER_INPUT_KEY, (dim, n_feat))]
    for l in range(layers):
        p = page_encoder_layer_prefix(l)
        spec += [(p + "norm1.weight", (dim,)), (p + "norm1.bias", (dim,)), (p + "qkv.weight", (3 * dim, dim))]
        if geometry:
            spec.append((p + "geometry.weight", (heads, EDGE_FEATURES)))
        spec += [(p + "out.weight", (dim, dim)), (p + "out.bias", (dim,)),
                 (p + "norm2.weight", (dim,)), (p + "norm2.bias", (dim,)),
                 (p + "ffn1.weight", (ffn_dim, dim)), (p + "ffn1.bias", (ffn_dim,)),
                 (p + "ffn2.weight", (dim, ffn_dim)), (p + "ffn2.bias", (dim,))]
    return spec + [(PAGE_ENCODER_NORM_KEYS[0], (dim,)), (PAGE_ENCODER_NORM_KEYS[1], (dim,))]


def is_layernorm_key(key):
    """A LayerNorm affine parameter of the page encoder (``...norm1.``, ``...norm2.``, ``page_encoder.norm.``)."""
    return key.startswith("page_encoder.") and key.rsplit(".", 2)[-2] in ("norm", "norm1", "norm2")


def attention_of(weight, D, prefix="gat."):
    """The scoring mode an ``attention_layer.weight`` belongs to, by its width: [1, 2D] is 'gat', [1, D] is 'gatv2'."""
    width = int(weight.shape[-1]) if weight.dim() else -1
    if width == 2 * D:
        return "gat"
    if width == D:
        return "gatv2"
    raise ValueError("%sattention_layer.weight has shape %s: neither [1, %d] (attention='gat') nor [1, %d] "
                     "(attention='gatv2')" % (prefix, tuple(weight.shape), 2 * D, D))


def _bn_entries(prefix, c):
    return [
        (prefix + "weight", (c,)),
        (prefix + "bias", (c,)),
        (prefix + "running_mean", (c,)),
        (prefix + "running_var", (c,)),
        (prefix + "num_batches_tracked", ()),
    ]


def check_backbone_layers(backbone="resnet18", backbone_layers=1):
    """1 = conv1..layer1 (the reference's children()[:-5]); 2 = also ResNet-18's layer2 (children()[:-4])."""
    if backbone_layers not in (1, 2) or isinstance(backbone_layers, bool):
        raise ValueError("backbone_layers must be 1 (the reference, models.py:49-51) or 2 (resnet18 layer2 kept)")
    if backbone_layers == 2 and backbone != "resnet18":
        raise ValueError("backbone_layers=2 is built for backbone='resnet18' only")


def backbone_channels(backbone="resnet18", backbone_layers=1):
    """Channels of the truncated ResNet's output: layer1 of ResNet-18 keeps 64, of ResNet-50 expands to 256; ResNet-18's
    layer2 has 128."""
    if backbone == "resnet18":
        check_backbone_layers(backbone, backbone_layers)
        return 2 * BACKBONE_CHANNELS if backbone_layers == 2 else BACKBONE_CHANNELS
    if backbone == "resnet50":
        return 4 * BACKBONE_CHANNELS
    raise ValueError("backbone must be 'resnet18' (the reference, models.py:49) or 'resnet50' (extension)")


def gat_prefixes(n_heads=1, n_gat_layers=1):
    """state_dict prefixes of the attention heads, [layer][head].  One single-head layer keeps the
    reference's keys (``gat.W_i.weight`` ..., models.py:78-79,161-165); the multi-head / stacked
    extension nests them as ``gat.layers.<l>.heads.<h>.``."""
    if n_heads == 1 and n_gat_layers == 1:
        return [["gat."]]
    return [["gat.layers.%d.heads.%d." % (l, h) for h in range(n_heads)] for l in range(n_gat_layers)]


def state_dict_spec(roi_output_size=(3, 3), n_classes=4, use_context=True, hidden_dim=384,
                    bbox_hidden_dim=32, n_additional_feat=0, backbone="resnet18", n_heads=1,
                    n_gat_layers=1, backbone_layers=1, edge_geometry=False, attention="gat", page_context_dim=0,
                    page_attention_dim=0, page_attention_heads=1, page_attention_geometry=False, page_encoder_dim=0,
                    page_encoder_heads=1, page_encoder_layers=1, page_encoder_ffn_dim=None, page_encoder_geometry=False):
    """Ordered (key, shape) list, identical to ``reference CoVA(...).state_dict()`` for the defaults.

    Extensions (BASELINE.json configs[2], configs[4]; absent from the reference, defaults keep its
    behaviour): ``backbone="resnet50"`` = torchvision resnet50 ``children()[:-5]`` (3 Bottleneck
    blocks, 256 output channels, torchvision's key names); ``n_heads`` / ``n_gat_layers`` = several
    GraphAttentionLayer heads of hidden_dim/n_heads channels each, concatenated, stacked n_gat_layers
    times (layer 0 reads the n_feat own features, later layers the previous layer's hidden_dim);
    ``backbone_layers=2`` = resnet18 ``children()[:-4]``: layer2 (two BasicBlocks, 64 -> 128 channels at stride 2, block 0
    with the 1x1 downsample) under ``convnet.5.`` with torchvision's key names;
    ``edge_geometry=True`` = one ``edge_layer.weight`` [1, 8] per attention head, behind its ``attention_layer.bias`` (W_i and
    W_j stay adjacent): the weights of the relative-geometry term of the attention score (cova_edge_geometry);
    ``attention="gatv2"`` = every ``attention_layer.weight`` is [1, hidden_dim/n_heads] instead of [1, 2 hidden_dim/n_heads]
    (the GATv2 score a . LeakyReLU(Wh_i + Wh_j) + b, cova_gat2_fwd): the shape only, keys and their order are unchanged;
    ``page_context_dim=G`` > 0 = the page readout (cova_page_readout_fwd; independent of ``use_context``): behind the GAT's
    entries and in front of the decoder's, ``page_readout.W.weight`` [G, n_feat], ``page_readout.attention_layer.weight``
    [1, G] and ``page_readout.attention_layer.bias`` [1]; the decoder is G columns wider;
    ``page_attention_dim=E`` > 0 = the page self-attention (cova_page_attn_fwd; independent of ``use_context`` and of
    ``page_context_dim``): behind the readout's entries and in front of the decoder's, ``page_attention.qkv.weight``
    [3E, n_feat], the same shape for every ``page_attention_heads``; the decoder is E columns wider;
    ``page_attention_geometry=True`` (needs ``page_attention_dim`` > 0) = ``page_attention.geometry.weight``
    [page_attention_heads, 8] directly behind ``page_attention.qkv.weight``: per head the weights of the relative-geometry
    bias of the attention scores (cova_page_attn_fwd_geo); the decoder's width is unchanged;
    ``page_encoder_dim=P`` > 0 = the page encoder (independent of ``use_context``, ``page_context_dim`` and
    ``page_attention_dim``): behind the page attention's entries and in front of the decoder's,
    ``page_encoder.input.weight`` [P, n_feat], then for each of ``page_encoder_layers`` layers under
    ``page_encoder.layers.<l>.``: ``norm1.weight`` / ``.bias`` [P], ``qkv.weight`` [3P, P], ``geometry.weight``
    [page_encoder_heads, 8] (``page_encoder_geometry=True`` only), ``out.weight`` [P, P], ``out.bias`` [P], ``norm2.weight`` /
    ``.bias`` [P], ``ffn1.weight`` [M, P], ``ffn1.bias`` [M], ``ffn2.weight`` [P, M], ``ffn2.bias`` [P] with M =
    ``page_encoder_ffn_dim`` (None: 2 P), then ``page_encoder.norm.weight`` / ``.bias`` [P]; the decoder is P columns wider."""
    check_backbone_layers(backbone, backbone_layers)
    check_attention(attention)
    page = page_options(locals())
    c = BACKBONE_CHANNELS
    spec = [("convnet.0.weight", (c, 3, 7, 7))]
    spec += _bn_entries("convnet.1.", c)
    if backbone == "resnet18":
        for blk in (0, 1):
            p = "convnet.4.%d." % blk
            spec.append((p + "conv1.weight", (c, c, 3, 3)))
            spec += _bn_entries(p + "bn1.", c)
            spec.append((p + "conv2.weight", (c, c, 3, 3)))
            spec += _bn_entries(p + "bn2.", c)
    else:
        cout = backbone_channels(backbone)
        for blk in (0, 1, 2):
            p = "convnet.4.%d." % blk
            cin = c if blk == 0 else cout
            spec.append((p + "conv1.weight", (c, cin, 1, 1)))
            spec += _bn_entries(p + "bn1.", c)
            spec.append((p + "conv2.weight", (c, c, 3, 3)))
            spec += _bn_entries(p + "bn2.", c)
            spec.append((p + "conv3.weight", (cout, c, 1, 1)))
            spec += _bn_entries(p + "bn3.", cout)
            if blk == 0:
                spec.append((p + "downsample.0.weight", (cout, c, 1, 1)))
                spec += _bn_entries(p + "downsample.1.", cout)
    if backbone_layers == 2:
        c2 = 2 * c
        for blk in (0, 1):
            p = "convnet.5.%d." % blk
            spec.append((p + "conv1.weight", (c2, c if blk == 0 else c2, 3, 3)))
            spec += _bn_entries(p + "bn1.", c2)
            spec.append((p + "conv2.weight", (c2, c2, 3, 3)))
            spec += _bn_entries(p + "bn2.", c2)
            if blk == 0:
                spec.append((p + "downsample.0.weight", (c2, c, 1, 1)))
                spec += _bn_entries(p + "downsample.1.", c2)
    n_visual = backbone_channels(backbone, backbone_layers) * roi_output_size[0] * roi_output_size[1]
    layout = head_layout(dict(page, use_context=use_context, hidden_dim=hidden_dim, bbox_hidden_dim=bbox_hidden_dim,
                              n_additional_feat=n_additional_feat), n_visual)
    n_feat, n_total = layout.F, layout.T
    if bbox_hidden_dim > 0:
        spec += [("bbox_feat_encoder.0.weight", (bbox_hidden_dim, 5)),
                 ("bbox_feat_encoder.0.bias", (bbox_hidden_dim,))]
        spec += _bn_entries("bbox_feat_encoder.1.", bbox_hidden_dim)
    if n_additional_feat > 0:
        spec += _bn_entries("bn_additional_feat.", n_additional_feat)
    if use_context:
        if hidden_dim % n_heads:
            raise ValueError("hidden_dim must be divisible by n_heads")
        dh = hidden_dim // n_heads
        for l, heads in enumerate(gat_prefixes(n_heads, n_gat_layers)):
            fin = n_feat if l == 0 else hidden_dim
            for p in heads:
                spec += [(p + "W_i.weight", (dh, fin)),
                         (p + "W_j.weight", (dh, fin)),
                         (p + "attention_layer.weight", (1, dh if attention == "gatv2" else 2 * dh)),
                         (p + "attention_layer.bias", (1,))]
                if edge_geometry:
                    spec.append((p + "edge_layer.weight", (1, EDGE_FEATURES)))
    G, E = page["page_context_dim"], page["page_attention_dim"]
    if G > 0:
        spec += [(PAGE_READOUT_KEYS[0], (G, n_feat)), (PAGE_READOUT_KEYS[1], (1, G)), (PAGE_READOUT_KEYS[2], (1,))]
    if E > 0:
        spec.append((PAGE_ATTENTION_KEY, (3 * E, n_feat)))
        if page["page_attention_geometry"]:
            spec.append((PAGE_ATTENTION_GEO_KEY, (page["page_attention_heads"], EDGE_FEATURES)))
    if page["page_encoder_dim"] > 0:
        spec += page_encoder_entries(n_feat, *(page[k] for k in PAGE_ENCODER_OPTIONS))
    spec += [("decoder.1.weight", (n_total, n_total)), ("decoder.1.bias", (n_total,))]
    spec += _bn_entries("decoder.2.", n_total)
    spec += [("decoder.5.weight", (n_classes, n_total)), ("decoder.5.bias", (n_classes,))]
    return spec


SPEC_OPTIONS = tuple(inspect.signature(state_dict_spec).parameters)     # the cfg entries that shape the state_dict


def seeded_state_dict(seed=123, logit_gain=1.0, **cfg):
    """Deterministic weights for every entry of :func:`state_dict_spec`.

    Conv weights ~ N(0, 2/fan_out) (the scheme torchvision's ResNet uses), Linear
    weights/biases ~ U(+-1/sqrt(fan_in)) (torch's default), BN affine/running stats away
    from their trivial values so that every BN term is exercised.  ``logit_gain`` scales
    the last Linear so that integer-prediction tests have decisive logit margins.
    ``edge_layer.weight`` (edge_geometry=True) starts at ZERO without drawing from the stream: a fresh edge-aware model
    computes what the plain model of the same seed computes.  ``page_attention.geometry.weight``
    (page_attention_geometry=True) starts at zero in the same way, and so does every ``geometry.weight`` of the page
    encoder (page_encoder_geometry=True).  The page encoder's LayerNorm weights and biases follow the BatchNorm affine rule
    (away from 1 and 0).
    """
    rs = np.random.RandomState(seed)
    spec = state_dict_spec(**cfg)
    bn_prefixes = {k.rsplit(".", 1)[0] for k, _ in spec if k.endswith("running_mean")}
    sd = OrderedDict()
    for key, shape in spec:
        prefix, leaf = key.rsplit(".", 1)
        is_bn = prefix in bn_prefixes or is_layernorm_key(key)
        if leaf == "num_batches_tracked":
            sd[key] = torch.tensor(0, dtype=torch.long)
            continue
        if prefix.endswith("edge_layer") or key == PAGE_ATTENTION_GEO_KEY or (
                key.startswith("page_encoder.") and key.endswith("geometry.weight")):
            sd[key] = torch.zeros(shape, dtype=torch.float32)
            continue
        if leaf == "running_mean":
            v = 0.1 * rs.standard_normal(shape)
        elif leaf == "running_var":
            v = rs.uniform(0.5, 1.5, shape)
        elif is_bn and leaf == "weight":
            v = rs.uniform(0.5, 1.5, shape)
        elif is_bn and leaf == "bias":
            v = 0.1 * rs.standard_normal(shape)
        elif len(shape) == 4:  # conv
            fan_out = shape[0] * shape[2] * shape[3]
            v = rs.standard_normal(shape) * np.sqrt(2.0 / fan_out)
        elif len(shape) == 2:  # linear weight
            bound = 1.0 / np.sqrt(shape[1])
            v = rs.uniform(-bound, bound, shape)
            if key == "decoder.5.weight":
                v = v * logit_gain
        else:  # Linear bias
            v = rs.uniform(-0.05, 0.05, shape)
            if key == "decoder.5.bias":
                v = v * logit_gain
        sd[key] = torch.from_numpy(np.asarray(v, dtype=np.float32).reshape(shape).copy())
    return sd
