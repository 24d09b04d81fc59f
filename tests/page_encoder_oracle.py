"""CPU restatement of the page encoder (engine.page_encoder_fwd), in torch with autograd:

    x = h input.weight^T
    per layer l (keys under page_encoder.layers.<l>.):
        a = LN(x; norm1);  qkv = a qkv.weight^T;  O = page attention of qkv (with geometry.weight: the biased scores)
        x = x + O out.weight^T + out.bias
        m = LN(x; norm2);  f = GELU(m ffn1.weight^T + ffn1.bias);  x = x + f ffn2.weight^T + ffn2.bias
    out = LN(x; page_encoder.norm)

LN is the biased-variance LayerNorm with eps = 1e-5, GELU the exact (erf) form.  The attention itself is imported from
page_attn_oracle / page_attn_geo_oracle.  It runs in the dtype of its inputs (float64 for the kernel tests); the backward is
autograd's.  Nothing here shares code with the kernels.  ``patched(...)`` is a hook in the manner of combined_oracle.patched:
it imports combined_oracle, does not edit it, and appends the encoder's columns behind [D | G | E]."""
import math

import torch

import combined_oracle as CO
import page_attn_geo_oracle as PG
import page_attn_oracle as PA

PREFIX = "page_encoder."
INPUT_KEY = PREFIX + "input.weight"
EPS = 1e-5


def layer_prefix(l):
    return "%slayers.%d." % (PREFIX, l)


def n_layers(sd):
    l = 0
    while layer_prefix(l) + "qkv.weight" in sd:
        l += 1
    return l


def layer_norm(x, weight, bias, eps=EPS, return_stats=False):
    """(x - mean) * rstd * weight + bias over the last dimension, rstd = 1 / sqrt(biased variance + eps)."""
    mean = x.mean(dim=-1, keepdim=True)
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(dim=-1, keepdim=True) + eps)
    out = d * rstd * weight + bias
    return (out, mean.squeeze(-1), rstd.squeeze(-1)) if return_stats else out


def gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def gelu_grad(z):
    """d gelu / dz, the closed form cova_gelu_bwd states."""
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def block(x, sd, prefix, page_start, heads, page_phi=None):
    """One pre-LN block on the stream x [N, P] -> the new stream."""
    a = layer_norm(x, sd[prefix + "norm1.weight"], sd[prefix + "norm1.bias"])
    qkv = a @ sd[prefix + "qkv.weight"].t()
    if prefix + "geometry.weight" in sd:
        O = PG.attend(qkv, page_start, heads, sd[prefix + "geometry.weight"], page_phi)[0]
    else:
        O = PA.attend(qkv, page_start, heads)[0]
    x = x + O @ sd[prefix + "out.weight"].t() + sd[prefix + "out.bias"]
    m = layer_norm(x, sd[prefix + "norm2.weight"], sd[prefix + "norm2.bias"])
    f = gelu(m @ sd[prefix + "ffn1.weight"].t() + sd[prefix + "ffn1.bias"])
    return x + f @ sd[prefix + "ffn2.weight"].t() + sd[prefix + "ffn2.bias"]


def page_encoder(h, sd, page_start, heads, page_phi=None):
    """The layer on the ``page_encoder.*`` entries of ``sd`` (its depth is read off the keys) -> [N, P]."""
    x = h @ sd[INPUT_KEY].t()
    for l in range(n_layers(sd)):
        x = block(x, sd, layer_prefix(l), page_start, heads, page_phi)
    return layer_norm(x, sd[PREFIX + "norm.weight"], sd[PREFIX + "norm.bias"])


def patched(page_start=None, bboxes=None, page_size=None, heads=1, keeps=None, attention_dropout=0.0, encoder_heads=1,
            tap=None):
    """combined_oracle.patched with the encoder's columns appended behind [D | G | E] when the state dict holds
    ``page_encoder.input.weight`` -> (gat, gat_stack), the replacements for oracle.cova_oracle.gat and
    oracle.cova_oracle.gat_stack.  ``heads`` are the page attention's, ``encoder_heads`` the encoder's."""
    gat, inner = CO.patched(page_start, bboxes, page_size, heads, keeps, attention_dropout, tap)
    ps = None if page_start is None else [int(v) for v in page_start]
    phi = {}

    def page_phi():
        if "phi" not in phi:
            phi["phi"] = PG.page_features(bboxes.detach().numpy(), ps, page_size[1], page_size[0])
        return phi["phi"]

    def gat_stack(h_i, context_indices, sd, alpha=0.2, routing=None):
        cols, attn0 = inner(h_i, context_indices, sd, alpha, routing)
        if INPUT_KEY in sd:
            geo = layer_prefix(0) + "geometry.weight" in sd
            cols = torch.cat((cols, page_encoder(h_i, sd, ps, encoder_heads, page_phi() if geo else None)), dim=1)
        return cols, attn0
    return gat, gat_stack
