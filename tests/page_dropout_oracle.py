"""CPU restatement of the dropout of the page layers (include/cova_hip.h: cova_page_attn_fwd_drop /
cova_page_attn_bwd_drop and their _geo_ forms, cova_gelu_fwd_drop / cova_gelu_bwd_drop, cova_dropout_add_fwd /
cova_dropout_regen_bwd; engine.page_dropout_seed).

    inv = float32(1) / (float32(1) - float32(p)),  a slot is kept when hash_uniform(seed, idx) >= float32(p)
    attention   idx = ((i * Hh + a) << 32) | j   for query batch row i, head a, key batch row j
                A = softmax(s) unchanged, lse undropped;  O_i = sum_j D_ij * inv * A_ij V_j
    rows        idx = r * C + c   of an [R, C] operand
    block       x += drop1(out(Attn_drop(qkv(LN1(x)))));  x += drop2(ffn2(drop_h(GELU(ffn1(LN2(x))))))
                sites 0 attention probabilities, 1 drop1, 2 the FFN hidden activations, 3 drop2
    stream      1 << 63 | (layer + 1) << 56 | (site + 1) << 48 | base;  the stand-alone page attention is layer 8, site 0

The hash is attn_dropout_oracle's numpy uint64 arithmetic, the stream rule plain Python integers, the layers float64 torch
with the masks as INPUTS and autograd's backward.  The attention probabilities, LayerNorm and GELU are page_attn_oracle's,
page_attn_geo_oracle's and page_encoder_oracle's.  No code shared with the kernels or with engine.py."""
import numpy as np
import torch
import torch.nn.functional as F

import page_attn_geo_oracle as PG
import page_attn_oracle as PA
import page_encoder_oracle as PE
from attn_dropout_oracle import hash_mix64, hash_uniform, inv_keep      # noqa: F401  (hash_mix64: re-exported)

MASK48 = (1 << 48) - 1
MAX_LAYERS = 8                         # the stand-alone page attention's ``layer``
SITES = 4
ATTN_KEY = PA.KEY


def page_dropout_seed(base, layer, site):
    assert 0 <= base <= MASK48 and 0 <= layer <= MAX_LAYERS and 0 <= site < SITES
    return (1 << 63) | ((layer + 1) << 56) | ((site + 1) << 48) | base


def attn_index(i, a, j, heads):
    """mask index of (query batch row i, head a, key batch row j): integer arrays broadcast -> uint64"""
    i, j = np.asarray(i, dtype=np.uint64), np.asarray(j, dtype=np.uint64)
    return ((i * np.uint64(heads) + np.uint64(a)) << np.uint64(32)) | j


def attn_keeps(p, seed, page_start, heads):
    """{(page, head): bool [n, n]} for every page with rows: the keep-mask of its scores"""
    ps = [int(v) for v in page_start]
    keeps = {}
    for pg in range(len(ps) - 1):
        lo, hi = ps[pg], ps[pg + 1]
        if hi > lo:
            rows = np.arange(lo, hi, dtype=np.uint64)
            for a in range(heads):
                keeps[(pg, a)] = hash_uniform(seed, attn_index(rows[:, None], a, rows[None, :], heads)) >= np.float32(p)
    return keeps


def all_keep_attn(page_start, heads):
    ps = [int(v) for v in page_start]
    return {(pg, a): np.ones((ps[pg + 1] - ps[pg],) * 2, dtype=bool)
            for pg in range(len(ps) - 1) if ps[pg + 1] > ps[pg] for a in range(heads)}


def row_keep(p, seed, R, C):
    """bool [R, C]: element (r, c) is kept when the uniform of r * C + c is >= p, compared in float32"""
    return (hash_uniform(seed, np.arange(R * C, dtype=np.uint64)) >= np.float32(p)).reshape(R, C)


def _scale(keep, p, like):
    return torch.as_tensor(np.asarray(keep), dtype=like.dtype) * inv_keep(p)


def attend(qkv, page_start, heads, keeps, p, geo_w=None, phi=None):
    """The attention with dropped probabilities -> (O [N, E], lse [N, heads] undropped).  ``keeps`` from attn_keeps (None:
    no dropout); ``geo_w`` / ``phi``: the geometry bias (page_attn_geo_oracle)."""
    if geo_w is None:
        out, A, lse = PA.attend(qkv, page_start, heads)
    else:
        out, A, lse = PG.attend(qkv, page_start, heads, geo_w, phi)
    if keeps is None:
        return out, lse
    E = qkv.shape[1] // 3
    dh = E // heads
    ps = [int(v) for v in page_start]
    rows = [qkv[:ps[0], :E] * 0]
    for pg in range(len(ps) - 1):
        lo, hi = ps[pg], ps[pg + 1]
        if hi > lo:
            rows.append(torch.cat([(A[(pg, a)] * _scale(keeps[(pg, a)], p, qkv))
                                   @ qkv[lo:hi, 2 * E + a * dh:2 * E + (a + 1) * dh] for a in range(heads)], dim=1))
    rows.append(qkv[ps[-1]:, :E] * 0)
    return torch.cat(rows, dim=0), lse


def page_attention(h, sd, page_start, heads, keeps, p, phi=None):
    """The stand-alone layer on ``page_attention.*`` of ``sd`` -> (O, lse, qkv)"""
    qkv = F.linear(h, sd[ATTN_KEY])
    out, lse = attend(qkv, page_start, heads, keeps, p, sd.get(PG.GEO_KEY), phi)
    return out, lse, qkv


def block(x, sd, prefix, page_start, heads, masks, p, page_phi=None):
    """One pre-LN block with its four sites.  ``masks`` = (attention keeps, drop1 [N, P], hidden [N, M], drop2 [N, P]),
    or None: no dropout."""
    if masks is None:
        return PE.block(x, sd, prefix, page_start, heads, page_phi)
    ka, k1, kh, k2 = masks
    a = PE.layer_norm(x, sd[prefix + "norm1.weight"], sd[prefix + "norm1.bias"])
    qkv = a @ sd[prefix + "qkv.weight"].t()
    O = attend(qkv, page_start, heads, ka, p, sd.get(prefix + "geometry.weight"), page_phi)[0]
    # drop(y W^T + b) written as (y W^T) * s + b * s, added in page_encoder_oracle.block's order: with all-keep masks at
    # p = 0 (s = 1) the sums are that block's, bit for bit
    s1, sh, s2 = _scale(k1, p, x), _scale(kh, p, x), _scale(k2, p, x)
    x = x + (O @ sd[prefix + "out.weight"].t()) * s1 + sd[prefix + "out.bias"] * s1
    m = PE.layer_norm(x, sd[prefix + "norm2.weight"], sd[prefix + "norm2.bias"])
    f = PE.gelu(m @ sd[prefix + "ffn1.weight"].t() + sd[prefix + "ffn1.bias"]) * sh
    return x + (f @ sd[prefix + "ffn2.weight"].t()) * s2 + sd[prefix + "ffn2.bias"] * s2


def encoder_masks(p, base, page_start, heads, N, P, Ms):
    """Per layer the four masks of the restated stream rule; ``Ms`` the layers' feed-forward widths."""
    return [(attn_keeps(p, page_dropout_seed(base, l, 0), page_start, heads),
             row_keep(p, page_dropout_seed(base, l, 1), N, P),
             row_keep(p, page_dropout_seed(base, l, 2), N, M),
             row_keep(p, page_dropout_seed(base, l, 3), N, P)) for l, M in enumerate(Ms)]


def all_keep_masks(page_start, heads, N, P, Ms):
    return [(all_keep_attn(page_start, heads), np.ones((N, P), bool), np.ones((N, M), bool), np.ones((N, P), bool))
            for M in Ms]


def ffn_widths(sd):
    return [sd[PE.layer_prefix(l) + "ffn1.weight"].shape[0] for l in range(PE.n_layers(sd))]


def page_encoder(h, sd, page_start, heads, masks, p, page_phi=None):
    """The encoder on ``page_encoder.*`` of ``sd`` with per-layer ``masks`` (None: page_encoder_oracle's) -> [N, P]"""
    if masks is None:
        return PE.page_encoder(h, sd, page_start, heads, page_phi)
    x = h @ sd[PE.INPUT_KEY].t()
    for l in range(PE.n_layers(sd)):
        x = block(x, sd, PE.layer_prefix(l), page_start, heads, masks[l], p, page_phi)
    return PE.layer_norm(x, sd[PE.PREFIX + "norm.weight"], sd[PE.PREFIX + "norm.bias"])


def patched(page_start, bboxes, page_size, base, heads=1, p_attn=0.0, encoder_heads=1, p_enc=0.0, keeps=None,
            attention_dropout=0.0):
    """combined_oracle.patched (GAT heads with their keep masks ``keeps`` at ``attention_dropout``, page readout) with the
    page attention's and the page encoder's columns stated HERE, with the masks of the step whose base is ``base`` under
    the restated stream rule -> (gat, gat_stack), the replacements for oracle.cova_oracle.gat and
    oracle.cova_oracle.gat_stack.  Columns: [D | G | E | P], each part present when its weights are in the state dict."""
    import combined_oracle as CO
    gat, inner = CO.patched(page_start, bboxes, page_size, heads, keeps, attention_dropout)
    ps = [int(v) for v in page_start]
    phi = {}

    def page_phi():
        if "phi" not in phi:
            phi["phi"] = PG.page_features(bboxes.detach().numpy(), ps, page_size[1], page_size[0])
        return phi["phi"]

    def gat_stack(h_i, context_indices, sd, alpha=0.2, routing=None):
        rest = {k: v for k, v in sd.items() if not k.startswith(("page_attention.", PE.PREFIX))}
        cols, attn0 = inner(h_i, context_indices, rest, alpha, routing)
        N = h_i.shape[0]
        if ATTN_KEY in sd:
            ka = attn_keeps(p_attn, page_dropout_seed(base, MAX_LAYERS, 0), ps, heads) if p_attn > 0 else None
            out = page_attention(h_i, sd, ps, heads, ka, p_attn, page_phi() if PG.GEO_KEY in sd else None)[0]
            cols = torch.cat((cols, out), dim=1)
        if PE.INPUT_KEY in sd:
            geo = PE.layer_prefix(0) + "geometry.weight" in sd
            masks = (encoder_masks(p_enc, base, ps, encoder_heads, N, sd[PE.INPUT_KEY].shape[0], ffn_widths(sd))
                     if p_enc > 0 else None)
            cols = torch.cat((cols, page_encoder(h_i, sd, ps, encoder_heads, masks, p_enc, page_phi() if geo else None)),
                             dim=1)
        return cols, attn0
    return gat, gat_stack
