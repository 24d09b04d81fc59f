"""CPU restatement of the attention dropout of the GAT head (include/cova_hip.h: cova_gat_fwd_drop / cova_gat_bwd_drop /
cova_gat2_fwd_drop / cova_gat2_bwd_drop).

    keep[e]   = hash_uniform(seed, e) >= float32(p)            e = i*K + k, the counter hash of csrc/common.h in uint64
    alphad    = keep ? attn * inv : 0                           inv = float32(1) / (float32(1) - float32(p))
    h'[i]     = sum_k alphad[i,k] * Wh_j[ctx[i,k]]              attn = the softmax of either scoring mode, undropped

The hash is numpy uint64 arithmetic (wrapping), the seed derivation plain Python integers, the layer float64 torch with the
mask as an INPUT and autograd's backward: no code shared with the kernels or with engine.py."""
import numpy as np
import torch
import torch.nn.functional as F

import gatv2_oracle as G2

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
M1, M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
MASK48 = (1 << 48) - 1


def hash_mix64(seed, idx):
    """splitmix64 finaliser over seed + golden * (idx + 1), modulo 2**64; ``idx`` an integer array -> uint64 array"""
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) + GOLDEN * (np.asarray(idx).astype(np.uint64) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
        return z ^ (z >> np.uint64(31))


def hash_uniform(seed, idx):
    """the top 24 bits as a float32 in [0, 1) (exact: 24 bits fit the significand, the scale is a power of two)"""
    return (hash_mix64(seed, idx) >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def keep_mask(p, seed, N, K):
    """bool [N, K]: slot (i, k) is kept when the uniform of element i*K + k is >= p, compared in float32"""
    return (hash_uniform(seed, np.arange(N * K, dtype=np.uint64)) >= np.float32(p)).reshape(N, K)


def inv_keep(p):
    """the kernels' scale: one float32 division"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def dropout_base(seed, call):
    """first stream of forward number ``call`` (1, 2, ...): the decoder's Dropouts draw from base and base + 1"""
    return (int(seed) * 0x9E3779B1 + 2 * int(call)) & MASK48


def attention_dropout_seed(base, layer, head):
    """stream of head (layer, head): the step's base below bit 48, head + 1 in bits 48..55, layer + 1 in bits 56..62"""
    assert 0 <= base <= MASK48 and 0 <= layer < 127 and 0 <= head < 255
    return ((layer + 1) << 56) | ((head + 1) << 48) | base


def static_scores(Wh_i, Wh_j_all, ctx, att_w, att_b, alpha=0.2, edge_w=None, phi=None, gate=None):
    """The reference's static score before the mask: LeakyReLU(a_i . Wh_i + a_j . Wh_j + b (+ edge_w . phi)); att_w [1, 2D].
    -> (lrelu(u) [N, K], u [N, K], valid [N, K], gathered Wh_j [N, K, D])"""
    N, K = ctx.shape
    D = Wh_i.shape[1]
    ok = (ctx >= 0) & (ctx < N)
    rows = torch.cat((Wh_j_all, torch.zeros((1, D), dtype=Wh_j_all.dtype)), dim=0)
    Wh_j = rows[torch.where(ok, ctx, torch.full_like(ctx, N)).reshape(-1)].view(N, K, D)
    a = att_w.reshape(-1)
    u = (Wh_i @ a[:D] + att_b.reshape(-1)[0]).unsqueeze(1) + Wh_j @ a[D:]
    if edge_w is not None:
        u = u + F.linear(phi, edge_w.view(1, -1)).squeeze(2)
    pos = (u > 0) if gate is None else gate.to(torch.bool).view(N, K)
    return torch.where(pos, u, alpha * u), u, ok, Wh_j


def attend(mode, Wh_i, Wh_j_all, ctx, att_w, att_b, keep=None, p=0.0, alpha=0.2, edge_w=None, phi=None, gate=None):
    """Either scoring mode ('gat': att_w [1, 2D], gate [N, K]; 'gatv2': att_w [1, D], gate [N, K, D]) with the keep-mask
    ``keep`` (bool [N, K] or None: no dropout) at rate ``p`` -> (h' [N, D], attn [N, K] BEFORE dropout, u or None)."""
    N, K = ctx.shape
    D = Wh_i.shape[1]
    if mode == "gatv2":
        _, attn = G2.attend(Wh_i, Wh_j_all, ctx, att_w, att_b, alpha, edge_w, phi, gate)
        ok = (ctx >= 0) & (ctx < N)
        rows = torch.cat((Wh_j_all, torch.zeros((1, D), dtype=Wh_j_all.dtype)), dim=0)
        Wh_j = rows[torch.where(ok, ctx, torch.full_like(ctx, N)).reshape(-1)].view(N, K, D)
        u = None
    else:
        assert mode == "gat"
        e, u, ok, Wh_j = static_scores(Wh_i, Wh_j_all, ctx, att_w, att_b, alpha, edge_w, phi, gate)
        attn = torch.softmax(torch.where(ok, e, -9e15 * torch.ones_like(e)), dim=1)
    w = attn
    if keep is not None:
        w = attn * torch.as_tensor(np.asarray(keep), dtype=attn.dtype) * inv_keep(p)
    w = torch.where(ok, w, torch.zeros_like(w))                # (an all-pad row has attn 1/K on slots that weigh nothing)
    return (w.unsqueeze(-1) * Wh_j).sum(1), attn, u


def head(mode, h_i, ctx, sd, prefix="gat.", keep=None, p=0.0, phi=None, gate=None, alpha=0.2):
    """A whole head on the state_dict entries under ``prefix`` -> (h', attn before dropout)"""
    Wh_i = F.linear(h_i, sd[prefix + "W_i.weight"])
    Wh_j = F.linear(h_i, sd[prefix + "W_j.weight"])
    hp, attn, _ = attend(mode, Wh_i, Wh_j, ctx, sd[prefix + "attention_layer.weight"], sd[prefix + "attention_layer.bias"],
                         keep, p, alpha, sd.get(prefix + "edge_layer.weight"), phi, gate)
    return hp, attn
