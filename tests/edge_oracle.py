"""CPU restatement of the edge-geometry extension (include/cova_hip.h: cova_edge_geometry, cova_gat_fwd_edge).

``edge_features``: numpy float32 arrays throughout, one numpy operation per rounding (numpy never fuses a multiply with an
add), parenthesised exactly as the header states the eight features.  ``gat``: oracle.cova_oracle.gat's operation order with
the edge term added to the pre-activation before the LeakyReLU; it runs in whatever dtype its inputs have (float64 for the
kernel tests)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import cova_oracle as O

_0, _1, _2, _64 = np.float32(0), np.float32(1), np.float32(2), np.float32(64)


def edge_features(bboxes, ctx, img_w, img_h):
    """float32 [N, K, 8].  bboxes [N,5] = page,x1,y1,x2,y2; ctx int64 [N,K] batch-global ids; a pad (j < 0) or an id >= N
    gives eight zeros."""
    bb = np.ascontiguousarray(bboxes, dtype=np.float32)
    ctx = np.asarray(ctx, dtype=np.int64)
    N, K = ctx.shape
    W, H = np.float32(img_w), np.float32(img_h)
    ok = (ctx >= 0) & (ctx < N)
    j = np.where(ok, ctx, 0)
    i = np.broadcast_to(np.arange(N, dtype=np.int64)[:, None], (N, K))
    if N == 0:
        return np.zeros((0, K, 8), np.float32)
    x1i, y1i, x2i, y2i = (bb[i, c] for c in (1, 2, 3, 4))
    x1j, y1j, x2j, y2j = (bb[j, c] for c in (1, 2, 3, 4))
    with np.errstate(all="ignore"):
        wi, hi, wj, hj = x2i - x1i, y2i - y1i, x2j - x1j, y2j - y1j
        f0 = ((x1j + x2j) - (x1i + x2i)) / (_2 * W)
        f1 = ((y1j + y2j) - (y1i + y2i)) / (_2 * H)
        f2 = (wj - wi) / ((wj + wi) + _1)
        f3 = (hj - hi) / ((hj + hi) + _1)
        f4 = np.maximum(_0, np.maximum(x1i, x1j) - np.minimum(x2i, x2j)) / W
        f5 = np.maximum(_0, np.maximum(y1i, y1j) - np.minimum(y2i, y2j)) / H
        iw = np.maximum(_0, np.minimum(x2i, x2j) - np.maximum(x1i, x1j))
        ih = np.maximum(_0, np.minimum(y2i, y2j) - np.maximum(y1i, y1j))
        inter = iw * ih
        uni = ((wi * hi) + (wj * hj)) - inter
        f6 = np.where(uni > _0, inter / np.where(uni > _0, uni, _1), _0)
        f7 = np.clip(j - i, -64, 64).astype(np.float32) / _64
    phi = np.stack([f0, f1, f2, f3, f4, f5, f6, f7], axis=2)
    assert phi.dtype == np.float32
    phi[~ok] = 0
    return phi


def gat(h_i, context_indices, sd, phi, alpha=0.2, return_attn_wts=False, prefix="gat.", routing=None):
    """oracle.cova_oracle.gat with ``+ edge_layer(phi)`` on the pre-activation; ``phi`` [N,K,8] tensor of h_i's dtype."""
    N, K = context_indices.shape
    W_i, W_j = sd[prefix + "W_i.weight"], sd[prefix + "W_j.weight"]
    D = W_i.shape[0]
    h_pad = torch.cat((h_i, torch.zeros((1, h_i.shape[1]), dtype=h_i.dtype)), dim=0)
    h_j = h_pad[context_indices.view(-1)].view(N, K, h_i.shape[1])
    Wh_i = F.linear(h_i, W_i)
    Wh_i_rep = Wh_i.repeat_interleave(K, dim=0).view(N, K, D)
    Wh_j = F.linear(h_j, W_j)
    e = F.linear(torch.cat((Wh_i_rep, Wh_j), dim=2), sd[prefix + "attention_layer.weight"],
                 sd[prefix + "attention_layer.bias"]).squeeze(2)
    e = e + F.linear(phi, sd[prefix + "edge_layer.weight"]).squeeze(2)
    e = O._leaky(e, alpha, routing, "gate_" + prefix + "leaky")
    e = torch.where(context_indices >= 0, e, -9e15 * torch.ones_like(e))
    attn = torch.softmax(e, dim=1)
    h_prime = (attn.unsqueeze(-1) * Wh_j).sum(1)
    if return_attn_wts:
        return h_prime, attn
    return h_prime


def patched_gat(bboxes, page_size):
    """A replacement for oracle.cova_oracle.gat (monkeypatch) that scores with the edge term of this batch: heads whose
    state_dict has an ``edge_layer.weight`` take it, the others run the plain oracle."""
    plain = O.gat
    cache = {}

    def fn(h_i, context_indices, sd, alpha=0.2, return_attn_wts=False, prefix="gat.", routing=None):
        if prefix + "edge_layer.weight" not in sd:
            return plain(h_i, context_indices, sd, alpha, return_attn_wts, prefix, routing)
        if "phi" not in cache:
            cache["phi"] = torch.from_numpy(edge_features(bboxes.detach().numpy(), context_indices.numpy(),
                                                          page_size[1], page_size[0]))
        return gat(h_i, context_indices, sd, cache["phi"].to(h_i.dtype), alpha, return_attn_wts, prefix, routing)
    return fn
