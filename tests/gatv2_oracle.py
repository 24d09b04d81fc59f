"""CPU restatement of the GATv2 scoring mode (include/cova_hip.h: cova_gat2_fwd / cova_gat2_bwd), in torch with autograd.

    z[i,k,d] = Wh_i[i,d] + Wh_j[ctx[i,k],d]          a pad (j < 0) or an id >= N: Wh_j row = 0
    u[i,k]   = b + sum_d a[d] * lrelu(z[i,k,d])      lrelu(z) = z > 0 ? z : alpha * z   (z == +-0: the alpha branch)
             (+ edge_layer(phi[i,k,:]), outside the non-linearity)
    mask (-9e15), softmax over k, h'[i] = sum_k attn[i,k] * Wh_j[ctx[i,k]]

It runs in the dtype of its inputs (float64 for the kernel tests).  ``gate`` [N,K,D] forces the branch of every lrelu (the
device's own decisions, for gradients that are comparable to round-off).  The backward is autograd's: the hand-written
kernels are tested against something that shares no code with them."""
import torch
import torch.nn.functional as F

from oracle import cova_oracle as O
import edge_oracle as EO


def attend(Wh_i, Wh_j_all, ctx, att_w, att_b, alpha=0.2, edge_w=None, phi=None, gate=None):
    """Wh_i, Wh_j_all [N, D] (the two projections of every node), ctx int64 [N, K], att_w [1, D] (or [D]), att_b [1],
    edge_w [1, 8] with phi [N, K, 8] or neither -> (h' [N, D], attn [N, K])."""
    N, K = ctx.shape
    D = Wh_i.shape[1]
    ok = (ctx >= 0) & (ctx < N)
    rows = torch.cat((Wh_j_all, torch.zeros((1, D), dtype=Wh_j_all.dtype)), dim=0)
    Wh_j = rows[torch.where(ok, ctx, torch.full_like(ctx, N)).reshape(-1)].view(N, K, D)
    z = Wh_i.unsqueeze(1) + Wh_j
    pos = (z > 0) if gate is None else gate.to(torch.bool).view(N, K, D)
    lr = torch.where(pos, z, alpha * z)
    u = F.linear(lr, att_w.view(1, D), att_b.view(1)).squeeze(2)
    if edge_w is not None:
        u = u + F.linear(phi, edge_w.view(1, -1)).squeeze(2)
    u = torch.where(ok, u, -9e15 * torch.ones_like(u))
    attn = torch.softmax(u, dim=1)
    return (attn.unsqueeze(-1) * Wh_j).sum(1), attn


def gat_v2(h_i, context_indices, sd, phi=None, alpha=0.2, return_attn_wts=False, prefix="gat.", gate=None):
    """A GATv2 head on the state_dict entries under ``prefix`` (attention_layer.weight [1, D]); ``phi`` when the head has
    an ``edge_layer.weight``."""
    Wh_i = F.linear(h_i, sd[prefix + "W_i.weight"])
    Wh_j = F.linear(h_i, sd[prefix + "W_j.weight"])
    h_prime, attn = attend(Wh_i, Wh_j, context_indices, sd[prefix + "attention_layer.weight"],
                           sd[prefix + "attention_layer.bias"], alpha, sd.get(prefix + "edge_layer.weight"), phi, gate)
    return (h_prime, attn) if return_attn_wts else h_prime


def is_v2(sd, prefix):
    return sd[prefix + "attention_layer.weight"].shape[1] == sd[prefix + "W_i.weight"].shape[0]


def patched_gat(bboxes=None, page_size=None):
    """A replacement for oracle.cova_oracle.gat (monkeypatch): heads whose ``attention_layer.weight`` is [1, D] run gat_v2
    (gates forced from ``routing["gate_" + prefix + "leaky"]`` [N,K,D] when given), the others the static oracle; heads
    with an ``edge_layer.weight`` take the edge features of this batch (``bboxes``, ``page_size`` = (height, width))."""
    plain = O.gat
    cache = {}

    def fn(h_i, context_indices, sd, alpha=0.2, return_attn_wts=False, prefix="gat.", routing=None):
        phi = None
        if prefix + "edge_layer.weight" in sd:
            if "phi" not in cache:
                cache["phi"] = torch.from_numpy(EO.edge_features(bboxes.detach().numpy(), context_indices.numpy(),
                                                                 page_size[1], page_size[0]))
            phi = cache["phi"].to(h_i.dtype)
        if not is_v2(sd, prefix):
            if phi is None:
                return plain(h_i, context_indices, sd, alpha, return_attn_wts, prefix, routing)
            return EO.gat(h_i, context_indices, sd, phi, alpha, return_attn_wts, prefix, routing)
        gate = routing.get("gate_" + prefix + "leaky") if routing else None
        return gat_v2(h_i, context_indices, sd, phi, alpha, return_attn_wts, prefix, gate)
    return fn
