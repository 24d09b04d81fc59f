"""CPU restatement of the page readout (include/cova_hip.h: cova_page_readout_fwd / cova_page_readout_bwd), in torch with
autograd.

    P = h W^T,  u_i = a . P_i + b,  e_i = u_i > 0 ? u_i : alpha * u_i      (u == +-0: the alpha branch)
    per page p (rows page_start[p] .. page_start[p + 1]):  beta = softmax(e),  r_p = sum_i beta_i P_i
    every row of the page receives r_p

It runs in the dtype of its inputs (float64 for the kernel tests).  ``gate`` [N] forces the branch of every LeakyReLU (the
device's own decisions, for gradients that are comparable to round-off).  The backward is autograd's; closed_form_bwd
restates the hand-derived one.  Nothing here shares code with the kernels."""
import torch
import torch.nn.functional as F

from oracle import cova_oracle as O

PREFIX = "page_readout."


def pool(P, att_w, att_b, page_start, alpha=0.2, gate=None):
    """P [N, G], att_w [1, G] (or [G]), att_b [1], page_start (a list or tensor of B + 1 offsets), gate bool [N] or None
    -> (rows [N, G], beta [N], r [B, G], u [N]).  Rows outside every page, and the r row of an empty page, are zero."""
    N, G = P.shape
    ps = [int(v) for v in page_start]
    u = F.linear(P, att_w.reshape(1, G), att_b.reshape(1)).squeeze(1)
    pos = (u > 0) if gate is None else gate.to(torch.bool).reshape(N)
    e = torch.where(pos, u, alpha * u)
    rows, betas, rs = [P[:ps[0]] * 0], [e[:ps[0]] * 0], []
    for p in range(len(ps) - 1):
        lo, hi = ps[p], ps[p + 1]
        if hi <= lo:
            rs.append(torch.zeros((G,), dtype=P.dtype))
            continue
        b = torch.softmax(e[lo:hi], dim=0)
        r = (b.unsqueeze(1) * P[lo:hi]).sum(0)
        betas.append(b)
        rs.append(r)
        rows.append(r.unsqueeze(0).expand(hi - lo, G))
    rows.append(P[ps[-1]:] * 0)
    betas.append(e[ps[-1]:] * 0)
    r_all = torch.stack(rs) if rs else torch.zeros((0, G), dtype=P.dtype)
    return torch.cat(rows, dim=0), torch.cat(betas, dim=0), r_all, u


def readout(h, sd, page_start, alpha=0.2, gate=None, prefix=PREFIX, return_all=False):
    """The readout on the state_dict entries under ``prefix`` -> rows [N, G] (or (rows, beta, r, u, P))."""
    P = F.linear(h, sd[prefix + "W.weight"])
    rows, beta, r, u = pool(P, sd[prefix + "attention_layer.weight"], sd[prefix + "attention_layer.bias"], page_start,
                            alpha, gate)
    return (rows, beta, r, u, P) if return_all else rows


def closed_form_bwd(g, P, att_w, att_b, page_start, alpha=0.2, gate=None):
    """The hand-derived backward of pool(): g = dL/drows [N, G] -> (dP [N, G], d_att_w [G], d_att_b [1])."""
    N, G = P.shape
    ps = [int(v) for v in page_start]
    a = att_w.reshape(G)
    _, beta, r, u = pool(P, att_w, att_b, ps, alpha, gate)
    pos = (u > 0) if gate is None else gate.to(torch.bool).reshape(N)
    dP, du = torch.zeros_like(P), torch.zeros_like(u)
    for p in range(len(ps) - 1):
        lo, hi = ps[p], ps[p + 1]
        if hi <= lo:
            continue
        gr = g[lo:hi].sum(0)
        dbeta = P[lo:hi] @ gr
        de = beta[lo:hi] * (dbeta - gr @ r[p])
        du[lo:hi] = de * torch.where(pos[lo:hi], torch.ones_like(de), alpha * torch.ones_like(de))
        dP[lo:hi] = beta[lo:hi].unsqueeze(1) * gr.unsqueeze(0) + du[lo:hi].unsqueeze(1) * a.unsqueeze(0)
    return dP, du @ P, du.sum().reshape(1)


def patched_gat_stack(page_start):
    """A replacement for oracle.cova_oracle.gat_stack (monkeypatch) that appends the readout columns to the context, so
    that O.forward / O.loss_and_grads state the whole model with ``page_context_dim``: [own | GAT context | r_page].  The
    decoder reads its widths from the state dict.  ``routing["gate_page_readout.leaky"]`` [N] forces the readout's gates.
    A state dict without attention heads (a ``use_context=False`` model, stated to O.forward with ``use_context=True`` so
    that this function is reached at all) gets the readout columns alone: [own | r_page].
    Not for stacking: without heads in the state dict the hook this one replaced is never called, so the columns of another
    page layer hooked beneath it would be dropped without a word; several page layers at once are stated by
    tests/combined_oracle.py."""
    plain = O.gat_stack

    def fn(h_i, context_indices, sd, alpha=0.2, routing=None):
        if O.gat_prefixes(sd):
            ctx, attn = plain(h_i, context_indices, sd, alpha, routing=routing)
        else:
            ctx, attn = h_i[:, :0], h_i[:, :0].detach()
        gate = routing.get("gate_" + PREFIX + "leaky") if routing else None
        return torch.cat((ctx, readout(h_i, sd, page_start, alpha, gate)), dim=1), attn
    return fn
