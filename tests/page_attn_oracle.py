"""CPU restatement of the page self-attention (include/cova_hip.h: cova_page_attn_fwd / cova_page_attn_bwd), in torch with
autograd, written per page and per head:

    [Q | K | V] = h qkv.weight^T,  head a owns the columns a*dh .. a*dh + dh of each third, dh = E / Hh
    for a row i of page p (rows page_start[p] .. page_start[p + 1]):
      s_ij = (Q_i . K_j) / sqrt(dh) over ALL rows j of the page,  A_ij = softmax_j s_ij,  O_i = sum_j A_ij V_j
      lse_i = log sum_j exp(s_ij)

It runs in the dtype of its inputs (float64 for the kernel tests).  The backward is autograd's.  Nothing here shares code
with the kernels."""
import math

import torch
import torch.nn.functional as F

from oracle import cova_oracle as O

KEY = "page_attention.qkv.weight"


def attend(qkv, page_start, heads):
    """qkv [N, 3E], page_start (B + 1 offsets), heads -> (O [N, E], A: {(page, head): [n, n]}, lse [N, heads]).
    Rows outside every page are zero."""
    N, E = qkv.shape[0], qkv.shape[1] // 3
    dh = E // heads
    ps = [int(v) for v in page_start]
    out_rows, lse_rows, A = [qkv[:ps[0], :E] * 0], [qkv[:ps[0], :heads] * 0], {}
    for p in range(len(ps) - 1):
        lo, hi = ps[p], ps[p + 1]
        if hi <= lo:
            continue
        o_heads, l_heads = [], []
        for a in range(heads):
            q = qkv[lo:hi, a * dh:(a + 1) * dh]
            k = qkv[lo:hi, E + a * dh:E + (a + 1) * dh]
            v = qkv[lo:hi, 2 * E + a * dh:2 * E + (a + 1) * dh]
            s = (q @ k.t()) / math.sqrt(dh)
            att = torch.softmax(s, dim=1)
            A[(p, a)] = att
            o_heads.append(att @ v)
            l_heads.append(torch.logsumexp(s, dim=1, keepdim=True))
        out_rows.append(torch.cat(o_heads, dim=1))
        lse_rows.append(torch.cat(l_heads, dim=1))
    out_rows.append(qkv[ps[-1]:, :E] * 0)
    lse_rows.append(qkv[ps[-1]:, :heads] * 0)
    return torch.cat(out_rows, dim=0), A, torch.cat(lse_rows, dim=0)


def page_attention(h, sd, page_start, heads, return_all=False):
    """The layer on the state_dict entry ``page_attention.qkv.weight`` -> O [N, E] (or (O, A, lse, qkv))."""
    qkv = F.linear(h, sd[KEY])
    out, A, lse = attend(qkv, page_start, heads)
    return (out, A, lse, qkv) if return_all else out


def patched_gat_stack(page_start, heads):
    """A replacement for oracle.cova_oracle.gat_stack (monkeypatch) that appends the attention columns to the context, so
    that O.forward / O.loss_and_grads state the whole model with ``page_attention_dim``: [own | GAT context | O].  The
    decoder reads its widths from the state dict.  A state dict without attention heads of the GAT (a ``use_context=False``
    model, stated to O.forward with ``use_context=True`` so that this function is reached at all) gets [own | O].
    Not for stacking: without heads in the state dict the hook this one replaced is never called, so the columns of another
    page layer hooked beneath it would be dropped without a word; several page layers at once are stated by
    tests/combined_oracle.py."""
    plain = O.gat_stack

    def fn(h_i, context_indices, sd, alpha=0.2, routing=None):
        if O.gat_prefixes(sd):
            ctx, attn = plain(h_i, context_indices, sd, alpha, routing=routing)
        else:
            ctx, attn = h_i[:, :0], h_i[:, :0].detach()
        return torch.cat((ctx, page_attention(h_i, sd, page_start, heads)), dim=1), attn
    return fn
