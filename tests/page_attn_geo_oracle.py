"""CPU restatement of the page self-attention with the box-geometry bias (include/cova_hip.h: cova_page_attn_fwd_geo /
cova_page_attn_bwd_geo): page_attn_oracle.attend with the bias added to every score,

    s_ij = (Q_i . K_j) / sqrt(dh) + w[a] . phi_ij,   phi_ij = edge_features(box of the QUERY i, box of the KEY j, dj = j - i)

``phi`` comes from edge_oracle.edge_features (numpy float32, the device's bits) on the page's dense table ``ctx[i] = all
rows of the page``; it is cast to the dtype of the inputs, everything else runs in that dtype (float64 for the kernel
tests) under autograd.  Nothing here shares code with the kernels."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cova_oracle as O
import edge_oracle as EO

KEY = "page_attention.qkv.weight"
GEO_KEY = "page_attention.geometry.weight"


def page_features(bboxes, page_start, img_w, img_h):
    """{page: float32 [n, n, 8]} for every page with rows: phi[i, j] = the features of (query i, key j)."""
    bb = np.ascontiguousarray(np.asarray(bboxes, dtype=np.float32))
    ps = [int(v) for v in page_start]
    phi = {}
    for p in range(len(ps) - 1):
        lo, hi = ps[p], ps[p + 1]
        if hi > lo:
            n = hi - lo
            ctx = np.broadcast_to(np.arange(n, dtype=np.int64)[None, :], (n, n))
            phi[p] = EO.edge_features(bb[lo:hi], ctx, img_w, img_h)
    return phi


def swapped(phi):
    """The features with the roles exchanged: phi'[i, j] = phi[j, i] (what a kernel that calls edge_features(key, query)
    would read)."""
    return {p: np.ascontiguousarray(f.transpose(1, 0, 2)) for p, f in phi.items()}


def attend(qkv, page_start, heads, geo_w, phi, return_scores=False):
    """qkv [N, 3E], page_start (B + 1 offsets), heads, geo_w [heads, 8], phi from page_features
    -> (O [N, E], A: {(page, head): [n, n]}, lse [N, heads]) (and the biased scores {(page, head): [n, n]}).
    Rows outside every page are zero."""
    N, E = qkv.shape[0], qkv.shape[1] // 3
    dh = E // heads
    ps = [int(v) for v in page_start]
    out_rows, lse_rows, A, S = [qkv[:ps[0], :E] * 0], [qkv[:ps[0], :heads] * 0], {}, {}
    for p in range(len(ps) - 1):
        lo, hi = ps[p], ps[p + 1]
        if hi <= lo:
            continue
        f = torch.from_numpy(phi[p]).to(qkv.dtype)
        o_heads, l_heads = [], []
        for a in range(heads):
            q = qkv[lo:hi, a * dh:(a + 1) * dh]
            k = qkv[lo:hi, E + a * dh:E + (a + 1) * dh]
            v = qkv[lo:hi, 2 * E + a * dh:2 * E + (a + 1) * dh]
            s = (q @ k.t()) / math.sqrt(dh) + f @ geo_w[a]
            att = torch.softmax(s, dim=1)
            A[(p, a)], S[(p, a)] = att, s
            o_heads.append(att @ v)
            l_heads.append(torch.logsumexp(s, dim=1, keepdim=True))
        out_rows.append(torch.cat(o_heads, dim=1))
        lse_rows.append(torch.cat(l_heads, dim=1))
    out_rows.append(qkv[ps[-1]:, :E] * 0)
    lse_rows.append(qkv[ps[-1]:, :heads] * 0)
    res = (torch.cat(out_rows, dim=0), A, torch.cat(lse_rows, dim=0))
    return res + (S,) if return_scores else res


def page_attention(h, sd, page_start, heads, phi, return_all=False):
    """The layer on the state_dict entries ``page_attention.qkv.weight`` and ``page_attention.geometry.weight``
    -> O [N, E] (or (O, A, lse, qkv))."""
    qkv = F.linear(h, sd[KEY])
    out, A, lse = attend(qkv, page_start, heads, sd[GEO_KEY], phi)
    return (out, A, lse, qkv) if return_all else out


def patched_gat_stack(page_start, heads, bboxes, page_size):
    """page_attn_oracle.patched_gat_stack with the geometry bias of this batch: [own | GAT context | O].  ``page_size`` =
    (height, width).
    Not for stacking: without heads in the state dict the hook this one replaced is never called, so the columns of another
    page layer hooked beneath it would be dropped without a word; several page layers at once are stated by
    tests/combined_oracle.py."""
    plain = O.gat_stack
    phi = page_features(bboxes.detach().numpy(), page_start, page_size[1], page_size[0])

    def fn(h_i, context_indices, sd, alpha=0.2, routing=None):
        if O.gat_prefixes(sd):
            ctx, attn = plain(h_i, context_indices, sd, alpha, routing=routing)
        else:
            ctx, attn = h_i[:, :0], h_i[:, :0].detach()
        return torch.cat((ctx, page_attention(h_i, sd, page_start, heads, phi)), dim=1), attn
    return fn


PAGE_W, PAGE_H = 96, 64                    # the tests' page: not square, so an exchange of W and H shows


def planted_boxes(sizes, seed):
    """float32 [N, 5] = page, x1, y1, x2, y2 on a PAGE_W x PAGE_H page.  Random boxes of 2..40 pixels a side (many pairs
    overlap); in every page of two or more rows the second box is the first again (identical boxes), of three or more
    the third has no area (the ``uni == 0`` branch, on the diagonal), of five or more the fourth and fifth sit in opposite
    corners (far apart)."""
    rs = np.random.RandomState(seed)
    rows = []
    for p, n in enumerate(sizes):
        wh = rs.uniform(2, 40, (n, 2))
        xy = rs.uniform(0, 1, (n, 2)) * (np.asarray([PAGE_W, PAGE_H]) - wh)
        b = np.concatenate([np.full((n, 1), float(p)), xy, xy + wh], axis=1)
        if n >= 2:
            b[1] = b[0]
        if n >= 3:
            b[2, 3:] = b[2, 1:3]
        if n >= 5:
            b[3, 1:] = [0, 0, 3, 2]
            b[4, 1:] = [PAGE_W - 4, PAGE_H - 3, PAGE_W, PAGE_H]
        rows.append(b)
    return np.concatenate(rows, axis=0).astype(np.float32) if rows else np.zeros((0, 5), np.float32)
