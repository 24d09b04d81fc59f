"""numpy float64 statement of the per-page ranking loss (cova_page_rank_loss_fwd / _bwd, include/cova_hip.h): a list is
(page p, class c >= 1) over the page's candidate rows (label in [0, NC), not the ignore label) with v_n = logits[n, c]; its
targets are the rows labelled c; a list with a target is scored, L_pc = lse_candidates(v) - lse_targets(v), and
dL_pc/dv_n = softmax_cand(v)_n - [n is a target] softmax_tgt(v)_n.  R = sum w_c L_pc ("sum") or that over sum w_c ("mean", 0
over a zero denominator); the step's term is weight * R."""
import numpy as np

from mining_oracle import page_bounds


def _lse(v):
    m = v.max()
    return m + np.log(np.exp(v - m).sum())


def candidates(labels, nc, ignore=None):
    """bool [N]: rows that may take part in a list of their page"""
    lab = np.asarray(labels).astype(np.int64)
    ok = (lab >= 0) & (lab < nc)
    if ignore is not None:
        ok &= lab != int(ignore)
    return ok


def rank_loss(logits, labels, page_start, class_weight=None, ignore=None, weight=1.0, reduction="sum", grad_scale=1.0):
    """-> dict(lists float64 [B, NC-1, 4] = lse of the candidates, lse of the targets, candidate count, target count (the
    table of the entry point); L float64 [B, NC-1] (0 where unscored); scored bool [B, NC-1]; cand bool [N]; target bool
    [N, NC]; acc float64 [3] = sum w_c L, sum w_c, scored lists; R; loss = weight * R; dlogits float64 [N, NC] =
    grad_scale * d loss / d logits)."""
    v = np.asarray(logits).astype(np.float64)
    lab = np.asarray(labels).astype(np.int64)
    n, nc = v.shape
    w = np.ones(nc) if class_weight is None else np.asarray(class_weight).astype(np.float64)
    bounds = page_bounds(page_start, n)
    cand = candidates(lab, nc, ignore)
    lists = np.zeros((len(bounds), nc - 1, 4))
    L = np.zeros((len(bounds), nc - 1))
    target = np.zeros((n, nc), dtype=bool)
    unit = np.zeros((n, nc))                      # d L_pc / d v, before any weight
    for p, (s, e) in enumerate(bounds):
        rows = s + np.nonzero(cand[s:e])[0]
        for c in range(1, nc):
            tgt = rows[lab[rows] == c]
            lists[p, c - 1, 2:] = (len(rows), len(tgt))
            if len(tgt) == 0:
                continue
            target[tgt, c] = True
            lse_a, lse_t = _lse(v[rows, c]), _lse(v[tgt, c])
            lists[p, c - 1, :2] = (lse_a, lse_t)
            L[p, c - 1] = lse_a - lse_t
            unit[rows, c] = np.exp(v[rows, c] - lse_a)
            unit[tgt, c] -= np.exp(v[tgt, c] - lse_t)
    scored = lists[:, :, 3] > 0
    wl = np.broadcast_to(w[1:], scored.shape)
    acc = np.array([(wl * L)[scored].sum(), wl[scored].sum(), float(scored.sum())])
    if reduction == "mean":
        s = 1.0 / acc[1] if acc[1] > 0 else 0.0
    else:
        assert reduction == "sum", reduction
        s = 1.0
    R = acc[0] * s
    return dict(lists=lists, L=L, scored=scored, cand=cand, target=target, acc=acc, R=R, loss=float(weight) * R,
                dlogits=float(grad_scale) * float(weight) * s * unit * w[None, :])
