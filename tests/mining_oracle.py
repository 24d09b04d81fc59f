"""numpy statement of cova_hard_negative_select's contract (include/cova_hip.h): per page the positives and the
k = max(min_keep, floor(ratio * positives)) background rows with the highest score s = lse - l[0] keep their labels, the other
background rows get the drop label.  Scores in float64 from the f32 logits; the order is a stable sort on (-key, index) of
integer keys (NaN above +inf, s <= 0 lowest), the quota is float64 arithmetic."""
import math

import numpy as np

NAN_KEY32 = 0x7FC00000
NAN_KEY64 = 0x7FF8000000000000


def scores64(logits):
    """-> (s, lse) in float64 from the given (f32) logits: m + log(sum exp(l - m)) - l[0]"""
    l = np.asarray(logits).astype(np.float64)
    with np.errstate(all="ignore"):
        m = l.max(axis=1)
        lse = m + np.log(np.exp(l - m[:, None]).sum(axis=1))
        return lse - l[:, 0], lse


def keys(scores):
    """integer keys of a score array, as int64 that compare like the kernel's: f32 scores give the kernel's uint32 keys
    (0x7FC00000 for NaN, the bits of s for s > 0, else 0), f64 scores the same construction on 64-bit patterns"""
    s = np.ascontiguousarray(scores)
    if s.dtype == np.float32:
        bits, nan_key = s.view(np.uint32).astype(np.int64), NAN_KEY32
    else:
        assert s.dtype == np.float64
        bits, nan_key = s.view(np.uint64).astype(np.int64), NAN_KEY64          # positive doubles fit int64
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(s), nan_key, np.where(s > 0, bits, 0)).astype(np.int64)


def quota(ratio, min_keep, n_pos, n_bg):
    q = max(float(min_keep), float(math.floor(float(ratio) * float(n_pos))))
    return n_bg if q >= n_bg else int(q)


def page_bounds(page_start, n):
    ps = [int(v) for v in np.asarray(page_start).tolist()]
    out = []
    for p in range(len(ps) - 1):
        s = min(max(ps[p], 0), n)
        out.append((s, min(max(ps[p + 1], s), n)))
    return out


def ranks(key, bg_idx):
    """rank of each background row among the page's background rows: stable sort on (-key, index)"""
    order = np.argsort(-key[bg_idx], kind="stable")
    r = np.empty(len(bg_idx), dtype=np.int64)
    r[order] = np.arange(len(bg_idx))
    return r


def _select(scores, labels, page_start, nc, ratio, min_keep, drop_label):
    labels = np.asarray(labels).astype(np.int64)
    key = keys(scores)
    out = labels.copy()
    bounds = page_bounds(page_start, labels.shape[0])
    counts = np.zeros((len(bounds), 3), dtype=np.int32)
    gaps, edge = np.full(len(bounds), np.inf), np.zeros(len(bounds))
    for p, (s, e) in enumerate(bounds):
        lab = labels[s:e]
        bg = s + np.nonzero(lab == 0)[0]
        n_pos = int(((lab >= 1) & (lab < nc)).sum())
        k = quota(ratio, min_keep, n_pos, len(bg))
        counts[p] = (n_pos, len(bg), k)
        r = ranks(key, bg)
        out[bg[r >= k]] = drop_label
        if 0 < k < len(bg):
            by_rank = np.asarray(scores, dtype=np.float64)[bg[np.argsort(r)]]
            gaps[p], edge[p] = abs(by_rank[k - 1] - by_rank[k]), abs(by_rank[k - 1])
    return out, counts, gaps, edge


def select_from_scores(scores_f32, labels, page_start, nc, ratio, min_keep, drop_label):
    """the selection that the contract prescribes for the given f32 scores -> (labels_out int64 [N], counts int32 [B, 3])"""
    s = np.ascontiguousarray(scores_f32)
    assert s.dtype == np.float32
    return _select(s, labels, page_start, nc, ratio, min_keep, drop_label)[:2]


def select(logits, labels, page_start, ratio, min_keep, drop_label):
    """the selection from float64 scores -> (labels_out, counts, gap [B], edge [B]): gap is the float64 distance between
    the k-th and the (k+1)-th hardest background score of the page (inf where the quota cuts nothing: k = 0 or
    k = n_bg), edge the |score| of the k-th"""
    s, _ = scores64(logits)
    return _select(s, labels, page_start, np.asarray(logits).shape[1], ratio, min_keep, drop_label)
