"""numpy restatement of cova_eval_page_ranks (include/cova_hip.h) for the tests: straight from the definition."""
import numpy as np


def page_ranks(logits, labels, page_start, n_classes):
    """-> (rank, top1) int32 [B, NC-1] for the pages of one batch, rows in batch order."""
    logits, labels = np.asarray(logits, dtype=np.float32), np.asarray(labels).astype(np.int64)
    B = len(page_start) - 1
    rank = np.full((B, n_classes - 1), -1, dtype=np.int32)
    top1 = np.full((B, n_classes - 1), -1, dtype=np.int32)
    for p in range(B):
        lo, hi = int(page_start[p]), int(page_start[p + 1])
        idx = np.arange(hi - lo)
        for c in range(1, n_classes):
            v = logits[lo:hi, c]
            if hi > lo:
                top1[p, c - 1] = int(np.argmax(v))                      # the first of equal maxima
            where = np.nonzero(labels[lo:hi] == c)[0]
            if where.size:
                t = int(where[0])
                rank[p, c - 1] = int(((v > v[t]) | ((v == v[t]) & (idx < t))).sum())
    return rank, top1


def split_tables(logits, labels, counts, n_classes):
    """The tables of a whole split whose pages lie back to back."""
    start = np.concatenate([[0], np.cumsum(counts)])
    return page_ranks(logits, labels, start, n_classes)


def margins(logits, labels, page_start, n_classes):
    """float64 [B, NC-1]: distance of the labelled box's score to the nearest other score of its column within the page
    (inf when there is no labelled box or no other box): how far a rank is from changing."""
    logits, labels = np.asarray(logits, dtype=np.float64), np.asarray(labels).astype(np.int64)
    B = len(page_start) - 1
    out = np.full((B, n_classes - 1), np.inf)
    for p in range(B):
        lo, hi = int(page_start[p]), int(page_start[p + 1])
        for c in range(1, n_classes):
            where = np.nonzero(labels[lo:hi] == c)[0]
            if where.size and hi - lo > 1:
                v = logits[lo:hi, c]
                out[p, c - 1] = np.abs(np.delete(v, where[0]) - v[where[0]]).min()
    return out
