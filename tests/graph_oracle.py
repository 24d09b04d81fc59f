"""CPU restatement (numpy) of cova_context_knn (include/cova_hip.h): the DOM-order window of datasets.py:117-128 followed by
the k nearest other boxes of the page, ordered by (gap2, ctr2, j).  float32 arrays throughout, one numpy operation per
rounding (numpy never fuses a multiply with an add), explicit parentheses, np.lexsort for the order."""
import numpy as np

_ZERO = np.float32(0)


def pair_keys(boxes, i):
    """(gap2, ctr2) float32 [n] of box ``i`` against every box of ``boxes`` [n,4] = x1,y1,x2,y2."""
    b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4)
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    with np.errstate(all="ignore"):
        dx = np.maximum(_ZERO, np.maximum(x1[i], x1) - np.minimum(x2[i], x2))
        dy = np.maximum(_ZERO, np.maximum(y1[i], y1) - np.minimum(y2[i], y2))
        gap2 = (dx * dx) + (dy * dy)
        sx, sy = x1 + x2, y1 + y2
        ex, ey = sx[i] - sx, sy[i] - sy
        ctr2 = (ex * ex) + (ey * ey)
    assert gap2.dtype == np.float32 and ctr2.dtype == np.float32
    return gap2, ctr2


def packed_keys(gap2, ctr2):
    """uint64 (bits(gap2) << 32) | bits(ctr2): what the kernel compares.  Orders as (gap2, ctr2) for non-negative floats."""
    g = np.ascontiguousarray(gap2, dtype=np.float32).view(np.uint32).astype(np.uint64)
    c = np.ascontiguousarray(ctr2, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (g << np.uint64(32)) | c


def candidates(n, i, context_size):
    """Ascending page-local indices that may be spatial neighbours of box i: not i, not a member of its window."""
    j = np.arange(n, dtype=np.int64)
    return j[np.abs(j - i) > context_size]


def spatial_neighbours(boxes, i, context_size, k):
    """The first ``k`` candidates of box i in (gap2, ctr2, j) order (fewer when the page runs out)."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    cand = candidates(b.shape[0], i, context_size)
    if k <= 0 or cand.size == 0:
        return cand[:0]
    gap2, ctr2 = pair_keys(b, i)
    g = gap2[cand]
    if cand.size > k:               # the k first all have gap2 <= the k-th smallest gap2: sort those alone (ties included)
        keep = g <= np.partition(g, k - 1)[k - 1]
        cand, g = cand[keep], g[keep]
    order = np.lexsort((cand, ctr2[cand], g))
    return cand[order][:k]


def window(n, i, context_size):
    return list(range(max(0, i - context_size), i)) + list(range(i + 1, min(n, i + context_size + 1)))


def page_graph(boxes, context_size, k):
    """int64 [n, 2*context_size + k] page-local table of one page (boxes [n,4] = x1,y1,x2,y2), -1 pads."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    n, cs = b.shape[0], int(context_size)
    out = np.full((n, 2 * cs + k), -1, dtype=np.int64)
    for i in range(n):
        w = window(n, i, cs)
        out[i, :len(w)] = w
        s = spatial_neighbours(b, i, cs, k)
        out[i, 2 * cs:2 * cs + s.shape[0]] = s
    return out


def batch_graph(bboxes, page_start, context_size, k):
    """int64 [N, 2*context_size + k] batch-global table.  bboxes [N,5] = page,x1,y1,x2,y2 (or [N,4]); page_start [B+1]."""
    bb = np.asarray(bboxes, dtype=np.float32)
    bb = bb[:, -4:]
    ps = [int(v) for v in np.asarray(page_start).reshape(-1)]
    parts = []
    for lo, hi in zip(ps[:-1], ps[1:]):
        t = page_graph(bb[lo:hi], context_size, k)
        t[t >= 0] += lo
        parts.append(t)
    if not parts:
        return np.zeros((0, 2 * int(context_size) + k), np.int64)
    return np.concatenate(parts, 0)


def tie_grid():
    """[131,4] boxes: a 13x10 grid of 30x20 boxes at pitch 40x30 (integer coordinates: heavy ties in both keys) and one box
    covering the whole grid (zero gap to everything)."""
    cells = [[40.0 * c, 30.0 * r, 40.0 * c + 30.0, 30.0 * r + 20.0] for r in range(10) for c in range(13)]
    cells.append([0.0, 0.0, 40.0 * 12 + 30.0, 30.0 * 9 + 20.0])
    return np.asarray(cells, dtype=np.float32)
