"""numpy restatement of cova_page_joint_decode (include/cova_hip.h) for the tests: straight from the definition -- the
candidate lists, itertools.product over the rank tuples, float64 sums in class order."""
import itertools

import numpy as np

NOT_EVALUATED, UNLABELLED = -2, -1
SCORE_MODES = {"logit": 0, "map": 1}


def scores(logits, score_mode):
    """float32 [n, C]: the score of every box for the classes 1..C; a NaN counts as -inf."""
    logits = np.asarray(logits, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        s = logits[:, 1:] - logits[:, :1] if score_mode else logits[:, 1:].copy()
    s = s.astype(np.float32)
    s[np.isnan(s)] = -np.inf
    return s


def column_order(v):
    """Page-local indices of one column: score descending, ties to the lower index."""
    return sorted(range(len(v)), key=lambda i: (-v[i], i)) if len(v) else []


def total(vals):
    """float64 sum of float32 scores in the order given; a NaN total counts as -inf."""
    t = float(vals[0])                      # a Python float is an IEEE double, a float32 converts exactly
    for v in vals[1:]:
        t = t + float(v)
    return -np.inf if t != t else t


def gap_of(best, other):
    """best total minus the runner-up's: 0 on a tie (two -inf or two +inf totals included)."""
    return 0.0 if best == other else float(np.float64(best) - np.float64(other))


def decode_page(logits, score_mode=1):
    """One page, logits [n, NC] -> (choice int list [C], gap float, best total or None)."""
    logits = np.asarray(logits, dtype=np.float32)
    n, C = logits.shape[0], logits.shape[1] - 1
    if n == 0:
        return [-1] * C, np.inf, None
    s = scores(logits, score_mode)
    m = min(n, C + 1)
    cand = [column_order(s[:, k].tolist())[:m] for k in range(C)]
    if n < C:
        return [cand[k][0] for k in range(C)], np.inf, None
    best, best_t, others = None, None, []
    for ranks in itertools.product(range(m), repeat=C):            # lexicographic: the first of equal totals wins
        boxes = [cand[k][r] for k, r in enumerate(ranks)]
        if len(set(boxes)) != C:
            continue
        t = total([s[b, k] for k, b in enumerate(boxes)])
        if best is None:
            best, best_t = boxes, t
        elif t > best_t:
            others.append(best_t)
            best, best_t = boxes, t
        else:
            others.append(t)
    return best, (gap_of(best_t, max(others)) if others else np.inf), best_t


def column_page(logits, score_mode=1):
    """The column decision of one page: the first of every column's order (-1 on an empty page)."""
    logits = np.asarray(logits, dtype=np.float32)
    s = scores(logits, score_mode)
    return [column_order(s[:, k].tolist())[0] if logits.shape[0] else -1 for k in range(logits.shape[1] - 1)]


def joint_decode(logits, labels, page_start, n_classes, score_mode=1, page_ids=None, P=None):
    """The kernel's three tables for one batch -> (choice int32 [P, C], hit int32 [P, C] or None, gap float64 [P]), with
    the caller's pre-fill (-2, -2, -1.0) in the rows the batch does not write."""
    logits = np.asarray(logits, dtype=np.float32).reshape(-1, n_classes)
    B, C = len(page_start) - 1, n_classes - 1
    ids = np.arange(B) if page_ids is None else np.asarray(page_ids)
    P = B if P is None else int(P)
    choice = np.full((P, C), NOT_EVALUATED, dtype=np.int32)
    hit = None if labels is None else np.full((P, C), NOT_EVALUATED, dtype=np.int32)
    gap = np.full(P, -1.0, dtype=np.float64)
    for p in range(B):
        row = int(ids[p])
        if row < 0 or row >= P:
            continue
        lo = max(int(page_start[p]), 0)
        hi = max(int(page_start[p + 1]), lo)
        ch, g, _ = decode_page(logits[lo:hi], score_mode)
        choice[row], gap[row] = ch, g
        if labels is not None:
            lab = np.asarray(labels)[lo:hi].astype(np.int64)
            for k in range(C):
                hit[row, k] = UNLABELLED if not (lab == k + 1).any() else int(lab[ch[k]] == k + 1)
    return choice, hit, gap
