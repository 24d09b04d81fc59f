"""The inputs of the joint-decoding kernel tests (numpy only): tests/test_joint_decode_gpu.py runs them through
cova_page_joint_decode, tests/test_joint_decode_cpu.py checks that they exercise what they are meant to."""
import functools

import numpy as np

import decode_oracle as DO

INF, NAN = np.inf, np.nan


def objectness_page(rs, n, nc, labelled=None):
    """Unit-variance logits whose class columns share a per-box "objectness" term of twice that spread: the strongest box
    tends to lead every column, which is where the joint and the column decision part.  Labels: one box of each class
    (of the first ``labelled`` classes), as far as the page has boxes."""
    logits = rs.standard_normal((n, nc)).astype(np.float32)
    logits[:, 1:] += (2.0 * rs.standard_normal((n, 1))).astype(np.float32)
    labels = np.zeros(n, dtype=np.int64)
    k = min(n, nc - 1 if labelled is None else labelled)
    labels[rs.permutation(n)[:k]] = np.arange(1, k + 1)
    return logits, labels


def batch_of(pages, nc):
    """[(logits [n, nc], labels [n])] -> dict(logits, labels, page_start, nc, sizes)."""
    sizes = [p[0].shape[0] for p in pages]
    return dict(logits=np.concatenate([p[0].reshape(-1, nc) for p in pages]).astype(np.float32),
                labels=np.concatenate([p[1] for p in pages]).astype(np.int64),
                page_start=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), nc=nc, sizes=sizes)


def random_batch(nc, sizes, seed, unlabelled_page=None):
    rs = np.random.RandomState(seed)
    pages = [objectness_page(rs, n, nc) for n in sizes]
    if unlabelled_page is not None:                    # a page that lacks its last class: the hit table's -1
        lab = pages[unlabelled_page][1]
        lab[lab == nc - 1] = 0
    return batch_of(pages, nc)


SIZES_NC4 = [0, 1, 2, 3, 4, 5, 63, 64, 65, 90, 300]
SIZES_NC2 = [0, 1, 2, 65]
SIZES_NC7 = [0, 5, 6, 7, 8, 130]


def special_pages():
    """name -> (logits [n, 4], labels [n]): the pages the definition treats one by one."""
    rs = np.random.RandomState(11)
    out = {}
    out["empty"] = (np.zeros((0, 4), np.float32), np.zeros(0, np.int64))
    out["fewer_boxes_than_classes"] = objectness_page(rs, 2, 4)
    out["one_box"] = objectness_page(rs, 1, 4)
    out["as_many_boxes_as_classes"] = objectness_page(rs, 3, 4)
    out["all_scores_equal"] = (np.full((10, 4), 0.5, np.float32), np.array([0, 0, 3, 0, 1, 0, 0, 2, 0, 0]))
    lg, lab = objectness_page(rs, 8, 4)
    lg[5, 1:] = [9.0, 8.0, 7.0]                        # box 5 leads every column
    out["one_box_leads_every_column"] = (lg, lab)
    lg, lab = objectness_page(rs, 9, 4)
    lg[:, 2] = NAN                                     # a column that is all NaN
    lg[0, 1], lg[3, 1], lg[4, 3], lg[7, 3] = -INF, NAN, -INF, NAN
    out["minus_inf_and_nan"] = (lg, lab)
    lg, lab = objectness_page(rs, 6, 4)
    lg[:, 0] = 0.0
    lg[:, 1], lg[:, 3] = INF, -INF                     # every total is +inf + x + -inf: NaN, so -inf, and every gap 0
    out["plus_inf_against_minus_inf"] = (lg, lab)
    lg, lab = objectness_page(rs, 5, 4)
    lg[:, 0] = 0.0
    lg[2, 1], lg[1, 2] = INF, -INF                     # some totals +inf, some -inf, some NaN
    out["mixed_infinities"] = (lg, lab)
    lg, lab = objectness_page(rs, 12, 4)
    out["quantised_ties"] = ((np.round(lg * 2) / 2).astype(np.float32), lab)
    return out


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """name -> dict(batch..., score_mode): every kernel-against-oracle case of the GPU test."""
    cases = {}
    for mode in (0, 1):
        cases["nc4_mode%d" % mode] = dict(random_batch(4, SIZES_NC4, 5, unlabelled_page=7), score_mode=mode)
        cases["special_mode%d" % mode] = dict(batch_of(list(special_pages().values()), 4), score_mode=mode)
    cases["nc2"] = dict(random_batch(2, SIZES_NC2, 6), score_mode=1)
    cases["nc7"] = dict(random_batch(7, SIZES_NC7, 7, unlabelled_page=4), score_mode=1)
    cases["nc4_2500"] = dict(random_batch(4, [2500], 8), score_mode=0)
    return cases


@functools.lru_cache(maxsize=None)
def oracle_tables(name):
    """(choice, hit, gap) of a case under the numpy oracle, computed once for all tests of a session."""
    c = gpu_cases()[name]
    return DO.joint_decode(c["logits"], c["labels"], c["page_start"], c["nc"], c["score_mode"])


def pages_of(case):
    """[(logits, labels)] of a case, page by page."""
    ps = case["page_start"]
    return [(case["logits"][ps[p]:ps[p + 1]], case["labels"][ps[p]:ps[p + 1]]) for p in range(len(ps) - 1)]
