"""CPU restatement (numpy) of the sampled input pipeline: the key formula of cova_sample_boxes (include/cova_hip.h), the
selection rule of WebDataset.__getitem__ (datasets.py:101-110) expressed over keys, and the collation of the kept boxes
(datasets.py:112-128,159-178).  Pinned against tests/golden/collate_sampled.npz, the reference's own output."""
import numpy as np

_GOLDEN, _M1, _M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def mix(s, x):
    """z ^ (z >> 31) of z = s + golden * (x + 1) after the two multiply-xorshift rounds, modulo 2^64 (arrays or scalars)."""
    with np.errstate(over="ignore"):
        s, x = np.asarray(s, dtype=np.uint64), np.asarray(x, dtype=np.uint64)
        z = s + _GOLDEN * (x + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def stream_seed(seed, epoch):
    return mix(mix(np.uint64(0), np.uint64(seed)), np.uint64(epoch))


def hash_keys(seed, epoch, page_id, n):
    """int64 [n]: key of every box of dataset page ``page_id`` in epoch ``epoch`` of the run seeded ``seed``."""
    return (mix(mix(stream_seed(seed, epoch), np.uint64(page_id)), np.arange(n, dtype=np.uint64)) >> np.uint64(1)).astype(np.int64)


def keys_from_permutation(perm):
    """Keys under which ``select`` keeps what ``perm[:m]`` keeps: key[perm[j]] = j."""
    perm = np.asarray(perm, dtype=np.int64)
    keys = np.empty_like(perm)
    keys[perm] = np.arange(perm.shape[0], dtype=np.int64)
    return keys


def select(rows, m, keys):
    """Ascending indices of the kept boxes of one page: rank among (key, index) below m, or a non-zero label."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 5)
    n = rows.shape[0]
    order = np.lexsort((np.arange(n), np.asarray(keys, dtype=np.int64)))       # primary key, ties to the lower index
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    return np.nonzero((rank < m) | (rows[:, 4] != 0))[0]


def collate(u8_pages, rows_per_page, context_size, sampling_fraction, keys_per_page=None, seed=0, epoch=0, page_ids=None,
            additional_feats=None):
    """-> dict of numpy arrays: images, bboxes, labels, context_indices, additional_feats, page_start, kept (the kept
    page-local indices per page).  ``additional_feats``: list of [n,A] per page, or None."""
    cs = int(context_size)
    images = np.ascontiguousarray(np.transpose(np.asarray(u8_pages), (0, 3, 1, 2))).astype(np.float32) / np.float32(255)
    boxes, labels, ctxs, addl, kept, starts = [], [], [], [], [], [0]
    for p, rows in enumerate(rows_per_page):
        rows = np.asarray(rows, dtype=np.float32).reshape(-1, 5)
        n = rows.shape[0]
        if keys_per_page is not None:
            keys = keys_per_page[p]
        else:
            keys = hash_keys(seed, epoch, p if page_ids is None else int(page_ids[p]), n)
        idx = select(rows, int(sampling_fraction * n), keys)
        kept.append(idx)
        r = rows[idx]
        k = r.shape[0]
        labels.append(r[:, 4].astype(np.int64))
        b = np.empty((k, 5), dtype=np.float32)
        b[:, 0] = p
        b[:, 1:3] = r[:, 0:2]
        b[:, 3:5] = r[:, 0:2] + r[:, 2:4]                       # float32 adds
        boxes.append(b)
        ctx = np.full((k, 2 * cs), -1, dtype=np.int64)
        for i in range(k):
            c = list(range(max(0, i - cs), i)) + list(range(i + 1, min(k, i + cs + 1)))
            ctx[i, :len(c)] = np.asarray(c, dtype=np.int64) + starts[-1]
        ctxs.append(ctx)
        if additional_feats is not None:
            addl.append(np.asarray(additional_feats[p], dtype=np.float32)[idx])        # [n,A] per page
        starts.append(starts[-1] + k)
    n_out = starts[-1]
    return dict(images=images, bboxes=np.concatenate(boxes, 0), labels=np.concatenate(labels, 0),
                context_indices=np.concatenate(ctxs, 0) if cs else np.zeros((0, 0), np.int64),
                additional_feats=np.concatenate(addl, 0) if additional_feats is not None else np.zeros((n_out, 0), np.float32),
                page_start=np.asarray(starts, dtype=np.int64), kept=kept)
