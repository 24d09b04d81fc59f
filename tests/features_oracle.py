"""numpy restatement of cova_feat_rows_gather and of the row ids a DeviceDataset batch carries (tests only)."""
import numpy as np


def gather_rows(table, row_ids, out, C=None):
    """-> a copy of ``out`` [M, ld] (M >= N) with out[g, :C] = table[row_ids[g], :C], zeros for an id outside [0, R);
    columns >= C and rows >= N keep what they held."""
    table, ids = np.asarray(table), np.asarray(row_ids, dtype=np.int64)
    C = table.shape[1] if C is None else C
    res = np.array(out, copy=True)
    ok = (ids >= 0) & (ids < table.shape[0])
    block = np.zeros((ids.shape[0], C), dtype=table.dtype)
    block[ok] = table[ids[ok], :C]
    res[:ids.shape[0], :C] = block
    return res


def kept_row_ids(starts, page_ids, kept_local):
    """Table row ids of a batch: ``kept_local[i]`` = ascending page-local indices of the kept boxes of page
    ``page_ids[i]``; ``starts`` = the dataset's row offsets."""
    parts = [int(starts[p]) + np.asarray(k, dtype=np.int64) for p, k in zip(page_ids, kept_local)]
    return np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
