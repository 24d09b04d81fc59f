"""numpy statement of cova_weight_average and of HotPathTrainer's averaging schedule (include/cova_hip.h, "weight
averaging"), written from the formulas and independent of trainer.py."""
import numpy as np


def average_update(avg, p, rows, one_minus_decay):
    """avg[i] + w * (p[i] - avg[i]) over the table rows {lo, hi, ...}, every operation one float32 operation -> a new
    float32 array.  A row outside 0 <= lo <= hi <= n is skipped as the kernel skips it; elements outside the rows keep
    their bits."""
    avg = np.ascontiguousarray(avg, dtype=np.float32)
    p = np.ascontiguousarray(p, dtype=np.float32)
    out, n, w = avg.copy(), avg.shape[0], np.float32(one_minus_decay)
    for row in rows:
        lo, hi = int(row[0]), int(row[1])
        if not 0 <= lo <= hi <= n:
            continue
        d = (p[lo:hi] - avg[lo:hi]).astype(np.float32)
        t = (w * d).astype(np.float32)
        out[lo:hi] = (avg[lo:hi] + t).astype(np.float32)
    return out


def one_minus_decay(kind, decay, warmup, n_averaged):
    """The weight of the sample that joins an average of ``n_averaged`` samples, in double."""
    if kind == "swa":                                  # running mean: mean_{n+1} = mean_n + (x - mean_n) / (n + 1)
        return 1.0 / (n_averaged + 1.0)
    assert kind == "ema"
    d = float(decay)
    if warmup is not None:
        d = min(d, (1.0 + n_averaged) / (float(warmup) + n_averaged))
    return 1.0 - d


def schedule(kind, decay, warmup, start, every, n_steps):
    """Per optimizer step 1..n_steps what happens at its end: None (nothing), "copy" (the average becomes the
    parameters) or the one_minus_decay of the update; with start == 0 the copy happened at construction.
    -> (actions, n_averaged after the last step)."""
    n, actions = (1 if start == 0 else 0), []
    for s in range(1, n_steps + 1):
        if s < start or (s - start) % every:
            actions.append(None)
        elif s == start:
            actions.append("copy")
            n = 1
        else:
            actions.append(one_minus_decay(kind, decay, warmup, n))
            n += 1
    return actions, n
