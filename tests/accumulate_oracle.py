"""numpy statement of cova_grad_accumulate and of HotPathTrainer's accumulation cycle (include/cova_hip.h, "gradient
accumulation"), written from the formulas and independent of trainer.py."""
import numpy as np

OPEN, ADD, CLOSE, ADD_CLOSE = range(4)
MODES = {OPEN: "open", ADD: "add", CLOSE: "close", ADD_CLOSE: "add-close"}


def accumulate(mode, acc, g, rows, scale=1.0, clip=None):
    """One launch -> (acc, g) as new float32 arrays.  Per element of the rows {lo, hi, ...} that lies inside ``clip``
    (flat [lo, hi), None: everything), every operation one float32 operation:
        open       acc = g                 (acc is not read)
        add        acc = acc + g
        close      g   = acc * s
        add-close  g   = (acc + g) * s     s = float32(scale)
    A row outside 0 <= lo <= hi <= n is skipped as the kernel skips it; elements outside rows or clip keep their bits."""
    acc = np.ascontiguousarray(acc, dtype=np.float32)
    g = np.ascontiguousarray(g, dtype=np.float32)
    n, s = g.shape[0], np.float32(scale)
    c0, c1 = (0, n) if clip is None else (max(int(clip[0]), 0), min(int(clip[1]), n))
    acc_out, g_out = acc.copy(), g.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for row in rows:
            lo, hi = int(row[0]), int(row[1])
            if not 0 <= lo <= hi <= n:
                continue
            a, b = max(lo, c0), min(hi, c1)
            if a >= b:
                continue
            if mode == OPEN:
                acc_out[a:b] = g[a:b]
            elif mode == ADD:
                acc_out[a:b] = (acc[a:b] + g[a:b]).astype(np.float32)
            elif mode == CLOSE:
                g_out[a:b] = (acc[a:b] * s).astype(np.float32)
            elif mode == ADD_CLOSE:
                t = (acc[a:b] + g[a:b]).astype(np.float32)
                g_out[a:b] = (t * s).astype(np.float32)
            else:
                raise ValueError(mode)
    return acc_out, g_out


def accumulated_gradient(grads, rows, scale):
    """The gradient bucket after a cycle over the micro-batch gradients ``grads`` (in order) that ends with the last
    micro-step's add-close -> float32 array; elements outside the rows are those of the last gradient."""
    acc = np.full_like(np.asarray(grads[0], dtype=np.float32), np.nan)       # never read before it is opened
    for i, g in enumerate(grads[:-1]):
        acc, _ = accumulate(OPEN if i == 0 else ADD, acc, g, rows)
    if len(grads) == 1:                                                      # (no cycle: the gradient as it is)
        return np.ascontiguousarray(grads[0], dtype=np.float32).copy()
    return accumulate(ADD_CLOSE, acc, grads[-1], rows, scale)[1]


def flushed_gradient(grads, rows, scale):
    """The gradient bucket after flush() over the pending ``grads``: open, adds, then a close -> float32 array."""
    acc = np.full_like(np.asarray(grads[0], dtype=np.float32), np.nan)
    for i, g in enumerate(grads):
        acc, _ = accumulate(OPEN if i == 0 else ADD, acc, g, rows)
    return accumulate(CLOSE, acc, grads[-1], rows, scale)[1]


def scale_of(loss_reduction, m):
    """The closing scale of an update made from ``m`` micro-batches, in double."""
    if loss_reduction == "sum":
        return 1.0
    assert loss_reduction == "mean"
    return 1.0 / m


def schedule(n, batches_per_epoch, n_epochs=1, loss_reduction="mean", update_count=0):
    """What an epoch loop (train_step per batch, flush at the end of every epoch) issues with accumulate_steps ``n``:
    one entry per event, (event, launch, scale, accumulated after it, update_count after it).  ``event`` is "step" or
    "flush"; ``launch`` is None (n == 1: no accumulate launch; or a flush with nothing pending), "open", "add",
    "add-close" or "close"; ``scale`` is None unless the launch closes."""
    out, pending = [], 0
    for _ in range(n_epochs):
        for _ in range(batches_per_epoch):
            if n == 1:
                update_count += 1
                out.append(("step", None, None, 0, update_count))
                continue
            pending += 1
            if pending < n:
                out.append(("step", "open" if pending == 1 else "add", None, pending, update_count))
            else:
                update_count += 1
                out.append(("step", "add-close", scale_of(loss_reduction, pending), 0, update_count))
                pending = 0
        if n > 1:
            if pending:
                update_count += 1
                out.append(("flush", "close", scale_of(loss_reduction, pending), 0, update_count))
                pending = 0
            else:
                out.append(("flush", None, None, 0, update_count))
    return out
