"""numpy statement of cova_optim_step's AdamW and SGD updates (include/cova_hip.h, "optimizer options"), one float32
operation per operation of the formulas, written from them and independent of trainer.py.  The hyper-parameters are
converted as the entry point converts them: the bias corrections, 1 - lr * wd and 1 - dampening in double, then to float32."""
import math

import numpy as np

F = np.float32


def fmaf(a, b, c):
    """float32 arrays -> a * b + c rounded once.  The product of two float32 is exact in double; the double sum s is off
    the exact value by e (TwoSum), and float32(s) is the exact value's rounding unless s lies exactly half way between two
    float32 while e is not zero: then e decides."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)
    r = s.astype(F)
    d = s - r.astype(np.float64)                             # exact: what the rounding to float32 dropped
    other = np.nextafter(r, np.where(d > 0, F(np.inf), F(-np.inf)).astype(F))
    tie = (d != 0) & (np.abs(d) == np.abs(other.astype(np.float64) - s))
    return np.where(tie & (e != 0), np.where((e > 0) == (other > r), other, r), r).astype(F)


def adamw(p, g, m, v, step, lr, weight_decay, betas, eps):
    """One AdamW step on float32 arrays -> (p, m, v): torch.optim.AdamW's p.mul_(1 - lr * wd), the moments, and
    p += -(lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps)) with the last product and sum fused."""
    lr_, b1, b2, eps_ = F(lr), F(betas[0]), F(betas[1]), F(eps)
    bc1, bc2_sqrt = F(1.0 - betas[0] ** step), F(math.sqrt(1.0 - betas[1] ** step))
    p = p * F(1.0 - lr * weight_decay)
    m = b1 * m + (F(1) - b1) * g
    v = b2 * v + (F(1) - b2) * g * g
    denom = np.sqrt(v) / bc2_sqrt + eps_
    return fmaf(np.full_like(p, -(lr_ / bc1)), m / denom, p), m, v


def sgd(p, g, buf, has_buf, lr, weight_decay, momentum, dampening, nesterov):
    """One torch.optim.SGD step with momentum on float32 arrays -> (p, buf); ``has_buf`` False: the group's first step
    (buf = g)."""
    lr_, wd, mom, damp1 = F(lr), F(weight_decay), F(momentum), F(1.0 - dampening)
    if wd != 0:
        g = g + wd * p
    if mom != 0:
        buf = mom * buf + damp1 * g if has_buf else g
        g = g + mom * buf if nesterov else buf
    return p - lr_ * g, buf
