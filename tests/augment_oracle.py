"""CPU restatement (numpy) of the page augmentation (include/cova_hip.h: cova_pages_u8_augment_f32, cova_boxes_translate) and of
the parameter formulas of pipeline.PageAugment.params, written from their contracts without importing the package.

Pixels: float32 arrays throughout, one numpy operation per rounding (numpy never fuses a multiply with an add), explicit
parentheses.  Parameters: Python integers for the 64-bit hash, Python floats (float64) for everything after it."""
import numpy as np

_M64 = (1 << 64) - 1
LUMA = (0.299, 0.587, 0.114)
INT_MAX = 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------ parameters
def mix64(s, x):
    z = (s + 0x9E3779B97F4A7C15 * ((x + 1) & _M64)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def stream_seed(seed, epoch):
    return mix64(mix64(0, int(seed) & _M64), int(epoch) & _M64)


def uniform(seed, epoch, pid, slot):
    aug_stream = mix64(stream_seed(seed, epoch), 1)
    return (mix64(mix64(aug_stream, int(pid)), slot) >> 11) * 2.0 ** -53


def page_params(pid, epoch, seed=0, max_shift=(0, 0), brightness=0.0, contrast=0.0, saturation=0.0, channel_gain=0.0,
                invert_prob=0.0):
    """((dx, dy), 12 float64 values = row-major 3x4) of one page."""
    u = [uniform(seed, epoch, pid, slot) for slot in range(9)]
    # u < 1, so floor(u*(2s+1)) <= 2s unless the float64 product rounds up to 2s+1 (u within 2**-53 of 1): held inside
    dx, dy = (min(int(np.floor(u[a] * (2 * s + 1))), 2 * s) - s for a, s in enumerate(max_shift))
    beta = (2 * u[2] - 1) * brightness
    c = 1 + (2 * u[3] - 1) * contrast
    s = 1 + (2 * u[4] - 1) * saturation
    g = [1 + (2 * u[5 + k] - 1) * channel_gain for k in range(3)]
    sigma = -1.0 if u[8] < invert_prob else 1.0
    m = []
    for k in range(3):
        m += [sigma * c * g[k] * (s * (1.0 if k == l else 0.0) + (1 - s) * LUMA[l]) for l in range(3)]
        m.append(sigma * (0.5 * (1 - c) + beta) + (1.0 if sigma < 0 else 0.0))
    return (dx, dy), m


def params(page_ids, epoch, **kw):
    """(shift int32 [n,2], color float32 [n,12]) of PageAugment(**kw).params(page_ids, epoch)."""
    out = [page_params(int(p), epoch, **kw) for p in np.asarray(page_ids).reshape(-1)]
    shift = np.asarray([o[0] for o in out], dtype=np.int64).reshape(-1, 2).astype(np.int32)
    color = np.asarray([o[1] for o in out], dtype=np.float64).reshape(-1, 12).astype(np.float32)
    return shift, color


def identity(n):
    return np.tile(np.asarray([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (n, 1))


def inversion(n):
    return np.tile(np.asarray([-1, 0, 0, 1, 0, -1, 0, 1, 0, 0, -1, 1], np.float32), (n, 1))


# ------------------------------------------------------------------------------------------------ pixels
def fill_bytes(fill_rgb):
    return np.asarray([(fill_rgb >> 16) & 255, (fill_rgb >> 8) & 255, fill_rgb & 255], np.uint8)


def shifted_bytes(page, dx, dy, fill_rgb):
    """uint8 [H,W,3]: out[y,x] = page[y-dy, x-dx] inside the page, else the fill colour."""
    H, W, _ = page.shape
    sy, sx = np.arange(H, dtype=np.int64) - int(dy), np.arange(W, dtype=np.int64) - int(dx)
    oky, okx = (sy >= 0) & (sy < H), (sx >= 0) & (sx < W)
    v = np.empty((H, W, 3), np.uint8)
    v[:] = fill_bytes(fill_rgb)
    if oky.any() and okx.any():
        v[np.ix_(oky, okx)] = page[np.ix_(sy[oky], sx[okx])]
    return v


def color_transform(t, m):
    """t float32 [H,W,3] in [0,1], m float32 [12] -> float32 [3,H,W], every operation a float32 ufunc of its own."""
    t = np.ascontiguousarray(t, dtype=np.float32)
    m = np.asarray(m, dtype=np.float32)
    out = np.empty((3,) + t.shape[:2], np.float32)
    zero, one = np.float32(0), np.float32(1)
    with np.errstate(all="ignore"):
        for c in range(3):
            y = ((m[4 * c] * t[..., 0] + m[4 * c + 1] * t[..., 1]) + m[4 * c + 2] * t[..., 2]) + m[4 * c + 3]
            assert y.dtype == np.float32
            out[c] = np.where(y > zero, np.minimum(y, one), zero)
    return out


def pages(store_u8, page_idx=None, shift=None, color=None, fill_rgb=0xFFFFFF, out=None):
    """cova_pages_u8_augment_f32: float32 [B,3,H,W].  ``out`` (prefilled) keeps the pages whose index is outside [0,P)."""
    store = np.asarray(store_u8)
    P, H, W, _ = store.shape
    idx = np.arange(P if page_idx is None else len(page_idx)) if page_idx is None else np.asarray(page_idx).reshape(-1)
    B = idx.shape[0]
    shift = np.zeros((B, 2), np.int32) if shift is None else np.asarray(shift).reshape(B, 2)
    color = identity(B) if color is None else np.asarray(color, dtype=np.float32).reshape(B, 12)
    out = np.zeros((B, 3, H, W), np.float32) if out is None else np.array(out, dtype=np.float32)
    for b in range(B):
        if not (0 <= idx[b] < P):
            continue
        v = shifted_bytes(store[idx[b]], shift[b, 0], shift[b, 1], fill_rgb)
        out[b] = color_transform(v.astype(np.float32) / np.float32(255), color[b])
    return out


def pages_naive(store_u8, page_idx, shift, color, fill_rgb):
    """The contract pixel by pixel (Python loops, numpy float32 scalars): for tiny pages only."""
    store = np.asarray(store_u8)
    P, H, W, _ = store.shape
    fb = [(fill_rgb >> 16) & 255, (fill_rgb >> 8) & 255, fill_rgb & 255]
    f = np.float32
    out = np.zeros((len(page_idx), 3, H, W), np.float32)
    for b, p in enumerate(page_idx):
        dx, dy = int(shift[b][0]), int(shift[b][1])
        m = [f(v) for v in color[b]]
        for y in range(H):
            for x in range(W):
                sx, sy = x - dx, y - dy
                inside = 0 <= sx < W and 0 <= sy < H
                t = [f(int(store[p, sy, sx, k]) if inside else fb[k]) / f(255) for k in range(3)]
                for c in range(3):
                    a = f(m[4 * c] * t[0])
                    a = f(a + f(m[4 * c + 1] * t[1]))
                    a = f(a + f(m[4 * c + 2] * t[2]))
                    a = f(a + m[4 * c + 3])
                    out[b, c, y, x] = min(a, f(1)) if a > 0 else f(0)
    return out


# ------------------------------------------------------------------------------------------------ boxes
def translate(bboxes, shift):
    """cova_boxes_translate: rows [N,5] = page,x1,y1,x2,y2; a row whose page column truncates outside [0,B) stays."""
    bb = np.array(bboxes, dtype=np.float32).reshape(-1, 5)
    sh = np.asarray(shift).reshape(-1, 2)
    B = sh.shape[0]
    with np.errstate(all="ignore"):
        p = np.trunc(bb[:, 0].astype(np.float64))
    ok = np.isfinite(p) & (p >= 0) & (p < B)
    pi = np.where(ok, p, 0).astype(np.int64)
    fx, fy = sh[pi, 0].astype(np.float32), sh[pi, 1].astype(np.float32)
    for col, d in ((1, fx), (2, fy), (3, fx), (4, fy)):
        bb[:, col] = np.where(ok, bb[:, col] + d, bb[:, col])
    return bb
