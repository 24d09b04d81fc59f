"""CPU restatement (numpy) of the page zoom (include/cova_hip.h: cova_pages_u8_resample_f32, cova_boxes_affine) and of the
parameter formulas of pipeline.PageAugment.resample_params, written from their contracts without importing the package.

Pixels: Python / numpy int64 up to the integer tap sum q, then one float32 division and the colour row of
tests/augment_oracle.py.  Parameters: Python integers and floats (float64), rounded to float32 once at the end."""
import numpy as np

from augment_oracle import color_transform, fill_bytes, identity, page_params, uniform

DEN = 255 * 65536


# ------------------------------------------------------------------------------------------------ parameters
def zoom(pid, epoch, seed=0, scale=(1.0, 1.0)):
    """Slot 9 of the page stream: s = lo + u*(hi - lo), float64."""
    lo, hi = float(scale[0]), float(scale[1])
    return lo + uniform(seed, epoch, pid, 9) * (hi - lo)


def page_resample_params(pid, epoch, W, seed=0, scale=(1.0, 1.0), **kw):
    """((inv, inv), (org_x, org_y) Python integers, (sx, sy, tx, ty) float64) of one page of width W."""
    (dx, dy), _ = page_params(pid, epoch, seed=seed, **kw)
    dx, dy, W = int(dx), int(dy), int(W)
    inv = int(round(65536.0 / zoom(pid, epoch, seed, scale)))              # ties to even, as numpy's rint
    s_eff = 65536.0 / inv
    org_x = (W - 1) * 32768 + ((1 - W - 2 * dx) * inv) // 2
    org_y = -32768 + ((1 - 2 * dy) * inv) // 2
    return (inv, inv), (org_x, org_y), (s_eff, s_eff, W / 2 + dx - (W / 2) * s_eff, float(dy))


def resample_params(page_ids, epoch, W, **kw):
    """(step int32 [n,2], origin int64 [n,2], affine float32 [n,4]) of PageAugment(**kw).resample_params(page_ids, epoch, W)."""
    out = [page_resample_params(int(p), epoch, W, **kw) for p in np.asarray(page_ids).reshape(-1)]
    step = np.asarray([o[0] for o in out], dtype=np.int64).reshape(-1, 2).astype(np.int32)
    origin = np.asarray([o[1] for o in out], dtype=np.int64).reshape(-1, 2)
    affine = np.asarray([o[2] for o in out], dtype=np.float64).reshape(-1, 4).astype(np.float32)
    return step, origin, affine


# ------------------------------------------------------------------------------------------------ pixels
def tap_sums(page, inv, org, fill_rgb):
    """int64 [H,W,3]: q of every output pixel of one page (uint8 [H,W,3]); inv = (inv_x, inv_y), org = (org_x, org_y)."""
    H, W, _ = page.shape
    padded = np.empty((H + 1, W + 1, 3), np.int64)                         # row H / column W hold the fill colour
    padded[:] = fill_bytes(fill_rgb).astype(np.int64)
    padded[:H, :W] = page
    px = int(org[0]) + np.arange(W, dtype=np.int64) * int(inv[0])
    py = int(org[1]) + np.arange(H, dtype=np.int64) * int(inv[1])
    ix, fx = px >> 16, (px >> 8) & 255
    iy, fy = py >> 16, (py >> 8) & 255
    q = np.zeros((H, W, 3), np.int64)
    for ty, wy in ((iy, 256 - fy), (iy + 1, fy)):
        ry = np.where((ty >= 0) & (ty < H), ty, H)
        for tx, wx in ((ix, 256 - fx), (ix + 1, fx)):
            rx = np.where((tx >= 0) & (tx < W), tx, W)
            q += (wy[:, None] * wx[None, :])[:, :, None] * padded[np.ix_(ry, rx)]
    return q


def pages(store_u8, page_idx, step, origin, color=None, fill_rgb=0xFFFFFF, out=None):
    """cova_pages_u8_resample_f32: float32 [B,3,H,W].  ``out`` (prefilled) keeps the pages whose index is outside [0,P)."""
    store = np.asarray(store_u8)
    P, H, W, _ = store.shape
    idx = np.arange(len(step)) if page_idx is None else np.asarray(page_idx).reshape(-1)
    B = idx.shape[0]
    color = identity(B) if color is None else np.asarray(color, dtype=np.float32).reshape(B, 12)
    out = np.zeros((B, 3, H, W), np.float32) if out is None else np.array(out, dtype=np.float32)
    for b in range(B):
        if not (0 <= idx[b] < P):
            continue
        q = tap_sums(store[idx[b]], step[b], origin[b], fill_rgb)
        assert q.min() >= 0 and q.max() <= DEN
        out[b] = color_transform(q.astype(np.float32) / np.float32(DEN), color[b])
    return out


def pages_naive(store_u8, page_idx, step, origin, color, fill_rgb):
    """The contract pixel by pixel (Python integers, numpy float32 scalars): for tiny pages only."""
    store = np.asarray(store_u8)
    P, H, W, _ = store.shape
    fb = [(fill_rgb >> 16) & 255, (fill_rgb >> 8) & 255, fill_rgb & 255]
    f = np.float32
    out = np.zeros((len(page_idx), 3, H, W), np.float32)
    for b, p in enumerate(page_idx):
        inv_x, inv_y, org_x, org_y = int(step[b][0]), int(step[b][1]), int(origin[b][0]), int(origin[b][1])
        m = [f(v) for v in color[b]]
        for y in range(H):
            for x in range(W):
                px, py = org_x + x * inv_x, org_y + y * inv_y
                ix, iy, fx, fy = px >> 16, py >> 16, (px >> 8) & 255, (py >> 8) & 255
                t = []
                for k in range(3):
                    q = 0
                    for ty, wy in ((iy, 256 - fy), (iy + 1, fy)):
                        for tx, wx in ((ix, 256 - fx), (ix + 1, fx)):
                            v = int(store[p, ty, tx, k]) if 0 <= tx < W and 0 <= ty < H else fb[k]
                            q += wy * wx * v
                    t.append(f(q) / f(DEN))
                for c in range(3):
                    a = f(m[4 * c] * t[0])
                    a = f(a + f(m[4 * c + 1] * t[1]))
                    a = f(a + f(m[4 * c + 2] * t[2]))
                    a = f(a + m[4 * c + 3])
                    out[b, c, y, x] = min(a, f(1)) if a > 0 else f(0)
    return out


# ------------------------------------------------------------------------------------------------ boxes
def affine_boxes(bboxes, affine):
    """cova_boxes_affine: rows [N,5] = page,x1,y1,x2,y2; a row whose page column truncates outside [0,B) stays."""
    bb = np.array(bboxes, dtype=np.float32).reshape(-1, 5)
    af = np.asarray(affine, dtype=np.float32).reshape(-1, 4)
    B = af.shape[0]
    with np.errstate(all="ignore"):
        p = np.trunc(bb[:, 0].astype(np.float64))
    ok = np.isfinite(p) & (p >= 0) & (p < B)
    pi = np.where(ok, p, 0).astype(np.int64)
    for col, s, t in ((1, 0, 2), (2, 1, 3), (3, 0, 2), (4, 1, 3)):
        with np.errstate(all="ignore"):
            prod = bb[:, col] * af[pi, s]                                  # one float32 multiply ...
            moved = prod + af[pi, t]                                       # ... then one float32 add
        assert moved.dtype == np.float32
        bb[:, col] = np.where(ok, moved, bb[:, col])
    return bb
