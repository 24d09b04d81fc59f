"""Device-side input pipeline and attention export around the hot path.

``DeviceCollate`` replaces the tensor work of ``WebDataset.__getitem__`` + ``custom_collate_fn``
(reference datasets.py:94-132,159-190): the host hands over uint8 HWC pixels and the raw
``x,y,w,h,label`` rows; ToTensor (/255, CHW), the xywh->xyxy conversion, the page-index column,
the labels and the batch-global context-window table are produced on the GPU
(cova_images_u8_to_f32, cova_collate_boxes).  4x fewer bytes over PCIe than fp32 images.
With ``sampling_fraction < 1`` the background boxes are sampled on the device as datasets.py:101-110
does on the host (cova_sample_boxes, cova_collate_selected).

``DeviceDataset`` keeps a whole split on the card (pages as uint8, rows, additional features) and yields
shuffled, sampled, collated batches (``load_data``, datasets.py:193-265): a batch is a page gather by
index (cova_pages_u8_gather_f32) plus the same sampling and collation kernels; ``epoch_plan`` is the
host-side order of an epoch.

With ``spatial_k > 0`` (both classes) the context table is ``[N, 2*context_size + spatial_k]``: the DOM-order window plus
the ``spatial_k`` nearest other boxes of the page, built by one cova_context_knn launch over the collated (kept) boxes --
after the sampling, on the stream that collated them.  ``DeviceDataset.with_context`` gives the same resident split another
graph.

``PageAugment`` (opt-in, both classes and ``evaluation.fit``; the reference augments nothing) gives every page of every
epoch an integer viewport shift with a constant fill colour and a 3x4 affine colour transform, a function of
``(seed, epoch, page id)`` alone.  The page gather applies both in its one pass (cova_pages_u8_augment_f32) and one
cova_boxes_translate launch moves the collated boxes with the pixels, before the spatial graph is built.  With
``scale=(lo, hi)`` a page also zooms about the centre of its top edge: the gather becomes a fixed-point bilinear resample
(cova_pages_u8_resample_f32) and the boxes take cova_boxes_affine, one launch each in the same places.

``attention_rows`` is the dump of extract_attn_wts_and_visualize.py:104-135.
"""
import numpy as np
import torch

from . import engine
from ._lib import call

_M64 = (1 << 64) - 1


def mix64(s, x):
    """The 64-bit counter hash of csrc/common.h (hash_mix64) on Python integers."""
    z = (s + 0x9E3779B97F4A7C15 * ((x + 1) & _M64)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def stream_seed(seed, epoch):
    """The sampling stream of one epoch: key(page, box) = mix64(mix64(stream_seed, page id), box) >> 1."""
    return mix64(mix64(0, int(seed) & _M64), int(epoch) & _M64)


def keep_count(sampling_fraction, n):
    """Size of the reference's draw for a page of n boxes (datasets.py:103), in Python float64 as there."""
    return int(sampling_fraction * n)


def _check_fraction(sampling_fraction):
    sf = float(sampling_fraction)
    if not (0.0 < sf <= 1.0):                              # datasets.py:37
        raise ValueError("sampling_fraction must be in (0, 1], got %r" % (sampling_fraction,))
    return sf


def _check_rows(r, where):
    try:
        a = np.asarray(r, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError("%s: rows are not numeric" % where)
    if a.size % 5 or (a.ndim == 2 and a.shape[1] != 5) or a.ndim > 2:
        raise ValueError("%s: rows must be [n,5] = x,y,w,h,label, got shape %s" % (where, a.shape))
    a = a.reshape(-1, 5)
    if not np.isfinite(a).all():
        raise ValueError("%s: rows hold non-finite values" % where)
    return a


def _check_graph(context_size, spatial_k):
    """(context_size, spatial_k) as ints; ValueError for a negative spatial_k or a table wider than the GAT kernels take."""
    cs, ks = int(context_size), int(spatial_k)
    if ks < 0:
        raise ValueError("spatial_k must be >= 0, got %r" % (spatial_k,))
    if ks and 2 * cs + ks > engine.GAT_MAX_K:
        raise ValueError("context table of width 2*%d + %d = %d: the graph attention kernels take at most %d neighbour slots"
                         % (cs, ks, 2 * cs + ks, engine.GAT_MAX_K))
    return cs, ks


def _context_knn(bboxes, offs_d, B, cs, ks):
    """cova_context_knn on the current stream: the [N, 2*cs + ks] table of collated boxes (page offsets ``offs_d``)."""
    n = int(bboxes.shape[0])
    ctx = torch.empty((n, 2 * cs + ks), dtype=torch.int64, device=bboxes.device)
    call("cova_context_knn", bboxes, offs_d, B, n, cs, ks, ctx)
    return ctx


def _read_kept_total(out_offs, B):
    """The host read of a sampled batch: 4 bytes, after the two sampling launches on the current stream."""
    return int(out_offs[B].item())


def _mix64_np(s, x):
    """``mix64`` on uint64 arrays (arithmetic modulo 2**64)."""
    with np.errstate(over="ignore"):
        z = s + np.uint64(0x9E3779B97F4A7C15) * (x + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


class PageAugment:
    """Per-page augmentation parameters of cova_pages_u8_augment_f32 / cova_boxes_translate (host only, numpy).

    ``max_shift=(sx, sy)``: the viewport moves by dx in [-sx, sx], dy in [-sy, sy] pixels (content and boxes move right /
    down for positive values); what scrolls in has the colour ``fill`` (R, G, B bytes).  ``brightness`` (an offset in
    [-b, b]), ``contrast``, ``saturation``, ``channel_gain`` (factors in [1-m, 1+m], m < 1) and ``invert_prob`` (light /
    dark theme) fold into one 3x4 matrix per page.  Everything is a function of ``(seed, epoch, page id)``: a stream of
    its own beside the box sampling's, so the kept boxes do not change when augmentation is switched on, and a page's
    pixels do not depend on the batch it lands in, the batch size, the rank or the world size.  Zero magnitudes give zero
    shifts and the exact identity matrix.

    ``scale=(lo, hi)``, 0.5 <= lo <= hi <= 2: the page is also zoomed by a factor drawn from [lo, hi] (slot 9 of the same
    stream, so no shift, colour or sampled box moves when it is switched on) about the centre of its top edge -- pages are
    centred horizontally and grow downwards -- and ``max_shift`` keeps its meaning in output pixels.  The default (1, 1)
    leaves every table and launch as without it (``scales`` is False); ``resample_params`` are the tables otherwise."""

    LUMA = (0.299, 0.587, 0.114)

    def __init__(self, max_shift=(0, 0), brightness=0.0, contrast=0.0, saturation=0.0, channel_gain=0.0, invert_prob=0.0,
                 fill=(255, 255, 255), seed=0, scale=(1.0, 1.0)):
        try:
            lo, hi = (float(v) for v in scale)
        except (TypeError, ValueError):
            raise ValueError("scale must be a pair (lo, hi) of numbers, got %r" % (scale,))
        if not (np.isfinite(lo) and np.isfinite(hi) and 0.5 <= lo <= hi <= 2.0):
            raise ValueError("scale must be finite with 0.5 <= lo <= hi <= 2.0, got %r" % (scale,))
        self.scale = (lo, hi)
        try:
            sx, sy = (int(v) for v in max_shift)
        except (TypeError, ValueError):
            raise ValueError("max_shift must be a pair (sx, sy) of integers, got %r" % (max_shift,))
        if sx < 0 or sy < 0 or sx >= 2 ** 31 or sy >= 2 ** 31:
            raise ValueError("max_shift must be non-negative int32 values, got %r" % (max_shift,))
        self.max_shift = (sx, sy)
        self.brightness, self.contrast = float(brightness), float(contrast)
        self.saturation, self.channel_gain = float(saturation), float(channel_gain)
        self.invert_prob = float(invert_prob)
        for name in ("brightness", "contrast", "saturation", "channel_gain"):
            v = getattr(self, name)
            if not (v >= 0.0) or not np.isfinite(v):
                raise ValueError("%s must be a finite value >= 0, got %r" % (name, v))
            if name != "brightness" and v >= 1.0:
                raise ValueError("%s must be < 1 (the factor stays positive), got %r" % (name, v))
        if not (0.0 <= self.invert_prob <= 1.0):
            raise ValueError("invert_prob must be in [0, 1], got %r" % (invert_prob,))
        try:
            f = tuple(int(v) for v in fill)
        except (TypeError, ValueError):
            raise ValueError("fill must be three bytes (R, G, B), got %r" % (fill,))
        if len(f) != 3 or any(v < 0 or v > 255 or v != w for v, w in zip(f, fill)):
            raise ValueError("fill must be three bytes (R, G, B) in 0..255, got %r" % (fill,))
        self.fill = f
        self.seed = int(seed)

    @property
    def fill_rgb(self):
        return (self.fill[0] << 16) | (self.fill[1] << 8) | self.fill[2]

    @property
    def shifts(self):
        """Whether any page can move (then the boxes need their cova_boxes_translate launch)."""
        return self.max_shift != (0, 0)

    def check_page(self, W, H):
        if self.max_shift[0] >= int(W) or self.max_shift[1] >= int(H):
            raise ValueError("max_shift %r must be smaller than the page (W, H) = (%d, %d) in both directions"
                             % (self.max_shift, W, H))

    @property
    def scales(self):
        """Whether any page can zoom (then the gather is cova_pages_u8_resample_f32 and the boxes take cova_boxes_affine)."""
        return self.scale != (1.0, 1.0)

    def _uniforms(self, page_ids, epoch, slots):
        """float64 [len(slots), n]: u(pid, slot) of the page stream (``params``), one row per requested slot."""
        pids = np.asarray(page_ids).reshape(-1)
        if pids.size and (pids.dtype.kind not in "iu" or (pids < 0).any()):
            raise ValueError("page ids must be non-negative integers")
        stream = np.uint64(mix64(stream_seed(self.seed, epoch), 1))
        page = _mix64_np(stream, pids.astype(np.uint64))
        u = np.empty((len(slots), pids.shape[0]), np.float64)
        for k, slot in enumerate(slots):
            u[k] = (_mix64_np(page, np.uint64(slot)) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        return u

    def _shifts(self, u):
        """int32 [n,2] = dx,dy from the uniforms of slots 0 and 1 (``u[0]``, ``u[1]``)."""
        shift = np.empty((u.shape[1], 2), np.int32)
        for a, s in enumerate(self.max_shift):         # u < 1; the minimum keeps a product that rounds up to 2s+1 inside
            shift[:, a] = np.minimum(np.floor(u[a] * (2 * s + 1)), 2 * s) - s
        return shift

    def resample_params(self, page_ids, epoch, W):
        """-> (step int32 [n,2] = inv_x,inv_y, origin int64 [n,2] = org_x,org_y, affine float32 [n,4] = sx,sy,tx,ty): the
        tables of cova_pages_u8_resample_f32 / cova_boxes_affine for pages of width ``W``.

        Slot 9 of the page stream is the zoom: s = lo + u*(hi - lo) in float64 (slots 0-8 are ``params``'s, untouched).
        inv = round(65536 / s) on both axes, s_eff = 65536 / inv.  The anchor is the horizontal centre of the top edge: it
        maps to itself plus the viewport shift (dx, dy) of ``params``, in output pixels:
        org_x = (W-1)*32768 + ((1 - W - 2*dx)*inv) // 2,  org_y = -32768 + ((1 - 2*dy)*inv) // 2  (integers, floor division);
        boxes: sx = sy = s_eff, tx = W/2 + dx - (W/2)*s_eff, ty = dy, float64 rounded to float32 at the end.  With
        scale == (1, 1): inv = 65536, org = -d*65536, sx = 1, (tx, ty) = (dx, dy)."""
        W = int(W)
        u = self._uniforms(page_ids, epoch, (0, 1, 9))
        n = u.shape[1]
        d = self._shifts(u).astype(np.int64)
        lo, hi = self.scale
        inv = np.rint(65536.0 / (lo + u[2] * (hi - lo))).astype(np.int64)
        s_eff = 65536.0 / inv
        origin = np.empty((n, 2), np.int64)
        origin[:, 0] = (W - 1) * 32768 + ((1 - W - 2 * d[:, 0]) * inv) // 2
        origin[:, 1] = -32768 + ((1 - 2 * d[:, 1]) * inv) // 2
        affine = np.empty((n, 4), np.float64)
        affine[:, 0] = affine[:, 1] = s_eff
        affine[:, 2] = W / 2 + d[:, 0] - (W / 2) * s_eff
        affine[:, 3] = d[:, 1]
        return np.stack([inv, inv], 1).astype(np.int32), origin, affine.astype(np.float32)

    def resample_table(self, page_ids, epoch, W):
        """``resample_params`` as ONE int32 array [n*2 + n*4 + n*4] = steps, the origins' int64 as int32 pairs, the affine
        rows' float32 bits: what goes up behind ``table`` when ``scales`` (the origins 8-byte aligned by the caller)."""
        step, origin, affine = self.resample_params(page_ids, epoch, W)
        return np.concatenate([step.reshape(-1), origin.reshape(-1).view(np.int32), affine.reshape(-1).view(np.int32)])

    def params(self, page_ids, epoch):
        """-> (shift int32 [n,2] = dx,dy, color float32 [n,12] = row-major 3x4, the offset last in a row).

        aug_stream = mix64(stream_seed(seed, epoch), 1);  u(pid, slot) = (mix64(mix64(aug_stream, pid), slot) >> 11) * 2**-53,
        then float64: slots 0, 1: d = floor(u * (2*s + 1)) - s;  2: beta = (2u-1)*brightness;  3: c = 1 + (2u-1)*contrast;
        4: s = 1 + (2u-1)*saturation;  5-7: g_k = 1 + (2u-1)*channel_gain;  8: sigma = -1 if u < invert_prob else 1;
        M[k][l] = sigma*c*g_k*(s*(k==l) + (1-s)*w[l]),  b_k = sigma*(0.5*(1-c) + beta) + (sigma < 0),  w = LUMA; rounded to
        float32 at the end."""
        u = self._uniforms(page_ids, epoch, range(9))
        n = u.shape[1]
        shift = self._shifts(u)
        beta = (2.0 * u[2] - 1.0) * self.brightness
        c = 1.0 + (2.0 * u[3] - 1.0) * self.contrast
        sat = 1.0 + (2.0 * u[4] - 1.0) * self.saturation
        gain = 1.0 + (2.0 * u[5:8] - 1.0) * self.channel_gain
        sigma = np.where(u[8] < self.invert_prob, -1.0, 1.0)
        color = np.empty((n, 3, 4), np.float64)
        for k in range(3):
            for l in range(3):
                color[:, k, l] = sigma * c * gain[k] * (sat * float(k == l) + (1.0 - sat) * self.LUMA[l])
            color[:, k, 3] = sigma * (0.5 * (1.0 - c) + beta) + np.where(sigma < 0, 1.0, 0.0)
        return shift, color.reshape(n, 12).astype(np.float32)

    def table(self, page_ids, epoch):
        """``params`` as ONE int32 array [n*2 + n*12] = shifts, then the colour table's float32 bits (one upload)."""
        shift, color = self.params(page_ids, epoch)
        return np.concatenate([shift.reshape(-1), color.reshape(-1).view(np.int32)])


def _split_aug_table(tab_d, n):
    """(shift int32 [n,2], color float32 [n,12]) views of a device copy of ``PageAugment.table``."""
    return tab_d[:2 * n].view(n, 2), tab_d[2 * n:14 * n].view(torch.float32).view(n, 12)


def _split_resample_table(tab_d, n):
    """(step int32 [n,2], origin int64 [n,2], affine float32 [n,4]) views of a device copy of ``PageAugment.resample_table``
    that starts on an 8-byte boundary."""
    return (tab_d[:2 * n].view(n, 2), tab_d[2 * n:6 * n].view(torch.int64).view(n, 2),
            tab_d[6 * n:10 * n].view(torch.float32).view(n, 4))


def _sample_and_collate(dev, cs, A, rows_d, addl_d, offs_d, starts_d, pid_d, keep_d, keys_d, B, N, sseed, n_out=None,
                        want_sel=False, ks=0, shift_d=None, affine_d=None):
    """cova_sample_boxes + cova_collate_selected on the current stream.  ``n_out`` is the number of kept boxes when the
    host knows it (everything kept); None reads it back from the device: the one 4-byte host read of a sampled batch.
    ``want_sel``: also return the kept SOURCE row ids (int32 [n_out]) under "sel".  ``ks > 0``: the collation writes no
    window; cova_context_knn builds the whole [n_out, 2*cs + ks] table over the kept boxes.  ``shift_d`` (device int32
    [B,2]): cova_boxes_translate moves the collated boxes before the graph is built; ``affine_d`` (device float32 [B,4],
    a zooming augmentation): cova_boxes_affine does, in its place."""
    ws = torch.empty((N + B,), dtype=torch.int32, device=dev)
    sel = torch.empty((N,), dtype=torch.int32, device=dev)
    out_offs = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    call("cova_sample_boxes", rows_d, offs_d, starts_d, pid_d, keep_d, B, N, keys_d, sseed, ws, sel, out_offs)
    if n_out is None:
        n_out = _read_kept_total(out_offs, B)
    K = 0 if ks else 2 * cs
    bboxes = torch.empty((n_out, 5), dtype=torch.float32, device=dev)
    labels = torch.empty((n_out,), dtype=torch.int64, device=dev)
    ctx = torch.empty((n_out, K) if K else (0, 0), dtype=torch.int64, device=dev)   # datasets.py:130
    addl = torch.empty((n_out, A), dtype=torch.float32, device=dev)
    call("cova_collate_selected", rows_d, sel, out_offs, B, n_out, K // 2, bboxes, labels, ctx if K else None,
         addl_d if A else None, A, addl if A else None)
    if affine_d is not None:
        call("cova_boxes_affine", bboxes, n_out, affine_d, B)
    elif shift_d is not None:
        call("cova_boxes_translate", bboxes, n_out, shift_d, B)
    if ks:
        ctx = _context_knn(bboxes, out_offs, B, cs, ks)
    out = dict(bboxes=bboxes, additional_feats=addl, context_indices=ctx, labels=labels,
               page_start=out_offs.to(torch.int64))
    if want_sel:
        out["sel"] = sel[:n_out]
    return out


class DeviceCollate:
    def __init__(self, context_size, device, n_additional_feat=0, pin=False, sampling_fraction=1.0, seed=0, spatial_k=0,
                 augment=None):
        assert context_size >= 0
        self.cs, self.ks = _check_graph(context_size, spatial_k)
        self.device, self.A = torch.device(device), int(n_additional_feat)
        self.pin = bool(pin)            # stage host arrays in pinned memory: H2D copies become asynchronous
        self.sf, self.seed = _check_fraction(sampling_fraction), int(seed)
        self.augment = augment          # a PageAugment: keyed by page_ids (default: the position) and epoch, as the sampler

    def __call__(self, u8_pages, rows_per_page, additional_feats=None, page_ids=None, epoch=0, keys=None):
        """u8_pages: uint8 [B,H,W,3] (numpy or torch, host or device); rows_per_page: list of
        float32 [n,5] arrays.  Returns the batch dict the trainer / CoVA.forward consume.

        With ``sampling_fraction < 1`` each page keeps its labelled boxes and the int(sf * n) boxes of smallest key
        (datasets.py:101-110).  The key of a box is a hash of (seed, epoch, page id, box index); ``page_ids`` are the
        dataset-wide page ids (default: the position in the batch).  ``keys`` (int64 [N], non-negative) injects the keys
        instead: ``keys[perm[j]] = j`` per page reproduces the reference's ``np.random.permutation`` draw ``perm``.

        With ``spatial_k > 0`` ``context_indices`` is [N, 2*context_size + spatial_k] (cova_context_knn over the kept
        boxes); the rows must be finite (ValueError).

        With ``augment`` the pages go through cova_pages_u8_augment_f32 and the collated boxes through
        cova_boxes_translate (before the spatial graph); the batch carries ``aug_shift`` (device int32 [B,2] = dx,dy).
        With ``augment.scales`` the two launches are cova_pages_u8_resample_f32 and cova_boxes_affine and the batch also
        carries ``aug_affine`` (device float32 [B,4] = sx,sy,tx,ty).  Boxes are neither clipped nor dropped."""
        u8 = torch.as_tensor(np.ascontiguousarray(u8_pages) if isinstance(u8_pages, np.ndarray)
                             else u8_pages)
        assert u8.dtype == torch.uint8 and u8.dim() == 4 and u8.shape[3] == 3
        B, H, W, _ = u8.shape
        assert len(rows_per_page) == B
        if self.ks:
            rows_per_page = [_check_rows(r, "page %d" % i) for i, r in enumerate(rows_per_page)]
        counts = [int(np.asarray(r).reshape(-1, 5).shape[0]) for r in rows_per_page]
        N = sum(counts)
        rows = np.concatenate([np.asarray(r, dtype=np.float32).reshape(-1, 5) for r in rows_per_page], 0) \
            if N else np.zeros((0, 5), np.float32)
        offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        dev = self.device
        host = (lambda t: t.pin_memory()) if self.pin else (lambda t: t)
        u8 = (host(u8) if u8.device.type == "cpu" else u8).to(dev, non_blocking=True).contiguous()
        rows_d = host(torch.from_numpy(rows)).to(dev, non_blocking=True)
        images = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
        shift_d = aug_shift = aug_affine = None
        if self.augment is None:
            call("cova_images_u8_to_f32", u8, images, B, H, W)
        else:
            self.augment.check_page(W, H)
            aug_ids = np.arange(B, dtype=np.int64) if page_ids is None else np.asarray(page_ids, dtype=np.int64).reshape(-1)
            if aug_ids.shape[0] != B:
                raise ValueError("page_ids must hold one id in [0, 2**31) per page")
            tab = self.augment.table(aug_ids, epoch)
            if self.augment.scales:             # 14*B ints so far: the zoom tables start on an 8-byte boundary
                tab = np.concatenate([tab, self.augment.resample_table(aug_ids, epoch, W)])
            tab_d = host(torch.from_numpy(tab)).to(dev, non_blocking=True)
            aug_shift, color_d = _split_aug_table(tab_d, B)
            if self.augment.scales:
                step_d, origin_d, aug_affine = _split_resample_table(tab_d[14 * B:], B)
                call("cova_pages_u8_resample_f32", u8, None, B, B, H, W, step_d, origin_d, color_d, self.augment.fill_rgb,
                     images)
            else:
                call("cova_pages_u8_augment_f32", u8, None, B, B, H, W, aug_shift, color_d, self.augment.fill_rgb, images)
                shift_d = aug_shift if self.augment.shifts else None
        if self.sf < 1.0 or keys is not None:
            out = self._sampled(images, rows_d, counts, offs, additional_feats, page_ids, epoch, keys, host, shift_d,
                                aug_affine)
            if aug_shift is not None:
                out["aug_shift"] = aug_shift
            if aug_affine is not None:
                out["aug_affine"] = aug_affine
            return out
        offs_d = host(torch.from_numpy(offs)).to(dev, non_blocking=True)
        bboxes = torch.empty((N, 5), dtype=torch.float32, device=dev)
        labels = torch.empty((N,), dtype=torch.int64, device=dev)
        K = 0 if self.ks else 2 * self.cs
        ctx = torch.empty((N, K) if K else (0, 0), dtype=torch.int64, device=dev)   # datasets.py:130
        call("cova_collate_boxes", rows_d, offs_d, B, N, K // 2, bboxes, labels, ctx if K else None)
        if aug_affine is not None:
            call("cova_boxes_affine", bboxes, N, aug_affine, B)
        elif shift_d is not None:
            call("cova_boxes_translate", bboxes, N, shift_d, B)
        if self.ks:
            ctx = _context_knn(bboxes, offs_d, B, self.cs, self.ks)
        if additional_feats is None:
            addl = torch.empty((N, 0), dtype=torch.float32, device=dev)
        else:
            addl = torch.as_tensor(additional_feats, dtype=torch.float32).to(dev).contiguous()
        out = dict(images=images, bboxes=bboxes, additional_feats=addl, context_indices=ctx,
                   labels=labels, page_start=offs_d.to(torch.int64))
        if aug_shift is not None:
            out["aug_shift"] = aug_shift
        if aug_affine is not None:
            out["aug_affine"] = aug_affine
        return out

    def _sampled(self, images, rows_d, counts, offs, additional_feats, page_ids, epoch, keys, host, shift_d=None,
                 affine_d=None):
        dev, B, N = self.device, len(counts), int(offs[-1])
        if page_ids is None:
            pids = np.arange(B, dtype=np.int64)
        else:
            pids = np.asarray(page_ids, dtype=np.int64).reshape(-1)
            if pids.shape[0] != B or (pids < 0).any() or (pids >= 2 ** 31).any():
                raise ValueError("page_ids must hold one id in [0, 2**31) per page")
        keep = np.asarray([keep_count(self.sf, n) for n in counts], dtype=np.int64)
        ints = np.concatenate([offs.astype(np.int64), keep, pids]).astype(np.int32)      # one small upload
        ints_d = host(torch.from_numpy(ints)).to(dev, non_blocking=True)
        offs_d, keep_d, pid_d = ints_d[:B + 1], ints_d[B + 1:2 * B + 1], ints_d[2 * B + 1:]
        keys_d = None
        if keys is not None:
            k = np.ascontiguousarray(np.asarray(keys, dtype=np.int64).reshape(-1))
            if k.shape[0] != N or (k < 0).any():
                raise ValueError("keys must hold one non-negative integer per box")
            keys_d = host(torch.from_numpy(k)).to(dev, non_blocking=True)
        A, addl_d = 0, None
        if additional_feats is not None:
            addl_d = torch.as_tensor(additional_feats, dtype=torch.float32).to(dev).contiguous()
            if addl_d.dim() != 2 or addl_d.shape[0] != N:
                raise ValueError("additional_feats must be [N, A] with one row per box")
            A = int(addl_d.shape[1])
        out = _sample_and_collate(dev, self.cs, A, rows_d, addl_d, offs_d, None, pid_d, keep_d, keys_d, B, N,
                                  stream_seed(self.seed, epoch), ks=self.ks, shift_d=shift_d, affine_d=affine_d)
        out["images"] = images
        return out


def epoch_plan(n_pages, batch_size, shuffle, seed, epoch, drop_last=False, rank=0, world_size=1, order=None):
    """Page ids of every step of one epoch for this rank (host only): a list of int64 arrays.

    The order is ``order`` if given (any sequence of ids in [0, n_pages)), else a permutation that is a function of
    ``(seed, epoch)`` alone when ``shuffle`` (numpy's frozen RandomState stream seeded with the two; torch's
    RandomSampler stream is NOT reproduced), else 0..n_pages-1.  A global batch is ``batch_size * world_size``
    consecutive entries; a rank takes ``trainer.shard_pages`` of it, i.e. the pages ``trainer.shard_batch`` cuts out of
    the single-process batch.  The short last batch is kept (DataLoader drop_last=False) unless ``drop_last``; a last
    global batch with fewer pages than ranks is always dropped (some rank would get no page and the step's collectives
    would not match)."""
    from .trainer import shard_pages
    n_pages, batch_size, rank, world_size = int(n_pages), int(batch_size), int(rank), int(world_size)
    if n_pages < 0 or batch_size < 1 or world_size < 1 or not (0 <= rank < world_size):
        raise ValueError("epoch_plan: need n_pages >= 0, batch_size >= 1 and 0 <= rank < world_size")
    if order is not None:
        ids = np.asarray(order).reshape(-1)
        if ids.size and (ids.dtype.kind not in "iu" or (ids < 0).any() or (ids >= n_pages).any()):
            raise ValueError("epoch_plan: order must hold integer page ids in [0, %d)" % n_pages)
        ids = ids.astype(np.int64)
    elif shuffle:
        ids = np.random.RandomState([int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF,
                                     (int(epoch) >> 32) & 0xFFFFFFFF]).permutation(n_pages).astype(np.int64)
    else:
        ids = np.arange(n_pages, dtype=np.int64)
    g = batch_size * world_size
    plan = []
    for s in range(0, ids.shape[0], g):
        glob = ids[s:s + g]
        if glob.shape[0] < (g if drop_last else world_size):
            break
        lo, hi = shard_pages(glob.shape[0], rank, world_size)
        plan.append(glob[lo:hi].copy())
    return plan


class DeviceDataset:
    """A whole split resident on the GPU: ``[P,H,W,3]`` uint8 pages, the x,y,w,h,label rows of every page back to back
    and (optionally) the additional features.  ``batches`` yields ``DeviceCollate``'s batch dict for the pages of every
    step of ``epoch_plan``, plus ``page_ids`` (device int64 [B]) and ``img_ids`` (host array of names).
    ``spatial_k > 0``: ``context_indices`` is [N, 2*context_size + spatial_k], the window plus the nearest other boxes of
    the page among the KEPT boxes (cova_context_knn, one launch behind the collation)."""

    STAGING_BYTES = 64 << 20           # pinned staging buffer of the one-off upload

    def __init__(self, u8_pages, rows_per_page, context_size, device, additional_feats=None, img_ids=None, spatial_k=0):
        if int(context_size) < 0:
            raise ValueError("context_size must be >= 0")
        self.cs, self.ks = _check_graph(context_size, spatial_k)
        self.device = torch.device(device)
        if isinstance(u8_pages, (list, tuple)):
            pages = [torch.as_tensor(np.ascontiguousarray(p) if isinstance(p, np.ndarray) else p) for p in u8_pages]
            if not pages or any(p.shape != pages[0].shape for p in pages):
                raise ValueError("u8_pages: a non-empty list of equal-shape pages is needed")
            shape = (len(pages),) + tuple(pages[0].shape)
        else:
            pages = torch.as_tensor(np.ascontiguousarray(u8_pages) if isinstance(u8_pages, np.ndarray) else u8_pages)
            shape = tuple(pages.shape)
        first = pages[0] if isinstance(pages, list) else pages
        if len(shape) != 4 or shape[3] != 3 or shape[0] < 1 or first.dtype != torch.uint8:
            raise ValueError("u8_pages must be uint8 [P,H,W,3], got %s %s" % (first.dtype, shape))
        P, H, W, _ = shape
        self.P, self.H, self.W = P, H, W
        if len(rows_per_page) != P:
            raise ValueError("rows_per_page must hold one [n,5] array per page")
        rows = [_check_rows(r, "page %d" % i) for i, r in enumerate(rows_per_page)]
        self.counts = np.asarray([r.shape[0] for r in rows], dtype=np.int64)          # host copies: the plan of an epoch
        self.starts = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)  # is computed without a device read
        n_total = int(self.starts[-1])
        if n_total >= 2 ** 31:
            raise ValueError("too many boxes for int32 row ids")
        rows = np.concatenate(rows, 0) if n_total else np.zeros((0, 5), np.float32)
        self.A, addl = 0, None
        if additional_feats is not None:
            if isinstance(additional_feats, (list, tuple)):
                parts = [np.asarray(a, dtype=np.float32).reshape(int(n), -1) if int(n) else None
                         for a, n in zip(additional_feats, self.counts)]
                parts = [a for a in parts if a is not None]
                if len(additional_feats) != P or any(a.shape[1] != parts[0].shape[1] for a in parts):
                    raise ValueError("additional_feats must hold one [n,A] array per page")
                addl = np.concatenate(parts, 0) if parts else np.zeros((0, 0), np.float32)
            else:
                addl = np.asarray(torch.as_tensor(additional_feats).cpu(), dtype=np.float32)
            if addl.ndim != 2 or addl.shape[0] != n_total or not np.isfinite(addl).all():
                raise ValueError("additional_feats must be finite [N, A] with one row per box")
            self.A = int(addl.shape[1])
        if img_ids is None:
            self.img_ids = np.asarray([str(i) for i in range(P)])
        else:
            self.img_ids = np.asarray(img_ids)
            if self.img_ids.shape != (P,):
                raise ValueError("img_ids must hold one name per page")
        dev = self.device
        self.rows = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
        self.addl = torch.from_numpy(np.ascontiguousarray(addl)).to(dev) if self.A else None
        self.store = torch.empty((P, H, W, 3), dtype=torch.uint8, device=dev)
        self._upload(pages)
        torch.cuda.synchronize(dev)

    def _upload(self, pages):
        if not isinstance(pages, list) and pages.device.type != "cpu":
            self.store.copy_(pages)
            return
        page_bytes = self.H * self.W * 3
        chunk = max(1, min(self.P, self.STAGING_BYTES // max(page_bytes, 1)))
        staging = torch.empty((chunk, self.H, self.W, 3), dtype=torch.uint8).pin_memory()
        stream = torch.cuda.current_stream(self.device)
        for lo in range(0, self.P, chunk):
            hi = min(self.P, lo + chunk)
            if isinstance(pages, list):
                for k in range(lo, hi):
                    staging[k - lo].copy_(pages[k])
            else:
                staging[:hi - lo].copy_(pages[lo:hi])
            self.store[lo:hi].copy_(staging[:hi - lo], non_blocking=True)
            stream.synchronize()                          # the staging buffer is reused by the next chunk

    def __len__(self):
        return self.P

    def with_context(self, context_size=None, spatial_k=None):
        """The same resident split with another context graph (None keeps a value): the store, the rows, the additional
        features and the names are SHARED -- nothing is uploaded, nothing is copied.  One resident split and one
        features.FeatureCache (it stamps the conv stack and the boxes, not the graph) serve a sweep over graphs."""
        cs = self.cs if context_size is None else int(context_size)
        if cs < 0:
            raise ValueError("context_size must be >= 0")
        cs, ks = _check_graph(cs, self.ks if spatial_k is None else spatial_k)
        other = object.__new__(type(self))
        other.__dict__.update(self.__dict__)
        other.cs, other.ks = cs, ks
        return other

    def batches(self, batch_size, shuffle=False, sampling_fraction=1.0, seed=0, epoch=0, drop_last=False, rank=0,
                world_size=1, order=None, prefetch=True, features=None, augment=None):
        """One epoch of batches (a generator).  Train: ``shuffle=True, sampling_fraction=sf``; val / test: batch 10,
        no shuffle, no sampling (datasets.py:227-258).  With ``prefetch`` batch i+1 is assembled on a side stream while
        the consumer works on batch i.  With ``sampling_fraction == 1`` there is no host read at all; otherwise one
        4-byte read per batch (the number of kept boxes), on the side stream.
        ``features`` (a features.FeatureCache built over this dataset): the pages are not gathered; the batch has no
        ``images`` and carries ``visual_feats`` = (the cache's table, the kept boxes' row ids) instead.
        ``augment`` (a PageAugment; None, the default, is exactly the path above): every page gets the shift and the colour
        transform of ``augment.params(page id, epoch)``; the parameters of the whole epoch go up with the index tables, the
        step's gather is one cova_pages_u8_augment_f32 launch and, when ``max_shift`` is not (0, 0), one
        cova_boxes_translate launch moves the collated boxes before cova_context_knn.  Boxes are neither clipped nor
        dropped: RoIPool / RoIAlign clamp, and a box pushed wholly off the page pools zeros and keeps its label and its
        place in DOM order.  The batch gains ``aug_shift`` (device int32 [B,2] = dx,dy).  With ``augment.scales`` the zoom
        tables ride behind the others in the same copy, the gather is one cova_pages_u8_resample_f32 launch, the boxes take
        one cova_boxes_affine launch in cova_boxes_translate's place and the batch also gains ``aug_affine`` (device float32
        [B,4] = sx,sy,tx,ty: x' = x*sx + tx, y' = y*sy + ty).  Not with ``features``
        (ValueError): cached rows were pooled from unaugmented pixels."""
        if augment is not None:
            if features is not None:
                raise ValueError("augment cannot be combined with features: the cached rows were pooled from unaugmented "
                                 "pixels")
            augment.check_page(self.W, self.H)
        sf = _check_fraction(sampling_fraction)
        if features is not None:
            features.check_dataset(self)
        plan = epoch_plan(self.P, batch_size, shuffle, seed, epoch, drop_last, rank, world_size, order)
        return self._iterate(plan, sf, stream_seed(seed, epoch), bool(prefetch), features, augment, epoch)

    def _iterate(self, plan, sf, sseed, prefetch, features=None, augment=None, epoch=0):
        if not plan:
            return
        dev = self.device
        # the whole epoch's index tables go up in one copy: per step [page ids | batch offsets | row starts | keep counts]
        parts, where, pos = [], [], 0
        for ids in plan:
            n = self.counts[ids]
            part = np.concatenate([ids, np.concatenate([[0], np.cumsum(n)]), self.starts[ids],
                                   [keep_count(sf, int(c)) for c in n]]).astype(np.int32)
            parts.append(part)
            where.append((pos, int(ids.shape[0]), int(n.sum())))
            pos += part.shape[0]
        if augment is not None:     # behind the steps' tables, in the same copy: every page's shift, then the colour bits
            parts.append(augment.table(np.concatenate(plan), epoch))
            if augment.scales:      # and the zoom tables behind those, on an 8-byte boundary (the origins are int64)
                zoom_at = pos + parts[-1].shape[0]
                if zoom_at % 2:
                    parts.append(np.zeros(1, np.int32))
                    zoom_at += 1
                parts.append(augment.resample_table(np.concatenate(plan), epoch, self.W))
        table = torch.from_numpy(np.concatenate(parts)).to(dev)
        ids64 = torch.from_numpy(np.concatenate(plan)).to(dev)
        starts64 = np.concatenate([[0], np.cumsum([len(ids) for ids in plan])])
        zooms = augment is not None and augment.scales
        if augment is not None:
            shifts_d, colors_d = _split_aug_table(table[pos:], int(starts64[-1]))
        if zooms:
            steps_d, origins_d, affines_d = _split_resample_table(table[zoom_at:], int(starts64[-1]))

        def assemble(step):
            pos, B, N = where[step]
            ids_d, offs_d = table[pos:pos + B], table[pos + B:pos + 2 * B + 1]
            starts_d, keep_d = table[pos + 2 * B + 1:pos + 3 * B + 1], table[pos + 3 * B + 1:pos + 4 * B + 1]
            aug_shift = aug_affine = None
            if features is None:
                images = torch.empty((B, 3, self.H, self.W), dtype=torch.float32, device=dev)
                if augment is None:
                    call("cova_pages_u8_gather_f32", self.store, ids_d, self.P, B, self.H, self.W, images)
                else:
                    lo = int(starts64[step])
                    aug_shift = shifts_d[lo:lo + B]
                    if zooms:
                        aug_affine = affines_d[lo:lo + B]
                        call("cova_pages_u8_resample_f32", self.store, ids_d, self.P, B, self.H, self.W, steps_d[lo:lo + B],
                             origins_d[lo:lo + B], colors_d[lo:lo + B], augment.fill_rgb, images)
                    else:
                        call("cova_pages_u8_augment_f32", self.store, ids_d, self.P, B, self.H, self.W, aug_shift,
                             colors_d[lo:lo + B], augment.fill_rgb, images)
            out = _sample_and_collate(dev, self.cs, self.A, self.rows, self.addl, offs_d, starts_d, ids_d, keep_d, None,
                                      B, N, sseed, n_out=N if sf == 1.0 else None, want_sel=features is not None,
                                      ks=self.ks, shift_d=aug_shift if aug_shift is not None and augment.shifts else None,
                                      affine_d=aug_affine)
            if aug_shift is not None:
                out["aug_shift"] = aug_shift
            if aug_affine is not None:
                out["aug_affine"] = aug_affine
            if features is None:
                out["images"] = images
            else:       # the sampler's kept SOURCE row ids are the table's row ids (with sf == 1 it keeps every row)
                out["visual_feats"] = (features.table, out.pop("sel"))
            out["page_size"] = (self.H, self.W)        # host ints (edge geometry on a batch without images reads them)
            out["page_ids"] = ids64[int(starts64[step]):int(starts64[step + 1])]
            out["img_ids"] = self.img_ids[plan[step]]
            return out

        if not prefetch:
            for step in range(len(plan)):
                yield assemble(step)
            return
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))           # the tables above were uploaded on the caller's stream

        def preload(step):
            with torch.cuda.stream(side):
                batch = assemble(step)
                ev = torch.cuda.Event()
                ev.record(side)
            return batch, ev

        pending = preload(0)
        for step in range(len(plan)):
            batch, ev = pending
            cur = torch.cuda.current_stream(dev)
            cur.wait_event(ev)
            for v in batch.values():
                if torch.is_tensor(v):
                    v.record_stream(cur)         # allocated on the side stream, consumed on this one
            if features is not None:
                batch["visual_feats"][1].record_stream(cur)
            pending = preload(step + 1) if step + 1 < len(plan) else None
            yield batch


class Prefetcher:
    """Iterates device batches while the NEXT one is uploaded and collated on a side stream.

    ``source`` yields ``(u8_pages, rows_per_page)`` (or with a third ``additional_feats`` item).  The
    uint8 upload (19.7 MB per 1280x1280 page fp32 -> 4.9 MB) and the two collate kernels of batch i+1
    run on their own HIP stream under the train step of batch i; ``__next__`` makes the consumer's
    stream wait on the upload's event -- the PCIe time never shows in the step time."""

    def __init__(self, collate, source):
        self.collate, self.it = collate, iter(source)
        self.stream = torch.cuda.Stream(device=collate.device)
        self._pending = None
        self._preload()

    def _preload(self):
        try:
            item = next(self.it)
        except StopIteration:
            self._pending = None
            return
        with torch.cuda.stream(self.stream):
            batch = self.collate(*item)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._pending = (batch, ev)

    def __iter__(self):
        return self

    def __next__(self):
        if self._pending is None:
            raise StopIteration
        batch, ev = self._pending
        cur = torch.cuda.current_stream(self.collate.device)
        cur.wait_event(ev)
        for v in batch.values():
            if torch.is_tensor(v):
                v.record_stream(cur)         # allocated on the side stream, consumed on this one
        self._preload()
        return batch


@torch.no_grad()
def attention_rows(trainer, batch):
    """float32 [M, 5+5K] rows for the boxes with label > 0, eval mode (running statistics)."""
    _, sv = engine.model_fwd(trainer.cfg, trainer.params, trainer.buffers, batch["images"],
                             batch["bboxes"], batch["additional_feats"], batch["context_indices"],
                             False, save=True, page_size=batch.get("page_size"))
    attn, ctx = sv["gat"][-1]["heads"][0]["attn"], batch["context_indices"]
    N, K = ctx.shape
    out = torch.empty((N, 5 + 5 * K), dtype=torch.float32, device=attn.device)
    call("cova_attn_export_rows", batch["bboxes"], ctx, attn, batch["labels"], N, K, out)
    return out[batch["labels"] > 0]
