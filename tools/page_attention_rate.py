"""What the page self-attention costs, one process (CoVA(page_attention_dim=E, page_attention_heads=4), cova_page_attn_fwd,
cova_page_attn_bwd).

Kernels: cova_page_attn_fwd / cova_page_attn_bwd at Hh = 4 heads and E = 128 and 384 beside the static attention pair
cova_gat_fwd / cova_gat_bwd at D = E channels and K = 24 and K = 48 neighbour slots, at the head shape of configs[1]
(16 pages x 90 boxes = 1440 rows) and of configs[4] (32 pages x 300 boxes = 9600 rows): device events around ``--launches``
back-to-back launches on one stream, divided by their number (launch overhead that the stream cannot hide is in it), the
median of ``--rounds`` such windows after a warm-up window.  The projections (cova_sgemm) of either operator are left out:
the layer's is one [N, F] x [F, 3E] product where the attention head's is [N, F] x [F, 2D].  The layer touches boxes / K
times the static pair's edges (3.75x at 90 boxes and K = 24, 6.25x at 300 boxes and K = 48): the table gives the ratio of
the pairs next to that multiple.

Step: the train step at configs[1] (16 pages of 1280x1280, 90 boxes a page, the hybrid graph) with page_attention_dim 0
and 128, two trainers over the SAME resident split, legs interleaved and repeated (0, 128, 0, 128, ...): the spread of a
repeated leg is the yardstick for a difference.  Times are a host clock around work that ends in a device synchronise.
No threshold is set.

``--geometry``: the geometry leg instead (CoVA(page_attention_geometry=True), cova_page_attn_fwd_geo /
cova_page_attn_bwd_geo), written to profiles/page_attention_geometry_rate.txt.  Kernels: the ``_geo`` forward and backward
beside the plain pair, same process, same windows, at the same four shapes, boxes drawn like the step's; the share of the
``_geo`` time that the bias adds (the eight features with their correctly rounded divisions, the fma chain, the d w sums)
is (geo - plain) / geo.  Step: configs[1] with page_attention_dim=128, page_attention_heads=4, without and with the option,
interleaved and repeated as above.  The yardstick is the plain pair and the step without the option.

    python tools/page_attention_rate.py [--geometry] [--rounds 7] [--steps 40] [--pages 256] [--launches 200] [--out FILE]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--pages", type=int, default=256, help="pages of the resident split (a multiple of 16)")
ap.add_argument("--launches", type=int, default=200, help="back-to-back kernel launches per timed window")
ap.add_argument("--img", type=int, default=1280, help="page side of the step legs (configs[1]: 1280)")
ap.add_argument("--geometry", action="store_true", help="the geometry leg: the _geo pair against the plain pair")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join(ROOT, "profiles", "page_attention_geometry_rate.txt" if args.geometry
                            else "page_attention_rate.txt")

import numpy as np  # noqa: E402
import torch  # noqa: E402
import cova_amd  # noqa: E402,F401
from cova_web_object_detection_amd import weights  # noqa: E402
from cova_web_object_detection_amd._lib import call, query  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402

assert torch.cuda.is_available(), "page_attention_rate.py measures on the GPU only"
dev = "cuda:0"
WARMUP = 6
HEADS = 4
out = []


# ------------------------------------------------------------------------------------------------ the launches alone
def windows(fn):
    v = []
    for rnd in range(args.rounds + 1):                                  # window 0 is the warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if rnd:
            v.append(1e3 * e0.elapsed_time(e1) / args.launches)
    return np.asarray(v)


def kernel_legs(what, B, boxes, E):
    N, D = B * boxes, E
    tg = torch.Generator(device=dev).manual_seed(1)
    rnd_ = lambda *shape: torch.randn(shape, device=dev, generator=tg)
    new = lambda *shape: torch.empty(shape, device=dev)
    ps = torch.arange(B + 1, dtype=torch.int64, device=dev) * boxes
    # the layer's operands: qkv [N, 3E]
    qkv, gr = rnd_(N, 3 * E), rnd_(N, E)
    o, lse, dqkv = new(N, E), new(N, HEADS), new(N, 3 * E)
    launches = [
        ("cova_page_attn_fwd", lambda: call("cova_page_attn_fwd", qkv, 3 * E, ps, B, N, E, HEADS, o, E, lse)),
        ("cova_page_attn_bwd", lambda: call("cova_page_attn_bwd", gr, E, qkv, 3 * E, o, E, lse, ps, B, N, E, HEADS, dqkv,
                                            3 * E)),
    ]
    # the static pair's: Wh [N, 2D], K page-local neighbours per row
    Wh, aw, ab = rnd_(N, 2 * D), rnd_(2 * D) / D ** 0.5, rnd_(1)
    s, t, hp = new(N), new(N), new(N, D)
    dWh, dsv, dtv, daw, dab = new(N, 2 * D), new(N), new(N), new(2 * D), new(1)
    keep = []
    for K in (24, 48):
        local = torch.randint(0, boxes, (N, K), device=dev, generator=tg)
        ctx = (local + (torch.arange(N, device=dev) // boxes * boxes).view(-1, 1)).to(torch.int64).contiguous()
        attn, du = new(N, K), new(N, K)
        csr = torch.zeros((query("cova_gat_transpose_ints", N, K),), dtype=torch.int32, device=dev)
        call("cova_gat_transpose", ctx, N, K, csr)
        keep.append((ctx, attn, du, csr))
        launches.append(("cova_gat_fwd K=%d" % K,
                         lambda ctx=ctx, attn=attn, K=K: call("cova_gat_fwd", Wh, 2 * D, aw, ab, ctx, N, K, D, 0.2, s, t,
                                                              attn, hp, D)))
        launches.append(("cova_gat_bwd K=%d" % K,
                         lambda ctx=ctx, attn=attn, du=du, csr=csr, K=K: call(
                             "cova_gat_bwd", gr, D, Wh, 2 * D, s, t, attn, ctx, aw, N, K, D, 0.2, dWh, 2 * D, dsv, dtv, daw,
                             dab, csr, du)))
    out.append("page_attention_rate, launches at %s: %d pages x %d boxes = %d rows, E = D = %d, Hh = %d; %d back-to-back "
               "calls per window, %d windows after one warm-up window; us per call (cova_page_attn_fwd issues 1 kernel, "
               "cova_page_attn_bwd 2, cova_gat_fwd 2, cova_gat_bwd 3)" % (what, B, boxes, N, E, HEADS, args.launches, args.rounds))
    med = {}
    for name, fn in launches:
        v = windows(fn)
        med[name] = float(np.median(v))
        out.append("  %-20s median %8.2f us  min %8.2f  max %8.2f" % (name, np.median(v), v.min(), v.max()))
    pair = med["cova_page_attn_fwd"] + med["cova_page_attn_bwd"]
    for K in (24, 48):
        gat = med["cova_gat_fwd K=%d" % K] + med["cova_gat_bwd K=%d" % K]
        out.append("  attention pair / static pair at K = %d: forward %.2f, backward %.2f, the pair %.2f (edges: %.2fx)"
                   % (K, med["cova_page_attn_fwd"] / med["cova_gat_fwd K=%d" % K],
                      med["cova_page_attn_bwd"] / med["cova_gat_bwd K=%d" % K], pair / gat, boxes / K))
    # what the pair's matrix products are, against the time: 2 products forward (pass 1 repeats Q K^T: 3), 7 backward
    flops = 2.0 * B * boxes * boxes * E
    out.append("  useful matrix work: forward %.1f GFLOP/s of 2 products, backward %.1f GFLOP/s of 5 products (the kernels "
               "issue 3 and 7: pass 1 and the key side recompute the scores)"
               % (2 * flops / med["cova_page_attn_fwd"] / 1e3, 5 * flops / med["cova_page_attn_bwd"] / 1e3))


def page_rows(rs, boxes, img_w, img_h):
    wh = np.stack([rs.uniform(8, 400, boxes), rs.uniform(8, 200, boxes)], 1)
    xy = rs.uniform(0, 1, (boxes, 2)) * (np.asarray([img_w, img_h]) - wh)
    lab = np.zeros((boxes, 1))
    lab[rs.permutation(boxes)[:3], 0] = [1, 2, 3]
    return np.concatenate([xy, wh, lab], 1).astype(np.float32)


def geometry_kernel_legs(what, B, boxes, E):
    """The _geo pair beside the plain pair on the same qkv, g and pages; boxes as page_rows draws them on a 1280 x 1280 page."""
    N, img = B * boxes, float(args.img)
    tg = torch.Generator(device=dev).manual_seed(1)
    rnd_ = lambda *shape: torch.randn(shape, device=dev, generator=tg)
    new = lambda *shape: torch.empty(shape, device=dev)
    ps = torch.arange(B + 1, dtype=torch.int64, device=dev) * boxes
    qkv, gr, gw = rnd_(N, 3 * E), rnd_(N, E), rnd_(HEADS, 8)
    o, lse, dqkv, dgw = new(N, E), new(N, HEADS), new(N, 3 * E), new(HEADS, 8)
    rs = np.random.RandomState(2)
    rows = np.concatenate([page_rows(rs, boxes, img, img) for _ in range(B)])
    bb = np.concatenate([np.repeat(np.arange(B), boxes)[:, None], rows[:, :2], rows[:, :2] + rows[:, 2:4]], 1)
    bb = torch.from_numpy(bb.astype(np.float32)).to(dev)
    ws = new(query("cova_page_attn_geo_workspace_floats", B, N, HEADS))
    launches = [
        ("cova_page_attn_fwd", lambda: call("cova_page_attn_fwd", qkv, 3 * E, ps, B, N, E, HEADS, o, E, lse)),
        ("cova_page_attn_fwd_geo", lambda: call("cova_page_attn_fwd_geo", qkv, 3 * E, ps, bb, gw, img, img, B, N, E, HEADS, o,
                                                E, lse)),
        ("cova_page_attn_bwd", lambda: call("cova_page_attn_bwd", gr, E, qkv, 3 * E, o, E, lse, ps, B, N, E, HEADS, dqkv,
                                            3 * E)),
        ("cova_page_attn_bwd_geo", lambda: call("cova_page_attn_bwd_geo", gr, E, qkv, 3 * E, o, E, lse, ps, bb, gw, img, img,
                                                B, N, E, HEADS, dqkv, 3 * E, dgw, ws)),
    ]
    out.append("page_attention_rate --geometry, launches at %s: %d pages x %d boxes = %d rows, E = %d, Hh = %d (dh = %d); %d "
               "back-to-back calls per window, %d windows after one warm-up window; us per call (the forwards issue 1 "
               "kernel, cova_page_attn_bwd 2, cova_page_attn_bwd_geo 3)"
               % (what, B, boxes, N, E, HEADS, E // HEADS, args.launches, args.rounds))
    med = {}
    for name, fn in launches:
        v = windows(fn)
        med[name] = float(np.median(v))
        out.append("  %-24s median %8.2f us  min %8.2f  max %8.2f" % (name, np.median(v), v.min(), v.max()))
    f, fg, b, bg = (med["cova_page_attn_" + k] for k in ("fwd", "fwd_geo", "bwd", "bwd_geo"))
    out.append("  geo / plain: forward %.2f, backward %.2f, the pair %.2f; share of the _geo time that the bias adds: forward "
               "%.0f %%, backward %.0f %%, the pair %.0f %%"
               % (fg / f, bg / b, (fg + bg) / (f + b), 100 * (fg - f) / fg, 100 * (bg - b) / bg,
                  100 * (fg + bg - f - b) / (fg + bg)))
    scores = B * boxes * boxes * HEADS
    out.append("  feature evaluations: %.2f M per pass (2 passes forward, 2 sides backward); added time per evaluation: "
               "forward %.1f ps, backward %.1f ps" % (scores / 1e6, 1e6 * (fg - f) / (2 * scores), 1e6 * (bg - b) / (2 * scores)))


for shape in (("configs[1]'s head", 16, 90, 128), ("configs[1]'s head", 16, 90, 384), ("configs[4]'s head", 32, 300, 128),
              ("configs[4]'s head", 32, 300, 384)):
    (geometry_kernel_legs if args.geometry else kernel_legs)(*shape)


# ------------------------------------------------------------------------------------------------ the train step

CFG = dict(roi_output_size=(3, 3), n_classes=4, use_context=True, hidden_dim=384, bbox_hidden_dim=32,
           n_additional_feat=0, drop_prob=0.2)
BATCH, IMG, BOXES, CS, KS = 16, args.img, 90, 6, 12
NP = max(BATCH, args.pages // BATCH * BATCH)
rs = np.random.RandomState(0)
g = torch.Generator(device=dev).manual_seed(0)
u8_dev = torch.empty((NP, IMG, IMG, 3), dtype=torch.uint8, device=dev)
for lo in range(0, NP, 64):
    u8_dev[lo:lo + 64] = torch.randint(0, 256, (min(64, NP - lo), IMG, IMG, 3), dtype=torch.uint8, device=dev, generator=g)
ds = DeviceDataset(u8_dev, [page_rows(rs, BOXES, IMG, IMG) for _ in range(NP)], CS, dev, spatial_k=KS)
legs = ["off", "on"] if args.geometry else [0, 128]          # the first leg is the yardstick
trainers = {}
for E in legs:
    cfg = (dict(CFG, page_attention_dim=128, page_attention_heads=HEADS, page_attention_geometry=E == "on") if args.geometry
           else dict(CFG, page_attention_dim=E, page_attention_heads=HEADS))
    sd = weights.seeded_state_dict(123, **{k: v for k, v in cfg.items() if k != "drop_prob"})
    if args.geometry and E == "on":      # (a zero weight costs what any weight costs; a seeded one shows a live bias)
        key = "page_attention.geometry.weight"
        sd[key] = torch.from_numpy(np.random.RandomState(5).standard_normal(tuple(sd[key].shape)).astype(np.float32))
    trainers[E] = HotPathTrainer(cfg, sd, dev)


def steps(tr, n, epoch0):
    done, epoch = 0, epoch0
    while done < n:
        for b in ds.batches(BATCH, shuffle=True, sampling_fraction=1.0, seed=1, epoch=epoch):
            tr.train_step(b)
            done += 1
            if done == n:
                break
        epoch += 1


for E in legs:                          # warm-up: every shape and code path of the timed window
    steps(trainers[E], WARMUP, 0)
torch.cuda.synchronize()
ms = {E: [] for E in legs}
for rnd in range(args.rounds):
    for E in legs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps(trainers[E], args.steps, rnd + 1)
        torch.cuda.synchronize()
        ms[E].append(1e3 * (time.perf_counter() - t0) / args.steps)

out.append("page_attention_rate, step: %d pages resident (%.2f GB uint8), batch %d x %dx%d, %d boxes/page, hybrid graph "
           "(context_size %d, spatial_k %d), sampling fraction 1; %d rounds x %d steps, warm-up %d steps; ms per train step"
           % (NP, NP * IMG * IMG * 3 / 1e9, BATCH, IMG, IMG, BOXES, CS, KS, args.rounds, args.steps, WARMUP))
label = "page_attention_dim=128, page_attention_geometry=%-3s" if args.geometry else "page_attention_dim=%-3d"
for E in legs:
    v = np.asarray(ms[E])
    out.append(("leg " + label + " median %.3f  min %.3f  max %.3f  spread %.3f  [%s]")
               % (E, np.median(v), v.min(), v.max(), v.max() - v.min(), " ".join("%.3f" % x for x in v)))
base, spread = float(np.median(ms[legs[0]])), float(np.max(ms[legs[0]]) - np.min(ms[legs[0]]))
d = float(np.median(ms[legs[1]])) - base
out.append("leg %s - leg %s: %+.3f ms/step (%+.2f %%); spread of the repeated leg %s: %.3f ms"
           % (legs[1], legs[0], d, 100 * d / base, legs[0], spread))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(out) + "\n")
print("\n".join(out))
