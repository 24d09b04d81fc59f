"""What a spatial context graph costs, one process (pipeline.DeviceDataset(spatial_k=), cova_context_knn).

Kernel: the time of one cova_context_knn launch at the configs[1] shape (16 pages x 90 boxes, K = 24) and at the configs[4]
shape (300 boxes a page, K = 48), each as pure spatial, hybrid and window-only table: device events around ``--launches``
back-to-back launches on one stream, divided by their number (launch overhead that the stream cannot hide is in it), the
median of ``--rounds`` such windows after a warm-up.

Step: the train step at configs[1] (16 pages of 1280x1280, 90 boxes a page) fed by DeviceDataset with
  w  context_size 12, spatial_k 0    the DOM-order window, as today (no cova_context_knn launch)
  s  context_size 0,  spatial_k 24   the 24 nearest boxes
  h  context_size 6,  spatial_k 12   window + nearest boxes
over the SAME resident split (DeviceDataset.with_context), legs interleaved and repeated: the spread of a repeated leg is the
yardstick for a difference.  All three tables are 24 wide; what differs is the launch that builds them and the rows of the
transposed CSR the GAT backward walks (an irregular graph has hubs).  Times are a host clock around work that ends in a device
synchronise.  No threshold is set.

    python tools/graph_rate.py [--rounds 7] [--steps 40] [--pages 256] [--launches 200] [--out profiles/graph_rate.txt]
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_rate.txt"))
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import cova_amd  # noqa: E402,F401
from cova_web_object_detection_amd import weights  # noqa: E402
from cova_web_object_detection_amd._lib import call  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402

assert torch.cuda.is_available(), "graph_rate.py measures on the GPU only"
dev = "cuda:0"
WARMUP = 6
out = []


def page_rows(rs, boxes, img_w, img_h):
    wh = np.stack([rs.uniform(8, 400, boxes), rs.uniform(8, 200, boxes)], 1)
    xy = rs.uniform(0, 1, (boxes, 2)) * (np.asarray([img_w, img_h]) - wh)
    lab = np.zeros((boxes, 1))
    lab[rs.permutation(boxes)[:3], 0] = [1, 2, 3]
    return np.concatenate([xy, wh, lab], 1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the kernel alone
def kernel_us(pages, boxes, img_w, img_h, cs, k):
    rs = np.random.RandomState(boxes)
    rows = np.concatenate([page_rows(rs, boxes, img_w, img_h) for _ in range(pages)], 0)
    n = rows.shape[0]
    bb = np.zeros((n, 5), np.float32)
    bb[:, 0] = np.repeat(np.arange(pages), boxes)
    bb[:, 1:3] = rows[:, 0:2]
    bb[:, 3:5] = rows[:, 0:2] + rows[:, 2:4]
    bb_d = torch.from_numpy(bb).to(dev)
    offs_d = torch.arange(0, n + 1, boxes, dtype=torch.int32, device=dev)
    ctx = torch.empty((n, 2 * cs + k), dtype=torch.int64, device=dev)
    windows = []
    for rnd in range(args.rounds + 1):                                  # window 0 is the warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            call("cova_context_knn", bb_d, offs_d, pages, n, cs, k, ctx)
        e1.record()
        torch.cuda.synchronize()
        if rnd:
            windows.append(1e3 * e0.elapsed_time(e1) / args.launches)
    return np.asarray(windows)


out.append("graph_rate, kernel: cova_context_knn, %d back-to-back launches per window, %d windows after one warm-up window; "
           "us per launch" % (args.launches, args.rounds))
for label, pages, boxes, w, h, shapes in (
        ("configs[1] 16 pages x 90 boxes", 16, 90, 1280, 1280, ((0, 24), (6, 12), (12, 0))),
        ("configs[4] 16 pages x 300 boxes", 16, 300, 1280, 4096, ((0, 48), (12, 24), (24, 0)))):
    for cs, k in shapes:
        v = kernel_us(pages, boxes, w, h, cs, k)
        out.append("  %-32s context_size %2d spatial_k %2d (K = %2d): median %7.2f us  min %7.2f  max %7.2f"
                   % (label, cs, k, 2 * cs + k, np.median(v), v.min(), v.max()))

# ------------------------------------------------------------------------------------------------ the train step
CFG = dict(roi_output_size=(3, 3), n_classes=4, use_context=True, hidden_dim=384, bbox_hidden_dim=32,
           n_additional_feat=0, drop_prob=0.2)
BATCH, IMG, BOXES = 16, args.img, 90
P = max(BATCH, args.pages // BATCH * BATCH)
rs = np.random.RandomState(0)
g = torch.Generator(device=dev).manual_seed(0)
u8_dev = torch.empty((P, IMG, IMG, 3), dtype=torch.uint8, device=dev)
for lo in range(0, P, 64):
    u8_dev[lo:lo + 64] = torch.randint(0, 256, (min(64, P - lo), IMG, IMG, 3), dtype=torch.uint8, device=dev, generator=g)
rows = [page_rows(rs, BOXES, IMG, IMG) for _ in range(P)]
window = DeviceDataset(u8_dev, rows, 12, dev)
sets = dict(w=window, s=window.with_context(0, 24), h=window.with_context(6, 12))
assert all(d.store.data_ptr() == window.store.data_ptr() for d in sets.values())
wcfg = {k: v for k, v in CFG.items() if k != "drop_prob"}
tr = HotPathTrainer(CFG, weights.seeded_state_dict(123, **wcfg), dev)


def steps(ds, n, epoch0):
    done, epoch = 0, epoch0
    while done < n:
        for b in ds.batches(BATCH, shuffle=True, sampling_fraction=1.0, seed=1, epoch=epoch):
            tr.train_step(b)
            done += 1
            if done == n:
                break
        epoch += 1


legs = ["w", "s", "h"]
for name in legs:                       # warm-up: every shape and code path of the timed window
    steps(sets[name], WARMUP, 0)
torch.cuda.synchronize()
ms = {name: [] for name in legs}
for rnd in range(args.rounds):
    for name in legs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps(sets[name], args.steps, rnd + 1)
        torch.cuda.synchronize()
        ms[name].append(1e3 * (time.perf_counter() - t0) / args.steps)

# in-degree of the graphs of one batch: the rows of the transposed CSR the GAT backward walks
indeg = {}
for name in legs:
    ctx = next(iter(sets[name].batches(BATCH, prefetch=False)))["context_indices"]
    d = torch.bincount(ctx[ctx >= 0].reshape(-1), minlength=ctx.shape[0])
    indeg[name] = (float(d.float().mean()), int(d.max()), int((ctx >= 0).sum()))

what = dict(w="window  context_size 12, spatial_k  0", s="spatial context_size  0, spatial_k 24",
            h="hybrid  context_size  6, spatial_k 12")
out.append("graph_rate, step: %d pages resident (%.2f GB uint8), batch %d x %dx%d, %d boxes/page, sampling fraction 1; %d rounds "
           "x %d steps, warm-up %d steps; ms per train step" % (P, P * IMG * IMG * 3 / 1e9, BATCH, IMG, IMG, BOXES, args.rounds,
                                                                 args.steps, WARMUP))
for name in legs:
    v = np.asarray(ms[name])
    out.append("leg %s  %-38s median %.3f  min %.3f  max %.3f  spread %.3f  [%s]  in-degree mean %.1f max %d, %d edges"
               % (name, what[name], np.median(v), v.min(), v.max(), v.max() - v.min(), " ".join("%.3f" % x for x in v),
                  indeg[name][0], indeg[name][1], indeg[name][2]))
base, spread = float(np.median(ms["w"])), float(np.max(ms["w"]) - np.min(ms["w"]))
for name in ("s", "h"):
    d = float(np.median(ms[name])) - base
    out.append("leg %s - leg w: %+.3f ms/step (%+.2f %%); spread of the repeated leg w: %.3f ms" % (name, d, 100 * d / base, spread))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(out) + "\n")
print("\n".join(out))
