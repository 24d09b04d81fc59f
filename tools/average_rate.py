"""What weight averaging costs, one process (HotPathTrainer(average=), cova_weight_average).

Launch: the averaging launches of the configs[1] trainer alone -- the parameter bucket (1.6 M floats, one table row) and
the BatchNorm statistics (one row) -- with cova_adam_step over the same bucket beside them: device events around
``--launches`` back-to-back launches on one stream, divided by their number (launch overhead that the stream cannot hide
is in it), the median of ``--rounds`` such windows after a warm-up window.

Step: the train step at configs[1] (16 pages of 1280x1280, 90 boxes a page) on DeviceDataset-fed trainers over the SAME
resident split in three legs: "off" (average=None), "ema" (average="ema": two launches and one counter copy per step) and
"nobuf" (average="swa", average_buffers=False: one launch), interleaved and repeated (off, ema, nobuf, off, ...).  The
overhead is reported against leg "off" of this same run; the spread of the repeated leg "off" is the yardstick for a
difference.  Times are a host clock around work that ends in a device synchronise.  No threshold is set.

    python tools/average_rate.py [--rounds 7] [--steps 40] [--pages 256] [--launches 200] [--out profiles/average_rate.txt]
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "average_rate.txt"))
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import cova_amd  # noqa: E402,F401
from cova_web_object_detection_amd import engine, weights  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer, average_weight  # noqa: E402

assert torch.cuda.is_available(), "average_rate.py measures on the GPU only"
dev = "cuda:0"
WARMUP = 6
CS = 6
out = []

CFG = dict(roi_output_size=(3, 3), n_classes=4, use_context=True, hidden_dim=384, bbox_hidden_dim=32,
           n_additional_feat=0, drop_prob=0.2)
legs = {"off": dict(), "ema": dict(average="ema"), "nobuf": dict(average="swa", average_buffers=False)}
sd = weights.seeded_state_dict(123, **{k: v for k, v in CFG.items() if k != "drop_prob"})
trainers = {name: HotPathTrainer(CFG, sd, dev, **kw) for name, kw in legs.items()}


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


tr = trainers["ema"]
n, nb = tr.pbucket.flat.numel(), tr.bbucket.flat.numel()
w = average_weight("ema", 0.999, None, 1)
g = torch.randn(n, device=dev) * 1e-3
m, v2 = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
p = tr.pbucket.flat.clone()
avg, bavg = tr.abucket.flat.clone(), tr.abbucket.flat.clone()
calls = (("cova_weight_average  parameters", n, lambda: engine.call(
              "cova_weight_average", avg, p, n, *tr._run_table.args(), w)),
         ("cova_weight_average  statistics", nb, lambda: engine.call(
              "cova_weight_average", bavg, tr.bbucket.flat, nb, *tr._stat_table.args(), w)),
         ("cova_adam_step       parameters", n, lambda: engine.call(
              "cova_adam_step", p, g, m, v2, n, 1, 5e-4, 0.9, 0.999, 1e-8, 1e-3)))
out.append("average_rate, launch: the configs[1] trainer's buckets; %d back-to-back calls per window, %d windows after one "
           "warm-up window; us per call" % (args.launches, args.rounds))
for name, numel, fn in calls:
    fn()
    v = windows(fn)
    out.append("  %-32s %8d floats (%5.2f MB)  median %7.2f us  min %7.2f  max %7.2f"
               % (name, numel, 4 * numel / 1e6, np.median(v), v.min(), v.max()))


# ------------------------------------------------------------------------------------------------ the train step
def page_rows(rs, boxes, img_w, img_h):
    wh = np.stack([rs.uniform(8, 400, boxes), rs.uniform(8, 200, boxes)], 1)
    xy = rs.uniform(0, 1, (boxes, 2)) * (np.asarray([img_w, img_h]) - wh)
    lab = np.zeros((boxes, 1))
    lab[rs.permutation(boxes)[:3], 0] = [1, 2, 3]
    return np.concatenate([xy, wh, lab], 1).astype(np.float32)


BATCH, IMG, BOXES = 16, args.img, 90
P = max(BATCH, args.pages // BATCH * BATCH)
rs = np.random.RandomState(0)
gen = torch.Generator(device=dev).manual_seed(0)
u8_dev = torch.empty((P, IMG, IMG, 3), dtype=torch.uint8, device=dev)
for lo in range(0, P, 64):
    u8_dev[lo:lo + 64] = torch.randint(0, 256, (min(64, P - lo), IMG, IMG, 3), dtype=torch.uint8, device=dev, generator=gen)
rows = [page_rows(rs, BOXES, IMG, IMG) for _ in range(P)]
ds = DeviceDataset(u8_dev, rows, CS, dev)


def steps(tr, n_steps, epoch0):
    done, epoch = 0, epoch0
    while done < n_steps:
        for b in ds.batches(BATCH, shuffle=True, sampling_fraction=1.0, seed=1, epoch=epoch):
            tr.train_step(b)
            done += 1
            if done == n_steps:
                break
        epoch += 1


for name in legs:                       # warm-up: every shape and code path of the timed window
    steps(trainers[name], WARMUP, 0)
torch.cuda.synchronize()
ms = {name: [] for name in legs}
for rnd in range(args.rounds):
    for name in legs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps(trainers[name], args.steps, rnd + 1)
        torch.cuda.synchronize()
        ms[name].append(1e3 * (time.perf_counter() - t0) / args.steps)

out.append("average_rate, step: %d pages resident (%.2f GB uint8), batch %d x %dx%d, %d boxes/page (3 labelled), context_size %d, "
           "sampling fraction 1; %d rounds x %d steps, warm-up %d steps; ms per train step"
           % (P, P * IMG * IMG * 3 / 1e9, BATCH, IMG, IMG, BOXES, CS, args.rounds, args.steps, WARMUP))
for name, kw in legs.items():
    v = np.asarray(ms[name])
    out.append("leg %-5s %-44s median %.3f  min %.3f  max %.3f  spread %.3f  [%s]"
               % (name, ", ".join("%s=%r" % kv for kv in kw.items()) or "average=None", np.median(v), v.min(), v.max(),
                  v.max() - v.min(), " ".join("%.3f" % x for x in v)))
base, spread = float(np.median(ms["off"])), float(np.max(ms["off"]) - np.min(ms["off"]))
for a in ("ema", "nobuf"):
    d = float(np.median(ms[a])) - base
    out.append("leg %s - leg off (this run's step with average=None): %+.3f ms/step (%+.2f %% of leg off)" % (a, d, 100 * d / base))
out.append("spread of the repeated leg off: %.3f ms (%.2f %%)" % (spread, 100 * spread / base))
out.append("n_averaged after the run: ema %d, nobuf %d" % (trainers["ema"].n_averaged, trainers["nobuf"].n_averaged))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(out) + "\n")
print("\n".join(out))
