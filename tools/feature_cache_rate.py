"""Head-only training and evaluation with cached RoI features (features.FeatureCache) against the recomputing path, one
process, the configs[1] shape (16 pages of 1280x1280, 90 boxes a page, context 12), a frozen backbone
(frozen=("convnet.",), bn_eval=("convnet.",)).  Legs, interleaved and repeated (the spread of a repeated leg is the yardstick
for a difference):
  a  frozen-backbone train steps fed by pipeline.DeviceDataset (shuffle, sampling_fraction 0.9), as today
  b  the same steps with batches(features=cache): no page gather, conv stack or RoI op; one row gather
  c  FeatureCache.build over the resident split, per page
  d  evaluation.evaluate_split(features=cache) over the split, per page
  e  evaluation.evaluate_split without the cache, per page
Times are a host clock around work that ends in a device synchronise.  The gate is median(b) <= 0.5 * median(a).

    python tools/feature_cache_rate.py [--legs a,b,c,d,e] [--rounds 7] [--steps 40] [--pages 256] [--cache PATH]
                                       [--out profiles/feature_cache_rate.txt]

``--cache PATH`` loads the cache from PATH when it exists (else builds and saves it there): a kernel trace of leg b alone,

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/feature_cache_rate.py --legs b --rounds 1 --steps 400 \\
        --cache PATH --out DIR/leg_b.txt

then holds no conv-stack launch.  ``--trace-stats DIR --trace-steps N --out FILE`` (no GPU needed) sums the kernel
durations of that trace's ``*kernel_stats.csv`` over N steps and appends the GPU-busy time per step of leg b to FILE.
"""
import argparse
import csv
import glob
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="a,b,c,d,e")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--pages", type=int, default=256, help="pages of the resident split (a multiple of 16, at least 64)")
ap.add_argument("--cache", default=None, help="load the feature cache from this file if it exists, else build and save it")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_cache_rate.txt"))
ap.add_argument("--trace-stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of leg b")
ap.add_argument("--trace-steps", type=int, default=0, help="train steps inside that trace (warm-up included)")
args = ap.parse_args()
WARMUP = 6


def summarise_trace():
    files = sorted(glob.glob(os.path.join(args.trace_stats, "**", "*kernel_stats.csv"), recursive=True))
    if not files or args.trace_steps < 1:
        raise SystemExit("no *kernel_stats.csv under %s, or --trace-steps missing" % args.trace_stats)
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += list(csv.DictReader(fh))
    for r in rows:                         # (column names by prefix: Name, Calls, TotalDurationNs, ...)
        for want in ("Name", "Calls", "TotalDurationNs"):
            if want not in r:
                r[want] = r[[k for k in r if k.lower().startswith(want.lower()[:9])][0]]
    total_ns = sum(float(r["TotalDurationNs"]) for r in rows)
    rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
    lines = ["", "leg b under rocprofv3 --kernel-trace --stats (a run of its own, cache loaded from a file): %d steps, "
             "%d kernel names" % (args.trace_steps, len(rows)),
             "GPU-busy time of leg b: %.3f ms/step (sum of all kernel durations of the process / steps; the one-off fill "
             "of the resident pages is in it)" % (total_ns / 1e6 / args.trace_steps),
             "launches per step: %.1f" % (sum(int(r["Calls"]) for r in rows) / args.trace_steps)]
    conv = [r["Name"] for r in rows if any(s in r["Name"] for s in ("conv", "roipool", "roialign", "maxpool", "u8"))]
    lines.append("conv-stack / RoI / page-gather kernels in the trace: %s" % (", ".join(conv) if conv else "none"))
    for r in rows[:12]:
        lines.append("  %8.2f us/step  %6.1f calls/step  %s" % (float(r["TotalDurationNs"]) / 1e3 / args.trace_steps,
                                                                int(r["Calls"]) / args.trace_steps, r["Name"][:110]))
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if args.trace_stats:
    summarise_trace()
    raise SystemExit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import cova_amd  # noqa: E402,F401
from cova_web_object_detection_amd import weights  # noqa: E402
from cova_web_object_detection_amd.evaluation import evaluate_split  # noqa: E402
from cova_web_object_detection_amd.features import FeatureCache  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402

legs = args.legs.split(",")
assert torch.cuda.is_available(), "feature_cache_rate.py measures on the GPU only"

dev = "cuda:0"
CFG = dict(roi_output_size=(3, 3), n_classes=4, use_context=True, hidden_dim=384, bbox_hidden_dim=32,
           n_additional_feat=0, drop_prob=0.2)
BATCH, IMG, BOXES, CS, SF = 16, 1280, 90, 12, 0.9
P = max(64, args.pages // BATCH * BATCH)
rs = np.random.RandomState(0)
g = torch.Generator(device=dev).manual_seed(0)
u8_dev = torch.empty((P, IMG, IMG, 3), dtype=torch.uint8, device=dev)
for lo in range(0, P, 64):
    u8_dev[lo:lo + 64] = torch.randint(0, 256, (min(64, P - lo), IMG, IMG, 3), dtype=torch.uint8, device=dev, generator=g)
rows = []
for _p in range(P):
    wh = np.stack([rs.uniform(8, 400, BOXES), rs.uniform(8, 200, BOXES)], 1)
    xy = rs.uniform(0, 1, (BOXES, 2)) * (IMG - wh)
    lab = np.zeros((BOXES, 1))
    lab[rs.permutation(BOXES)[:3], 0] = [1, 2, 3]
    rows.append(np.concatenate([xy, wh, lab], 1).astype(np.float32))
ds = DeviceDataset(u8_dev, rows, CS, dev)
wcfg = {k: v for k, v in CFG.items() if k != "drop_prob"}
tr = HotPathTrainer(CFG, weights.seeded_state_dict(123, **wcfg), dev, frozen=("convnet.",), bn_eval=("convnet.",))

if args.cache and os.path.exists(args.cache):
    cache = FeatureCache.load(args.cache, dev)
else:
    cache = FeatureCache.build(tr, ds, batch_size=BATCH)
    if args.cache:
        cache.save(args.cache)
cache.check(tr, ds)


def train_steps(n, features, epoch0):
    done, epoch = 0, epoch0
    while done < n:
        for b in ds.batches(BATCH, shuffle=True, sampling_fraction=SF, seed=1, epoch=epoch, features=features):
            tr.train_step(b)
            done += 1
            if done == n:
                break
        epoch += 1


def leg(name, n, rnd):
    """-> the number of units (steps or pages) the leg's time is divided by"""
    if name == "a":
        train_steps(n, None, 100 * rnd)
        return n
    if name == "b":
        train_steps(n, cache, 100 * rnd)
        return n
    if name == "c":
        FeatureCache.build(tr, ds, batch_size=BATCH)
        return P
    if name == "d":
        for _ in range(4):
            evaluate_split(tr, ds, batch_size=BATCH, features=cache)
        return 4 * P
    if name == "e":
        evaluate_split(tr, ds, batch_size=BATCH)
        return P
    raise SystemExit("unknown leg %r" % name)


for name in legs:                      # warm-up: every shape and code path of the timed window
    leg(name, WARMUP, 0)
torch.cuda.synchronize()
ms = {name: [] for name in legs}
for rnd in range(args.rounds):
    for name in legs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        units = leg(name, args.steps, rnd + 1)
        torch.cuda.synchronize()
        ms[name].append(1e3 * (time.perf_counter() - t0) / units)

what = dict(a=("frozen steps, DeviceDataset (recomputed)", "ms/step"), b=("frozen steps, batches(features=cache)", "ms/step"),
            c=("FeatureCache.build", "ms/page"), d=("evaluate_split(features=cache)", "ms/page"),
            e=("evaluate_split (recomputed)", "ms/page"))
out = ["feature_cache_rate: %d pages resident (%.2f GB uint8), batch %d x %dx%d, %d boxes/page, context %d, sampling "
       "fraction %.1f; table %d rows x %d = %.1f MB; %d rounds x %d steps (legs a, b), warm-up %d steps"
       % (P, P * IMG * IMG * 3 / 1e9, BATCH, IMG, IMG, BOXES, CS, SF, len(cache), cache.n_vis, cache.nbytes / 1e6,
          args.rounds, args.steps, WARMUP)]
for name in legs:
    v = np.asarray(ms[name])
    out.append("leg %s  %-42s median %.4f %s  min %.4f  max %.4f  spread %.4f  [%s]"
               % (name, what[name][0], np.median(v), what[name][1], v.min(), v.max(), v.max() - v.min(),
                  " ".join("%.4f" % x for x in v)))
if "a" in ms and "b" in ms:
    ma, mb = float(np.median(ms["a"])), float(np.median(ms["b"]))
    out.append("gate: median(b) <= 0.5 * median(a): %.4f <= %.4f  %s  (b / a = %.3f)"
               % (mb, 0.5 * ma, "PASS" if mb <= 0.5 * ma else "FAIL", mb / ma))
if "d" in ms and "e" in ms:
    out.append("evaluate_split: cached / recomputed = %.3f" % (float(np.median(ms["d"])) / float(np.median(ms["e"]))))
out.append("train steps in this process (for a kernel trace of it): %d"
           % sum((WARMUP + args.rounds * args.steps) for name in legs if name in "ab"))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(out) + "\n")
print("\n".join(out))
