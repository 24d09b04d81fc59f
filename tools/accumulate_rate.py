"""What gradient accumulation costs, one process (HotPathTrainer(accumulate_steps=), cova_grad_accumulate).

Launch: the four modes of cova_grad_accumulate over the configs[1] trainer's gradient bucket (1.6 M floats, one table
row), with cova_weight_average over the same table beside them: device events around ``--launches`` back-to-back launches
on one stream, divided by their number (launch overhead that the stream cannot hide is in it).  The five calls take turns
inside every round, so each round times all of them under the same conditions; the figure is the median of ``--rounds``
such windows per call after a warm-up round.  The acceptance figure is relative: each mode at most 1.25 x
cova_weight_average of this same process (both move the same bytes per element; the margin is for the multiply and the
other read / write mix of a kernel that is launch-latency bound at this size).  It is reported, not asserted.

Step: the train step at configs[1] (16 pages of 1280x1280, 90 boxes a page) on DeviceDataset-fed trainers over the SAME
resident split in two legs, "n1" (accumulate_steps=1) and "n4" (accumulate_steps=4: three micro-steps with one
accumulate launch, a fourth with one and the update), interleaved and repeated (n1, n4, n1, ...).  ms per micro-step
against leg "n1" of this same run; the spread of the repeated leg "n1" is the yardstick for a difference.  Times are a
host clock around work that ends in a device synchronise.

    python tools/accumulate_rate.py [--rounds 7] [--steps 40] [--pages 256] [--launches 200] [--out profiles/accumulate_rate.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=40, help="micro-steps per timed window (a multiple of 4)")
ap.add_argument("--pages", type=int, default=256, help="pages of the resident split (a multiple of 16)")
ap.add_argument("--launches", type=int, default=200, help="back-to-back kernel launches per timed window")
ap.add_argument("--img", type=int, default=1280, help="page side of the step legs (configs[1]: 1280)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accumulate_rate.txt"))
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import cova_amd  # noqa: E402,F401
from cova_web_object_detection_amd import engine, weights  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import ACC_ADD, ACC_ADD_CLOSE, ACC_CLOSE, ACC_OPEN, HotPathTrainer  # noqa: E402

assert torch.cuda.is_available(), "accumulate_rate.py measures on the GPU only"
dev = "cuda:0"
WARMUP = 8
CS = 6
LIMIT = 1.25
out = []

CFG = dict(roi_output_size=(3, 3), n_classes=4, use_context=True, hidden_dim=384, bbox_hidden_dim=32,
           n_additional_feat=0, drop_prob=0.2)
legs = {"n1": dict(accumulate_steps=1), "n4": dict(accumulate_steps=4)}
sd = weights.seeded_state_dict(123, **{k: v for k, v in CFG.items() if k != "drop_prob"})
trainers = {name: HotPathTrainer(CFG, sd, dev, **kw) for name, kw in legs.items()}


# ------------------------------------------------------------------------------------------------ the launches alone
def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / args.launches


tr = trainers["n4"]
n, (seg, n_seg, total) = tr.gbucket.flat.numel(), tr._run_table.args()
g0 = torch.randn(n, device=dev) * 1e-3
g = g0.clone()
acc, avg, p = torch.zeros(n, device=dev), tr.pbucket.flat.clone(), tr.pbucket.flat.clone()


def accumulate(mode, scale):
    return lambda: engine.call("cova_grad_accumulate", mode, acc, g, n, seg, n_seg, total, 0, n, scale)


# (every window starts from the same gradient and a zero accumulator)
calls = (("cova_weight_average", lambda: engine.call("cova_weight_average", avg, p, n, seg, n_seg, total, 1e-3)),
         ("cova_grad_accumulate open", accumulate(ACC_OPEN, 1.0)),
         ("cova_grad_accumulate add", accumulate(ACC_ADD, 1.0)),
         ("cova_grad_accumulate close", accumulate(ACC_CLOSE, 1.0)),
         ("cova_grad_accumulate add-close", accumulate(ACC_ADD_CLOSE, 1.0)))
us = {name: [] for name, _ in calls}
for rnd in range(args.rounds + 1):                                      # round 0 is the warm-up
    for name, fn in calls:
        acc.zero_()
        g.copy_(g0)
        v = window(fn)
        if rnd:
            us[name].append(v)
out.append("accumulate_rate, launch: the configs[1] trainer's gradient bucket, %d floats (%.2f MB), %d table row(s); %d "
           "back-to-back calls per window, the five calls in turn in each of %d rounds after one warm-up round; us per call"
           % (n, 4 * n / 1e6, n_seg, args.launches, args.rounds))
base = float(np.median(us["cova_weight_average"]))
for name, _ in calls:
    v = np.asarray(us[name])
    ratio = float(np.median(v)) / base
    verdict = "" if name == "cova_weight_average" else \
        "  %.2f x cova_weight_average (limit %.2f: %s)" % (ratio, LIMIT, "met" if ratio <= LIMIT else "MISSED")
    out.append("  %-32s median %7.2f us  min %7.2f  max %7.2f%s" % (name, np.median(v), v.min(), v.max(), verdict))


# ------------------------------------------------------------------------------------------------ the train step
def page_rows(rs, boxes, img_w, img_h):
    wh = np.stack([rs.uniform(8, 400, boxes), rs.uniform(8, 200, boxes)], 1)
    xy = rs.uniform(0, 1, (boxes, 2)) * (np.asarray([img_w, img_h]) - wh)
    lab = np.zeros((boxes, 1))
    lab[rs.permutation(boxes)[:3], 0] = [1, 2, 3]
    return np.concatenate([xy, wh, lab], 1).astype(np.float32)


BATCH, IMG, BOXES = 16, args.img, 90
P = max(BATCH, args.pages // BATCH * BATCH)
STEPS = max(4, args.steps // 4 * 4)                                    # whole cycles: no leg ends with work pending
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


for name in legs:                       # warm-up: every shape and code path of the timed window, two whole cycles
    steps(trainers[name], WARMUP, 0)
torch.cuda.synchronize()
ms = {name: [] for name in legs}
for rnd in range(args.rounds):
    for name in legs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps(trainers[name], STEPS, rnd + 1)
        torch.cuda.synchronize()
        ms[name].append(1e3 * (time.perf_counter() - t0) / STEPS)

out.append("accumulate_rate, step: %d pages resident (%.2f GB uint8), batch %d x %dx%d, %d boxes/page (3 labelled), context_size %d, "
           "sampling fraction 1; %d rounds x %d micro-steps, warm-up %d; ms per micro-step"
           % (P, P * IMG * IMG * 3 / 1e9, BATCH, IMG, IMG, BOXES, CS, args.rounds, STEPS, WARMUP))
for name, kw in legs.items():
    v = np.asarray(ms[name])
    out.append("leg %-3s %-20s median %.3f  min %.3f  max %.3f  spread %.3f  [%s]"
               % (name, ", ".join("%s=%r" % kv for kv in kw.items()), np.median(v), v.min(), v.max(), v.max() - v.min(),
                  " ".join("%.3f" % x for x in v)))
base, spread = float(np.median(ms["n1"])), float(np.max(ms["n1"]) - np.min(ms["n1"]))
d = float(np.median(ms["n4"])) - base
out.append("leg n4 - leg n1 (this run's step with accumulate_steps=1): %+.3f ms/micro-step (%+.2f %% of leg n1); leg n4 makes "
           "one update per four micro-steps, leg n1 one per step" % (d, 100 * d / base))
out.append("spread of the repeated leg n1: %.3f ms (%.2f %%)" % (spread, 100 * spread / base))
out.append("after the run: n1 %d steps = %d updates; n4 %d micro-steps, %d updates, %d pending"
           % (trainers["n1"].step_count, trainers["n1"].update_count, trainers["n4"].step_count,
              trainers["n4"].update_count, trainers["n4"].accumulated))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(out) + "\n")
print("\n".join(out))
