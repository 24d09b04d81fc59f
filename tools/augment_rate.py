"""What page augmentation costs, one process (pipeline.PageAugment, cova_pages_u8_augment_f32, cova_boxes_translate).

Kernel: 16 pages of 1280x1280 gathered out of a resident uint8 store.  The yardstick is the plain gather
(cova_pages_u8_gather_f32); beside it cova_pages_u8_augment_f32 with every page shifted by dx = 36 + r, r = dx % 4 in 0..3
(dy = -20), once without a colour table (NULL: the identity) and once with a random one.  All legs move the same bytes
(3 in, 12 out per pixel).  Device events around ``--launches`` back-to-back launches on one stream, divided by their number;
the legs are interleaved (gather, r = 0 .. 3 without, r = 0 .. 3 with, gather, ...) and the median of ``--rounds`` such windows
after a warm-up round is reported; the spread of the repeated gather leg is the yardstick for a difference.

Step: the train step at configs[1] (16 pages of 1280x1280, 90 boxes a page) on a DeviceDataset-fed trainer in two legs over the
SAME resident split: "off" (augment=None: the gather, as before) and "on" (every magnitude non-zero: one
cova_pages_u8_augment_f32 and one cova_boxes_translate launch per step), interleaved and repeated.  Times are a host clock
around work that ends in a device synchronise.  No threshold is set.

    python tools/augment_rate.py [--rounds 7] [--steps 40] [--pages 256] [--launches 50] [--out profiles/augment_rate.txt]
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
ap.add_argument("--launches", type=int, default=50, help="back-to-back kernel launches per timed window")
ap.add_argument("--img", type=int, default=1280, help="page side (configs[1]: 1280)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_rate.txt"))
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import cova_amd  # noqa: E402,F401
from cova_web_object_detection_amd import engine, weights  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset, PageAugment  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402

assert torch.cuda.is_available(), "augment_rate.py measures on the GPU only"
dev = "cuda:0"
WARMUP = 6
CS = 6
BATCH, IMG, BOXES = 16, args.img, 90
P = max(BATCH, args.pages // BATCH * BATCH)
out = []

rs = np.random.RandomState(0)
g = torch.Generator(device=dev).manual_seed(0)
u8_dev = torch.empty((P, IMG, IMG, 3), dtype=torch.uint8, device=dev)
for lo in range(0, P, 64):
    u8_dev[lo:lo + 64] = torch.randint(0, 256, (min(64, P - lo), IMG, IMG, 3), dtype=torch.uint8, device=dev, generator=g)


# ------------------------------------------------------------------------------------------------ the launch alone
def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / args.launches


idx = torch.from_numpy(rs.permutation(P)[:BATCH].astype(np.int32)).to(dev)
images = torch.empty((BATCH, 3, IMG, IMG), dtype=torch.float32, device=dev)
color = rs.uniform(-2, 2, (BATCH, 12)).astype(np.float32)
color[:, 3::4] = rs.uniform(-1, 1, (BATCH, 3))
color_d = torch.from_numpy(color).to(dev)
legs = {"cova_pages_u8_gather_f32": lambda: engine.call("cova_pages_u8_gather_f32", u8_dev, idx, P, BATCH, IMG, IMG, images)}
for table in (None, color_d):
    for r in range(4):
        shift_d = torch.tensor([[36 + r, -20]] * BATCH, dtype=torch.int32, device=dev)
        legs["cova_pages_u8_augment_f32 dx%%4=%d %s" % (r, "no colour table" if table is None else "colour table   ")] = \
            (lambda s=shift_d, t=table: engine.call("cova_pages_u8_augment_f32", u8_dev, idx, P, BATCH, IMG, IMG, s, t,
                                                    0xFFFFFF, images))
us = {name: [] for name in legs}
for rnd in range(args.rounds + 1):                                      # round 0 is the warm-up
    for name, fn in legs.items():
        v = window(fn)
        if rnd:
            us[name].append(v)
nbytes = BATCH * IMG * IMG * (3 + 12)
out.append("augment_rate, launch: %d pages of %dx%d out of a %d-page store (%.1f MB read + written per launch), dy = -20; %d "
           "back-to-back launches per window, %d interleaved rounds after one warm-up round; us per launch"
           % (BATCH, IMG, IMG, P, nbytes / 1e6, args.launches, args.rounds))
base = np.asarray(us["cova_pages_u8_gather_f32"])
for name, v in us.items():
    v = np.asarray(v)
    out.append("  %-56s median %8.2f us  min %8.2f  max %8.2f  %6.0f GB/s  %+6.2f %% of the gather"
               % (name, np.median(v), v.min(), v.max(), nbytes / np.median(v) / 1e3,
                  100 * (np.median(v) - np.median(base)) / np.median(base)))
out.append("  spread of the repeated gather leg: %.2f us (%.2f %%)"
           % (base.max() - base.min(), 100 * (base.max() - base.min()) / np.median(base)))


# ------------------------------------------------------------------------------------------------ the train step
def page_rows(boxes, img_w, img_h):
    wh = np.stack([rs.uniform(8, 400, boxes), rs.uniform(8, 200, boxes)], 1)
    xy = rs.uniform(0, 1, (boxes, 2)) * (np.asarray([img_w, img_h]) - wh)
    lab = np.zeros((boxes, 1))
    lab[rs.permutation(boxes)[:3], 0] = [1, 2, 3]
    return np.concatenate([xy, wh, lab], 1).astype(np.float32)


CFG = dict(roi_output_size=(3, 3), n_classes=4, use_context=True, hidden_dim=384, bbox_hidden_dim=32,
           n_additional_feat=0, drop_prob=0.2)
ds = DeviceDataset(u8_dev, [page_rows(BOXES, IMG, IMG) for _ in range(P)], CS, dev)
AUG = PageAugment(max_shift=(64, 128), brightness=0.2, contrast=0.3, saturation=0.3, channel_gain=0.1, invert_prob=0.2, seed=1)
step_legs = {"off": None, "on": AUG}
sd = weights.seeded_state_dict(123, **{k: v for k, v in CFG.items() if k != "drop_prob"})
trainers = {name: HotPathTrainer(CFG, sd, dev) for name in step_legs}


def steps(name, n, epoch0):
    done, epoch = 0, epoch0
    while done < n:
        for b in ds.batches(BATCH, shuffle=True, sampling_fraction=1.0, seed=1, epoch=epoch, augment=step_legs[name]):
            trainers[name].train_step(b)
            done += 1
            if done == n:
                break
        epoch += 1


for name in step_legs:                  # warm-up: every shape and code path of the timed window
    steps(name, WARMUP, 0)
torch.cuda.synchronize()
ms = {name: [] for name in step_legs}
for rnd in range(args.rounds):
    for name in step_legs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps(name, args.steps, rnd + 1)
        torch.cuda.synchronize()
        ms[name].append(1e3 * (time.perf_counter() - t0) / args.steps)

out.append("augment_rate, step: %d pages resident (%.2f GB uint8), batch %d x %dx%d, %d boxes/page (3 labelled), context_size %d, "
           "sampling fraction 1; %d rounds x %d steps, warm-up %d steps; ms per train step"
           % (P, P * IMG * IMG * 3 / 1e9, BATCH, IMG, IMG, BOXES, CS, args.rounds, args.steps, WARMUP))
for name in step_legs:
    v = np.asarray(ms[name])
    out.append("leg %-3s %-44s median %.3f  min %.3f  max %.3f  spread %.3f  [%s]"
               % (name, "augment=None" if step_legs[name] is None else "max_shift=(64,128), every magnitude non-zero",
                  np.median(v), v.min(), v.max(), v.max() - v.min(), " ".join("%.3f" % x for x in v)))
base_ms, spread = float(np.median(ms["off"])), float(np.max(ms["off"]) - np.min(ms["off"]))
d = float(np.median(ms["on"])) - base_ms
out.append("leg on - leg off: %+.3f ms/step (%+.2f %% of leg off)" % (d, 100 * d / base_ms))
out.append("spread of the repeated leg off: %.3f ms (%.2f %%)" % (spread, 100 * spread / base_ms))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(out) + "\n")
print("\n".join(out))
