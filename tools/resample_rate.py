"""What page zoom costs, one process (pipeline.PageAugment(scale=), cova_pages_u8_resample_f32, cova_boxes_affine).

Kernel: 16 pages of 1280x1280 gathered out of a resident uint8 store.  The yardstick is cova_pages_u8_augment_f32 with every
page shifted by dx = 37 (dx % 4 = 1, dy = -20), untouched by the zoom and timed in the same windows; beside it
cova_pages_u8_resample_f32 at inv = 131072, 65536, 47836 and 32768 (zoom 0.5, 1, 1.37, 2) about the page's top centre, all with
the same random colour table.  By compulsory bytes a launch at zoom s moves (3/s^2 + 12)/15 of the shift launch's bytes (the
source pixels under the output, once, plus the whole output; never below the output's 12/15); the second source row is
expected from cache.  The allowance is 1.5 times that ratio times the shift launch's median.  Device events around
``--launches`` back-to-back launches on one stream, divided by their number; the legs are interleaved (shift, the four steps,
shift, ...) and the median of ``--rounds`` such windows after a warm-up round is reported.

Step: the train step at configs[1] (16 pages of 1280x1280, 90 boxes a page) on a DeviceDataset-fed trainer over the SAME
resident split in three legs with every other magnitude equal: "off" (scale (1, 1): the shift kernel), "on" (scale
(0.6, 1.8): one cova_pages_u8_resample_f32 and one cova_boxes_affine launch per step) and "off2" (off again), interleaved and
repeated.  Times are a host clock around work that ends in a device synchronise.  No threshold is set.

    python tools/resample_rate.py [--rounds 7] [--steps 40] [--pages 256] [--launches 50] [--out profiles/resample_rate.txt]
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_rate.txt"))
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import cova_amd  # noqa: E402,F401
from cova_web_object_detection_amd import engine, weights  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset, PageAugment  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402

assert torch.cuda.is_available(), "resample_rate.py measures on the GPU only"
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
shift_d = torch.tensor([[37, -20]] * BATCH, dtype=torch.int32, device=dev)
SHIFT = "cova_pages_u8_augment_f32  dx%4=1"
legs = {SHIFT: lambda: engine.call("cova_pages_u8_augment_f32", u8_dev, idx, P, BATCH, IMG, IMG, shift_d, color_d, 0xFFFFFF,
                                   images)}
INVS = (131072, 65536, 47836, 32768)
ratio = {}
for inv in INVS:
    org_x = (IMG - 1) * 32768 + ((1 - IMG - 2 * 37) * inv) // 2           # the loader's origin for (dx, dy) = (37, -20)
    org_y = -32768 + ((1 + 2 * 20) * inv) // 2
    step_d = torch.tensor([[inv, inv]] * BATCH, dtype=torch.int32, device=dev)
    origin_d = torch.tensor([[org_x, org_y]] * BATCH, dtype=torch.int64, device=dev)
    name = "cova_pages_u8_resample_f32 inv=%-6d" % inv
    ratio[name] = (3.0 * (inv / 65536.0) ** 2 + 12.0) / 15.0
    legs[name] = (lambda s=step_d, o=origin_d: engine.call("cova_pages_u8_resample_f32", u8_dev, idx, P, BATCH, IMG, IMG, s, o,
                                                           color_d, 0xFFFFFF, images))
us = {name: [] for name in legs}
for rnd in range(args.rounds + 1):                                      # round 0 is the warm-up
    for name, fn in legs.items():
        v = window(fn)
        if rnd:
            us[name].append(v)
nbytes = BATCH * IMG * IMG * (3 + 12)
out.append("resample_rate, launch: %d pages of %dx%d out of a %d-page store (the shift launch reads + writes %.1f MB), colour "
           "table, (dx, dy) = (37, -20); %d back-to-back launches per window, %d interleaved rounds after one warm-up round; us "
           "per launch; GB/s over the compulsory bytes of the leg" % (BATCH, IMG, IMG, P, nbytes / 1e6, args.launches, args.rounds))
base = np.asarray(us[SHIFT])
for name, v in us.items():
    v = np.asarray(v)
    r = ratio.get(name, 1.0)
    line = "  %-40s median %8.2f us  min %8.2f  max %8.2f  %6.0f GB/s" % (name, np.median(v), v.min(), v.max(),
                                                                          r * nbytes / np.median(v) / 1e3)
    if name in ratio:
        allow = 1.5 * r * np.median(base)
        line += "  byte ratio %.3f  allowance %8.2f us  %s" % (r, allow, "inside" if np.median(v) <= allow else "ABOVE")
    out.append(line)
out.append("  spread of the repeated shift leg: %.2f us (%.2f %%)"
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
MAGS = dict(max_shift=(64, 128), brightness=0.2, contrast=0.3, saturation=0.3, channel_gain=0.1, invert_prob=0.2, seed=1)
step_legs = {"off": PageAugment(**MAGS), "on": PageAugment(scale=(0.6, 1.8), **MAGS), "off2": PageAugment(**MAGS)}
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

out.append("resample_rate, step: %d pages resident (%.2f GB uint8), batch %d x %dx%d, %d boxes/page (3 labelled), context_size %d, "
           "sampling fraction 1, max_shift=(64,128) and every colour magnitude non-zero in all legs; %d rounds x %d steps, "
           "warm-up %d steps; ms per train step" % (P, P * IMG * IMG * 3 / 1e9, BATCH, IMG, IMG, BOXES, CS, args.rounds, args.steps,
                                                    WARMUP))
for name in step_legs:
    v = np.asarray(ms[name])
    out.append("leg %-4s %-22s median %.3f  min %.3f  max %.3f  spread %.3f  [%s]"
               % (name, "scale=%r" % (step_legs[name].scale,), np.median(v), v.min(), v.max(), v.max() - v.min(),
                  " ".join("%.3f" % x for x in v)))
off = np.concatenate([ms["off"], ms["off2"]])
base_ms, spread = float(np.median(off)), float(off.max() - off.min())
d = float(np.median(ms["on"])) - base_ms
out.append("leg on - legs off: %+.3f ms/step (%+.2f %% of the off legs' median %.3f)" % (d, 100 * d / base_ms, base_ms))
out.append("off2 - off (the same work twice): %+.3f ms/step; spread of all off windows: %.3f ms (%.2f %%)"
           % (float(np.median(ms["off2"]) - np.median(ms["off"])), spread, 100 * spread / base_ms))
launch_us = float(np.median(us["cova_pages_u8_resample_f32 inv=%-6d" % 65536]))
out.append("the zoom launch at inv=65536 is %.2f %% of the off step" % (100 * launch_us / 1e3 / base_ms))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(out) + "\n")
print("\n".join(out))
