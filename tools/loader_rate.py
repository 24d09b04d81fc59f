"""Train-step rate by the way the batch reaches the step, one process, the configs[1] shape (16 pages of 1280x1280, 90 boxes a
page, context 12).  Legs, interleaved and repeated (the spread of a repeated leg is the yardstick for a difference):
  a  one fixed device-resident batch (what bench.py times)
  b  host-fed: pipeline.Prefetcher over four pre-stacked, pre-pinned uint8 batches (tools/pcie_inclusive.py)
  c  pipeline.DeviceDataset, shuffle, sampling_fraction 1 (page gather + sampling + collate launches, no host read)
  d  the same with sampling_fraction 0.9 (one 4-byte host read per batch on the side stream; fewer boxes per step)
  e  leg d without the side stream (prefetch=False): the host read then waits for the previous step
  f  leg c without the side stream
  k  no train step (not a rate; for a kernel trace): cova_images_u8_to_f32 of 16 pages and cova_pages_u8_gather_f32 of 16
     shuffled pages in turn, then DeviceDataset batches (sf 0.9, prefetch=False) alone on the device

    python tools/loader_rate.py [--legs a,b,c,d,e,f] [--rounds 7] [--steps 40] [--pages 1024]

An epoch of the resident split is pages / 16 steps (64 at the default; fold 1 of the reference's data has 283): the per-epoch
work -- one index-table upload, a new side stream -- is amortised as it is in a training run.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import cova_amd  # noqa
from cova_web_object_detection_amd import weights
from cova_web_object_detection_amd._lib import call
from cova_web_object_detection_amd.pipeline import DeviceCollate, DeviceDataset, Prefetcher
from cova_web_object_detection_amd.trainer import HotPathTrainer

ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="a,b,c,d,e,f")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--pages", type=int, default=1024, help="pages of the resident split (a multiple of 16)")
args = ap.parse_args()
legs = args.legs.split(",")
assert torch.cuda.is_available(), "loader_rate.py measures on the GPU only"

dev = "cuda:0"
CFG = dict(roi_output_size=(3, 3), n_classes=4, use_context=True, hidden_dim=384, bbox_hidden_dim=32,
           n_additional_feat=0, drop_prob=0.2)
BATCH, IMG, BOXES, CS = 16, 1280, 90, 12
P = max(BATCH, args.pages // BATCH * BATCH)
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
host_batches = [(u8_dev[i * BATCH:(i + 1) * BATCH].cpu().pin_memory(), rows[i * BATCH:(i + 1) * BATCH])
                for i in range(min(4, P // BATCH))]
fixed = DeviceCollate(CS, dev)(u8_dev[:BATCH], rows[:BATCH])
wcfg = {k: v for k, v in CFG.items() if k != "drop_prob"}
tr = HotPathTrainer(CFG, weights.seeded_state_dict(123, **wcfg), dev)


def dataset_steps(n, sf, prefetch, epoch0):
    done, epoch = 0, epoch0
    while done < n:
        for b in ds.batches(BATCH, shuffle=True, sampling_fraction=sf, seed=1, epoch=epoch, prefetch=prefetch):
            tr.train_step(b)
            done += 1
            if done == n:
                break
        epoch += 1


def host_source(n):
    for i in range(n):
        yield host_batches[i % len(host_batches)]


def leg(name, n, rnd):
    if name == "a":
        for _ in range(n):
            tr.train_step(fixed)
    elif name == "b":
        for b in Prefetcher(DeviceCollate(CS, dev, pin=True), host_source(n)):
            tr.train_step(b)
    elif name == "c":
        dataset_steps(n, 1.0, True, 100 * rnd)
    elif name == "d":
        dataset_steps(n, 0.9, True, 100 * rnd)
    elif name == "e":
        dataset_steps(n, 0.9, False, 100 * rnd)
    elif name == "f":
        dataset_steps(n, 1.0, False, 100 * rnd)
    elif name == "k":
        out = torch.empty((BATCH, 3, IMG, IMG), dtype=torch.float32, device=dev)
        for i in range(n):
            idx = torch.from_numpy(np.random.RandomState(i).permutation(P)[:BATCH].astype(np.int32)).to(dev)
            call("cova_images_u8_to_f32", u8_dev[:BATCH], out, BATCH, IMG, IMG)
            call("cova_pages_u8_gather_f32", u8_dev, idx, P, BATCH, IMG, IMG, out)
        for i, b in enumerate(ds.batches(BATCH, shuffle=True, sampling_fraction=0.9, seed=1, epoch=rnd, prefetch=False)):
            if i + 1 == n:
                break
    else:
        raise SystemExit("unknown leg %r" % name)


for name in legs:                      # warm-up: every shape and code path of the timed window
    leg(name, 6, 0)
torch.cuda.synchronize()
ms = {name: [] for name in legs}
for rnd in range(args.rounds):
    for name in legs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        leg(name, args.steps, rnd + 1)
        torch.cuda.synchronize()
        ms[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
print("loader_rate: %d pages resident (%.2f GB uint8), batch %d x %dx%d, %d boxes/page, context %d; %d rounds x %d steps"
      % (P, P * IMG * IMG * 3 / 1e9, BATCH, IMG, IMG, BOXES, CS, args.rounds, args.steps))
what = dict(a="fixed device-resident batch", b="host-fed Prefetcher (4 pinned batches)",
            c="DeviceDataset shuffle sf=1", d="DeviceDataset shuffle sf=0.9", e="DeviceDataset sf=0.9, prefetch=False",
            f="DeviceDataset sf=1, prefetch=False")
for name in legs:
    v = np.asarray(ms[name])
    print("leg %s  %-40s median %.3f ms/step  min %.3f  max %.3f  spread %.3f  [%s]"
          % (name, what[name], np.median(v), v.min(), v.max(), v.max() - v.min(), " ".join("%.3f" % x for x in v)))
if "a" in ms:
    base, spread = float(np.median(ms["a"])), float(np.max(ms["a"]) - np.min(ms["a"]))
    for name in legs:
        if name != "a":
            d = float(np.median(ms[name])) - base
            print("leg %s - leg a: %+.3f ms/step (%+.2f %%); spread of the repeated leg a: %.3f ms"
                  % (name, d, 100 * d / base, spread))
