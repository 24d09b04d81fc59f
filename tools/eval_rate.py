"""Time of evaluating a resident split by the way the decisions reach the host, one process, the configs[1] page (1280x1280,
90 boxes a page, context 12): 40 pages at batch 10.  Legs, interleaved and repeated after a warm-up of every shape (the
spread of a repeated leg is the yardstick for a difference):
  a  evaluation.evaluate_split: predict + one cova_eval_page_ranks launch per batch, one device-to-host copy per split
  b  the per-batch route: HotPathTrainer.evaluate (cova_page_class_topk + about twenty torch operators) and the .cpu() of its
     result every batch, which a caller needs to fold the booleans on the host
  c  the floor: HotPathTrainer.predict per batch, one synchronise at the end
  l  leg a with with_loss=True (one more launch per batch: cova_ce_loss_fwd)

    python tools/eval_rate.py [--legs a,b,c,l] [--rounds 7] [--pages 40] [--out profiles/eval_rate.txt]
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
from cova_web_object_detection_amd.evaluation import evaluate_split
from cova_web_object_detection_amd.pipeline import DeviceDataset
from cova_web_object_detection_amd.trainer import HotPathTrainer

ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="a,b,c,l")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--pages", type=int, default=40)
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()
legs = args.legs.split(",")
assert torch.cuda.is_available(), "eval_rate.py measures on the GPU only"
assert args.rounds >= 5

dev = "cuda:0"
CFG = dict(roi_output_size=(3, 3), n_classes=4, use_context=True, hidden_dim=384, bbox_hidden_dim=32,
           n_additional_feat=0, drop_prob=0.2)
BATCH, IMG, BOXES, CS, P = 10, 1280, 90, 12, args.pages
rs = np.random.RandomState(0)
g = torch.Generator(device=dev).manual_seed(0)
u8_dev = torch.randint(0, 256, (P, IMG, IMG, 3), dtype=torch.uint8, device=dev, generator=g)
rows = []
for _p in range(P):
    wh = np.stack([rs.uniform(8, 400, BOXES), rs.uniform(8, 200, BOXES)], 1)
    xy = rs.uniform(0, 1, (BOXES, 2)) * (IMG - wh)
    lab = np.zeros((BOXES, 1))
    lab[rs.permutation(BOXES)[:3], 0] = [1, 2, 3]
    rows.append(np.concatenate([xy, wh, lab], 1).astype(np.float32))
ds = DeviceDataset(u8_dev, rows, CS, dev)
wcfg = {k: v for k, v in CFG.items() if k != "drop_prob"}
tr = HotPathTrainer(CFG, weights.seeded_state_dict(123, **wcfg), dev)


def leg(name):
    if name == "a":
        return evaluate_split(tr, ds, BATCH).hits(1)
    if name == "l":
        return evaluate_split(tr, ds, BATCH, with_loss=True).hits(1)
    if name == "b":
        return np.concatenate([tr.evaluate(b, b["page_start"], k=1)[1].cpu().numpy() for b in ds.batches(BATCH)])
    if name == "c":
        for b in ds.batches(BATCH):
            tr.predict(b)
        torch.cuda.synchronize()
        return None
    raise SystemExit("unknown leg %r" % name)


got = {}
for _ in range(2):                     # warm-up: every shape and code path of the timed window
    for name in legs:
        got[name] = leg(name)
torch.cuda.synchronize()
ms = {name: [] for name in legs}
for rnd in range(args.rounds):
    for name in legs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        leg(name)
        torch.cuda.synchronize()
        ms[name].append(1e3 * (time.perf_counter() - t0))
lines = ["eval_rate: %d pages resident, batch %d x %dx%d, %d boxes/page, context %d; %d rounds, ms per split"
         % (P, BATCH, IMG, IMG, BOXES, CS, args.rounds)]
if "a" in got and "b" in got:
    lines.append("legs a and b take the same %d decisions: %s" % (got["a"].size, bool(np.array_equal(got["a"], got["b"]))))
what = dict(a="evaluate_split", b="trainer.evaluate + .cpu() per batch", c="trainer.predict, one synchronise",
            l="evaluate_split(with_loss=True)")
for name in legs:
    v = np.asarray(ms[name])
    lines.append("leg %s  %-36s median %.3f ms  min %.3f  max %.3f  spread %.3f  [%s]"
                 % (name, what[name], np.median(v), v.min(), v.max(), v.max() - v.min(), " ".join("%.3f" % x for x in v)))
med = {n: float(np.median(ms[n])) for n in legs}
spread = {n: float(np.max(ms[n]) - np.min(ms[n])) for n in legs}
if "a" in med and "b" in med:
    lines.append("leg a - leg b: %+.3f ms per split (%+.2f %%); spread of the repeated leg b: %.3f ms"
                 % (med["a"] - med["b"], 100 * (med["a"] - med["b"]) / med["b"], spread["b"]))
if "a" in med and "c" in med:
    lines.append("leg a - leg c (the floor): %+.3f ms per split (%+.2f %%); spread of the repeated leg c: %.3f ms"
                 % (med["a"] - med["c"], 100 * (med["a"] - med["c"]) / med["c"], spread["c"]))
if "l" in med and "a" in med:
    lines.append("leg l - leg a: %+.3f ms per split" % (med["l"] - med["a"]))
print("\n".join(lines))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
