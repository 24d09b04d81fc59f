"""What joint page decoding costs, one process (cova_page_joint_decode, evaluate_split(decode="joint")).

Kernel: the new entry point alone (labels, hit and gap tables given, score_mode 1) on random logits whose class columns share
an objectness term, so that columns do compete for boxes, at 16 pages of 90 boxes with n_classes 4 (configs[1]), 16 of 300
with n_classes 4 (configs[4]) and 16 of 90 with n_classes 7 (7^6 rank tuples a page: the largest enumeration the entry
point takes), with cova_eval_page_ranks at the same shape beside it in the same windows: device events around ``--launches``
back-to-back calls on one stream, divided by their number (launch overhead that the stream cannot hide is in it), the
median of ``--rounds`` such windows after a warm-up window.

Split: ``evaluate_split`` over a resident split at configs[1] (batches of 16 pages of 1280x1280, 90 boxes a page) in two legs
over the SAME split and trainer, "column" (the default) and "joint" (one more launch per batch, the tables in the same
buffer and copy), interleaved and repeated (column, joint, column, ...): the spread of the repeated column leg is the
yardstick for the difference; the first round is a warm-up and is not counted.  Times are a host clock around a call that
ends in its device-to-host copy.  No threshold is set.

    python tools/joint_decode_rate.py [--rounds 7] [--pages 128] [--launches 200] [--out profiles/joint_decode_rate.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--pages", type=int, default=128, help="pages of the resident split (a multiple of 16)")
ap.add_argument("--launches", type=int, default=200, help="back-to-back kernel launches per timed window")
ap.add_argument("--img", type=int, default=1280, help="page side of the split legs (configs[1]: 1280)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_decode_rate.txt"))
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import cova_amd  # noqa: E402,F401
from cova_web_object_detection_amd import engine, weights  # noqa: E402
from cova_web_object_detection_amd.evaluation import evaluate_split  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402

assert torch.cuda.is_available(), "joint_decode_rate.py measures on the GPU only"
dev = "cuda:0"
CS = 6
out = []


# ------------------------------------------------------------------------------------------------ the launch alone
def windows(fns):
    """us per call of every function, timed in the same rounds one after the other."""
    v = {name: [] for name in fns}
    for rnd in range(args.rounds + 1):                                  # round 0 is the warm-up
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                v[name].append(1e3 * e0.elapsed_time(e1) / args.launches)
    return {name: np.asarray(x) for name, x in v.items()}


out.append("joint_decode_rate, calls: score_mode 1, labels / hit / gap given, one labelled box per class and page; %d "
           "back-to-back calls per window, %d windows after one warm-up window; us per call" % (args.launches, args.rounds))
tg = torch.Generator(device=dev).manual_seed(1)
for B, n, NC in ((16, 90, 4), (16, 300, 4), (16, 90, 7)):
    N = B * n
    logits = torch.randn((N, NC), device=dev, generator=tg)
    logits[:, 1:] += 2 * torch.randn((N, 1), device=dev, generator=tg)
    labels = torch.zeros(N, dtype=torch.int64, device=dev)
    labels.view(B, n)[:, 5:5 + NC - 1] = torch.arange(1, NC, device=dev)
    page_start = torch.arange(B + 1, device=dev) * n
    tabs = torch.full((4, B, NC - 1), -2, dtype=torch.int32, device=dev)
    gap = torch.full((B,), -1.0, dtype=torch.float64, device=dev)
    fns = {
        "cova_page_joint_decode": lambda: engine.call("cova_page_joint_decode", logits, labels, page_start, None, B, NC, B,
                                                      1, tabs[2], tabs[3], gap),
        "cova_eval_page_ranks": lambda: engine.call("cova_eval_page_ranks", logits, labels, page_start, None, B, NC, B,
                                                    tabs[0], tabs[1]),
    }
    v = windows(fns)
    apart = int((tabs[1] != tabs[2]).any(dim=1).sum().item())
    for name, x in v.items():
        out.append("  %2d pages x %4d boxes, n_classes %d  %-24s median %8.2f us  min %8.2f  max %8.2f%s"
                   % (B, n, NC, name, np.median(x), x.min(), x.max(),
                      "  (joint != column on %d pages)" % apart if name == "cova_page_joint_decode" else ""))


# ------------------------------------------------------------------------------------------------ the split
def page_rows(rs, boxes, img_w, img_h):
    wh = np.stack([rs.uniform(8, 400, boxes), rs.uniform(8, 200, boxes)], 1)
    xy = rs.uniform(0, 1, (boxes, 2)) * (np.asarray([img_w, img_h]) - wh)
    lab = np.zeros((boxes, 1))
    lab[rs.permutation(boxes)[:3], 0] = [1, 2, 3]
    return np.concatenate([xy, wh, lab], 1).astype(np.float32)


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
ds = DeviceDataset(u8_dev, rows, CS, dev)
tr = HotPathTrainer(CFG, weights.seeded_state_dict(123, **{k: v for k, v in CFG.items() if k != "drop_prob"}), dev)

legs = {"column": dict(), "joint": dict(decode="joint")}
reports = {name: evaluate_split(tr, ds, batch_size=BATCH, **kw) for name, kw in legs.items()}       # warm-up
torch.cuda.synchronize()
ms = {name: [] for name in legs}
for rnd in range(args.rounds + 1):                                      # round 0 is the warm-up, as for the launches
    for name, kw in legs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        evaluate_split(tr, ds, batch_size=BATCH, **kw)
        if rnd:
            ms[name].append(1e3 * (time.perf_counter() - t0))

out.append("joint_decode_rate, split: %d pages resident (%.2f GB uint8), batches of %d x %dx%d, %d boxes/page (3 labelled), "
           "context_size %d; %d rounds after one warm-up round; ms per evaluate_split"
           % (P, P * IMG * IMG * 3 / 1e9, BATCH, IMG, IMG, BOXES, CS, args.rounds))
for name, kw in legs.items():
    v = np.asarray(ms[name])
    out.append("leg %-6s %-16s median %.3f  min %.3f  max %.3f  spread %.3f  [%s]"
               % (name, ", ".join("%s=%r" % kv for kv in kw.items()) or "default", np.median(v), v.min(), v.max(),
                  v.max() - v.min(), " ".join("%.3f" % x for x in v)))
base, spread = float(np.median(ms["column"])), float(np.max(ms["column"]) - np.min(ms["column"]))
d = float(np.median(ms["joint"])) - base
out.append("leg joint - leg column: %+.3f ms per split (%+.2f %% of leg column), %+.1f us per batch"
           % (d, 100 * d / base, 1e3 * d / (P // BATCH)))
out.append("spread of the repeated leg column: %.3f ms (%.2f %%): the difference lies %s it"
           % (spread, 100 * spread / base, "inside" if abs(d) <= spread else "OUTSIDE"))
rep = reports["joint"]
same = np.array_equal(rep.ranks, reports["column"].ranks) and np.array_equal(rep.top1, reports["column"].top1)
out.append("joint leg: ranks / top1 equal the column leg's: %s; joint != column on %d of %d pages; class accuracy column %s, "
           "joint %s" % (same, int((rep.joint_top1 != rep.top1).any(axis=1).sum()), P,
                         " ".join("%.2f" % a for a in rep.class_acc(1)[1:]),
                         " ".join("%.2f" % a for a in rep.class_acc(1, "joint")[1:])))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(out) + "\n")
print("\n".join(out))
