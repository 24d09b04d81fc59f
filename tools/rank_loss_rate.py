"""What the per-page ranking loss costs, one process (HotPathTrainer(page_rank_weight=), cova_page_rank_loss_fwd / _bwd).

Kernels: the two new entry points alone on random logits (n_classes 4, 3 labelled boxes a page) at 16 pages of 90 boxes
(configs[1]), 16 of 230 (the largest page of the reference's data), 16 of 300 (configs[4]) and 2 of 3000 (a wave loops over
its page), with cova_ce_loss_fwd at the same shape beside them: device events around ``--launches`` back-to-back calls on
one stream, divided by their number (launch overhead that the stream cannot hide is in it; the forward is two launches),
the median of ``--rounds`` such windows after a warm-up window.

Step: the train step at configs[1] (16 pages of 1280x1280, 90 boxes a page) on a DeviceDataset-fed trainer in three legs over
the SAME resident split: "off" (the default step: cova_ce_sum), "pair" (ignore_index=-100 and nothing to ignore: the
cova_ce_loss_fwd / cova_ce_loss_bwd pair that the term needs, without the term) and "on" (page_rank_weight=0.5),
interleaved and repeated (off, pair, on, off, ...): the spread of a repeated leg is the yardstick for a difference.  Times
are a host clock around work that ends in a device synchronise.  No threshold is set.

    python tools/rank_loss_rate.py [--rounds 7] [--steps 40] [--pages 256] [--launches 200] [--out profiles/rank_loss_rate.txt]
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_loss_rate.txt"))
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import cova_amd  # noqa: E402,F401
from cova_web_object_detection_amd import engine, weights  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402

assert torch.cuda.is_available(), "rank_loss_rate.py measures on the GPU only"
dev = "cuda:0"
WARMUP = 6
CS = 6
WEIGHT = 0.5
out = []


# ------------------------------------------------------------------------------------------------ the launch alone
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


NC = 4
out.append("rank_loss_rate, calls: n_classes %d, 3 labelled boxes a page, weight %g; %d back-to-back calls per window, %d "
           "windows after one warm-up window; us per call" % (NC, WEIGHT, args.launches, args.rounds))
tg = torch.Generator(device=dev).manual_seed(1)
for B, n in ((16, 90), (16, 230), (16, 300), (2, 3000)):
    N = B * n
    logits = torch.randn((N, NC), device=dev, generator=tg) * 4
    labels = torch.zeros(N, dtype=torch.int64, device=dev)
    labels.view(B, n)[:, 5:8] = torch.tensor([1, 2, 3], device=dev)
    page_start = torch.arange(B + 1, device=dev) * n
    lists = torch.empty((B, NC - 1, 4), dtype=torch.float64, device=dev)
    acc = torch.empty(3, dtype=torch.float64, device=dev)
    loss, dl = torch.zeros(1, device=dev), torch.zeros((N, NC), device=dev)
    opts = engine.check_loss_options(NC, ignore_index=-100)
    ws = torch.empty(engine.query("cova_ce_loss_workspace_doubles", N), dtype=torch.float64, device=dev)
    rank_fwd = lambda: engine.call("cova_page_rank_loss_fwd", logits, labels, page_start, B, N, NC, None, -100, 1, lists,  # noqa: E731
                                   acc)
    rank_bwd = lambda: engine.call("cova_page_rank_loss_bwd", logits, labels, page_start, B, N, NC, None, -100, 1, lists,  # noqa: E731
                                   acc, WEIGHT, 0, None, loss, dl, 0)
    fwd = lambda: engine.ce_loss_fwd(logits, labels, None, opts, workspace=ws)  # noqa: E731
    rank_fwd()
    scored = int(acc[2].item())
    for name, fn in (("cova_page_rank_loss_fwd", rank_fwd), ("cova_page_rank_loss_bwd", rank_bwd), ("cova_ce_loss_fwd", fwd)):
        v = windows(fn)
        out.append("  %2d pages x %4d boxes  %-26s median %7.2f us  min %7.2f  max %7.2f%s"
                   % (B, n, name, np.median(v), v.min(), v.max(),
                      "  (%d scored lists)" % scored if fn is rank_fwd else ""))


# ------------------------------------------------------------------------------------------------ the train step
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

legs = {"off": dict(), "pair": dict(ignore_index=-100), "on": dict(page_rank_weight=WEIGHT)}
sd = weights.seeded_state_dict(123, **{k: v for k, v in CFG.items() if k != "drop_prob"})
trainers = {name: HotPathTrainer(CFG, sd, dev, **kw) for name, kw in legs.items()}


def steps(tr, n, epoch0):
    done, epoch = 0, epoch0
    while done < n:
        for b in ds.batches(BATCH, shuffle=True, sampling_fraction=1.0, seed=1, epoch=epoch):
            tr.train_step(b)
            done += 1
            if done == n:
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

out.append("rank_loss_rate, step: %d pages resident (%.2f GB uint8), batch %d x %dx%d, %d boxes/page (3 labelled), context_size %d, "
           "sampling fraction 1; %d rounds x %d steps, warm-up %d steps; ms per train step"
           % (P, P * IMG * IMG * 3 / 1e9, BATCH, IMG, IMG, BOXES, CS, args.rounds, args.steps, WARMUP))
for name, kw in legs.items():
    v = np.asarray(ms[name])
    out.append("leg %-4s %-52s median %.3f  min %.3f  max %.3f  spread %.3f  [%s]"
               % (name, ", ".join("%s=%r" % kv for kv in kw.items()) or "default", np.median(v), v.min(), v.max(),
                  v.max() - v.min(), " ".join("%.3f" % x for x in v)))
base, spread = float(np.median(ms["off"])), float(np.max(ms["off"]) - np.min(ms["off"]))
for a, b in (("on", "off"), ("pair", "off"), ("on", "pair")):
    d = float(np.median(ms[a])) - float(np.median(ms[b]))
    out.append("leg %s - leg %s: %+.3f ms/step (%+.2f %% of leg off)" % (a, b, d, 100 * d / base))
out.append("spread of the repeated leg off: %.3f ms (%.2f %%)" % (spread, 100 * spread / base))
c = trainers["on"].last_rank_acc.cpu()
out.append("last step of leg on: %d scored lists, rank term R %.4f" % (int(c[2]), float(c[0])))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(out) + "\n")
print("\n".join(out))
