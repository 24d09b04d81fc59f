"""What the attention dropout costs, one process (CoVA(attention_dropout=p); cova_gat_fwd_drop / cova_gat_bwd_drop,
cova_gat2_fwd_drop / cova_gat2_bwd_drop).

Kernels: the forward + backward pair with dropout at p = 0.5 beside the pair without it, on the same operands, for both
scoring modes, at the head shape of configs[1] (16 pages x 90 boxes = 1440 nodes, hybrid table context_size 6 + spatial_k
12 = K 24, D = 384) and of configs[4] (K = 48 = context_size 12 + spatial_k 24, one of two heads of D = 192): device events
around ``--launches`` back-to-back launches on one stream, divided by their number (launch overhead that the stream cannot
hide is in it), the median of ``--rounds`` such windows after a warm-up window.  The _drop kernels hash every slot once per
kernel (three 64-bit multiplies) and skip nothing: the forward still loads the rows of dropped slots.

Step: the train step at configs[1] (16 pages of 1280x1280, 90 boxes a page, the hybrid graph) without the option and with
attention_dropout = 0.5, two trainers over the SAME resident split, legs interleaved and repeated (off, on, off, on, ...):
the spread of a repeated leg is the yardstick for a difference.  Times are a host clock around work that ends in a device
synchronise.  No threshold is set: the yardstick is the existing kernels in the same run.

    python tools/attn_dropout_rate.py [--rounds 7] [--steps 40] [--pages 256] [--launches 200] [--out profiles/attn_dropout_rate.txt]
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_dropout_rate.txt"))
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import cova_amd  # noqa: E402,F401
from cova_web_object_detection_amd import engine, weights  # noqa: E402
from cova_web_object_detection_amd._lib import call, query  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402

assert torch.cuda.is_available(), "attn_dropout_rate.py measures on the GPU only"
dev = "cuda:0"
WARMUP = 6
RATE = 0.5
SEED = engine.attention_dropout_seed(engine.dropout_base(123, 1), 0, 0)
out = []


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


def kernel_legs(what, cs, ks, D):
    ctx = next(iter(DeviceDataset(u8_dev[:BATCH], rows[:BATCH], cs, dev, spatial_k=ks).batches(BATCH, prefetch=False)))[
        "context_indices"]
    N, K = ctx.shape
    tg = torch.Generator(device=dev).manual_seed(1)
    rnd_ = lambda *shape: torch.randn(shape, device=dev, generator=tg)
    Wh, aw, ab, gr = rnd_(N, 2 * D), rnd_(2 * D) / D ** 0.5, rnd_(1), rnd_(N, D)
    aw2 = aw[:D].clone()
    new = lambda *shape: torch.empty(shape, device=dev)
    s, t, attn, hp = new(N), new(N), new(N, K), new(N, D)
    dWh, dsv, dtv, daw, dab, du = new(N, 2 * D), new(N), new(N), new(2 * D), new(1), new(N, K)
    ws = new(query("cova_gat2_workspace_floats", N, K, D))
    csr = torch.zeros((query("cova_gat_transpose_ints", N, K),), dtype=torch.int32, device=dev)
    call("cova_gat_transpose", ctx, N, K, csr)

    def static_pair():
        call("cova_gat_fwd", Wh, 2 * D, aw, ab, ctx, N, K, D, 0.2, s, t, attn, hp, D)
        call("cova_gat_bwd", gr, D, Wh, 2 * D, s, t, attn, ctx, aw, N, K, D, 0.2, dWh, 2 * D, dsv, dtv, daw, dab, csr, du)

    def static_drop_pair():
        call("cova_gat_fwd_drop", Wh, 2 * D, aw, ab, ctx, None, None, N, K, D, 0.2, RATE, SEED, s, t, attn, hp, D)
        call("cova_gat_bwd_drop", gr, D, Wh, 2 * D, s, t, attn, ctx, aw, None, None, N, K, D, 0.2, RATE, SEED, dWh, 2 * D, dsv,
             dtv, daw, dab, None, csr, du, None)

    def v2_pair():
        call("cova_gat2_fwd", Wh, 2 * D, aw2, ab, ctx, None, None, N, K, D, 0.2, attn, hp, D)
        call("cova_gat2_bwd", gr, D, Wh, 2 * D, attn, ctx, aw2, None, None, N, K, D, 0.2, dWh, 2 * D, daw, dab, None, csr, du, ws)

    def v2_drop_pair():
        call("cova_gat2_fwd_drop", Wh, 2 * D, aw2, ab, ctx, None, None, N, K, D, 0.2, RATE, SEED, attn, hp, D)
        call("cova_gat2_bwd_drop", gr, D, Wh, 2 * D, attn, ctx, aw2, None, None, N, K, D, 0.2, RATE, SEED, dWh, 2 * D, daw, dab,
             None, csr, du, ws)

    out.append("attn_dropout_rate, launches at %s: N %d, K %d (context_size %d + spatial_k %d), D %d, p %.1f; %d back-to-back "
               "forward + backward pairs per window, %d windows after one warm-up window; us per pair (5 kernels static, 4 GATv2)"
               % (what, N, K, cs, ks, D, RATE, args.launches, args.rounds))
    med = {}
    for name, fn in (("gat", static_pair), ("gat + dropout", static_drop_pair), ("gatv2", v2_pair),
                     ("gatv2 + dropout", v2_drop_pair)):
        v = windows(fn)
        med[name] = float(np.median(v))
        out.append("  %-16s median %7.2f us  min %7.2f  max %7.2f" % (name, np.median(v), v.min(), v.max()))
    out.append("  with dropout / without: gat %.3f, gatv2 %.3f"
               % (med["gat + dropout"] / med["gat"], med["gatv2 + dropout"] / med["gatv2"]))


kernel_legs("configs[1]'s head", 6, 12, 384)
kernel_legs("configs[4]'s head (one of two)", 12, 24, 192)

# ------------------------------------------------------------------------------------------------ the train step
CS, KS = 6, 12
ds = DeviceDataset(u8_dev, rows, CS, dev, spatial_k=KS)
legs = ["off", "on"]
trainers = {}
sd = weights.seeded_state_dict(123, **{k: v for k, v in CFG.items() if k != "drop_prob"})
for name in legs:
    trainers[name] = HotPathTrainer(dict(CFG, attention_dropout=RATE) if name == "on" else CFG, sd, dev)


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

out.append("attn_dropout_rate, step: %d pages resident (%.2f GB uint8), batch %d x %dx%d, %d boxes/page, hybrid graph "
           "(context_size %d, spatial_k %d), sampling fraction 1; %d rounds x %d steps, warm-up %d steps; ms per train step"
           % (P, P * IMG * IMG * 3 / 1e9, BATCH, IMG, IMG, BOXES, CS, KS, args.rounds, args.steps, WARMUP))
for name in legs:
    v = np.asarray(ms[name])
    out.append("leg attention_dropout %-3s median %.3f  min %.3f  max %.3f  spread %.3f  [%s]"
               % (name, np.median(v), v.min(), v.max(), v.max() - v.min(), " ".join("%.3f" % x for x in v)))
base, spread = float(np.median(ms["off"])), float(np.max(ms["off"]) - np.min(ms["off"]))
d = float(np.median(ms["on"])) - base
out.append("leg on - leg off: %+.3f ms/step (%+.2f %%); spread of the repeated leg off: %.3f ms" % (d, 100 * d / base, spread))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(out) + "\n")
print("\n".join(out))
