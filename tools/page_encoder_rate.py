"""What the page encoder costs, one process (CoVA(page_encoder_dim=P, ...), engine.page_encoder_fwd / page_encoder_bwd:
cova_layernorm_fwd / _bwd, cova_gelu_fwd / _bwd, cova_page_attn_fwd / _bwd, cova_sgemm, cova_colsum).

Chain: the forward + backward chain of the layer on given own features at the configs[1] head shape (16 pages x 90 boxes =
1440 rows, F = 608) and at 32 pages x 300 boxes (9600 rows), P = 128, M = 256, Hh = 4, L = 1 and L = 2.  Two figures per chain:
  * kernel time: a device-event pair around EVERY C-ABI call of the chain (_lib.PROFILE), summed by entry point, the median
    over ``--rounds`` repetitions after a warm-up; the events' own cost is in every figure, the two device copies and the two
    fills of a layer (torch) are not;
  * window time: device events around ``--launches`` back-to-back chains, divided by their number: what the stream sees,
    with whatever launch overhead the host cannot hide behind these 5 to 30 us kernels.
L = 2 minus L = 1 is the cost of one more layer (the input projection, the final LayerNorm and dh are in both).  Beside
them, in the same windows: the plain page-attention pair (cova_page_attn_fwd + cova_page_attn_bwd at E = 128, Hh = 4) alone.

Step: the train step at configs[1] (16 pages of 1280x1280, 90 boxes a page, the hybrid graph) with page_encoder_dim 0 and 128
(Hh = 4, L = 1, M = 256), two trainers over the SAME resident split, legs interleaved and repeated (0, 128, 0, 128, ...): the
spread of the repeated leg is the yardstick for a difference.  Times are a host clock around work that ends in a device
synchronise.  No threshold is set.

    python tools/page_encoder_rate.py [--rounds 7] [--steps 40] [--pages 256] [--launches 50] [--out FILE]
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
ap.add_argument("--launches", type=int, default=50, help="back-to-back chains per timed window")
ap.add_argument("--img", type=int, default=1280, help="page side of the step legs (configs[1]: 1280)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "page_encoder_rate.txt"))
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import cova_amd  # noqa: E402,F401
from cova_web_object_detection_amd import _lib, engine, weights  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402

assert torch.cuda.is_available(), "page_encoder_rate.py measures on the GPU only"
dev = "cuda:0"
WARMUP = 6
F, P, M, HEADS = 608, 128, 256, 4
out = []


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n


def by_entry_point(fn):
    """us per entry point of one run of ``fn``: the device-event pairs _lib.PROFILE puts around every call."""
    _lib.PROFILE = {n: [] for n in _lib.lib().fn}
    try:
        fn()
        torch.cuda.synchronize()
        return {n: sum(1e3 * a.elapsed_time(b) for a, b, _, _ in v) for n, v in _lib.PROFILE.items() if v}
    finally:
        _lib.PROFILE = None


def chain_legs(what, B, boxes):
    N = B * boxes
    tg = torch.Generator(device=dev).manual_seed(1)
    h, g = torch.randn((N, F), device=dev, generator=tg), torch.randn((N, P), device=dev, generator=tg)
    ps = torch.arange(B + 1, dtype=torch.int64, device=dev) * boxes
    enc_out, dh = torch.empty((N, P), device=dev), torch.zeros((N, F), device=dev)
    out.append("page_encoder_rate, chain at %s: %d pages x %d boxes = %d rows, F = %d, P = %d, M = %d, Hh = %d; us per forward + "
               "backward chain, median [min, max] of %d repetitions (kernel time) and of %d windows of %d chains (window time)"
               % (what, B, boxes, N, F, P, M, HEADS, args.rounds, args.rounds, args.launches))
    med = {}
    for L in (1, 2):
        sd = weights.seeded_state_dict(3, roi_output_size=(3, 3), bbox_hidden_dim=32, page_encoder_dim=P, page_encoder_heads=HEADS,
                                       page_encoder_layers=L, page_encoder_ffn_dim=M)
        params = {k: v.to(dev) for k, v in sd.items() if k.startswith("page_encoder.")}

        def chain():
            sv = engine.page_encoder_fwd(h, F, N, F, ps, params, HEADS, L, enc_out, P)
            engine.page_encoder_bwd(sv, g, P, params, dh, F)
        chain()
        by_entry_point(chain)                                            # warm-up of both measurements
        reps = [by_entry_point(chain) for _ in range(args.rounds)]
        tot = np.asarray([sum(r.values()) for r in reps])
        win = np.asarray([window(chain, args.launches) for _ in range(args.rounds + 1)][1:])
        med[L] = (float(np.median(tot)), float(np.median(win)))
        out.append("  L = %d: kernel time %8.1f [%8.1f, %8.1f]   window time %8.1f [%8.1f, %8.1f]   (%d C-ABI calls)"
                   % (L, np.median(tot), tot.min(), tot.max(), np.median(win), win.min(), win.max(),
                      n_calls(chain)))
        for name in sorted(reps[0]):
            out.append("      %-22s %8.1f" % (name, np.median([r[name] for r in reps])))
    out.append("  one more layer (L = 2 minus L = 1): kernel time %.1f us, window time %.1f us" % (med[2][0] - med[1][0], med[2][1] - med[1][1]))
    # the plain page-attention pair alone, same process, same windows
    qkv = torch.randn((N, 3 * P), device=dev, generator=tg)
    o, lse, dqkv = torch.empty((N, P), device=dev), torch.empty((N, HEADS), device=dev), torch.empty((N, 3 * P), device=dev)

    def pair():
        engine.call("cova_page_attn_fwd", qkv, 3 * P, ps, B, N, P, HEADS, o, P, lse)
        engine.call("cova_page_attn_bwd", g, P, qkv, 3 * P, o, P, lse, ps, B, N, P, HEADS, dqkv, 3 * P)
    pair()
    by_entry_point(pair)
    reps = np.asarray([sum(by_entry_point(pair).values()) for _ in range(args.rounds)])
    win = np.asarray([window(pair, 4 * args.launches) for _ in range(args.rounds + 1)][1:])
    out.append("  plain page-attention pair (E = %d): kernel time %8.1f [%8.1f, %8.1f]   window time %8.1f [%8.1f, %8.1f]; one more "
               "encoder layer / the pair: %.2f (kernel time), %.2f (window time)"
               % (P, np.median(reps), reps.min(), reps.max(), np.median(win), win.min(), win.max(),
                  (med[2][0] - med[1][0]) / np.median(reps), (med[2][1] - med[1][1]) / np.median(win)))


def n_calls(fn):
    _lib.PROFILE = {n: [] for n in _lib.lib().fn}
    try:
        fn()
        torch.cuda.synchronize()
        return sum(len(v) for v in _lib.PROFILE.values())
    finally:
        _lib.PROFILE = None


chain_legs("configs[1]'s head", 16, 90)
chain_legs("32 pages x 300 boxes", 32, 300)


# ------------------------------------------------------------------------------------------------ the train step
def page_rows(rs, boxes, img_w, img_h):
    wh = np.stack([rs.uniform(8, 400, boxes), rs.uniform(8, 200, boxes)], 1)
    xy = rs.uniform(0, 1, (boxes, 2)) * (np.asarray([img_w, img_h]) - wh)
    lab = np.zeros((boxes, 1))
    lab[rs.permutation(boxes)[:3], 0] = [1, 2, 3]
    return np.concatenate([xy, wh, lab], 1).astype(np.float32)


CFG = dict(roi_output_size=(3, 3), n_classes=4, use_context=True, hidden_dim=384, bbox_hidden_dim=32,
           n_additional_feat=0, drop_prob=0.2)
BATCH, IMG, BOXES, CS, KS = 16, args.img, 90, 6, 12
NP = max(BATCH, args.pages // BATCH * BATCH)
rs = np.random.RandomState(0)
gen = torch.Generator(device=dev).manual_seed(0)
u8_dev = torch.empty((NP, IMG, IMG, 3), dtype=torch.uint8, device=dev)
for lo in range(0, NP, 64):
    u8_dev[lo:lo + 64] = torch.randint(0, 256, (min(64, NP - lo), IMG, IMG, 3), dtype=torch.uint8, device=dev, generator=gen)
ds = DeviceDataset(u8_dev, [page_rows(rs, BOXES, IMG, IMG) for _ in range(NP)], CS, dev, spatial_k=KS)
legs = [0, P]                                                        # the first leg is the yardstick
trainers = {}
for E in legs:
    cfg = dict(CFG, page_encoder_dim=E, page_encoder_heads=HEADS, page_encoder_layers=1, page_encoder_ffn_dim=M if E else None)
    sd = weights.seeded_state_dict(123, **{k: v for k, v in cfg.items() if k != "drop_prob"})
    trainers[E] = HotPathTrainer(cfg, sd, dev)


def steps(tr, n, epoch0):
    done, epoch = 0, epoch0
    while done < n:
        for b in ds.batches(BATCH, shuffle=True, sampling_fraction=1.0, seed=1, epoch=epoch):
            tr.train_step(b)
            done += 1
            if done == n:
                break
        epoch += 1


for E in legs:                          # warm-up: every shape and code path of the timed window
    steps(trainers[E], WARMUP, 0)
torch.cuda.synchronize()
ms = {E: [] for E in legs}
for rnd in range(args.rounds):
    for E in legs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps(trainers[E], args.steps, rnd + 1)
        torch.cuda.synchronize()
        ms[E].append(1e3 * (time.perf_counter() - t0) / args.steps)

out.append("page_encoder_rate, step: %d pages resident (%.2f GB uint8), batch %d x %dx%d, %d boxes/page, hybrid graph "
           "(context_size %d, spatial_k %d), sampling fraction 1; %d rounds x %d steps, warm-up %d steps; ms per train step"
           % (NP, NP * IMG * IMG * 3 / 1e9, BATCH, IMG, IMG, BOXES, CS, KS, args.rounds, args.steps, WARMUP))
for E in legs:
    v = np.asarray(ms[E])
    out.append("leg page_encoder_dim=%-3d median %.3f  min %.3f  max %.3f  spread %.3f  [%s]"
               % (E, np.median(v), v.min(), v.max(), v.max() - v.min(), " ".join("%.3f" % x for x in v)))
base, spread = float(np.median(ms[legs[0]])), float(np.max(ms[legs[0]]) - np.min(ms[legs[0]]))
d = float(np.median(ms[legs[1]])) - base
out.append("leg %d - leg %d: %+.3f ms/step (%+.2f %%); spread of the repeated leg %d: %.3f ms%s"
           % (legs[1], legs[0], d, 100 * d / base, legs[0], spread,
              " -- the difference is inside that spread" if abs(d) <= spread else ""))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(out) + "\n")
print("\n".join(out))
