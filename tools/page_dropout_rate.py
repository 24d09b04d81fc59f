"""What dropout in the page layers costs, one process, at p = 0.1 (CoVA(page_attention_dropout=, page_encoder_dropout=),
DESIGN.md section 39: cova_page_attn_fwd_drop / _bwd_drop and their _geo_ forms, cova_gelu_fwd_drop / _bwd_drop,
cova_dropout_add_fwd, cova_dropout_regen_bwd).

Pairs: the plain, DROP, GEO and GEO + DROP attention pairs (forward + backward, E = 128, Hh = 4) on the same qkv at the
configs[1] head shape (16 pages x 90 boxes) and at 32 pages x 300 boxes.  Two figures per pair:
  * kernel time: a device-event pair around both C-ABI calls (_lib.PROFILE), summed, the median over ``--rounds`` repetitions
    after a warm-up; the events' own cost is in every figure;
  * window time: device events around ``--launches`` back-to-back pairs, divided by their number.
The ratios DROP / plain and GEO / plain come from the same run: the hash against the geometry features on the same loops.
Rows: the four row kernels on [1440, 256] (and [9600, 256]) against cova_gelu_fwd / cova_gelu_bwd, both figures per launch.
Layer: one encoder layer (F = 608, P = 128, M = 256, Hh = 4, L = 1), forward + backward chain, with and without dropout.
Step: the train step at configs[1] (16 pages of 1280x1280, 90 boxes a page, the hybrid graph) with page_encoder_dim = 128,
L = 1, page_encoder_dropout 0 and 0.1, two trainers over the SAME resident split, legs interleaved and repeated: the spread of
the repeated leg is the yardstick for a difference.  Times are a host clock around work that ends in a device synchronise.
No threshold is set.

    python tools/page_dropout_rate.py [--rounds 7] [--steps 40] [--pages 256] [--launches 50] [--out FILE]
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "page_dropout_rate.txt"))
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import cova_amd  # noqa: E402,F401
from cova_web_object_detection_amd import _lib, engine, weights  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402

assert torch.cuda.is_available(), "page_dropout_rate.py measures on the GPU only"
dev = "cuda:0"
WARMUP = 6
F, P, M, HEADS, RATE = 608, 128, 256, 4, 0.1
SEED = engine.page_dropout_seed(engine.dropout_base(123, 1), 0, 0)
PAGE_W = PAGE_H = 1280.0
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


def measured(fn, launches):
    """-> (kernel-time samples, window-time samples) of ``fn`` after a warm-up of both measurements"""
    fn()
    by_entry_point(fn)
    reps = np.asarray([sum(by_entry_point(fn).values()) for _ in range(args.rounds)])
    win = np.asarray([window(fn, launches) for _ in range(args.rounds + 1)][1:])
    return reps, win


def fmt(v):
    return "%8.1f [%8.1f, %8.1f]" % (np.median(v), v.min(), v.max())


def random_boxes(gen, B, boxes):
    wh = torch.rand((B * boxes, 2), device=dev, generator=gen) * 300 + 8
    xy = torch.rand((B * boxes, 2), device=dev, generator=gen) * (PAGE_W - 308)
    page = torch.arange(B, device=dev, dtype=torch.float32).repeat_interleave(boxes).view(-1, 1)
    return torch.cat((page, xy, xy + wh), dim=1).contiguous()


def legs_at(what, B, boxes):
    N = B * boxes
    tg = torch.Generator(device=dev).manual_seed(1)
    g, qkv = torch.randn((N, P), device=dev, generator=tg), torch.randn((N, 3 * P), device=dev, generator=tg)
    ps = torch.arange(B + 1, dtype=torch.int64, device=dev) * boxes
    bb, gw = random_boxes(tg, B, boxes), torch.randn((HEADS, 8), device=dev, generator=tg)
    o, lse, dqkv = torch.empty((N, P), device=dev), torch.empty((N, HEADS), device=dev), torch.empty((N, 3 * P), device=dev)
    dgw = torch.empty((HEADS, 8), device=dev)
    ws = torch.empty((engine.query("cova_page_attn_geo_workspace_floats", B, N, HEADS),), device=dev)
    out.append("page_dropout_rate, attention pairs at %s: %d pages x %d boxes = %d rows, E = %d, Hh = %d, p = %.1f; us per forward "
               "+ backward pair, median [min, max] of %d repetitions (kernel time) and of %d windows of %d pairs (window time)"
               % (what, B, boxes, N, P, HEADS, RATE, args.rounds, args.rounds, 4 * args.launches))

    def pair(geo, drop):
        tail = (RATE, SEED) if drop else ()
        stem = "_geo" if geo else ""
        stem += "_drop" if drop else ""
        if geo:
            def fn():
                engine.call("cova_page_attn_fwd" + stem, qkv, 3 * P, ps, bb, gw, PAGE_W, PAGE_H, B, N, P, HEADS, o, P, lse, *tail)
                engine.call("cova_page_attn_bwd" + stem, g, P, qkv, 3 * P, o, P, lse, ps, bb, gw, PAGE_W, PAGE_H, B, N, P, HEADS,
                            dqkv, 3 * P, dgw, ws, *tail)
        else:
            def fn():
                engine.call("cova_page_attn_fwd" + stem, qkv, 3 * P, ps, B, N, P, HEADS, o, P, lse, *tail)
                engine.call("cova_page_attn_bwd" + stem, g, P, qkv, 3 * P, o, P, lse, ps, B, N, P, HEADS, dqkv, 3 * P, *tail)
        return fn
    med = {}
    for geo in (False, True):
        for drop in (False, True):
            name = ("GEO" if geo else "plain") + (" + DROP" if drop and geo else " DROP" if drop else "")
            name = "DROP" if name == "plain DROP" else name
            reps, win = measured(pair(geo, drop), 4 * args.launches)
            med[(geo, drop)] = (float(np.median(reps)), float(np.median(win)))
            out.append("  %-11s kernel time %s   window time %s" % (name, fmt(reps), fmt(win)))
    for i, kind in enumerate(("kernel time", "window time")):
        pl = med[(False, False)][i]
        out.append("  %s: DROP / plain %.2f, GEO / plain %.2f, GEO + DROP / GEO %.2f, GEO + DROP / plain %.2f"
                   % (kind, med[(False, True)][i] / pl, med[(True, False)][i] / pl, med[(True, True)][i] / med[(True, False)][i],
                      med[(True, True)][i] / pl))
    # the row kernels, [N, M] operands
    z, gz = torch.randn((N, M), device=dev, generator=tg), torch.randn((N, M), device=dev, generator=tg)
    f, x = torch.empty((N, M), device=dev), torch.randn((N, M), device=dev, generator=tg)
    rows = {"cova_gelu_fwd": lambda: engine.call("cova_gelu_fwd", z, M, N, M, f, M),
            "cova_gelu_fwd_drop": lambda: engine.call("cova_gelu_fwd_drop", z, M, N, M, f, M, RATE, SEED),
            "cova_gelu_bwd": lambda: engine.call("cova_gelu_bwd", gz, M, z, M, N, M, f, M),
            "cova_gelu_bwd_drop": lambda: engine.call("cova_gelu_bwd_drop", gz, M, z, M, N, M, f, M, RATE, SEED),
            "cova_dropout_add_fwd": lambda: engine.call("cova_dropout_add_fwd", z, M, x, M, f, M, N, M, RATE, SEED),
            "cova_dropout_regen_bwd": lambda: engine.call("cova_dropout_regen_bwd", gz, M, f, M, N, M, RATE, SEED)}
    out.append("  row kernels on [%d, %d]: us per launch, kernel time and window time (%d launches a window)"
               % (N, M, 4 * args.launches))
    rmed = {}
    for name, fn in rows.items():
        reps, win = measured(fn, 4 * args.launches)
        rmed[name] = (float(np.median(reps)), float(np.median(win)))
        out.append("      %-24s kernel time %s   window time %s" % (name, fmt(reps), fmt(win)))
    out.append("      kernel time against the plain GELU of the same direction: gelu_fwd_drop %.2f, dropout_add_fwd %.2f (forward); "
               "gelu_bwd_drop %.2f, dropout_regen_bwd %.2f (backward)"
               % (rmed["cova_gelu_fwd_drop"][0] / rmed["cova_gelu_fwd"][0], rmed["cova_dropout_add_fwd"][0] / rmed["cova_gelu_fwd"][0],
                  rmed["cova_gelu_bwd_drop"][0] / rmed["cova_gelu_bwd"][0], rmed["cova_dropout_regen_bwd"][0] / rmed["cova_gelu_bwd"][0]))
    # one encoder layer with and without dropout
    h = torch.randn((N, F), device=dev, generator=tg)
    enc_out, dh = torch.empty((N, P), device=dev), torch.zeros((N, F), device=dev)
    sd = weights.seeded_state_dict(3, roi_output_size=(3, 3), bbox_hidden_dim=32, page_encoder_dim=P, page_encoder_heads=HEADS,
                                   page_encoder_layers=1, page_encoder_ffn_dim=M)
    params = {k: v.to(dev) for k, v in sd.items() if k.startswith("page_encoder.")}
    lmed = {}
    for rate in (0.0, RATE):
        def chain():
            sv = engine.page_encoder_fwd(h, F, N, F, ps, params, HEADS, 1, enc_out, P, dropout=rate,
                                         seed_base=engine.dropout_base(123, 1), training=True)
            engine.page_encoder_bwd(sv, g, P, params, dh, F)
        reps, win = measured(chain, args.launches)
        lmed[rate] = (float(np.median(reps)), float(np.median(win)))
        out.append("  one encoder layer (F = %d, P = %d, M = %d, L = 1), dropout %.1f: kernel time %s   window time %s"
                   % (F, P, M, rate, fmt(reps), fmt(win)))
    out.append("  dropout %.1f / dropout 0: %.2f (kernel time), %.2f (window time)"
               % (RATE, lmed[RATE][0] / lmed[0.0][0], lmed[RATE][1] / lmed[0.0][1]))


legs_at("configs[1]'s head", 16, 90)
legs_at("32 pages x 300 boxes", 32, 300)


# ------------------------------------------------------------------------------------------------ the train step
def page_rows(rs, boxes, img_w, img_h):
    wh = np.stack([rs.uniform(8, 400, boxes), rs.uniform(8, 200, boxes)], 1)
    xy = rs.uniform(0, 1, (boxes, 2)) * (np.asarray([img_w, img_h]) - wh)
    lab = np.zeros((boxes, 1))
    lab[rs.permutation(boxes)[:3], 0] = [1, 2, 3]
    return np.concatenate([xy, wh, lab], 1).astype(np.float32)


CFG = dict(roi_output_size=(3, 3), n_classes=4, use_context=True, hidden_dim=384, bbox_hidden_dim=32,
           n_additional_feat=0, drop_prob=0.2, page_encoder_dim=P, page_encoder_heads=HEADS, page_encoder_layers=1,
           page_encoder_ffn_dim=M)
BATCH, IMG, BOXES, CS, KS = 16, args.img, 90, 6, 12
NP = max(BATCH, args.pages // BATCH * BATCH)
rs = np.random.RandomState(0)
gen = torch.Generator(device=dev).manual_seed(0)
u8_dev = torch.empty((NP, IMG, IMG, 3), dtype=torch.uint8, device=dev)
for lo in range(0, NP, 64):
    u8_dev[lo:lo + 64] = torch.randint(0, 256, (min(64, NP - lo), IMG, IMG, 3), dtype=torch.uint8, device=dev, generator=gen)
ds = DeviceDataset(u8_dev, [page_rows(rs, BOXES, IMG, IMG) for _ in range(NP)], CS, dev, spatial_k=KS)
legs = [0.0, RATE]                                                   # the first leg is the yardstick
sd = weights.seeded_state_dict(123, **{k: v for k, v in CFG.items() if k != "drop_prob"})
trainers = {r: HotPathTrainer(dict(CFG, page_encoder_dropout=r), sd, dev) for r in legs}


def steps(tr, n, epoch0):
    done, epoch = 0, epoch0
    while done < n:
        for b in ds.batches(BATCH, shuffle=True, sampling_fraction=1.0, seed=1, epoch=epoch):
            tr.train_step(b)
            done += 1
            if done == n:
                break
        epoch += 1


for r in legs:                          # warm-up: every shape and code path of the timed window
    steps(trainers[r], WARMUP, 0)
torch.cuda.synchronize()
ms = {r: [] for r in legs}
for rnd in range(args.rounds):
    for r in legs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps(trainers[r], args.steps, rnd + 1)
        torch.cuda.synchronize()
        ms[r].append(1e3 * (time.perf_counter() - t0) / args.steps)

out.append("page_dropout_rate, step: %d pages resident (%.2f GB uint8), batch %d x %dx%d, %d boxes/page, hybrid graph "
           "(context_size %d, spatial_k %d), page_encoder_dim %d, L = 1; %d rounds x %d steps, warm-up %d steps; ms per train step"
           % (NP, NP * IMG * IMG * 3 / 1e9, BATCH, IMG, IMG, BOXES, CS, KS, P, args.rounds, args.steps, WARMUP))
for r in legs:
    v = np.asarray(ms[r])
    out.append("leg page_encoder_dropout=%.1f median %.3f  min %.3f  max %.3f  spread %.3f  [%s]"
               % (r, np.median(v), v.min(), v.max(), v.max() - v.min(), " ".join("%.3f" % x for x in v)))
base, spread = float(np.median(ms[legs[0]])), float(np.max(ms[legs[0]]) - np.min(ms[legs[0]]))
d = float(np.median(ms[legs[1]])) - base
out.append("leg %.1f - leg %.1f: %+.3f ms/step (%+.2f %%); spread of the repeated leg %.1f: %.3f ms%s"
           % (legs[1], legs[0], d, 100 * d / base, legs[0], spread,
              " -- the difference is inside that spread" if abs(d) <= spread else ""))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(out) + "\n")
print("\n".join(out))
