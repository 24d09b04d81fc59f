"""Two builds of the library against each other on the row and page entry points whose kernels tools/isa_diff.py reports as
different: every output bit, and us per call.  The method is tools/gat_ab.py's.

``--parent`` is the other build (libcova_hip.so of the commit to compare with); the tree's own library is "new".  This
process never touches the GPU: it starts one child per (library, pass), COVA_HIP_LIB naming the library, each under its own
time limit, and checks the exit status before the next child starts.  A child runs cova_page_class_topk,
cova_eval_page_ranks, cova_hard_negative_select, cova_page_rank_loss_fwd / _bwd, cova_sample_boxes, cova_grad_norm and, as
the control, cova_page_joint_decode (4 and 7 classes: its kernels are identical) on seeded inputs (16 pages of 90 boxes; 4M gradient elements), writes the SHA-256 of
every output buffer and the us per call: device events around ``--launches`` back-to-back calls, the median of ``--rounds``
windows after a warm-up window.  Passes alternate parent, new, parent, new (``--pairs`` of them).  Limit per case: the
parent's slowest pass plus the parent's own spread (slowest minus fastest pass); the mean of the new passes may not exceed
it.  A pass of these 8 to 80 us launches can run 1 us slow as a whole: ``--new`` naming the parent's library as well shows
what the rule gives for no change at all.  ``--bench``: bench.py on both.

    python tools/helper_ab.py --parent /path/to/parent/libcova_hip.so [--bench] [--out profiles/helper_share_isa.txt]

The report is appended to ``--out``.  The exit status is 1 when an output differs or a case is over its limit.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--parent", help="the library to compare with")
ap.add_argument("--new", help="the library to compare (default: the tree's; the same file on both sides shows the rule's own miss rate)")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--pairs", type=int, default=2, help="alternating (parent, new) pairs of passes")
ap.add_argument("--bench", action="store_true", help="also run bench.py on both libraries")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "helper_share_isa.txt"))
ap.add_argument("--json", help=argparse.SUPPRESS)           # set in a child
args = ap.parse_args()


def child():
    import numpy as np
    import torch
    import cova_amd  # noqa: F401
    from cova_web_object_detection_amd._lib import call, query

    dev, B, BOXES = "cuda:0", 16, 90
    N = B * BOXES
    tg = torch.Generator(device=dev).manual_seed(7)
    new = lambda dtype, *shape: torch.zeros(shape, dtype=dtype, device=dev)
    i32, i64, f32, f64 = torch.int32, torch.int64, torch.float32, torch.float64
    page_start = torch.arange(0, N + 1, BOXES, dtype=i64, device=dev)
    offs32, ids32 = page_start.to(i32), torch.arange(B, dtype=i32, device=dev)
    cases = {}
    for nc in (7, 4):                                                 # (4 last: the lambdas below read its tensors)
        logits = torch.randn((N, nc), device=dev, generator=tg) + torch.randn((N, 1), device=dev, generator=tg)
        labels = new(i64, N)
        for c in range(1, nc):                                        # one box of every class a page
            labels[torch.arange(B, device=dev) * BOXES + 11 * c] = c
        choice, hit, gap = new(i32, B, nc - 1), new(i32, B, nc - 1), new(f64, B)
        cases["cova_page_joint_decode NC %d" % nc] = (
            lambda lg=logits, lb=labels, n=nc, o=(choice, hit, gap): call("cova_page_joint_decode", lg, lb, page_start, None, B,
                                                                          n, B, 1, *o), (choice, hit, gap))
        if nc == 7:
            continue
        topk, ranks, top1 = new(i64, B, nc, 3), new(i32, B, nc - 1), new(i32, B, nc - 1)
        cases["cova_page_class_topk k 3"] = (lambda: call("cova_page_class_topk", logits, page_start, B, nc, 3, topk), (topk,))
        cases["cova_eval_page_ranks"] = (
            lambda: call("cova_eval_page_ranks", logits, labels, page_start, ids32, B, nc, B, ranks, top1), (ranks, top1))
        mined, score, counts = new(i64, N), new(f32, N), new(i32, B, 3)
        cases["cova_hard_negative_select"] = (
            lambda: call("cova_hard_negative_select", logits, labels, page_start, B, N, nc, 3.0, 0, -100, mined, score, counts),
            (mined, score, counts))
        lists, acc, loss, dl = new(f64, B, nc - 1, 4), new(f64, 3), new(f32, 1), new(f32, N, nc)
        cases["cova_page_rank_loss_fwd"] = (
            lambda: call("cova_page_rank_loss_fwd", logits, labels, page_start, B, N, nc, None, -100, 1, lists, acc), (lists, acc))
        cases["cova_page_rank_loss_bwd"] = (
            lambda: call("cova_page_rank_loss_bwd", logits, labels, page_start, B, N, nc, None, -100, 1, lists, acc, 1.0, 1, None,
                         loss, dl, 0), (loss, dl))
        rows = torch.rand((N, 5), device=dev, generator=tg)
        rows[:, 4] = labels.to(f32)
        keep = torch.full((B,), int(0.9 * BOXES), dtype=i32, device=dev)
        ws, sel, out_offs = new(i32, query("cova_sample_boxes_workspace_ints", B, N)), new(i32, N), new(i32, B + 1)
        cases["cova_sample_boxes"] = (
            lambda: call("cova_sample_boxes", rows, offs32, None, None, keep, B, N, None, 12345, ws, sel, out_offs), (sel, out_offs))
    n = 4_000_000
    g = torch.randn((n,), device=dev, generator=tg)
    segs = torch.tensor([[0, n, 0, 0]], dtype=i64, device=dev)
    nws, norm = new(f64, query("cova_grad_norm_workspace_doubles", n)), new(f32, 2)
    cases["cova_grad_norm 4M"] = (lambda: call("cova_grad_norm", g, n, segs, 1, n, 1.0, nws, norm), (norm,))

    res = {}
    for name, (fn, bufs) in cases.items():
        v = []
        for rnd in range(args.rounds + 1):                            # window 0 is the warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                v.append(1e3 * e0.elapsed_time(e1) / args.launches)
        sha = hashlib.sha256(b"".join(np.ascontiguousarray(b.cpu().numpy()).tobytes() for b in bufs)).hexdigest()
        res[name] = (float(np.median(v)), sha)
    with open(args.json, "w") as fh:
        json.dump(res, fh)


if args.json:
    child()
    sys.exit(0)


def run(cmd, lib, limit):
    r = subprocess.run(cmd, env=dict(os.environ, COVA_HIP_LIB=lib) if lib else dict(os.environ), timeout=limit,
                       stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit("helper_ab: %s on %s ended with status %d; nothing more is started"
                 % (os.path.basename(cmd[1]), lib or "the tree's library", r.returncode))
    return r.stdout


if not args.parent or not os.path.exists(args.parent):
    sys.exit("helper_ab: --parent must name the library to compare with")
parent = os.path.abspath(args.parent)
passes = []
with tempfile.TemporaryDirectory() as tmp:
    for i, lib in enumerate((parent, args.new) * args.pairs):
        path = os.path.join(tmp, "pass%d.json" % i)
        run([sys.executable, os.path.abspath(__file__), "--json", path, "--rounds", str(args.rounds), "--launches",
             str(args.launches)], lib, 300)
        with open(path) as fh:
            passes.append(json.load(fh))
out = ["", "The entry points of the kernels that differ, the parent commit's library against this one on one MI355X in one session",
       "(tools/helper_ab.py): us per call, median of %d windows of %d back-to-back calls after a warm-up window; 16 pages of 90"
       % (args.rounds, args.launches), "boxes; %d passes of each library, alternating (parent, new, parent, new, ...).  Limit: the "
       "parent's slowest pass plus the" % args.pairs, "parent's own spread (slowest minus fastest pass); the mean of the new passes "
       "may not exceed it.  bits: the SHA-256 of the", "outputs, all passes.", "",
       "  %-30s %-*s %-*s %8s" % ("case", 9 * args.pairs, "parent passes", 9 * args.pairs, "new passes", "limit")]
bad = 0
for k in passes[0]:
    t, sha = [p[k][0] for p in passes], set(p[k][1] for p in passes)
    old, cur = t[0::2], t[1::2]
    limit = max(old) + (max(old) - min(old))
    ok, same = sum(cur) / len(cur) <= limit, len(sha) == 1
    bad += (not ok) + (not same)
    out.append("  %-30s %s %s %8.2f  %s  bits %s" % (k, "".join(" %8.2f" % x for x in old), "".join(" %8.2f" % x for x in cur), limit,
                                                    "met" if ok else "MISSED", "identical" if same else "DIFFER"))
if args.bench:
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline",
           "--no-ab", "--no-clock-leg"]
    v = [json.loads([ln for ln in run(cmd, lib, 900).splitlines() if ln.startswith("{")][-1])["value"] for lib in (parent, args.new)]
    out += ["", "bench.py --gpus 1 --steps 20 --warmup 5, pages/s: parent %.1f, new %.1f" % (v[0], v[1])]
with open(args.out, "a") as fh:
    fh.write("\n".join(out) + "\n")
print("\n".join(out))
sys.exit(1 if bad else 0)
