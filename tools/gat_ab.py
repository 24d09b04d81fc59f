"""Two builds of the library against each other on the graph-attention entry points: every output bit, and us per launch.

``--parent`` is the other build (libcova_hip.so of the commit to compare with); the tree's own library is "new".  This
process never touches the GPU: it starts one child per (library, job), COVA_HIP_LIB naming the library, each under its own
time limit, and checks the exit status before the next child starts.

Bits: cova_gat_fwd / _edge / _drop, cova_gat_bwd / _edge / _drop and cova_gat2_fwd / _bwd (/ _drop) with and without edge
term and dropout, on the case tables of tests/test_attn_dropout_gpu.py (static and GATv2), tests/test_edge_gpu.py and on the
(D, K) list of the option-16 tests of tests/test_kernels_gpu.py, each with cova_set_option(16, .) at 0 and at 1.  A child
writes the SHA-256 of every output buffer; the two lists must be equal.

Speed: us per call of the six static entry points, tools/edge_rate.py's launch windows (device events around ``--launches``
back-to-back calls, the median of ``--rounds`` windows after a warm-up window), 1440 nodes (16 pages of 90 boxes, DOM-order
windows), passes alternating parent, new, parent, new.  Limit per case: the parent's slower pass plus the parent's own
pass-to-pass difference; the mean of the new passes may not exceed it; ``--repeat`` takes the four passes again.  ``--bench``: bench.py on both libraries, twice each.
``--trace``: one more timing child per library under ``rocprofv3 --kernel-trace --stats``, mean duration of every GAT kernel.

The exit status is 1 when an output differs or a case is over its limit in every repetition (with the default, one
repetition, that is the rule as it stands; a pass of these 10 to 60 us launches can run 1 to 3 us slow as a whole, and the
parent's library against itself -- COVA_HIP_LIB set to it as well -- is over some limit in most repetitions).

    python tools/gat_ab.py --parent /path/to/parent/libcova_hip.so [--bench] [--trace] [--out profiles/gat_unify_ab.txt]
"""
import argparse
import csv
import glob
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--parent", help="the library to compare with")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--repeat", type=int, default=1, help="how many times the four alternating timing passes are taken")
ap.add_argument("--bench", action="store_true", help="also run bench.py on both libraries")
ap.add_argument("--trace", action="store_true", help="also take the kernels' durations from a kernel trace of each library")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gat_unify_ab.txt"))
ap.add_argument("--child", choices=("bits", "time"), help=argparse.SUPPRESS)
ap.add_argument("--json", help=argparse.SUPPRESS)
args = ap.parse_args()

OPTION16_DK = [(96, 24), (384, 24), (64, 1), (200, 64), (330, 48), (512, 7), (40, 13), (512, 64)]
#             K    D  option 16    (the instantiations <KP, ND> they reach: <1, 6>, <1, 1>, <2, 1>, <1, 8>, and <1, 1> in the
#                                  place of the former wide kernels at ND = 1)
TIMED = [(24, 384, 1), (24, 384, 0), (100, 384, 1), (24, 512, 1), (24, 64, 1)]
ENTRY = ("cova_gat_fwd", "cova_gat_fwd_edge", "cova_gat_fwd_drop", "cova_gat_bwd", "cova_gat_bwd_edge", "cova_gat_bwd_drop")


# ------------------------------------------------------------------------------------------------ children (GPU)
def child_bits():
    os.environ.setdefault("COVA_ALLOW_OPTION_CHANGES", "1")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import cova_amd  # noqa: F401
    from cova_web_object_detection_amd import engine
    import edge_oracle as EO
    import test_attn_dropout_gpu as AD
    import test_edge_gpu as TE
    import test_gatv2_gpu as TG

    cases = [("dropout/%s-%s" % c, AD.gat_case(*c)) for c in AD.CASES]
    cases += [("edge/%s" % n, dict(TE.gat_case(n), mode="gat", pad=0)) for n in ("wide", "general", "hub", "k2")]
    for D, K in OPTION16_DK:
        N = 211
        rs = np.random.RandomState(1000 * D + K)
        ctx = TG.make_table(rs, N, K)
        cases.append(("option16/D%d-K%d" % (D, K), dict(
            mode="gat", N=N, K=K, D=D, pad=0, ctx=ctx, Wh=rs.standard_normal((N, 2 * D)).astype(np.float32),
            phi=EO.edge_features(TG.random_boxes(rs, N, 1280.0), ctx, 1280.0, 1280.0),
            aw=(rs.standard_normal(2 * D) / np.sqrt(D)).astype(np.float32), ab=rs.standard_normal(1).astype(np.float32),
            g=rs.standard_normal((N, D)).astype(np.float32))))
    digests = {}
    for wide in (0, 1):
        engine.query("cova_set_option", 16, wide)
        for name, case in cases:
            for edge in (False, True):
                for drop in (None, (0.5, AD.SEED)):
                    got = AD.launch(case, edge=edge, drop=drop)
                    for k, v in sorted(got.items()):
                        key = "opt16=%d %s edge=%d drop=%d %s" % (wide, name, edge, drop is not None, k)
                        digests[key] = hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()
    engine.query("cova_set_option", 16, 1)
    with open(args.json, "w") as fh:
        json.dump(digests, fh)


def child_time():
    os.environ.setdefault("COVA_ALLOW_OPTION_CHANGES", "1")
    import numpy as np
    import torch
    import cova_amd  # noqa: F401
    from cova_web_object_detection_amd._lib import call, query

    dev, PAGES, BOXES = "cuda:0", 16, 90
    N = PAGES * BOXES

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
        return float(np.median(v))

    res = {}
    for K, D, wide in TIMED:
        query("cova_set_option", 16, wide)
        pos = np.arange(BOXES)[:, None] + np.arange(K)[None, :] - K // 2    # DOM-order window inside the page, pads outside
        ctx = np.concatenate([np.where((pos >= 0) & (pos < BOXES), pos + p * BOXES, -1) for p in range(PAGES)]).astype(np.int64)
        ctx = torch.from_numpy(ctx).to(dev)
        tg = torch.Generator(device=dev).manual_seed(1)
        rnd_ = lambda *shape: torch.randn(shape, device=dev, generator=tg)
        new = lambda *shape: torch.empty(shape, device=dev)
        Wh, aw, ab, ew, gr = rnd_(N, 2 * D), rnd_(2 * D) / D ** 0.5, rnd_(1), rnd_(8), rnd_(N, D)
        phi = rnd_(N, K, 8) * (ctx >= 0)[:, :, None]
        s, t, attn, hp = new(N), new(N), new(N, K), new(N, D)
        dWh, dsv, dtv, daw, dab, dew, du = new(N, 2 * D), new(N), new(N), new(2 * D), new(1), new(8), new(N, K)
        ws = new(query("cova_gat_edge_workspace_floats", N, K))
        csr = torch.zeros((query("cova_gat_transpose_ints", N, K),), dtype=torch.int32, device=dev)
        call("cova_gat_transpose", ctx, N, K, csr)
        p, seed = 0.5, 12345
        fns = {
            "cova_gat_fwd": lambda: call("cova_gat_fwd", Wh, 2 * D, aw, ab, ctx, N, K, D, 0.2, s, t, attn, hp, D),
            "cova_gat_fwd_edge": lambda: call("cova_gat_fwd_edge", Wh, 2 * D, aw, ab, ctx, phi, ew, N, K, D, 0.2, s, t, attn,
                                              hp, D),
            "cova_gat_fwd_drop": lambda: call("cova_gat_fwd_drop", Wh, 2 * D, aw, ab, ctx, phi, ew, N, K, D, 0.2, p, seed, s, t,
                                              attn, hp, D),
            "cova_gat_bwd": lambda: call("cova_gat_bwd", gr, D, Wh, 2 * D, s, t, attn, ctx, aw, N, K, D, 0.2, dWh, 2 * D, dsv,
                                         dtv, daw, dab, csr, du),
            "cova_gat_bwd_edge": lambda: call("cova_gat_bwd_edge", gr, D, Wh, 2 * D, s, t, attn, ctx, aw, phi, ew, N, K, D, 0.2,
                                              dWh, 2 * D, dsv, dtv, daw, dab, dew, csr, du, ws),
            "cova_gat_bwd_drop": lambda: call("cova_gat_bwd_drop", gr, D, Wh, 2 * D, s, t, attn, ctx, aw, phi, ew, N, K, D, 0.2,
                                              p, seed, dWh, 2 * D, dsv, dtv, daw, dab, dew, csr, du, ws),
        }
        for name in ENTRY:                                                   # (the forwards first: the backwards read attn)
            res["K %3d D %3d option16 %d  %s" % (K, D, wide, name)] = windows(fns[name])
    query("cova_set_option", 16, 1)
    with open(args.json, "w") as fh:
        json.dump(res, fh)


if args.child:
    {"bits": child_bits, "time": child_time}[args.child]()
    sys.exit(0)


# ------------------------------------------------------------------------------------------------ the driver (no GPU)
def run_child(job, lib, tmp, limit, prefix=(), rounds=None):
    path = os.path.join(tmp, "%s_%d.json" % (job, len(os.listdir(tmp))))
    env = dict(os.environ, COVA_HIP_LIB=lib) if lib else dict(os.environ)
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", job, "--json", path, "--rounds",
                          str(rounds or args.rounds), "--launches", str(args.launches)]
    rc = subprocess.run(cmd, env=env, timeout=limit).returncode
    if rc != 0:
        sys.exit("gat_ab: child %s on %s ended with status %d; nothing more is started" % (job, lib or "the tree's library", rc))
    with open(path) as fh:
        return json.load(fh)


def run_trace(lib, tmp, limit):
    """kernel name -> (launches, mean us) of the GAT kernels of one timing child under a kernel trace"""
    d = os.path.join(tmp, "trace_%d" % len(os.listdir(tmp)))
    run_child("time", lib, tmp, limit, ("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"), 3)
    res = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as fh:
            for row in csv.reader(fh):
                m = re.search(r"(gat_(?:fwd|bwd_src|bwd_dst)(?:_wide)?_kernel<[^>]*>)", row[0])
                if m:
                    res[m.group(1)] = (int(row[1]), float(row[3]) / 1e3)
    return res


def run_bench(lib, limit):
    env = dict(os.environ, COVA_HIP_LIB=lib) if lib else dict(os.environ)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline",
           "--no-ab", "--no-clock-leg"]
    r = subprocess.run(cmd, env=env, timeout=limit, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit("gat_ab: bench.py on %s ended with status %d; nothing more is started" % (lib or "the tree's library", r.returncode))
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["value"]


if not args.parent or not os.path.exists(args.parent):
    sys.exit("gat_ab: --parent must name the library to compare with")
parent = os.path.abspath(args.parent)
out = ["Graph-attention entry points, the parent commit's library against this one on one MI355X in one session (tools/gat_ab.py)."]
with tempfile.TemporaryDirectory() as tmp:
    bits = [run_child("bits", lib, tmp, 600) for lib in (parent, None)]
    diff = sorted(k for k in set(bits[0]) | set(bits[1]) if bits[0].get(k) != bits[1].get(k))
    out += ["", "Bits: %d output buffers (cova_gat_fwd / _edge / _drop, cova_gat_bwd / _edge / _drop, cova_gat2_fwd / _bwd / _drop; "
            "the case tables of test_attn_dropout_gpu.py, test_edge_gpu.py, test_gatv2_gpu.py and the option-16 (D, K) list; "
            "option 16 at 0 and at 1): %s" % (len(bits[1]), "identical" if not diff else "%d DIFFER" % len(diff))]
    out += ["  differs: " + k for k in diff[:40]]
    out += ["", "Speed: us per call, median of %d windows of %d back-to-back calls after a warm-up window; N = 1440; passes alternate"
            % (args.rounds, args.launches), "(parent1, new1, parent2, new2).  Limit: the parent's slower pass plus the parent's own "
            "pass-to-pass difference; the mean of", "the new passes may not exceed it.  The four passes are taken %d time(s), "
            "each time judged by itself." % args.repeat]
    missed, over = 0, {}
    for rep in range(args.repeat):
        passes = [run_child("time", lib, tmp, 300) for lib in (parent, None, parent, None)]
        out += ["", "  %-46s %8s %8s %8s %8s %8s" % ("case (repetition %d)" % (rep + 1), "parent1", "parent2", "new1", "new2", "limit")]
        for k in passes[0]:
            p1, n1, p2, n2 = (p[k] for p in passes)
            limit = max(p1, p2) + abs(p1 - p2)
            ok = 0.5 * (n1 + n2) <= limit
            missed += not ok
            over[k] = over.get(k, 0) + (not ok)
            out.append("  %-46s %8.2f %8.2f %8.2f %8.2f %8.2f  %s" % (k, p1, p2, n1, n2, limit, "met" if ok else "MISSED"))
    always = sum(v == args.repeat for v in over.values())
    out += ["", "cases over the limit: %d of %d judged; over it in every repetition: %d" % (missed, args.repeat * len(over), always)]
    if args.trace:
        tr = [run_trace(lib, tmp, 300) for lib in (parent, None)]
        out += ["", "Kernel durations, us: mean over the launches of one timing pass per library under rocprofv3 --kernel-trace --stats",
                "(3 windows per case; a kernel that serves several cases mixes them):"]
        for which, t in zip(("parent", "new"), tr):
            out += ["  %-7s %-46s %6d launches %8.2f" % (which, k, t[k][0], t[k][1]) for k in sorted(t)]
    if args.bench:
        v = [run_bench(lib, 900) for lib in (parent, None, parent, None)]
        out += ["", "bench.py --gpus 1 --steps 20 --warmup 5, pages/s: parent %.1f, %.1f; new %.1f, %.1f" % (v[0], v[2], v[1], v[3])]
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(out) + "\n")
print("\n".join(out))
sys.exit(1 if diff or always else 0)
