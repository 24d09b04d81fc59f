"""Device time of the criterion launches at the box counts of bench.py's configs[1] (N = 1440) and configs[4] (N = 9600),
NC = 4: cova_ce_sum (the default step's criterion) and cova_ce_loss_fwd + cova_ce_loss_bwd with no option set, with class
weights + "mean", and as the focal loss (gamma 2); the two phases also on their own.  Then the whole configs[1] training
step (20 steps after warm-up, as bench.py times it) without options and with weights + smoothing + "mean" + metrics.

Each launch case is timed back to back on the device: a torch.cuda._sleep in front of the timed window lets the host
enqueue every call before the first one starts, so host-side Python and ctypes time is not in the figure (method of
tools/optim_bench.py; median of --reps windows).  Prints one JSON line.

    python tools/loss_bench.py [--calls 200] [--reps 5] [--no-step]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (("configs[1]", 1440), ("configs[4]", 9600))
NC = 4


def windows(fn, calls, reps):
    import torch
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(200_000_000)               # the host gets ahead of the device
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1000.0 / calls)
    out.sort()
    return dict(us_median=round(out[len(out) // 2], 2), us_min=round(out[0], 2), us_max=round(out[-1], 2))


def launch_cases(n, dev):
    """-> {case: zero-argument callable}; outputs are allocated once (the figure is the launches' device time)"""
    import torch
    from cova_web_object_detection_amd import engine
    g = torch.Generator(device=dev).manual_seed(n)
    logits = torch.randn(n, NC, generator=g, device=dev) * 4
    labels = torch.where(torch.rand(n, generator=g, device=dev) < 0.97, 0,
                         torch.randint(1, NC, (n,), generator=g, device=dev)).to(torch.int64)
    weight = torch.tensor([1.0, 4.0, 4.0, 4.0], device=dev)
    loss, dl = torch.empty(1, device=dev), torch.empty(n, NC, device=dev)
    pred, acc = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(3, dtype=torch.float64, device=dev)
    ws = torch.empty(engine.query("cova_ce_loss_workspace_doubles", n), dtype=torch.float64, device=dev)
    metrics = torch.zeros(NC * NC + 4, dtype=torch.int64, device=dev)

    def fwd(w, eps, gamma, m=None):
        engine.call("cova_ce_loss_fwd", logits, labels, n, NC, w, eps, gamma, 0, 0, acc, pred, m, ws)

    def bwd(w, eps, gamma, mean):
        engine.call("cova_ce_loss_bwd", logits, labels, n, NC, w, eps, gamma, 0, 0, acc, mean, None, loss, dl)

    def pair(w, eps, gamma, mean, m=None):
        return lambda: (fwd(w, eps, gamma, m), bwd(w, eps, gamma, mean))

    return {
        "cova_ce_sum": lambda: engine.call("cova_ce_sum", logits, labels, n, NC, 1.0, loss, dl, pred),
        "defaults": pair(None, 0.0, 0.0, 0),
        "defaults_fwd_only": lambda: fwd(None, 0.0, 0.0),
        "defaults_bwd_only": lambda: bwd(None, 0.0, 0.0, 0),
        "weights_mean": pair(weight, 0.0, 0.0, 1),
        "weights_smoothing_mean_metrics": pair(weight, 0.1, 0.0, 1, metrics),
        "focal": pair(None, 0.0, 2.0, 0),
    }


def step_ms(kw, steps=20, warmup=5):
    """the whole configs[1] training step as bench.py times it: events around `steps` steps after warm-up"""
    import torch
    import bench
    from cova_web_object_detection_amd import weights
    from cova_web_object_detection_amd.trainer import HotPathTrainer
    dev = "cuda:0"
    cfg = bench.model_cfg(bench.WORKLOADS[2])
    tr = HotPathTrainer(cfg, weights.seeded_state_dict(123, **bench.weight_cfg(cfg)), dev, **kw)
    batch = bench.make_device_batch(123, dev, config=2)
    for _ in range(warmup):
        tr.train_step(batch)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        tr.train_step(batch)
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / steps, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="skip the whole-step measurement")
    args = ap.parse_args()
    import torch
    import cova_amd  # noqa: F401
    dev = "cuda:0"
    out = dict(calls=args.calls, reps=args.reps, device=torch.cuda.get_device_name(0), n_classes=NC, sizes={})
    for name, n in SIZES:
        res = {case: windows(fn, args.calls, args.reps) for case, fn in launch_cases(n, dev).items()}
        base = res["cova_ce_sum"]["us_median"]
        for case in res:
            res[case]["vs_cova_ce_sum"] = round(res[case]["us_median"] / base, 3)
        out["sizes"][name] = dict(boxes=n, cases=res)
    if not args.no_step:
        options = dict(class_weight=[1.0, 4.0, 4.0, 4.0], label_smoothing=0.1, loss_reduction="mean", track_metrics=True)
        # interleaved, two rounds each: the difference is far below the box-to-box spread of a 9 ms step
        rounds = [(step_ms(dict()), step_ms(options)) for _ in range(2)]
        out["configs[1]_step_ms"] = dict(default=[r[0] for r in rounds], with_options=[r[1] for r in rounds])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
