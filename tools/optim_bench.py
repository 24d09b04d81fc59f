"""Device time of HotPathTrainer.optimizer_step() at the parameter counts of bench.py's configs[1] and configs[2]: today's
cova_adam_step, and cova_optim_step in adam / adamw / sgd (momentum 0.9) mode, each with clipping (cova_grad_norm first,
max_grad_norm=1.0) and without.  The gradient bucket holds fixed random values; the step count advances as in training.

Each case is timed back to back on the device: a torch.cuda._sleep in front of the timed window lets the host enqueue
every step before the first one starts, so host-side Python and ctypes time is not in the figure.  Bytes per parameter
are the HBM floor of one step (adam / adamw 28 B, sgd with momentum 20 B, +4 B for the norm); GB/s is that floor over
the measured time.  Prints one JSON line.

    python tools/optim_bench.py [--steps 200] [--reps 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [
    ("cova_adam_step", dict()),
    ("adam", dict(param_groups=[])),
    ("adam_clip", dict(param_groups=[], max_grad_norm=1.0)),
    ("adamw", dict(optimizer="adamw")),
    ("adamw_clip", dict(optimizer="adamw", max_grad_norm=1.0)),
    ("sgd", dict(optimizer="sgd", momentum=0.9)),
    ("sgd_clip", dict(optimizer="sgd", momentum=0.9, max_grad_norm=1.0)),
]
BYTES = dict(cova_adam_step=28, adam=28, adamw=28, sgd=20)


def time_case(tr, steps, reps):
    import torch
    for _ in range(10):                              # warm-up (code objects, the norm workspace)
        tr.step_count += 1
        tr.optimizer_step()
    torch.cuda.synchronize()
    best = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(200_000_000)               # the host gets ahead of the device
        e0.record()
        for _ in range(steps):
            tr.step_count += 1
            tr.optimizer_step()
        e1.record()
        torch.cuda.synchronize()
        best.append(e0.elapsed_time(e1) * 1000.0 / steps)
    return sorted(best)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import bench
    import cova_amd  # noqa: F401
    from cova_web_object_detection_amd import weights
    from cova_web_object_detection_amd.trainer import HotPathTrainer
    dev = "cuda:0"
    out = dict(steps=args.steps, reps=args.reps, device=torch.cuda.get_device_name(0), configs={})
    for config in (2, 3):
        wl = bench.WORKLOADS[config]
        cfg = bench.model_cfg(wl)
        sd = weights.seeded_state_dict(123, **bench.weight_cfg(cfg))
        res = {}
        for name, kw in CASES:
            tr = HotPathTrainer(cfg, sd, dev, **kw)
            gen = torch.Generator(device=dev).manual_seed(1)
            tr.gbucket.flat.copy_(torch.randn(tr.gbucket.flat.shape, generator=gen, device=dev) * 1e-3)
            n_params = sum(p.numel() for p in tr.params.values())
            us = time_case(tr, args.steps, args.reps)
            floor = BYTES[name.split("_clip")[0]] + (4 if "clip" in name else 0)
            res[name] = dict(us_median=round(us[len(us) // 2], 2), us_min=round(us[0], 2), us_max=round(us[-1], 2),
                             bytes_per_param=floor, gb_per_s=round(floor * n_params / (us[len(us) // 2] * 1e3), 1))
            del tr
            torch.cuda.empty_cache()
        base = res["cova_adam_step"]["us_median"]
        for name in res:
            res[name]["vs_cova_adam_step"] = round(res[name]["us_median"] / base, 3)
        out["configs"][wl["name"]] = dict(params=n_params, cases=res)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
