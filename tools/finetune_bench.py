"""ms/step of HotPathTrainer's fine-tuning steps at a bench.py workload (default configs[1]): the full step, a frozen stem
(conv1 + its BatchNorm), a frozen conv stack with train-mode BatchNorms, and the classic frozen backbone (conv stack frozen,
its BatchNorms in eval mode).  Steps are timed with HIP events on the stream after warm-up, every case on the same batches;
prints one JSON line.  Pair it with bench.py --full (its clock_leg) from the same box for context.

    python tools/finetune_bench.py [--config 2] [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [
    ("full", dict()),
    ("stem_frozen", dict(frozen=("convnet.0.", "convnet.1."))),
    ("convstack_frozen_bn_train", dict(frozen=("convnet.",))),
    ("convstack_frozen_bn_eval", dict(frozen=("convnet.",), bn_eval=("convnet.",))),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    import bench
    import cova_amd  # noqa: F401
    from cova_web_object_detection_amd import weights
    from cova_web_object_detection_amd.trainer import HotPathTrainer
    dev = "cuda:0"
    wl = bench.WORKLOADS[args.config]
    cfg = bench.model_cfg(wl)
    sd = weights.seeded_state_dict(123, **bench.weight_cfg(cfg))
    batches = [bench.make_device_batch(s, dev, config=args.config) for s in (1, 2)]
    out = dict(workload=wl["name"], pages=wl["pages"], steps=args.steps, warmup=args.warmup,
               device=torch.cuda.get_device_name(0), cases={})
    for name, kw in CASES:
        tr = HotPathTrainer(cfg, sd, dev, **kw)
        for i in range(args.warmup):
            tr.train_step(batches[i % 2])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.steps):
            tr.train_step(batches[i % 2])
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.steps
        out["cases"][name] = dict(ms_per_step=round(ms, 3), pages_per_s=round(wl["pages"] * 1000.0 / ms, 1),
                                  frozen=list(kw.get("frozen", ())), bn_eval=list(kw.get("bn_eval", ())),
                                  plan=sorted(tr.plan) if tr.plan is not None else "full")
        del tr
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
