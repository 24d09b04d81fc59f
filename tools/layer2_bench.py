"""ms/step of HotPathTrainer with the optional layer2 stage (backbone_layers=2) at a bench.py workload (default
configs[1]): backbone_layers 1 and 2, the full step and the "stem + layer1 frozen" step, timed with HIP events on the
stream after warm-up, every case on the same batches.  Also one profiled step of the backbone_layers=2 full case: the
in-step time of each new launch (csrc/conv_nhwc.hip) with its nominal FLOPs and the fraction of the f32-MFMA peak.
Prints one JSON line.

    python tools/layer2_bench.py [--config 2] [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FROZEN_L1 = ("convnet.0.", "convnet.1.", "convnet.4.")
CASES = [
    ("layers1_full", 1, dict()),
    ("layers1_stem_layer1_frozen", 1, dict(frozen=FROZEN_L1)),
    ("layers2_full", 2, dict()),
    ("layers2_stem_layer1_frozen", 2, dict(frozen=FROZEN_L1)),
]
F32_MFMA_PEAK_TF = 155.0        # measured peak of v_mfma_f32_32x32x2_f32


def conv_flops(name, ints):
    """nominal FLOPs of one conv_nhwc launch from its integer arguments (B, H, W, Ci, Co, k, stride, pad)"""
    B, H, W, Ci, Co, k, s, p = ints[-8:]
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    return 2.0 * B * Ho * Wo * Co * Ci * k * k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    import bench
    import cova_amd  # noqa: F401
    from cova_web_object_detection_amd import _lib, weights
    from cova_web_object_detection_amd.trainer import HotPathTrainer
    dev = "cuda:0"
    wl = bench.WORKLOADS[args.config]
    batches = [bench.make_device_batch(s, dev, config=args.config) for s in (1, 2)]
    out = dict(workload=wl["name"], pages=wl["pages"], steps=args.steps, warmup=args.warmup,
               device=torch.cuda.get_device_name(0), cases={})
    for name, layers, kw in CASES:
        cfg = dict(bench.model_cfg(wl), backbone_layers=layers)
        sd = weights.seeded_state_dict(123, **bench.weight_cfg(cfg))
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
        out["cases"][name] = dict(backbone_layers=layers, ms_per_step=round(ms, 3),
                                  pages_per_s=round(wl["pages"] * 1000.0 / ms, 1), frozen=list(kw.get("frozen", ())))
        if name == "layers2_full":
            # one profiled step: per-launch HIP events around every entry point of the new kernels
            _lib.PROFILE = {n: [] for n in _lib.lib().fn if n.startswith("cova_conv_nhwc")}
            try:
                tr.train_step(batches[0])
                torch.cuda.synchronize()
            finally:
                prof, _lib.PROFILE = _lib.PROFILE, None
            kern, tot_ms, tot_fl = [], 0.0, 0.0
            for ep, recs in prof.items():
                for a, b, ints, _ in recs:
                    t = a.elapsed_time(b)
                    fl = conv_flops(ep, ints) if ep != "cova_conv_nhwc_prep" else 0.0
                    tot_ms, tot_fl = tot_ms + t, tot_fl + fl
                    kern.append(dict(entry=ep, shape="k%d s%d %d->%d" % (ints[-3], ints[-2], ints[-5], ints[-4])
                                     if fl else "", ms=round(t, 3),
                                     tflops=round(fl / t / 1e9, 1) if fl else None,
                                     frac_f32_mfma_peak=round(fl / t / 1e9 / F32_MFMA_PEAK_TF, 3) if fl else None))
            out["layer2_launches"] = kern
            out["layer2_launch_total"] = dict(ms=round(tot_ms, 3), tflop=round(tot_fl / 1e12, 3),
                                              frac_f32_mfma_peak=round(tot_fl / tot_ms / 1e9 / F32_MFMA_PEAK_TF, 3))
        del tr
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
