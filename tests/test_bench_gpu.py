"""GPU test of bench.py's plain run: one JSON line with the headline fields, exactly --steps timed steps, none of the
--full legs, and --dump-outputs files (float32 / float64, under 64 MB) that are identical between two runs with the same
arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PAGES = 2
FULL_ONLY = ("roofline", "other_kernels", "forward_only", "ab", "sustained", "dropin_module_loop", "clock_leg", "cpu_baseline")


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--pages", str(PAGES), "--dump-outputs", out_dir]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_reports_headline_and_dumps_reproducible_outputs(tmp_path):
    a_dir, b_dir = str(tmp_path / "a"), str(tmp_path / "b")
    line = _bench(a_dir)
    assert line["metric"] == "webpages/sec fwd+bwd (90 bboxes, K=24)" and line["unit"] == "webpages/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 3 and line["warmup"] == 1 and line["config"]["pages_per_gpu"] == PAGES
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - PAGES * 1e3 / line["ms_per_step"]) <= 1e-2 * line["value"]
    assert not [k for k in FULL_ONLY if k in line]
    _bench(b_dir)
    names = sorted(os.listdir(a_dir))
    assert names == ["bn_buffers.npy", "grads.npy", "loss.npy", "params.npy", "pred.npy"]
    total = 0
    for n in names:
        x, y = np.load(os.path.join(a_dir, n)), np.load(os.path.join(b_dir, n))
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), n
        assert np.array_equal(x, y), "%s differs between two runs with the same arguments" % n
        total += x.nbytes
    assert total <= 64 << 20
    assert np.load(os.path.join(a_dir, "pred.npy")).size == line["config"]["boxes_per_gpu"]
