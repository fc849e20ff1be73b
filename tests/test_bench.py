"""bench.py's plain run: exactly --steps timed steps, the headline fields only, and --dump-outputs writing what the last timed step
computed (the image and the radii of the one view, float32)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest


@pytest.mark.gpu
def test_bench_py_plain_run_times_exactly_steps_and_dumps_its_outputs(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, steps = 20000, 7
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2", "--preheat-ms", "0",
           "--gaussians", str(n), "--dump-outputs", str(tmp_path / "out")]
    res = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-3000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == steps and d["unit"] == "views/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["config"]["windows"]["R"] == 1 and len(d["config"]["windows"]["ms_per_step_of_each_window"]) == 1
    assert d["ms_per_step"] > 0 and abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    for k in ("roofline", "bwd_ms", "cpu_baseline", "parity", "batched_8_views"):  # the --full legs stay out of a plain run
        assert k not in d, k
    color = np.load(tmp_path / "out" / "color.npy")
    radii = np.load(tmp_path / "out" / "radii.npy")
    assert color.dtype == np.float32 and color.shape == (1, 3, 256, 256)
    assert radii.dtype == np.float32 and radii.shape == (1, n)
    assert np.isfinite(color).all() and color.max() > 0 and (radii > 0).sum() > 0
