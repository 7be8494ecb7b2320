"""bench.py end to end on the GPU: --steps sets the timed steps, the stdout line carries ms_per_step, and --dump-outputs writes the
last timed step's results -- the same ones, from the same inputs, on a second run with the same arguments.  pytest -m gpu."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

ARRAYS = ("loss", "sample_index", "params", "grads", "exp_avg", "exp_avg_sq", "buffers")


def _bench(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4",
                        "--alt-steps", "0", "--profile-steps", "0", "--no-cpu-baseline", "--extras", "0", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(rows) == 1, r.stdout[-2000:]
    assert "[bench-detail] " in r.stderr
    return json.loads(rows[0])


def test_bench_dump_outputs_is_the_last_step_and_repeats(tmp_path):
    a = _bench(tmp_path / "a")
    b = _bench(tmp_path / "b")
    for d in (a, b):
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0
    total = 0
    for name in ARRAYS:
        x, y = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), name
        np.testing.assert_allclose(x, y, rtol=1e-5, atol=1e-7, err_msg=name)
        total += x.nbytes
    assert total <= 64 << 20
    assert float(np.load(tmp_path / "a" / "loss.npy")) == pytest.approx(a["config"]["final_loss"], rel=1e-6)
    assert np.load(tmp_path / "a" / "sample_index.npy").size == bench.DUMP_SAMPLE
    assert np.abs(np.load(tmp_path / "a" / "grads.npy")).max() > 0



def _detail(flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + flags, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert len([l for l in r.stdout.splitlines() if l.startswith("{")]) == 1, r.stdout[-2000:]
    rows = [l for l in r.stderr.splitlines() if l.startswith("[bench-detail] ")]
    assert len(rows) == 1, r.stderr[-2000:]
    return json.loads(rows[0][len("[bench-detail] "):])


def test_bench_plain_run_is_lean_and_full_adds_the_secondaries():
    """Without --full the run times the headline only (no instrumented steps, no fp32-instruction timing, no CPU baseline, no nested
    runs); --full brings the roofline and the fp32-instruction timing back into the same line."""
    plain = _detail(["--steps", "2", "--warmup", "1", "--batch", "4"])
    assert plain["config"]["full"] is False and plain["value"] > 0 and plain["steps"] == 2
    for k in ("roofline", "roofline_hbm", "f32_mfma_path", "cpu_baseline", "step_executed_frac"):
        assert plain[k] is None, k
    assert "other_configs" not in plain and "strong_1gpu" not in plain
    full = _detail(["--steps", "2", "--warmup", "1", "--batch", "4", "--full", "--alt-steps", "2", "--no-cpu-baseline"])
    assert full["config"]["full"] is True and full["value"] > 0
    assert full["roofline"]["achieved"] > 0 and full["roofline_hbm"]["achieved"] > 0
    assert full["f32_mfma_path"]["value"] > 0 and full["step_executed_frac"] > 0
