"""bench.py's output side without a GPU: the stdout line stays short enough for a reader that keeps only the end of stdout (the full
line goes to stderr), and --dump-outputs writes the last step's loss / arena sample / buffers in the stated format.  CPU only."""
import contextlib
import io
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _full_line():
    table = {"dn::kernel_%03d<%d, %d>" % (i, i, i + 1): {"GBps": 1234.5678 + i, "ms_per_step": 0.0123 + i, "launches_per_step": 2}
             for i in range(120)}
    return {"metric": bench.CONFIGS["vggbn128"][0], "value": 2000.5, "unit": "images/sec", "n_gpus": 1, "steps": 17, "warmup": 3,
            "ms_per_step": 15.9, "ms_per_step_median": 15.8, "higher_is_better": True,
            "config": {"name": "vggbn128", "workload": "w", "launch": "launch tape: 201 launches", "final_loss": 32.5},
            "roofline": {"kernel": "k", "achieved": 744.4, "peak": 2500.0, "unit": "TFLOP/s", "frac": 0.3, "by_kernel": table,
                         "algorithm": "x" * 300},
            "roofline_hbm": {"kernel": "h", "achieved": 5149.8, "peak": 8000.0, "unit": "GB/s", "frac": 0.64, "by_kernel": table,
                             "thin_layers": table},
            "cpu_baseline": {"value": 8.5, "unit": "images/sec", "cores": 32, "kind": "port", "sample": "y" * 400},
            "other_configs": {"dorn128": {"img_per_s": 1800.0}}, "strong_1gpu": {"b4_tape": {"img_per_s": 1150.0}}}


def test_emit_prints_one_short_line_and_the_full_detail_to_stderr():
    line = _full_line()
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        bench.emit(line)
    rows = out.getvalue().splitlines()
    assert len(rows) == 1 and len(rows[0]) < 3000, len(out.getvalue())
    d = json.loads(rows[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "config"):
        assert d[k] == line[k], k
    assert d["roofline"] == {k: line["roofline"].get(k) for k in bench.HEADLINE_KEEP["roofline"]}
    assert d["cpu_baseline"]["value"] == 8.5 and "other_configs" not in d and "strong_1gpu" not in d
    detail = [r for r in err.getvalue().splitlines() if r.startswith("[bench-detail] ")]
    assert len(detail) == 1 and json.loads(detail[0][len("[bench-detail] "):]) == line


def _fake_run(n, seed):
    g = torch.Generator().manual_seed(seed)
    arena = types.SimpleNamespace(flat_p=torch.randn(n, generator=g), flat_g=torch.randn(n, generator=g))
    opt = types.SimpleNamespace(arena=arena, exp_avg=torch.randn(n, generator=g), exp_avg_sq=torch.rand(n, generator=g))
    bn = torch.nn.BatchNorm2d(5)
    bn.running_mean.normal_(generator=g)
    return torch.tensor(1.25), opt, [bn]


def test_dump_outputs_writes_a_fixed_sample_of_the_arena(tmp_path):
    n = bench.DUMP_SAMPLE + 12345
    loss, opt, nets = _fake_run(n, 0)
    bench.dump_outputs(str(tmp_path / "a"), loss, opt, nets)
    bench.dump_outputs(str(tmp_path / "b"), *_fake_run(n, 0))
    names = {"loss", "sample_index", "params", "grads", "exp_avg", "exp_avg_sq", "buffers"}
    assert {f[:-4] for f in os.listdir(tmp_path / "a")} == names
    total = 0
    for name in names:
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.dtype in (np.float32, np.float64), name
        np.testing.assert_array_equal(a, b)                  # same arguments -> same file, position for position
        total += a.nbytes
    assert total <= 64 << 20
    assert float(np.load(tmp_path / "a" / "loss.npy")) == 1.25
    idx = np.load(tmp_path / "a" / "sample_index.npy").astype(np.int64)
    assert idx.size == bench.DUMP_SAMPLE and np.all(np.diff(idx) > 0) and idx[-1] < n
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "params.npy"), opt.arena.flat_p.numpy()[idx])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "exp_avg_sq.npy"), opt.exp_avg_sq.numpy()[idx])
    bufs = np.load(tmp_path / "a" / "buffers.npy")
    assert bufs.dtype == np.float64 and bufs.size == 5 + 5 + 1
    np.testing.assert_array_equal(bufs[:5], nets[0].running_mean.double().numpy())


def test_dump_outputs_keeps_a_small_arena_whole(tmp_path):
    loss, opt, nets = _fake_run(1000, 1)
    bench.dump_outputs(str(tmp_path), loss, opt, nets)
    np.testing.assert_array_equal(np.load(tmp_path / "grads.npy"), opt.arena.flat_g.numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "sample_index.npy"), np.arange(1000, dtype=np.float64))


def test_plain_run_resolves_every_secondary_measurement_off_and_full_on():
    """A plain `bench.py --gpus 1 --steps N --warmup W` runs no secondary timing and no instrumented steps; --full restores the old
    defaults; an explicit count or --per-layer still asks for its own part alone."""
    plain = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not plain.full and plain.alt_steps == 0 and plain.profile_steps == 0 and plain.steps == 7 and plain.warmup == 2
    full = bench.parse_args(["--gpus", "1", "--full"])
    assert full.full and full.alt_steps == 10 and full.profile_steps == 2
    assert bench.parse_args(["--per-layer"]).profile_steps == 2
    assert bench.parse_args(["--alt-steps", "3"]).alt_steps == 3
    off = bench.parse_args(["--full", "--alt-steps", "0", "--profile-steps", "0"])
    assert off.full and off.alt_steps == 0 and off.profile_steps == 0
