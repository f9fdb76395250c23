"""bench.py's own plumbing: the --dump-outputs sample and files (CPU), and one plain run on the GPU --
its result line, that the legs behind --full stay out of it, and its dumped outputs against a solve
of the same seeded problems through the library."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_rows_whole_batch_when_it_fits():
    np.testing.assert_array_equal(bench.dump_rows(1000, 2400), np.arange(1000))
    # config 2 and config 5 at the default batch fit whole (24 MB; 5.12 + 51.2 MB)
    assert len(bench.dump_rows(10000, 10 * 3 * 10 * 8)) == 10000
    assert len(bench.dump_rows(10000, 64 * 8 + 64 * 10 * 8)) == 10000


def test_dump_rows_fixed_sample_within_budget():
    B, row = 125000, 10 * 3 * 10 * 8  # config 3's shard: 300 MB of coefficients
    rows = bench.dump_rows(B, row)
    assert len(rows) * row <= 64 * 1000 * 1000 < (len(rows) + 1) * row
    assert len(np.unique(rows)) == len(rows) and rows.min() >= 0 and rows.max() < B
    assert (np.diff(rows) > 0).all()
    np.testing.assert_array_equal(rows, bench.dump_rows(B, row))  # the same rows every run
    assert len(bench.dump_rows(5, 10 ** 9)) == 1  # never empty


def test_dump_outputs_writes_f64_npy(tmp_path):
    a = np.arange(24, dtype=np.float64).reshape(4, 3, 2)
    c = np.arange(4, dtype=np.float64) + 0.5
    bench.dump_outputs(str(tmp_path / "d"), {"coeffs": a, "cost": c})
    assert sorted(os.listdir(tmp_path / "d")) == ["coeffs.npy", "cost.npy"]
    got = np.load(tmp_path / "d" / "coeffs.npy")
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, a)
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "cost.npy"), c)
    bench.dump_outputs(str(tmp_path / "d"), {"coeffs": a}, rank=1, world=2)
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "coeffs_rank1.npy"), a)


@pytest.mark.gpu
def test_plain_run_result_line_and_dumped_outputs(tmp_path, gpu_ctx):
    B, steps = 333, 7
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "2", "--min-warmup-ms", "0", "--batch", str(B), "--dump-outputs",
                        str(tmp_path / "out")], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == steps and d["warmup_steps_run"] == 2
    assert d["higher_is_better"] is True and d["dtype"] == "f64" and d["unit"] == "trajectories/s"
    assert d["ms_per_step"] > 0
    assert abs(d["value"] - B / (d["ms_per_step"] * 1e-3)) <= 1e-9 * d["value"]
    # a plain run carries none of the legs behind --full
    assert "end_to_end" not in d and d["cpu_baseline"] is None and d["roofline"]["kernel_ms_isolated"] is None
    # the dumped outputs are the solve of the seeded problems (the kernels are bit-reproducible)
    assert os.listdir(tmp_path / "out") == ["coeffs.npy"]
    got = np.load(tmp_path / "out" / "coeffs.npy")
    assert got.dtype == np.float64 and got.shape == (B, 10, 3, 10)
    values, mask, times = bench.make_problems("config2", 10, 10, B, bench.shard_seed0(0, B))
    want = gpu_ctx.solve_linear_batch(10, 4, values, mask, times)["coeffs"]
    np.testing.assert_array_equal(got, want)
