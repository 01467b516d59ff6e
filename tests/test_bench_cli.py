"""bench.py's command line on the GPU: a plain run prints the headline line only, --dump-outputs writes the last timed step's
results (the same arrays in two runs with the same arguments), --full adds the side measurements.  Small batches: this tests
the options, not the speed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "hbm_kernel", "f32_mfma_mode", "fast_mode", "small_batch", "cpu_baseline")


def _bench(*argv, env=None):
    res = subprocess.run([sys.executable, BENCH, "--batch", "32", "--warmup", "1"] + list(argv), env=env, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_and_dump_outputs(tmp_path):
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        line = _bench("--steps", "3", "--dump-outputs", str(d))
        assert all(k in line for k in HEADLINE), line.keys()
        assert line["steps"] == 3 and line["step_hip_events"]["steps"] == 3
        assert not any(k in line for k in FULL_ONLY), line.keys()
        assert abs(line["value"] - 32 * 3 / (line["ms_per_step"] * 3e-3)) / line["value"] < 1e-3
        files = sorted(os.listdir(d))
        assert {"output.npy", "loss.npy", "cut_positions.npy", "f1_mean.npy", "dcg_mean.npy", "grads.npy", "params.npy"} <= set(files)
        assert sum(os.path.getsize(d / f) for f in files) <= 64 * 10 ** 6
        arrays = {f: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert arrays["output.npy"].shape[:2] == (32, 300)
        assert abs(float(arrays["loss.npy"]) - line["train_state"]["loss"]) < 1e-5
        runs.append(arrays)
    for f, a in runs[0].items():
        assert np.array_equal(a, runs[1][f]), f


def test_full_run_adds_the_side_measurements():
    env = dict(os.environ, RLT_BENCH_SMALL="0")
    line = _bench("--steps", "2", "--full", "--other-steps", "1", "--no-cpu-baseline", env=env)
    assert all(k in line for k in HEADLINE)
    assert line["roofline"]["launches_timed"] > 0 and line["hbm_kernel"]["us_per_call"] > 0
    assert line["f32_mfma_mode"]["steps"] == 1 and line["fast_mode"]["steps"] == 1
