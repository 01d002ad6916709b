"""bench.py end to end on the GPU: a plain run prints the headline and writes the outputs of its last timed step,
--full adds the measurements the headline does not need."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "roofline_stats", "levels")


def run_bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c2"] + list(args),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_bench_plain_run_and_dump(tmp_path):
    d = tmp_path / "out"
    line = run_bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(d))
    assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY + ("cpu_baseline",))
    assert line["steps"] == 3 and line["config"]["em_iterations_timed"] == 3 * line["config"]["em_iterations_per_step"]
    assert line["ms_per_step"] > 0 and line["value"] > 0 and line["higher_is_better"] is True
    files = sorted(os.listdir(d))
    assert {"free_energy.npy", "theta_W.npy", "Kn_sample.npy", "lpj_sample.npy"} <= set(files)
    assert sum(os.path.getsize(d / f) for f in files) <= 64 * 10 ** 6
    arrays = {f: np.load(d / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
    assert float(arrays["free_energy.npy"]) == pytest.approx(line["config"]["free_energy_last"], rel=1e-12)
    assert arrays["theta_W.npy"].shape == (256, 128)
    ss = arrays["Kn_sample.npy"]
    assert ss.shape[1:] == (64, 128) and set(np.unique(ss)) <= {0.0, 1.0}
    for row in ss:  # K^n holds S distinct states per datapoint
        assert np.unique(row, axis=0).shape[0] == 64


def test_bench_full_run():
    line = run_bench("--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline")
    assert all(k in line for k in HEADLINE + FULL_ONLY)
    assert line["roofline"]["launches_timed"] > 0 and line["config"]["kernel_ms"]
    assert line["config"]["ms_per_em_iteration_eager_theta"] > 0
