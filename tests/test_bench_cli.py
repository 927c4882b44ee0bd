"""bench.py's command line on a small grid: a plain run prints the headline line and nothing of what --full measures,
--dump-outputs writes the state after the last timed step (the same arguments give the same state), --full adds the CPU
baseline.  Subprocesses with a hard timeout, one JSON line on stdout."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.common import rel_l2

ROOT = Path(__file__).resolve().parent.parent
N = 48


def _bench(*extra, timeout=300):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--n", str(N), *extra], cwd=ROOT,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _dumped(d):
    arrs = {k: np.load(d / f"{k}.npy") for k in ("state", "state_index", "state_summary")}
    assert all(a.dtype == np.float64 for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    return arrs


def test_bench_options_without_a_gpu():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_bench_plain_run_and_dump(tmp_path):
    out = _bench("--steps", "4", "--warmup", "2", "--dump-outputs", str(tmp_path / "a"))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline", "step_roofline"):
        assert k in out, k
    assert "cpu_baseline" not in out and "strong_scaling" not in out
    assert out["steps"] == 4 and out["warmup"] == 2
    assert out["ms_per_step"] > 0 and abs(out["value"] * out["ms_per_step"] - 1e3) <= 1e-6
    a = _dumped(tmp_path / "a")
    x, idx, summary = a["state"], a["state_index"], a["state_summary"]
    n = 2 * (N + 1) ** 3                                      # small grid: the whole unknown vector, in order
    assert len(x) == n and np.array_equal(idx, np.arange(n))
    assert summary[0] == n and summary[3] == x.min() and summary[4] == x.max()
    assert np.isclose(summary[1], x.sum(), rtol=1e-12) and np.isclose(summary[2], np.linalg.norm(x), rtol=1e-12)
    assert x.max() > 0.5                                      # a real field, not zeros
    # the same arguments give the same inputs: a second run computes the same state
    _bench("--steps", "4", "--warmup", "2", "--dump-outputs", str(tmp_path / "b"))
    assert rel_l2(_dumped(tmp_path / "b")["state"], x) <= 1e-10


@pytest.mark.gpu
def test_bench_full_adds_the_cpu_baseline():
    out = _bench("--steps", "2", "--warmup", "1", "--full", "--cpu-steps", "1")
    assert out["steps"] == 2
    assert out["cpu_baseline"]["value"] is not None and out["cpu_baseline"]["value"] > 0, out["cpu_baseline"]
