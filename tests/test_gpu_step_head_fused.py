"""The head of a compact warm step with the fit inside the right-hand-side launch (PG_STEP_FUSE=1, the default) against the
same step with k_guess_fit as a launch of its own (PG_STEP_FUSE=0): bit for bit.

Every case runs the same problem in two fresh child processes (tests/step_head_child.py), both with PG_GUESS_ALWAYS=1, and
asserts that
  - the state after the last step is bitwise equal,
  - iterations, products and degree of every solve are equal,
  - what pg_solver_guess_info reports after every step (states kept, ring offsets, coefficients, the two sampled residuals) is
    bitwise equal,
  - the exported right-hand side b̂ is bitwise equal.
Cases: the 40^3 sphere (BE, then 14 CN steps: the ring fills, every chunk of 256 rows is sampled, fit blocks meet block rows)
with the extrapolated state formed by the first update of x (the fit rides) and by the right-hand-side kernel (it does not: the
switch must change nothing there); the 768^2 disc (about 116 k rows
in the loop's numbering: the fit's stride is 3, chunks are skipped, the last one is partial); the sphere with another interface
value from step 7 on (two steps with changed data among quiet ones); the sphere with PG_GUESS_STATES=0 (no older states, no fit:
the switch changes nothing).
"""
import json
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
OFF = ("PG_STEP_FUSE", "PG_GUESS_STATES", "PG_GUESS_ALWAYS", "PG_GUESS_DEFER", "PG_GUESS_DEPTH", "PG_GUESS_MONITOR", "PG_DIAG_ELIM",
       "PG_GAMMA_ELIM", "PG_POLY", "PG_POLY_DEGREE", "PG_POLY_F32", "PG_SPMV_VARIANT", "PG_SPECULATE")


def child(case, steps, fuse, env, out_dir, timeout=240):
    e = {k: v for k, v in os.environ.items() if k not in OFF}
    e.update(env)
    e["PG_STEP_FUSE"] = fuse
    e["PG_GUESS_ALWAYS"] = "1"
    out_dir.mkdir()
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "step_head_child.py"), "--case", case, "--steps", str(steps), "--out",
                        str(out_dir)], cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads(lines[-1])
    assert r.returncode == 0 and out["ok"], (out.get("error"), r.stderr[-2000:])
    assert out["config"]["step_fuse"] == fuse and out["loop_is_compact"] == 1, out["config"]
    return out, np.load(out_dir / "state.npy"), np.load(out_dir / "bhat.npy")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def pair(case, steps, env, tmp_path):
    """both children of a case, held against each other; returns the fused one's record"""
    f, xf, bf = child(case, steps, "1", env, tmp_path / "fused")
    u, xu, bu = child(case, steps, "0", env, tmp_path / "unfused")
    assert f["n_own"] == u["n_own"] and len(f["steps"]) == len(u["steps"]) == steps
    assert f["first"] == u["first"]
    for k, (a, b) in enumerate(zip(f["steps"], u["steps"]), 1):
        assert a["unconverged"] == 0, (k, a)
        for key in ("iters", "products", "degree", "half_exits", "relres", "states_read"):
            assert a[key] == b[key], (case, k, key, a, b)
        assert a["guess"] == b["guess"], (case, k, a["guess"], b["guess"])
    assert xf.shape == xu.shape and np.array_equal(bits(xf), bits(xu)), (case, float(np.max(np.abs(xf - xu))))
    assert bf.shape == bu.shape and np.array_equal(bits(bf), bits(bu)), (case, float(np.max(np.abs(bf - bu))))
    return f


@pytest.mark.parametrize("defer", ["1", "0"])
def test_sphere_40_cubed(defer, tmp_path):
    f = pair("sphere3d", 14, {"PG_GUESS_DEFER": defer}, tmp_path)
    assert f["config"]["guess_defer"] == defer
    # the ring has filled and the start reads older states: the fit ran, inside the launch, and its coefficients were taken
    assert max(s["guess"]["kept"] for s in f["steps"]) == 7, [s["guess"]["kept"] for s in f["steps"]]
    assert sum(s["states_read"] for s in f["steps"]) > 0 and any(s["guess"]["offsets"] for s in f["steps"])


def test_disc_768_squared(tmp_path):
    f = pair("disc2d", 12, {}, tmp_path)
    nchunk = (f["n_own"] + 255) // 256
    assert nchunk // 128 == 3, (f["n_own"], nchunk)          # (the fit's stride: chunks are skipped)
    assert f["n_own"] % 256 != 0                               # (... and the last chunk is partial)
    assert sum(s["states_read"] for s in f["steps"]) > 0


def test_sphere_with_a_step_of_changed_data(tmp_path):
    f = pair("sphere3d_jump", 14, {}, tmp_path)
    kept = [s["guess"]["kept"] for s in f["steps"]]
    # (the history ends at the two steps with changed data and refills after them)
    assert kept[5] >= 2 and kept[6] == 0 and kept[7] == 0 and kept[-1] >= 2, kept


def test_sphere_without_older_states(tmp_path):
    f = pair("sphere3d", 6, {"PG_GUESS_STATES": "0"}, tmp_path)
    assert f["config"]["guess_states"] == "0"
    assert all(s["states_read"] == 0 and s["guess"]["kept"] == 0 for s in f["steps"])
