"""The compact loop with the constants of uniform groups of rows taken from the kernels' arguments (PG_ROW_CONST=1, the default)
against the same loop streaming them for every row (PG_ROW_CONST=0): bit for bit.

Every case runs the same problem in two fresh child processes (tests/row_const_child.py), both with PG_GUESS_ALWAYS=1, and
asserts that
  - the state after the last step and the exported right-hand side b̂ are bitwise equal,
  - iterations, products, degree, half exits and the relative residual of every solve are equal,
  - what pg_solver_guess_info reports after every step is bitwise equal.
The 128^3 sphere is the case in which both branches run inside one wave: pg_solver_row_const_info must report at least a fifth
of the groups of each table qualifying and at least a fifth not.
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
OFF = ("PG_ROW_CONST", "PG_STEP_FUSE", "PG_GUESS_STATES", "PG_GUESS_ALWAYS", "PG_GUESS_DEFER", "PG_GUESS_DEPTH", "PG_GUESS_MONITOR",
       "PG_DIAG_ELIM", "PG_GAMMA_ELIM", "PG_POLY", "PG_POLY_DEGREE", "PG_POLY_F32", "PG_SPMV_VARIANT", "PG_SPECULATE")


def child(case, steps, switch, env, out_dir, timeout=240):
    e = {k: v for k, v in os.environ.items() if k not in OFF}
    e.update(env)
    e["PG_ROW_CONST"] = switch
    e["PG_GUESS_ALWAYS"] = "1"
    out_dir.mkdir()
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "row_const_child.py"), "--case", case, "--steps", str(steps), "--out",
                        str(out_dir)], cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads(lines[-1])
    assert r.returncode == 0 and out["ok"], (out.get("error"), r.stderr[-2000:])
    assert out["config"]["row_const"] == switch and out["loop_is_compact"] == 1, out["config"]
    return out, np.load(out_dir / "state.npy"), np.load(out_dir / "bhat.npy")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def pair(case, steps, env, tmp_path):
    """both children of a case, held against each other; returns the record of the one with the switch on"""
    f, xf, bf = child(case, steps, "1", env, tmp_path / "on")
    u, xu, bu = child(case, steps, "0", env, tmp_path / "off")
    print(case, "row_const_info:", f["row_const"], "rows", f["n_own"])
    assert f["n_own"] == u["n_own"] and len(f["steps"]) == len(u["steps"]) == steps
    assert f["first"] == u["first"]
    for k, (a, b) in enumerate(zip(f["steps"], u["steps"]), 1):
        assert a["unconverged"] == 0, (k, a)
        for key in ("iters", "products", "degree", "half_exits", "relres", "states_read"):
            assert a[key] == b[key], (case, k, key, a, b)
        assert a["guess"] == b["guess"], (case, k, a["guess"], b["guess"])
    assert xf.shape == xu.shape and np.array_equal(bits(xf), bits(xu)), (case, float(np.max(np.abs(xf - xu))))
    assert bf.shape == bu.shape and np.array_equal(bits(bf), bits(bu)), (case, float(np.max(np.abs(bf - bu))))
    assert u["row_const"] == {"full_groups": 0, "full_const": 0, "loop_groups": 0, "loop_const": 0}, u["row_const"]
    assert all(s["bmark"] == {"valid": 0, "const": 0, "builds": 0, "uses": 0} for s in u["steps"]), [s["bmark"] for s in u["steps"]]
    print(case, "bconst mark per step (valid, groups, builds):", [(s["bmark"]["valid"], s["bmark"]["const"], s["bmark"]["builds"]) for s in f["steps"]])
    return f


def marks(f, valid, builds):
    """the steps whose launch took a bconst mark, and the marks built; a mark that stands covers at least a fifth of the
    groups (the bound of `mixed`: the branch that takes bconst from the arguments runs, beside the one that streams it) and no
    group that the table does not qualify"""
    rc = f["row_const"]
    assert [s["bmark"]["valid"] for s in f["steps"]] == valid, [s["bmark"] for s in f["steps"]]
    assert f["steps"][-1]["bmark"]["builds"] == builds, f["steps"][-1]["bmark"]
    for s in f["steps"]:
        if s["bmark"]["valid"]:
            assert 5 * s["bmark"]["const"] >= rc["full_groups"] and s["bmark"]["const"] <= rc["full_const"], (s["bmark"], rc)


def mixed(rc):
    """both branches are taken, by at least a fifth of the groups of each table each"""
    for t in ("full", "loop"):
        g, c = rc[t + "_groups"], rc[t + "_const"]
        assert g > 0 and 5 * c >= g and 5 * (g - c) >= g, (t, rc)


def test_sphere_128_cubed(tmp_path):
    f = pair("sphere128", 14, {}, tmp_path)
    mixed(f["row_const"])
    assert f["row_const"]["full_groups"] == (f["n_own"] + 15) // 16
    marks(f, [0] + [1] * 13, 1)          # (built at the second step with the same data, taken by every launch from then on)
    assert f["steps"][-1]["bmark"]["uses"] == 13
    assert sum(s["states_read"] for s in f["steps"]) > 0 and any(s["guess"]["offsets"] for s in f["steps"])


def test_disc_768_squared(tmp_path):
    f = pair("disc768", 12, {}, tmp_path)
    rc = f["row_const"]
    assert f["n_own"] % 16 != 0                                # (a partial last group)
    assert 2 * rc["full_const"] > rc["full_groups"] and 2 * rc["loop_const"] > rc["loop_groups"], rc   # (long runs)
    marks(f, [0] + [1] * 11, 1)


def test_sphere_40_cubed_has_no_uniform_group(tmp_path):
    f = pair("sphere40", 14, {}, tmp_path)
    rc = f["row_const"]
    assert rc["full_groups"] > 0 and rc["loop_groups"] > 0 and rc["full_const"] == 0 and rc["loop_const"] == 0, rc
    marks(f, [0] * 14, 0)                # (no group to mark: no mark is built or taken)


def test_sphere_128_with_a_step_of_changed_interface_value(tmp_path):
    f = pair("sphere128_jump", 12, {}, tmp_path)
    mixed(f["row_const"])
    kept = [s["guess"]["kept"] for s in f["steps"]]
    assert kept[5] >= 2 and kept[6] == 0 and kept[7] == 0 and kept[-1] >= 2, kept   # (two steps with coupling launches among quiet ones)
    marks(f, [0, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1], 2)   # (steps 7 and 8 have new data each: the mark is dropped, and built again at step 9)


def test_sphere_128_with_a_source_that_changes_every_step(tmp_path):
    f = pair("sphere128_source", 8, {}, tmp_path)
    mixed(f["row_const"])
    marks(f, [0] * 8, 0)                 # (no two steps with the same bconst: no mark is built, bconst streams)


def test_sphere_128_with_a_source_that_changes_once(tmp_path):
    f = pair("sphere128_fsteps", 10, {}, tmp_path)
    mixed(f["row_const"])
    # the mark of the first source serves steps 2..5; steps 6 and 7 have new data each; the second mark is built at step 8 --
    # a launch that took the first one there would compute another b̂ than the streamed form
    marks(f, [0, 1, 1, 1, 1, 0, 0, 1, 1, 1], 2)


def test_sphere_128_without_older_states(tmp_path):
    f = pair("sphere128", 4, {"PG_GUESS_STATES": "0"}, tmp_path)
    assert f["config"]["guess_states"] == "0"
    assert all(s["states_read"] == 0 and s["guess"]["kept"] == 0 for s in f["steps"])


def test_sphere_128_with_solves_past_their_half_step(tmp_path):
    # a degree too low for one application of the polynomial to reach the tolerance: the half-step test fails, the second
    # half runs: k_bicg_xrp (which streams its rows) follows a k_bicg_s_x that took the table
    f = pair("sphere128", 6, {"PG_POLY_DEGREE": "3"}, tmp_path)
    mixed(f["row_const"])
    assert all(s["degree"] == 3 for s in f["steps"]), [s["degree"] for s in f["steps"]]
    assert sum(s["half_exits"] for s in f["steps"]) < sum(s["iters"] for s in f["steps"]), f["steps"]
