"""What every solve REPORTS -- pg_step_info.{converged, resnorm, bnorm, iters}, pg_run_info.{worst_relres, unconverged_steps} --
held against host truth (tests/residual_truth.py) on every path that builds the weighted sums (r,r)_W and (b̂,b̂)_W: the start
kernels, k_renorm behind gamma_fix / diag_fix, the start folded into the right-hand-side kernel, the half-step exit, the
x / r updates.  The paths are chosen by PG_* variables read once per process: one child process per setting
(scripts/residual_truth_child.py), one after another, each bounded by its timeout; the tests assert on the child's JSON line.

Cases (one rank, a few hundred to a thousand rows): ball3d 12^3, ball3d_odd 13 x 12 x 10 (13 x 12 x 11 gives two odd n_own: one
extent less; box 4, ball at 2.01, r = 1, Dirichlet borders and interface), disc2d_robin 24 x 20 (Robin(1, 0.4, 0.7): blocked rows), diph2d 20^2 (ScalarJump / FluxJump: keeps the full
system), cg2d (the system of test_cg_method_on_symmetric_problem).  reltol 1e-6 and 1e-9, far above the attainable floor:
condition (d) of the checker (delta <= 1e-3 tol) holds on every solve, and the child fails where it does not.

What the device says about a solve beyond pg_step_info -- products, degree, half-step exit -- comes from a twin solver that
takes the same solves through pg_solver_run and is held to them bit for bit (the child's docstring).  The folded start has no
counter of its own: a quiet step is one in which the rows left out did not move at all (a start that was not folded would move
them by their rounding-level δ, which the tests exclude), and only the reltol 1e-9 cases with constant data have such steps --
at 1e-6 what the first solve leaves on those rows is beyond the noise threshold and every later step is finished on the full
system.  The folded start, the rows that stay and the half-step exit on such a step are covered by the 1e-9 cases alone.
"""
import json
import os
import pathlib
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
OFF = {"PG_DIAG_ELIM": None, "PG_GAMMA_ELIM": None, "PG_GUESS_STATES": None, "PG_GUESS_ALWAYS": None, "PG_GUESS_DEFER": None,
       "PG_POLY_F32": None, "PG_POLY_DEGREE": None, "PG_POLY": None, "PG_SPMV_VARIANT": None}


def child(args, env, timeout=240):
    e = {k: v for k, v in os.environ.items() if k not in OFF}
    e.update(env)
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "residual_truth_child.py"), *args], cwd=ROOT, env=e, capture_output=True,
                       text=True, timeout=timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads(lines[-1])
    assert r.returncode == 0 and out["ok"], (out.get("error"), out.get("violations"), r.stderr[-2000:])
    return out


def _solves(out):
    for c in out["cases"].values():
        yield c["first"]
        yield from c["steps"]


def _all_checked(recs):
    """what check_step enforced in the child, once more on the figures it printed"""
    n = 0
    for r in recs:
        assert r["delta_over_tol"] <= 1e-3 and r["res_gap_over_delta"] <= 1.0 and r["bnorm_err_over_bound"] <= 1.0, r
        assert "violation" not in r, r
        n += 1
    return n


def test_first_solves_from_zero_and_capped_solves():
    """plain BiCGStab on every case, the polynomial at degrees 2 and 5 on the two balls, CG, GMRES, BiCGStab(2), IDR(4); a
    solve capped one iteration below what it needed reports converged = 0 and a residual that is the state's"""
    out = child(["first"], {})
    recs = out["solves"]
    assert _all_checked(recs) >= 2 * (3 + 3 + 1 + 1) + 4 + 2 + 3
    assert out["n_own"]["ball3d"] % 2 != out["n_own"]["ball3d_odd"] % 2, out["n_own"]
    by = lambda **kw: [r for r in recs if all(r.get(k) == v for k, v in kw.items())]
    assert {r["degree"] for r in recs if r["label"].startswith("ball3d")} == {0, 2, 5}      # (what the device ran: the twin's run info)
    assert any(r["half_exit"] for r in recs if r["degree"] == 5) and all(r["products"] > 0 for r in recs if r["iters"] > 0)
    assert {r["method"] for r in recs} == {"bicgstab", "cg", "gmres", "bicgstabl", "idrs"}
    capped = by(capped=True)
    assert len(capped) == 4 and all(r["converged"] == 0 and r["res_true_rel"] > r["reltol"] for r in capped)
    assert all(r["converged"] == 1 for r in recs if not r.get("capped"))
    for r in recs:
        if r["method"] == "bicgstab" and r["label"].startswith("ball3d") and not r.get("capped"):
            assert abs(r["iters"] - r["it_ref"]) <= 1, r


def _warm(expect, env, extra=()):
    out = child(["warm", "--expect", expect, *extra], env)
    assert _all_checked(_solves(out)) > 0
    assert out["half_exits"] > 0 and out["half_exits"] == sum(r["half_exit"] for c in out["cases"].values() for r in c["steps"])
    return out


def _paths(out, want_ball):
    for key, c in out["cases"].items():
        want = want_ball if key.startswith("ball3d") else "full"
        assert c["path"] == want, (key, c["path"])
        if c["path"] != "full":
            assert c["loop_matrix_checked"]["rows"] == c["rows_matrix"] < c["n_own"] and c["loop_matrix_checked"]["coupling_nnz"] > 0, c
        if "run" in c:
            assert c["run"]["worst_relres"] == c["stepwise"]["worst_relres"] and c["run"]["unconverged_steps"] == c["stepwise"]["unconverged_steps"] == 0


def test_warm_steps_on_the_full_system():
    """PG_DIAG_ELIM=0 PG_GAMMA_ELIM=0: k_rhs_init's start sums, both parities of n_own, blocked rows, the diphasic system"""
    out = _warm("full", {"PG_DIAG_ELIM": "0", "PG_GAMMA_ELIM": "0"})
    _paths(out, "full")
    n = {k.split("/")[0]: c["n_own"] for k, c in out["cases"].items()}
    assert n["ball3d"] % 2 != n["ball3d_odd"] % 2 and set(n) == {"ball3d", "ball3d_odd", "disc2d_robin", "diph2d"}


def test_warm_steps_with_the_dirichlet_row_reduction():
    """PG_DIAG_ELIM=0: gamma_fix moves the residual, k_renorm sums it again; the sub-matrix is restrict_gamma of the full one"""
    out = _warm("gamma", {"PG_DIAG_ELIM": "0"}, ["--cases", "ball3d,ball3d_odd", "--data", "const,closure"])
    _paths(out, "gamma")
    for key, c in out["cases"].items():
        assert c["gamma_elim"] == 1 and c["rows_matrix"] == c["n_own"] - c["n_gamma_host"], (key, c)
        if "/closure/" in key:
            assert c["eliminated_rows_moved_by"] > 0.0


def test_warm_steps_on_the_compact_system():
    """the default: constant data (quiet steps: the start phase folded into k_rhs_init_c), a Dirichlet interface value as a plain
    closure of t (rows move every step: diag_fix and k_renorm), the same as a TimeSeparable (the device loop's data); the compact
    matrix is restrict_diag of the full one, entry for entry; pg_solver_run's totals equal the stepwise run's"""
    out = _warm("compact", {}, ["--cases", "ball3d,ball3d_odd", "--data", "const,closure,separable"])
    _paths(out, "compact")
    assert sum(out["n_c"]) % 2 == 1, out["n_c"]
    assert out["quiet_half_exits"] > 0          # a folded start with rows that stayed, ended at a half step
    for key, c in out["cases"].items():
        assert c["loop_is_compact"] == 1 and c["rows_matrix"] == c["n_c"] == c["n_own"] - c["n_e_host"], (key, c)
        assert c["n_e_host"] > c["n_gamma_host"] > 0                 # (border rows leave too: more than the γ block)
        if "/const/" in key:
            # quiet steps (the folded start, no coupling launch): the rows left out rest, bit for bit.  What the first solve
            # left on them -- a fraction of ITS tolerance -- moves them in the first step; at reltol 1e-6 that is beyond the
            # noise threshold in every later step too (CN on a Dirichlet row: x_new = 2 g - x_old), and those steps are
            # finished on the full system
            if key.endswith("/1e-09"):
                assert c["quiet_steps"] == len(c["steps"]) - 1, (key, c["eliminated_rows_moved_by_step"])
            assert all(v == 0.0 or v > 1e-13 for v in c["eliminated_rows_moved_by_step"][1:]), (key, c["eliminated_rows_moved_by_step"])
        else:
            assert c["quiet_steps"] == 0 and c["eliminated_rows_moved_by"] > 1e-3, (key, c["eliminated_rows_moved_by"])
        if "run" in c:
            assert c["run"]["poly_degree"] == 5


@pytest.mark.parametrize("defer", ["0", "1"])
def test_extrapolated_start(defer):
    """PG_GUESS_ALWAYS=1, eight quiet steps: older states are kept and read, the state written by the solve's first update of x
    (PG_GUESS_DEFER=1) or by k_rhs_init_c; the start sums are those of the extrapolated residual"""
    out = _warm("compact", {"PG_GUESS_ALWAYS": "1", "PG_GUESS_DEFER": defer},
                ["--cases", "ball3d,ball3d_odd", "--steps", "8", "--guess", "--one-reltol"])
    _paths(out, "compact")
    for key, c in out["cases"].items():
        assert c["guess_kept_max"] >= 2 and max(r["guess_states"] for r in c["steps"]) >= 1, (key, [r["guess_kept"] for r in c["steps"]])
        assert c["run"]["guess_states_read"] > 0, c["run"]
        assert c["quiet_steps"] == len(c["steps"]) - 1 and c["quiet_half_exits"] > 0, (key, c["quiet_steps"], c["quiet_half_exits"])


@pytest.mark.parametrize("f32", ["0", "1"])
def test_mixed_precision_chain(f32):
    """PG_POLY_F32: with the fp32 head of the Horner chain the reported residual is still the state's"""
    out = _warm("compact", {"PG_POLY_F32": f32}, ["--cases", "ball3d,ball3d_odd", "--steps", "5", "--one-reltol"])
    _paths(out, "compact")
    for key, c in out["cases"].items():
        assert (c["run"]["poly_f32_chains"] > 0) == (f32 == "1"), (key, c["run"])


def test_warm_iteration_counts_follow_the_host_restatement():
    """PG_GUESS_STATES=0 PG_POLY_F32=0, fixed degree: every warm step of the compact loop takes the iterations the restatement
    takes on the FULL exported system from the previous state with the eliminated rows snapped (same history in exact
    arithmetic: those rows have zero residual and the system is block triangular), within 1"""
    out = _warm("compact", {"PG_GUESS_STATES": "0", "PG_POLY_F32": "0"}, ["--cases", "ball3d,ball3d_odd", "--degree", "4", "--iters",
                                                                       "--data", "const,closure"])
    _paths(out, "compact")
    n = 0
    for c in out["cases"].values():
        for r in c["steps"]:
            assert abs(r["iters"] - r["it_ref"]) <= 1, r
            n += 1
        assert c["run"]["poly_degree"] == 4 if "run" in c else True
    assert n >= 16
