"""The numpy restatement of the device's restarted GMRES (tests/gmres_reference.py gmres_dev_ref: CGS2, the Givens estimate that
only ends a cycle, acceptance on the weighted true residual at the restarts, the lowered inner tolerance, maxiter in Arnoldi steps)
against direct solves and the oracle's IterativeSolvers restatement po.gmres_ref, and its own counting rules and edges.  CPU only."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import penguin_oracle as po
from tests.gmres_reference import gmres_dev_ref, heat_system, peclet_system, small_box_system, symmetric_scaling

RELTOL = 1e-10


@pytest.fixture(scope="module")
def systems():
    """name -> (Â, b̂, S, x of the direct solve).  peclet (32^2, uniform flow, cell Peclet number 12.5) and rotation (16^2): rows already
    divided by their diagonal, S = 1; GMRES(20) needs eight cycles on the first, GMRES(80) one on the second."""
    out = {"heat": symmetric_scaling(*heat_system(16)), "box": small_box_system(0.04), "box/10": small_box_system(0.004)}
    for key, n, kind in (("peclet", 32, "uniform"), ("rotation", 16, "rotation")):
        A, b = peclet_system(n, kind)
        out[key] = (A, b, np.ones(len(b)))
    return {k: (A, b, S, spla.spsolve(A.tocsc(), b)) for k, (A, b, S) in out.items()}


def _wrel(A, b, S, x):
    return np.linalg.norm(S * (b - A @ x)) / np.linalg.norm(S * b)


CASES = [("heat", 20), ("heat", 5), ("peclet", 20), ("peclet", 40), ("rotation", 80), ("box", 20), ("box", 5), ("box/10", 20), ("box/10", 5)]


@pytest.mark.parametrize("name,restart", CASES)
def test_solution_and_counts_against_direct_solve_and_the_mgs_restatement(systems, name, restart):
    """The same acceptance rule on the same system: the state of the direct solve and of po.gmres_ref(weights=S), iterations within
    2 of it (the bar test_gmres_heat_monophasic holds MGS and CGS2 to), the recomputed weighted residual within the tolerance."""
    A, b, S, direct = systems[name]
    x, info = gmres_dev_ref(A, b, restart=restart, reltol=RELTOL, weights=S)
    xm, itm, _ = po.gmres_ref(A, b, reltol=RELTOL, restart=restart, weights=S)
    print(name, restart, info, "mgs", itm)
    assert info["converged"] and not info["singular"] and not info["notfinite"]
    assert abs(info["iters"] - itm) <= 2, (info["iters"], itm)
    assert _wrel(A, b, S, x) <= 1.05 * RELTOL
    assert info["resnorm"] <= RELTOL * info["bnorm"]
    # ||x - x*|| <= ||Â⁻¹|| ||r||: both restatements stop on the same residual bound, so they differ from the direct solve alike
    scale = np.linalg.norm(direct)
    assert np.linalg.norm(x - direct) <= 1e-8 * scale and np.linalg.norm(x - xm) <= 1e-8 * scale
    xl, il = gmres_dev_ref(A, b, restart=restart, reltol=RELTOL, weights=S, long_sums=True)
    assert il["converged"] and abs(il["iters"] - info["iters"]) <= 1
    assert np.linalg.norm(x - xl) <= 1e-8 * scale


@pytest.mark.parametrize("name", ["box", "box/10"])
@pytest.mark.parametrize("restart", [20, 5])
def test_small_box_reaches_the_lowering_branch_and_discriminates(systems, name, restart):
    """The Givens estimate meets reltol cycles before the weighted residual does: at least one cycle starts with a lowered inner
    tolerance, and GMRES without the weighted rule ends at least 2 x above reltol in the weighted norm (measured: 2.9 x and 12 x on
    the box of 0.04, 27 x and 39 x on 0.004)."""
    A, b, S, _ = systems[name]
    _, info = gmres_dev_ref(A, b, restart=restart, reltol=RELTOL, weights=S)
    xu, itu, _ = po.gmres_ref(A, b, reltol=RELTOL, restart=restart)
    print(name, restart, "restatement", info["iters"], "lowered", info["lowered"], "unweighted", itu, _wrel(A, b, S, xu) / RELTOL)
    assert info["converged"] and info["lowered"] >= 1 and info["cycles"] >= 2
    assert _wrel(A, b, S, xu) >= 2.0 * RELTOL and itu < info["iters"]


@pytest.mark.parametrize("name,restart", CASES)
def test_maxiter_counts_arnoldi_steps(systems, name, restart):
    """maxiter = the uncapped count converges in exactly that many steps; one fewer runs exactly one fewer.  Where no cycle started
    with a lowered tolerance that solve ends unconverged.  Where one did, the lowered tolerance aims a factor 4 (on the squares) below
    the weighted test, so the step before the last may meet the test already (the box of 0.04 with restart 20, the Peclet system):
    the verdict then agrees with the residual recomputed here, and the cases known to end unconverged are pinned."""
    A, b, S, _ = systems[name]
    _, free = gmres_dev_ref(A, b, restart=restart, reltol=RELTOL, weights=S)
    x1, at = gmres_dev_ref(A, b, restart=restart, reltol=RELTOL, weights=S, maxiter=free["iters"])
    assert at["converged"] and at["iters"] == free["iters"]
    x0, below = gmres_dev_ref(A, b, restart=restart, reltol=RELTOL, weights=S, maxiter=free["iters"] - 1)
    assert below["iters"] == free["iters"] - 1
    print(name, restart, "uncapped", free["iters"], "lowered", free["lowered"], "one fewer:", below["converged"], _wrel(A, b, S, x0))
    if free["lowered"] == 0 or (name, restart) in (("box", 5), ("box/10", 20), ("box/10", 5)):
        assert not below["converged"]
    if below["converged"]:
        assert _wrel(A, b, S, x0) <= 1.05 * RELTOL
    else:
        assert _wrel(A, b, S, x0) > RELTOL / 1.05
    for cap in (1, restart, restart + 1):
        _, info = gmres_dev_ref(A, b, restart=restart, reltol=0.0, weights=S, maxiter=cap)       # (no tolerance: the cap alone ends it)
        assert info["iters"] == cap and not info["converged"]


def test_zero_right_hand_side(systems):
    A, b, S, _ = systems["heat"]
    x, info = gmres_dev_ref(A, np.zeros_like(b), reltol=RELTOL, weights=S)
    assert info["converged"] and info["iters"] == 0 and info["cycles"] == 0 and np.all(x == 0.0)
    assert info["resnorm"] == 0.0 and info["bnorm"] == 0.0


@pytest.mark.parametrize("restart", [161, 200, 1000])
def test_restart_beyond_n_is_one_cycle(systems, restart):
    A, b, S, direct = systems["box"]
    n = len(b)
    x, info = gmres_dev_ref(A, b, restart=restart, reltol=RELTOL, weights=S)
    # (restart = 1000 is cut to 200 first, then to n = 161)
    assert info["converged"] and info["cycles"] <= 2 and info["iters"] <= n
    assert np.linalg.norm(x - direct) <= 1e-8 * np.linalg.norm(direct)
    # a full cycle of n steps on a tiny system: the Krylov space is the whole space, one cycle whatever the tolerance
    T = sp.diags([np.full(5, -1.0), np.linspace(2.0, 3.0, 6), np.full(5, -1.0)], [-1, 0, 1]).tocsr()
    rhs = np.arange(1.0, 7.0)
    xt, it = gmres_dev_ref(T, rhs, restart=200, reltol=1e-14)
    assert it["converged"] and it["cycles"] == 1 and it["iters"] <= 6
    assert np.allclose(xt, spla.spsolve(T.tocsc(), rhs), rtol=1e-12)


def test_abstol_alone_decides(systems):
    """reltol = 0: accepted exactly when ||S r|| <= abstol -- the cycle-by-cycle weighted residuals of a run without tolerance
    (maxiter = k restart) are the record; the solve with abstol ends at the first of them that meets it."""
    A, b, S, _ = systems["heat"]
    restart = 5
    record = []
    for k in range(1, 9):
        x, info = gmres_dev_ref(A, b, restart=restart, reltol=0.0, abstol=0.0, weights=S, maxiter=k * restart)
        record.append(np.linalg.norm(S * (b - A @ x)))
    assert record[-1] < record[0]
    for abstol in (1.0001 * record[2], 0.9999 * record[2], 1.0001 * record[5]):
        x, info = gmres_dev_ref(A, b, restart=restart, reltol=0.0, abstol=abstol, weights=S)
        res = np.linalg.norm(S * (b - A @ x))
        assert info["converged"] and res <= abstol * (1 + 1e-12) and abs(info["resnorm"] - res) <= 1e-9 * res
        # no earlier restart of the same iteration met it (the lowered inner tolerance may end the last cycle early: <=)
        full = (info["iters"] - 1) // restart
        assert all(r > abstol for r in record[:full]), (abstol, record, info)
    loose, tight = (gmres_dev_ref(A, b, restart=restart, reltol=0.0, abstol=a, weights=S)[1]["iters"] for a in (record[1], record[6]))
    assert loose < tight


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_not_finite_right_hand_side_is_never_converged(systems, bad):
    A, b, S, _ = systems["heat"]
    bb = b.copy()
    bb[len(b) // 2] = bad
    x, info = gmres_dev_ref(A, bb, reltol=RELTOL, weights=S, maxiter=40)
    assert not info["converged"] and info["notfinite"] and not info["singular"] and info["iters"] == 0
    assert np.all(x == 0.0)


def test_not_finite_matrix_is_never_converged(systems):
    """A NaN that enters with the first product: caught at the step (h1 + h2, ||w||^2), x = 0."""
    A, b, S, _ = systems["heat"]
    An = A.copy().tolil()
    An[3, 3] = np.nan
    x, info = gmres_dev_ref(An.tocsr(), b, reltol=RELTOL, weights=S, maxiter=40)
    assert not info["converged"] and info["notfinite"] and info["iters"] == 1 and np.all(x == 0.0)


def test_singular_and_exhausted():
    """A v_0 = 0 (d = 0 at j = 0): singular, no column kept, x = 0 and unconverged.  An eigenvector as right-hand side: the Krylov
    space is exhausted at the first step (hn = 0 up to rounding) and the solve is exact."""
    Z = sp.csr_matrix((4, 4))
    x, info = gmres_dev_ref(Z, np.ones(4), reltol=1e-12)
    assert info["singular"] and not info["converged"] and info["iters"] == 1 and np.all(x == 0.0)
    D = sp.diags([2.0, 4.0, 8.0, 16.0]).tocsr()
    x, info = gmres_dev_ref(D, np.array([0.0, 1.0, 0.0, 0.0]), reltol=1e-12)
    assert info["converged"] and info["exhausted"] and info["iters"] == 1 and np.array_equal(x, [0.0, 0.25, 0.0, 0.0])
