"""The numpy restatement of BiCGStab(l) (tests/bicgstabl_reference.py) -- the definition the GPU tests of pg_bicgstabl.hip compare
with -- on the oracle's systems: the direct solve, the plain BiCGStab restatement, the product counts at cell Peclet number 12.5
and the confirmation of the true residual."""
import json
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from oracle import penguin_oracle as po
from tests.bicgstabl_reference import bicgstabl_ref, heat_system, peclet_system, small_solve

GOLDEN = Path(__file__).parent / "golden" / "bicgstabl_products.json"


@pytest.fixture(scope="module")
def heat():
    A, b = heat_system(16)
    return A, b, spla.spsolve(A.tocsc(), b)


@pytest.mark.parametrize("l", [1, 2, 4])
def test_heat_system_matches_the_direct_solve(heat, l):
    A, b, x_direct = heat
    x, info = bicgstabl_ref(A, b, l=l, reltol=1e-13)
    assert info["converged"] and info["confirmations"] >= 1
    assert info["products"] == 2 * info["iters"] + info["confirmations"]
    assert np.linalg.norm(x - x_direct) <= 1e-10 * np.linalg.norm(x_direct)
    assert info["resnorm"] <= 1e-13 * info["bnorm"]
    assert np.linalg.norm(b - A @ x) == pytest.approx(info["resnorm"], rel=1e-6)     # the TRUE residual is what is reported


def test_l1_is_bicgstab(heat):
    """Mathematically the same method: iters within 2 of po.bicgstab_ref."""
    A, b, _ = heat
    _, it, _ = po.bicgstab_ref(A, b, reltol=1e-13)
    _, info = bicgstabl_ref(A, b, l=1, reltol=1e-13)
    assert abs(info["iters"] - it) <= 2, (info["iters"], it)


def test_counting_and_caps(heat):
    A, b, _ = heat
    x, info = bicgstabl_ref(A, b, l=2, reltol=1e-13, maxiter=3)     # the second outer iteration starts at iters = 2 < 3
    assert info["iters"] == 4 and not info["converged"] and info["confirmations"] == 0 and info["products"] == 8
    assert np.all(np.isfinite(x))
    with pytest.raises(ValueError):
        bicgstabl_ref(A, b, l=9)
    x0, info0 = bicgstabl_ref(A, 0.0 * b, l=2)
    assert info0["converged"] and info0["iters"] == 0 and np.all(x0 == 0.0)


def test_small_solve_pivots_and_shrinks():
    rng = np.random.default_rng(3)
    R = rng.normal(size=(5, 40))
    G = R @ R.T
    gamma, k = small_solve(G, 4)
    assert k == 4 and np.allclose(gamma[1:], np.linalg.solve(G[1:, 1:], G[1:, 0]), rtol=1e-10)
    R[3] = 2.0 * R[1] - R[2]                      # the third power depends on the first two: the leading 2 x 2 block is solved
    G = R @ R.T
    gamma, k = small_solve(G, 4)
    assert k == 2 and np.all(gamma[3:] == 0.0) and np.allclose(gamma[1:3], np.linalg.solve(G[1:3, 1:3], G[1:3, 0]), rtol=1e-10)
    R[1] = 0.0                                    # A r = 0: nothing safe
    gamma, k = small_solve(R @ R.T, 4)
    assert k == 0 and np.all(gamma == 0.0)
    G = np.full((3, 3), np.nan)
    assert small_solve(G, 2)[1] == 0


def test_products_at_cell_peclet_12():
    """The two 32^2 rows of the table at cell Peclet number 12.5 (rigid rotation of amplitude 100, uniform flow (100, 30)) on the
    oracle's systems: BiCGStab(2) needs no more products than po.bicgstab_ref, here and in the counts
    tests/golden/make_bicgstabl_products.py recorded.  Both 32^2 systems are well conditioned (cond 2e2).  The 64^2 rotating
    geometry is skipped here: its direct solve shows the near-singular solid-cell unknown of DESIGN.md section 13 (cond 3e16), on
    which plain BiCGStab itself leaves a true residual of 1e-2 -- test_confirmation_of_the_true_residual uses it instead.
    The BiCGStab(2) count on the uniform-flow row moves by a few products under a one-ulp perturbation of b (recorded as
    bicgstabl2_one_ulp): the GPU tests do not compare counts with the restatement at this Peclet number."""
    golden = json.loads(GOLDEN.read_text())
    for kind in ("rotation", "uniform"):
        A, b = peclet_system(32, kind)
        x_direct = spla.spsolve(A.tocsc(), b)
        _, it, _ = po.bicgstab_ref(A, b, reltol=1e-12, maxiter=50000)
        x, info = bicgstabl_ref(A, b, l=2, reltol=1e-12)
        print(kind, "BiCGStab products", 2 * it, "BiCGStab(2)", info["products"], "golden", golden[kind])
        assert info["converged"] and np.linalg.norm(x - x_direct) <= 1e-9 * np.linalg.norm(x_direct)
        assert info["products"] <= 2 * it
        # (the recorded counts are not compared digit for digit: the plain count on the rotating row is chaotic -- it moves by
        #  thousands with the rounding of the dot products -- and only the inequality is the claim)
        assert golden[kind]["bicgstabl2"] <= golden[kind]["bicgstab"] and golden[kind]["bicgstabl2_converged"]


def test_confirmation_of_the_true_residual():
    """64^2 rigid rotation of amplitude 100 (the near-singular system): with the recurrence residual believed (confirm=False) the
    iteration reports 1e-12 while the true residual is O(1e-2) or worse -- the gap the confirmation exists for.  With it, a solve
    reported converged has the true residual it reports, and one whose true residual keeps failing is reported unconverged after
    three continuations; the state is finite either way.  (No GPU-sized case of this gap is run on the device: the confirmation
    path is tested here only.)"""
    A, b = peclet_system(64, "rotation")
    bn = np.linalg.norm(b)
    gaps = 0
    for l in (1, 2):
        x, info = bicgstabl_ref(A, b, l=l, reltol=1e-12, maxiter=6000, confirm=False)
        true = np.linalg.norm(b - A @ x) / bn
        if info["converged"] and true > 1e-6:
            gaps += 1
        x, info = bicgstabl_ref(A, b, l=l, reltol=1e-12, maxiter=6000)
        true = np.linalg.norm(b - A @ x) / bn
        print("l", l, {k: info[k] for k in ("iters", "confirmations", "continues", "converged")}, "true", true)
        assert np.all(np.isfinite(x)) and info["continues"] <= 3
        if info["converged"]:
            assert true <= 1.001e-12 and info["resnorm"] <= 1e-12 * info["bnorm"]
        else:
            assert info["confirmations"] == 0 or info["resnorm"] > 1e-12 * info["bnorm"] or info["iters"] >= 6000
    assert gaps >= 1


def test_python_options_l_opts_in_and_max_mv_products_is_converted():
    """method="bicgstabl" selects PG_METHOD_BICGSTABL only with the keyword l (which travels in `restart`); the bare name keeps
    mapping to BiCGStab; max_mv_products becomes maxiter = max_mv_products // 2 (BiCG sub-steps, two products each) unless
    maxiter is given.  No GPU: the options struct only."""
    from penguin.jl_amd import _lib as L
    from penguin.jl_amd.api import _krylov_opts

    def bicgstabl():   # stands in for IterativeSolvers.bicgstabl: only the name crosses the boundary
        raise AssertionError
    assert L.PG_METHOD["bicgstabl"] == 3
    o = _krylov_opts("bicgstabl", dict(l=4, max_mv_products=200))
    assert (o.method, o.restart, o.maxiter) == (3, 4, 100)
    o = _krylov_opts(bicgstabl, dict(l=2))
    assert (o.method, o.restart, o.maxiter) == (3, 2, 0)
    for bare in ("bicgstabl", bicgstabl):
        o = _krylov_opts(bare, dict(max_mv_products=200, maxiter=7, restart=5))
        assert (o.method, o.restart, o.maxiter) == (L.PG_METHOD["bicgstab"], 5, 7)
    assert _krylov_opts("gmres", dict(restart=6)).method == L.PG_METHOD["gmres"]


def test_header_and_python_agree_on_the_method_value():
    header = (Path(__file__).resolve().parents[1] / "include" / "penguin_hip.h").read_text()
    assert "PG_METHOD_BICGSTABL = 3" in header
