"""The numpy restatement of IDR(s) (tests/idrs_reference.py) -- the definition the GPU tests of pg_idrs.hip compare with -- on the
oracle's systems: the direct solve for s = 1, 2, 4, 8, the product counts at cell Peclet number 12.5, the honest flag of IDR(1),
more shadow vectors than unknowns, the counting rules, the start from an x0 and the routing of the Python options."""
import json
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import penguin_oracle as po
from oracle.geometry import Ball
from tests.idrs_reference import MAX_RESTARTS, idrs_ref, lower_solve, peclet_system, shadow

GOLDEN = Path(__file__).parent / "golden" / "idrs_products.json"
RELTOL = 1e-12


def _heat(scheme, n=24):
    mesh = po.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = po.make_capacity(Ball((2.01, 2.01), 1.0), mesh)
    M = (n + 1) ** 2
    ph = po.Phase(cap, po.make_diffusion_ops(cap), lambda x, y, z, t: 0.0, lambda x, y, z: 1.0)
    bcb = po.BorderConditions({k: po.Dirichlet(0.0) for k in ("left", "right", "top", "bottom")})
    s = po.DiffusionUnsteadyMono(ph, bcb, po.Dirichlet(1.0), 0.25 * (4.0 / n) ** 2, np.concatenate([np.zeros(M), np.ones(M)]), scheme)
    A, b, _ = po.remove_zero_rows_cols(s.A, s.b)
    return A.tocsr(), b


def _poisson(n=24):
    mesh = po.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = po.make_capacity(Ball((2.0, 2.0), 1.0), mesh)
    ph = po.Phase(cap, po.make_diffusion_ops(cap), lambda x, y, z, t=0.0: 4.0, lambda x, y, z: 1.0)
    s = po.DiffusionSteadyMono(ph, po.BorderConditions({}), po.Dirichlet(0.0))
    A, b, _ = po.remove_zero_rows_cols(s.A, s.b)
    return A.tocsr(), b


_made = {}


def _system(name):
    """(A, b, direct solve), made once and shared (read only)."""
    if name not in _made:
        A, b = {"heat-BE": lambda: _heat("BE"), "heat-CN": lambda: _heat("CN"), "poisson": _poisson,
                "uniform": lambda: peclet_system(32, "uniform"), "rotation": lambda: peclet_system(32, "rotation")}[name]()
        _made[name] = (A, b, spla.spsolve(A.tocsc(), b))
    return _made[name]


CASES = [(name, s) for name in ("heat-BE", "heat-CN", "poisson", "uniform", "rotation") for s in (2, 4, 8)] + [("rotation", 1)]


@pytest.mark.parametrize("name,s", CASES)
def test_matches_the_direct_solve(name, s):
    A, b, x_direct = _system(name)
    x, info = idrs_ref(A, b, s=s, reltol=RELTOL)
    print(name, s, {k: info[k] for k in ("iters", "products", "confirmations", "restarts")})
    assert info["converged"] and info["confirmations"] + info["restarts"] >= 1
    assert info["products"] == info["iters"] + info["restarts"] + info["confirmations"]
    assert np.linalg.norm(x - x_direct) <= 1e-10 * np.linalg.norm(x_direct)
    assert info["resnorm"] <= RELTOL * info["bnorm"]
    assert np.linalg.norm(b - A @ x) == pytest.approx(info["resnorm"], rel=1e-6)     # the TRUE residual is what is reported


def test_idr1_on_the_uniform_flow_ends_unconverged_with_a_finite_state():
    """IDR(1) stagnates on the uniform-flow system at cell Peclet number 12.5: it breaks down, restarts from the true residual
    MAX_RESTARTS times and gives up -- a finite state and an honest flag."""
    A, b, _ = _system("uniform")
    x, info = idrs_ref(A, b, s=1, reltol=RELTOL)
    true = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    print(info, true)
    assert np.all(np.isfinite(x))
    assert not info["converged"] and true > RELTOL and info["restarts"] == MAX_RESTARTS + 1 and not info["singular"]


def test_more_shadow_vectors_than_unknowns():
    """6 unknowns, s = 8: after six updates the residual is orthogonal to six independent shadow vectors, i.e. zero to rounding;
    the solve ends converged through a true residual (a confirmation or a restart), never through NaN."""
    rng = np.random.default_rng(1)
    A = sp.csr_matrix(4.0 * np.eye(6) + rng.normal(size=(6, 6)))
    b = rng.normal(size=6)
    x, info = idrs_ref(A, b, s=8, reltol=RELTOL)
    assert info["converged"] and np.all(np.isfinite(x)) and info["iters"] <= 8
    assert info["confirmations"] + info["restarts"] >= 1
    assert np.linalg.norm(b - A @ x) <= 1e-12 * np.linalg.norm(b)
    # a singular matrix: the state stays finite and the flag honest
    x, info = idrs_ref(sp.csr_matrix(np.zeros((6, 6))), b, s=8, reltol=RELTOL)
    assert not info["converged"] and np.all(np.isfinite(x))


def test_counting_caps_and_refusals():
    A, b, _ = _system("heat-BE")
    for s, cap in ((2, 3), (2, 4), (4, 5), (8, 1)):
        x, info = idrs_ref(A, b, s=s, reltol=RELTOL, maxiter=cap)
        assert info["iters"] == cap and not info["converged"] and info["products"] == cap and np.all(np.isfinite(x))
    with pytest.raises(ValueError):
        idrs_ref(A, b, s=9)
    x0, info0 = idrs_ref(A, 0.0 * b, s=4)
    assert info0["converged"] and info0["iters"] == 0 and np.all(x0 == 0.0)
    _, i8 = idrs_ref(A, b, s=0, reltol=RELTOL)
    _, j8 = idrs_ref(A, b, s=8, reltol=RELTOL)
    assert i8["products"] == j8["products"]          # s <= 0 means 8


def test_start_from_x0():
    A, b, x_direct = _system("poisson")
    x, cold = idrs_ref(A, b, s=4, reltol=RELTOL)
    y, again = idrs_ref(A, b, s=4, reltol=RELTOL, x0=x)
    assert again["converged"] and again["products"] == 1 and again["iters"] == 0 and np.array_equal(x, y)
    z, warm = idrs_ref(A, b, s=4, reltol=RELTOL, x0=x_direct * (1.0 + 1e-6))
    assert warm["converged"] and warm["products"] < cold["products"]
    assert warm["products"] == warm["iters"] + warm["restarts"] + warm["confirmations"] + 1
    assert np.linalg.norm(z - x_direct) <= 1e-10 * np.linalg.norm(x_direct)


def test_products_at_cell_peclet_12():
    """The recorded counts (tests/golden/make_idrs_products.py): IDR(4) and IDR(8) need fewer products than BiCGStab on both
    flows, and the counts move under a one-ulp perturbation of b -- which is why no test compares total counts of the device
    with the restatement's."""
    golden = json.loads(GOLDEN.read_text())
    for kind in ("rotation", "uniform"):
        g = golden[kind]
        A, b, _ = _system(kind)
        for s in (4, 8):
            _, info = idrs_ref(A, b, s=s, reltol=RELTOL)
            print(kind, s, info["products"], "golden", g[f"idrs{s}"], "one ulp", g[f"idrs{s}_one_ulp"], "BiCGStab", g["bicgstab"])
            assert info["converged"] and info["products"] < g["bicgstab"]
            assert g[f"idrs{s}_converged"] and g[f"idrs{s}"] < g["bicgstab"] and g[f"idrs{s}_one_ulp"] < g["bicgstab"]
        assert not golden["uniform"]["idrs1_converged"]
    moved = [abs(golden[k][f"idrs{s}"] - golden[k][f"idrs{s}_one_ulp"]) for k in ("rotation", "uniform") for s in (2, 4, 8)]
    assert max(moved) >= 1


def test_shadow_values_are_exact_and_lower_solve_refuses_what_is_not_finite():
    i = np.arange(4096)
    for k in range(8):
        p = shadow(i, k)
        assert p.dtype == np.float64 and np.all(p >= -1.0) and np.all(p < 1.0)
        assert np.all(p * 2.0 ** 52 == np.round(p * 2.0 ** 52))                       # multiples of 2^-52: exact in fp64
        assert abs(p.mean()) < 0.05 and abs(np.mean(p * p) - 1.0 / 3.0) < 0.02
    assert shadow(0, 0) != shadow(0, 1) and shadow(1, 0) != shadow(0, 0)
    rng = np.random.default_rng(5)
    M = np.tril(rng.normal(size=(8, 8))) + 4.0 * np.eye(8)
    rhs = rng.normal(size=8)
    out, ok = lower_solve(M, 2, 8, rhs)
    assert ok and np.all(out[:2] == 0.0) and np.allclose(M[2:, 2:] @ out[2:], rhs[2:], rtol=1e-12)
    M[5, 5] = 0.0
    out, ok = lower_solve(M, 2, 8, rhs)
    assert not ok and np.all(out == 0.0)
    out, ok = lower_solve(M, 0, 5, rhs)
    assert ok and np.all(out[5:] == 0.0)


def test_python_options_nshadow_opts_in_and_maxiter_is_passed_unchanged():
    """method="idrs" selects PG_METHOD_IDRS only with the keyword nshadow (which travels in `restart`); the bare name keeps mapping
    to BiCGStab; maxiter is passed unchanged (its unit is one product).  No GPU: the options struct only."""
    from penguin.jl_amd import _lib as L
    from penguin.jl_amd.api import _krylov_opts

    def idrs():   # stands in for IterativeSolvers.idrs: only the name crosses the boundary
        raise AssertionError
    assert L.PG_METHOD_IDRS == 4 and L.PG_METHOD.get("idrs", L.PG_METHOD["bicgstab"]) == 0
    o = _krylov_opts("idrs", dict(nshadow=4, maxiter=200, max_mv_products=50))
    assert (o.method, o.restart, o.maxiter) == (4, 4, 200)
    o = _krylov_opts(idrs, dict(nshadow=8, max_mv_products=50))
    assert (o.method, o.restart, o.maxiter) == (4, 8, 0)
    o = _krylov_opts("idrs", dict(nshadow=0))
    assert (o.method, o.restart) == (4, 0)
    for bare in ("idrs", idrs):
        o = _krylov_opts(bare, dict(maxiter=7, restart=5))
        assert (o.method, o.restart, o.maxiter) == (L.PG_METHOD["bicgstab"], 5, 7)
    assert _krylov_opts("bicgstabl", dict(l=2, nshadow=4)).method == L.PG_METHOD["bicgstabl"]
    assert _krylov_opts("gmres", dict(nshadow=4)).method == L.PG_METHOD["gmres"]


def test_header_and_python_agree_on_the_method_value():
    header = (Path(__file__).resolve().parents[1] / "include" / "penguin_hip.h").read_text()
    assert "PG_METHOD_IDRS = 4" in header and "src/solver.jl:158-188" in header
