"""The multigrid restatement (tests/mg_reference.py) on the oracle's own reduced, border-rowed, equilibrated steady systems:
it converges to the direct solve, it IS a preconditioner (a quarter of the plain applications at most), its count is nearly
independent of the mesh, and its level-0 transfer weights make P̂ᵀ Â P̂ the plain aggregation of the raw matrix."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import penguin_oracle as po
from oracle.geometry import Ball

from tests import mg_reference as mg
from tests.common import rel_l2


def _system(N, n, L, center, radius, complement, borders):
    mesh = po.Mesh((n,) * N, (L,) * N, (0.0,) * N)
    cap = po.make_capacity(Ball(center, radius, complement=complement), mesh)
    op = po.make_diffusion_ops(cap)
    ph = po.Phase(cap, op, lambda x, y=0.0, z=0.0: 1.0, lambda x, y=0.0, z=0.0: 1.0)
    bcb = po.BorderConditions({k: po.Dirichlet(0.0) for k in borders})
    s = po.DiffusionSteadyMono(ph, bcb, po.Dirichlet(0.0))
    Ar, br, idx = po.remove_zero_rows_cols(s.A, s.b)
    Ahat, ds = mg.equilibrate(Ar)
    return {"Ar": Ar, "br": br, "idx": idx, "Ahat": Ahat, "ds": ds, "bhat": ds * br, "ext": (n + 1,) * N}


_BORDERS_2D = ("left", "right", "top", "bottom")
_CACHE = {}


def outside_disc(n):
    if ("out", n) not in _CACHE:
        _CACHE[("out", n)] = _system(2, n, 4.0, (2.01, 2.01), 0.5, True, _BORDERS_2D)
    return _CACHE[("out", n)]


def inside_disc(n):
    if ("in", n) not in _CACHE:
        _CACHE[("in", n)] = _system(2, n, 4.0, (2.01, 2.01), 1.0, False, ())
    return _CACHE[("in", n)]


def sphere(n):
    if ("sph", n) not in _CACHE:
        _CACHE[("sph", n)] = _system(3, n, 4.0, (2.01, 2.01, 2.01), 1.0, False, ())
    return _CACHE[("sph", n)]


def _solve(sy, precond):
    M = mg.VCycle(mg.build_hierarchy(sy["Ahat"], sy["ds"], sy["idx"], sy["ext"])) if precond else None
    y, napp, _ = mg.bicgstab_right(sy["Ahat"], sy["bhat"], M, reltol=1e-12)
    return sy["ds"] * y, napp


_RUNS = {}


def _run(name, n, precond=True):
    key = (name, n, precond)
    if key not in _RUNS:
        sy = {"out": outside_disc, "in": inside_disc, "sph": sphere}[name](n)
        x, napp = _solve(sy, precond)
        direct = spla.spsolve(sp.csc_matrix(sy["Ar"]), sy["br"])
        _RUNS[key] = (rel_l2(x, direct), napp)
    return _RUNS[key]


@pytest.mark.parametrize("name,n", [("out", 32), ("out", 64), ("out", 128), ("in", 32), ("in", 64), ("in", 128), ("sph", 16)])
def test_preconditioned_solve_ends_at_the_direct_solve(name, n):
    err, napp = _run(name, n)
    print(f"{name} {n}: {napp} applications, rel L2 {err:.2e}")
    assert err <= 1e-10


def test_applications_at_128_are_bounded():
    assert _run("out", 128)[1] <= 60


def test_a_quarter_of_the_plain_applications_at_most():
    plain = _run("out", 128, precond=False)[1]
    with_mg = _run("out", 128)[1]
    print(f"128^2 outside disc: plain {plain}, multigrid {with_mg}")
    assert 4 * with_mg <= plain


def test_count_is_nearly_independent_of_the_mesh():
    assert _run("out", 128)[1] <= 2 * _run("out", 32)[1]


@pytest.mark.parametrize("name,n", [("out", 32), ("in", 32), ("sph", 16)])
def test_level_one_is_the_aggregation_of_the_raw_matrix(name, n):
    """P̂ᵀ Â P̂ with P̂ = S⁻¹ P equals Pᵀ A P of the un-equilibrated matrix, to rounding."""
    sy = {"out": outside_disc, "in": inside_disc, "sph": sphere}[name](n)
    H = mg.build_hierarchy(sy["Ahat"], sy["ds"], sy["idx"], sy["ext"])
    assert len(H.levels) >= 2
    agg, nf = H.levels[0].agg, sy["Ar"].shape[0]
    P = sp.csr_matrix((np.ones(nf), (np.arange(nf), agg)), shape=(nf, H.levels[1].A.shape[0]))
    raw = sp.csr_matrix(P.T @ sy["Ar"] @ P)
    bound = sp.csr_matrix(P.T @ abs(sp.csr_matrix(sy["Ar"])) @ P)
    diff = abs(H.levels[1].A - raw)
    assert diff.nnz == 0 or (diff - 1e-14 * bound).max() <= 0.0
    # kinds never mix, and coarse unknowns are numbered kind-major, then by coarse cell
    Mc = int(np.prod(H.levels[1].ext))
    assert np.all(np.diff(H.levels[1].key) > 0)
    M = int(np.prod(H.levels[0].ext))
    assert np.array_equal(H.levels[1].key[agg] // Mc, sy["idx"] // M)


def test_non_positive_diagonal_is_refused():
    sy = outside_disc(32)
    Ar = sp.lil_matrix(sy["Ar"])
    Ar[5, 5] = -Ar[5, 5]
    Ahat, ds = mg.equilibrate(sp.csr_matrix(Ar))
    with pytest.raises(ValueError, match="positive diagonal"):
        mg.build_hierarchy(Ahat, ds, sy["idx"], sy["ext"])
