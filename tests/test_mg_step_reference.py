"""precond="mg-step" (PG_PRECOND_MG_STEP) without a GPU: the restatement of the cell-aggregated V-cycle (tests/mgc_reference.py) as
right preconditioner of BiCGStab on the oracle's UNSTEADY systems, at steps of the order of h² and far above it.  The
preconditioned solve ends at the direct solve, needs at most a third of the plain loop's applications at Δt = 64 h², and the one
system of the family whose first Galerkin product has a non-positive diagonal entry is refused.  The enum value and the option's
name are pinned.

Measured when this file was written (applications of Â, plain -> preconditioned, and the rel L2 error of the preconditioned run)
stand in CASES below."""
import re
from pathlib import Path

import pytest

from tests import mgc_reference as mgc
from tests.mg_step_systems import run, system

ROOT = Path(__file__).resolve().parent.parent

# (family, n, scheme, interface condition, Δt / h²)
CASES = [
    ("mono", 32, "BE", "dirichlet", 1),
    ("mono", 32, "BE", "dirichlet", 64),
    ("mono", 32, "CN", "dirichlet", 1),
    ("mono", 32, "CN", "dirichlet", 64),
    ("mono", 32, "CN", "robin", 64),
    ("mono", 32, "CN", "neumann", 64),
    ("sphere", 12, "CN", "robin", 64),
]


@pytest.mark.parametrize("family,n,scheme,kind,ratio", CASES)
def test_preconditioned_solve_ends_at_the_direct_solve(family, n, scheme, kind, ratio):
    err, napp = run(family, n, scheme, kind, ratio)
    print(f"{family} {n} {scheme} {kind} dt/h2 = {ratio}: {napp} applications, rel L2 {err:.2e}")
    assert err <= 1e-10


@pytest.mark.parametrize("family,n,scheme,kind,ratio", [c for c in CASES if c[0] == "mono" and c[4] == 64])
def test_a_third_of_the_plain_applications_at_a_large_step(family, n, scheme, kind, ratio):
    napp = run(family, n, scheme, kind, ratio)[1]
    plain_err, plain = run(family, n, scheme, kind, ratio, precond=False)
    print(f"{family} {n} {scheme} {kind} dt/h2 = {ratio}: plain {plain} (rel L2 {plain_err:.2e}), V-cycle {napp}")
    assert 3 * napp <= plain


def test_robin_be_at_a_small_step_is_refused():
    """Backward Euler leaves the Robin interface rows without a mass term; at Δt = h² the first coarsening of the cell rule meets
    a coarse diagonal entry that is not positive.  The library refuses such a solve (tests/test_gpu_mg_step.py)."""
    sy = system("mono", 32, "BE", "robin", 1)
    with pytest.raises(ValueError, match="coarse diagonal entry is not positive"):
        mgc.build_hierarchy_cells(sy["Ahat"], sy["ds"], sy["idx"], sy["ext"])


def test_the_enum_value_is_minus_five_and_the_header_agrees():
    from penguin.jl_amd import _lib as L

    assert L.PG_PRECOND_MG_STEP == -5
    hdr = (ROOT / "include" / "penguin_hip.h").read_text(encoding="utf-8")
    m = re.search(r"enum\s*\{\s*PG_PRECOND_MG_STEP\s*=\s*(-?\d+)\s*\}", hdr)
    assert m and int(m.group(1)) == L.PG_PRECOND_MG_STEP
    jl = (ROOT / "julia" / "PenguinHIP.jl").read_text(encoding="utf-8")
    m = re.search(r"const PG_PRECOND_MG_STEP = Int32\((-?\d+)\)", jl)
    assert m and int(m.group(1)) == L.PG_PRECOND_MG_STEP
    assert (L.PG_PRECOND_MG, L.PG_PRECOND_MG_CELL, L.PG_PRECOND_POLY_EST) == (-2, -3, -4)


def test_the_option_name_parses():
    from penguin.jl_amd import _lib as L
    from penguin.jl_amd import api

    assert api._precond_value("mg-step") == L.PG_PRECOND_MG_STEP
    assert api._precond_value("MG-Step") == L.PG_PRECOND_MG_STEP
    assert api._precond_value("mg") == L.PG_PRECOND_MG and api._precond_value("mg-cell") == L.PG_PRECOND_MG_CELL
    assert api._precond_value(-5) == -5
    assert api._krylov_opts("bicgstab", {"precond": "mg-step"}).precond == -5
    with pytest.raises(ValueError):
        api._precond_value("mg-steps")
