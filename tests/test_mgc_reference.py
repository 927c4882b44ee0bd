"""The cell-aggregated multigrid restatement (tests/mgc_reference.py) on the oracle's own reduced, border-rowed steady systems
with the cell blocks of csrc/pg_precond.hip folded in: Robin, Neumann and Dirichlet interfaces.  The preconditioned solve ends
at the direct solve, the first Galerkin product has a positive diagonal, and the kind-separated aggregates of "mg" are refused on
the Robin system -- which is why the cell rule exists.  The enum value and the option's name are pinned without a GPU."""
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import penguin_oracle as po
from oracle.geometry import Ball

from tests import mg_reference as mg
from tests import mgc_reference as mgc
from tests.common import rel_l2

ROOT = Path(__file__).resolve().parent.parent
ONE = lambda x, y=0.0, z=0.0: 1.0
_BORDERS_2D = ("left", "right", "top", "bottom")


def overwritten_border_cells(mesh, borders):
    """linear cells whose bulk row a border condition overwrites (po._apply_border: Dirichlet and Periodic; Neumann in 1-D)"""
    out = []
    for ci, _ in mesh.border_cells:
        cond = borders.get(po.classify_boundary_cell_fast(ci, mesh))
        if isinstance(cond, (po.Dirichlet, po.Periodic)) or (isinstance(cond, po.Neumann) and mesh.N == 1):
            out.append(po.lin_index(mesh.ext, ci))
    return out


def _system(N, n, radius, complement, border_keys, bc_i):
    mesh = po.Mesh((n,) * N, (4.0,) * N, (0.0,) * N)
    cap = po.make_capacity(Ball((2.01,) * N, radius, complement=complement), mesh)
    ph = po.Phase(cap, po.make_diffusion_ops(cap), ONE, ONE)
    borders = {k: po.Dirichlet(0.0) for k in border_keys}
    s = po.DiffusionSteadyMono(ph, po.BorderConditions(borders), bc_i)
    Ar, br, idx = po.remove_zero_rows_cols(s.A, s.b)
    M = (n + 1) ** N
    Ahat, ds, Binv = mgc.cell_blocks(Ar, idx, M, overwritten_border_cells(mesh, borders))
    return {"Ar": Ar, "br": br, "idx": idx, "Ahat": Ahat, "ds": ds, "bhat": Binv @ (ds * br), "ext": (n + 1,) * N, "M": M}


SYSTEMS = {
    "robin-out": lambda n: _system(2, n, 0.5, True, _BORDERS_2D, po.Robin(1.0, 1.0, 0.0)),
    "robin-in": lambda n: _system(2, n, 1.0, False, (), po.Robin(1.0, 1.0, 0.0)),
    "neumann-out": lambda n: _system(2, n, 0.5, True, _BORDERS_2D, po.Neumann(0.0)),
    "dirichlet-out": lambda n: _system(2, n, 0.5, True, _BORDERS_2D, po.Dirichlet(0.0)),
    "robin-sphere": lambda n: _system(3, n, 1.0, False, (), po.Robin(1.0, 1.0, 0.0)),
}
_CACHE, _RUNS = {}, {}


def system(name, n):
    if (name, n) not in _CACHE:
        _CACHE[(name, n)] = SYSTEMS[name](n)
    return _CACHE[(name, n)]


def _run(name, n, precond=True):
    key = (name, n, precond)
    if key not in _RUNS:
        sy = system(name, n)
        M = mgc.VCycle(mgc.build_hierarchy_cells(sy["Ahat"], sy["ds"], sy["idx"], sy["ext"])) if precond else None
        y, napp, _ = mgc.bicgstab_right(sy["Ahat"], sy["bhat"], M, reltol=1e-12)
        direct = spla.spsolve(sp.csc_matrix(sy["Ar"]), sy["br"])
        _RUNS[key] = (rel_l2(sy["ds"] * y, direct), napp)
    return _RUNS[key]


CASES = [("robin-out", 32), ("robin-out", 64), ("robin-out", 128), ("robin-in", 32), ("robin-in", 64), ("neumann-out", 32),
         ("neumann-out", 64), ("dirichlet-out", 32), ("dirichlet-out", 64), ("robin-sphere", 16)]


# applications of Â of the prototype this preconditioner was proposed with (DESIGN.md section 15 has its table)
PROTOTYPE = {("robin-out", 32): 28, ("robin-out", 64): 35, ("robin-out", 128): 50, ("robin-in", 32): 21, ("robin-in", 64): 31,
             ("neumann-out", 32): 37, ("neumann-out", 64): 46, ("dirichlet-out", 32): 20, ("dirichlet-out", 64): 24,
             ("robin-sphere", 16): 19}


@pytest.mark.parametrize("name,n", CASES)
def test_preconditioned_solve_ends_at_the_direct_solve(name, n):
    """... and takes the prototype's applications, give or take 4: BiCGStab's count moves by an iteration or two with the order of
    the sums in another BLAS."""
    err, napp = _run(name, n)
    print(f"{name} {n}: {napp} applications (prototype {PROTOTYPE[(name, n)]}), rel L2 {err:.2e}")
    assert err <= 1e-10
    assert abs(napp - PROTOTYPE[(name, n)]) <= 4


def test_the_cell_blocks_leave_a_unit_diagonal_and_the_same_solution():
    sy = system("robin-out", 32)
    assert np.allclose(sy["Ahat"].diagonal(), 1.0, rtol=0, atol=1e-12)
    y = spla.spsolve(sp.csc_matrix(sy["Ahat"]), sy["bhat"])
    direct = spla.spsolve(sp.csc_matrix(sy["Ar"]), sy["br"])
    assert rel_l2(sy["ds"] * y, direct) <= 1e-10


@pytest.mark.parametrize("name,n", [("robin-out", 32), ("robin-in", 32), ("neumann-out", 32), ("dirichlet-out", 32), ("robin-sphere", 16)])
def test_level_one_has_a_positive_diagonal_and_one_unknown_per_coarse_cell(name, n):
    sy = system(name, n)
    H = mgc.build_hierarchy_cells(sy["Ahat"], sy["ds"], sy["idx"], sy["ext"])
    assert len(H.levels) >= 2
    l0, l1 = H.levels[0], H.levels[1]
    assert np.all(l1.A.diagonal() > 0.0)
    # ω and γ of a cell share their coarse unknown; coarse unknowns are numbered by coarse cell
    cell = sy["idx"] % sy["M"]
    e0, e1 = sy["ext"][0], sy["ext"][1] if len(sy["ext"]) > 1 else 1
    c0, c1 = (e0 + 1) >> 1, (e1 + 1) >> 1
    i, j, k = cell % e0, (cell // e0) % e1, cell // (e0 * e1)
    assert np.array_equal(l1.key[l0.agg], (i >> 1) + (j >> 1) * c0 + (k >> 1) * c0 * c1)
    assert np.all(np.diff(l1.key) > 0)
    assert np.any(sy["idx"] >= sy["M"])                            # (there are interface unknowns among the children)


@pytest.mark.parametrize("name,n", [("robin-out", 64), ("robin-in", 32), ("neumann-out", 32)])
def test_the_kind_rule_is_refused_on_the_robin_system(name, n):
    """Why the feature exists: with γ rows that are equations of their own, a coarse space of γ unknowns alone has a non-positive
    Galerkin diagonal.  (Robin outside the disc at 32^2 is the one 2-D system of the table on which the kind rule happens to
    build; at 64^2 and 128^2 it does not.)"""
    sy = system(name, n)
    with pytest.raises(ValueError, match="coarse diagonal entry is not positive"):
        mg.build_hierarchy(sy["Ahat"], sy["ds"], sy["idx"], sy["ext"])
    mgc.build_hierarchy_cells(sy["Ahat"], sy["ds"], sy["idx"], sy["ext"])


def test_it_is_a_preconditioner_on_the_robin_system():
    plain, with_mg = _run("robin-out", 128, precond=False)[1], _run("robin-out", 128)[1]
    print(f"128^2 Robin outside the disc: plain {plain}, cell-aggregated multigrid {with_mg}")
    assert 4 * with_mg <= plain


def test_the_enum_value_is_minus_three_and_the_header_agrees():
    from penguin.jl_amd import _lib as L

    assert L.PG_PRECOND_MG_CELL == -3
    hdr = (ROOT / "include" / "penguin_hip.h").read_text(encoding="utf-8")
    m = re.search(r"enum\s*\{\s*PG_PRECOND_MG_CELL\s*=\s*(-?\d+)\s*\}", hdr)
    assert m and int(m.group(1)) == L.PG_PRECOND_MG_CELL
    assert L.PG_PRECOND_MG == -2


def test_the_option_name_parses():
    from penguin.jl_amd import _lib as L
    from penguin.jl_amd import api

    assert api._precond_value("mg-cell") == L.PG_PRECOND_MG_CELL
    assert api._precond_value("MG-cell") == L.PG_PRECOND_MG_CELL
    assert api._precond_value("mg") == L.PG_PRECOND_MG
    assert api._precond_value(6) == 6 and api._precond_value(-1) == -1
    assert api._krylov_opts("bicgstab", {"precond": "mg-cell"}).precond == -3
    with pytest.raises(ValueError):
        api._precond_value("amg")
