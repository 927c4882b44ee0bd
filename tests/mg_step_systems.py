"""The oracle's unsteady systems precond="mg-step" is measured on, as the Krylov loop sees them (Â = B⁻¹ S A S): the builders of
tests/specest_systems.py with the step as an argument, Δt = ratio · h², and the padded extents the hierarchy needs.  Shared by
tests/test_mg_step_reference.py and the GPU tests; nothing here needs a GPU.

  mono     box 4 x 4, fluid outside the disc r = 1 at (2.01, 2.01), four Dirichlet(0) borders, T = 1 at t = 0
  diph     box 8 x 8, the disc r = 2 at the centre and its complement, ScalarJump(1, He, 0), FluxJump(1, 1, 0), no borders
           (tests/specest_systems.py::diph; `kind` is (He, D2))
  sphere   box 4^3, fluid inside the sphere r = 1 at (2.01, 2.01, 2.01), no borders (tests/test_mgc_reference.py "robin-sphere")
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import penguin_oracle as po
from oracle.geometry import Ball

from tests import mg_reference as mg
from tests import mgc_reference as mgc
from tests.common import rel_l2
from tests.specest_systems import BORDERS_2D, ZERO, _finish, const, overwritten_border_cells


def bc_of(kind):
    return {"dirichlet": po.Dirichlet(1.0), "robin": po.Robin(1.0, 1.0, 1.0), "neumann": po.Neumann(0.0)}[kind]


def mono(n, scheme, kind, ratio):
    mesh = po.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = po.make_capacity(Ball((2.01, 2.01), 1.0, complement=True), mesh)
    ph = po.Phase(cap, po.make_diffusion_ops(cap), ZERO, const(1.0))
    borders = {k: po.Dirichlet(0.0) for k in BORDERS_2D}
    M = (n + 1) ** 2
    s = po.DiffusionUnsteadyMono(ph, po.BorderConditions(borders), bc_of(kind), ratio * (4.0 / n) ** 2, np.ones(2 * M), scheme)
    sy = _finish(s, M, overwritten_border_cells(mesh, borders))
    sy["ext"] = (n + 1, n + 1)
    return sy


def sphere(n, scheme, kind, ratio):
    mesh = po.Mesh((n,) * 3, (4.0,) * 3, (0.0,) * 3)
    cap = po.make_capacity(Ball((2.01,) * 3, 1.0), mesh)
    ph = po.Phase(cap, po.make_diffusion_ops(cap), ZERO, const(1.0))
    M = (n + 1) ** 3
    s = po.DiffusionUnsteadyMono(ph, po.BorderConditions({}), bc_of(kind), ratio * (4.0 / n) ** 2, np.ones(2 * M), scheme)
    sy = _finish(s, M, [])
    sy["ext"] = (n + 1,) * 3
    return sy


def diph(n, scheme, kind, ratio):
    He, D2 = kind
    mesh = po.Mesh((n, n), (8.0, 8.0), (0.0, 0.0))
    c1 = po.make_capacity(Ball((4.0, 4.0), 2.0), mesh)
    c2 = po.make_capacity(Ball((4.0, 4.0), 2.0, complement=True), mesh)
    p1 = po.Phase(c1, po.make_diffusion_ops(c1), ZERO, const(1.0))
    p2 = po.Phase(c2, po.make_diffusion_ops(c2), ZERO, const(D2))
    ic = po.InterfaceConditions(po.ScalarJump(1.0, He, 0.0), po.FluxJump(1.0, 1.0, 0.0))
    M = (n + 1) ** 2
    u0 = np.concatenate([np.ones(M), np.ones(M), np.zeros(M), np.zeros(M)])
    sy = _finish(po.DiffusionUnsteadyDiph(p1, p2, po.BorderConditions({}), ic, ratio * (8.0 / n) ** 2, u0, scheme), M, [])
    sy["ext"] = (n + 1, n + 1)
    return sy


_CACHE, _RUNS = {}, {}


def system(family, n, scheme, kind, ratio):
    key = (family, n, scheme, kind, ratio)
    if key not in _CACHE:
        _CACHE[key] = {"mono": mono, "sphere": sphere, "diph": diph}[family](n, scheme, kind, ratio)
    return _CACHE[key]


def run(family, n, scheme, kind, ratio, precond=True):
    """BiCGStab from zero to reltol 1e-12 on Â, with the cell rule's V-cycle or plain: (rel L2 against spsolve, applications of Â).
    Computed once per case and kept."""
    key = (family, n, scheme, kind, ratio, precond)
    if key not in _RUNS:
        sy = system(family, n, scheme, kind, ratio)
        M = mg.VCycle(mgc.build_hierarchy_cells(sy["Ahat"], sy["ds"], sy["idx"], sy["ext"])) if precond else None
        y, napp, _ = mg.bicgstab_right(sp.csr_matrix(sy["Ahat"]), sy["bhat"], M, reltol=1e-12)
        direct = spla.spsolve(sp.csc_matrix(sy["Ar"]), sy["br"])
        _RUNS[key] = (rel_l2(sy["ds"] * y, direct), napp)
    return _RUNS[key]
