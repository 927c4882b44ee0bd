"""The oracle's systems the spectral estimate (precond="poly-est") is measured on, as the Krylov loop sees them: Â = B⁻¹ S A S of
the reduced matrix (tests/mgc_reference.cell_blocks follows csrc/pg_precond.hip).  Shared by tests/test_specest_reference.py and
the GPU tests; nothing here needs a GPU.

  diph   benchmark/Heat_2ph_2D.jl family (config 5): box 8^N, ball r = 2 at the centre and its complement, ScalarJump(1, He, 0),
         FluxJump(1, 1, 0), no borders, Δt = 0.5 h²
  mono   box 4 x 4, fluid outside the disc r = 1 at (2.01, 2.01), four Dirichlet(0) borders, Δt = 0.5 h², T = 1 at t = 0
"""
from __future__ import annotations

import numpy as np

from oracle import penguin_oracle as po
from oracle.geometry import Ball

from tests import mgc_reference as mgc

ZERO = lambda x, y=0.0, z=0.0, t=0.0: 0.0
BORDERS_2D = ("left", "right", "top", "bottom")


def const(v):
    return lambda x, y=0.0, z=0.0: v


def overwritten_border_cells(mesh, borders):
    out = []
    for ci, _ in mesh.border_cells:
        cond = borders.get(po.classify_boundary_cell_fast(ci, mesh))
        if isinstance(cond, (po.Dirichlet, po.Periodic)) or (isinstance(cond, po.Neumann) and mesh.N == 1):
            out.append(po.lin_index(mesh.ext, ci))
    return out


def _finish(s, M, border_cells):
    Ar, br, idx = po.remove_zero_rows_cols(s.A, s.b)
    Ahat, ds, Binv = mgc.cell_blocks(Ar, idx, M, border_cells)
    return {"Ar": Ar, "br": br, "idx": idx, "Ahat": Ahat, "ds": ds, "bhat": Binv @ (ds * br), "M": M}


def diph(n, scheme, He=1.0, D2=1.0, N=2):
    mesh = po.Mesh((n,) * N, (8.0,) * N, (0.0,) * N)
    c1 = po.make_capacity(Ball((4.0,) * N, 2.0), mesh)
    c2 = po.make_capacity(Ball((4.0,) * N, 2.0, complement=True), mesh)
    p1 = po.Phase(c1, po.make_diffusion_ops(c1), ZERO, const(1.0))
    p2 = po.Phase(c2, po.make_diffusion_ops(c2), ZERO, const(D2))
    ic = po.InterfaceConditions(po.ScalarJump(1.0, He, 0.0), po.FluxJump(1.0, 1.0, 0.0))
    M = (n + 1) ** N
    u0 = np.concatenate([np.ones(M), np.ones(M), np.zeros(M), np.zeros(M)])
    dt = 0.5 * (8.0 / n) ** 2
    return _finish(po.DiffusionUnsteadyDiph(p1, p2, po.BorderConditions({}), ic, dt, u0, scheme), M, [])


def mono(n, scheme, bc_i):
    """scheme None: the steady system"""
    mesh = po.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = po.make_capacity(Ball((2.01, 2.01), 1.0, complement=True), mesh)
    ph = po.Phase(cap, po.make_diffusion_ops(cap), ZERO, const(1.0))
    borders = {k: po.Dirichlet(0.0) for k in BORDERS_2D}
    M = (n + 1) ** 2
    if scheme is None:
        s = po.DiffusionSteadyMono(ph, po.BorderConditions(borders), bc_i)
    else:
        s = po.DiffusionUnsteadyMono(ph, po.BorderConditions(borders), bc_i, 0.5 * (4.0 / n) ** 2, np.ones(2 * M), scheme)
    return _finish(s, M, overwritten_border_cells(mesh, borders))


SYSTEMS = {
    "diph-be": lambda n: diph(n, "BE"),
    "diph-cn": lambda n: diph(n, "CN"),
    "diph-cn-c5": lambda n: diph(n, "CN", He=0.5, D2=2.0),        # the coefficients of the config-5 parity test
    "diph-cn-d10": lambda n: diph(n, "CN", He=0.5, D2=10.0),
    "robin-cn": lambda n: mono(n, "CN", po.Robin(1.0, 1.0, 1.0)),
    "neumann-be": lambda n: mono(n, "BE", po.Neumann(0.0)),
    "dirichlet-cn": lambda n: mono(n, "CN", po.Dirichlet(1.0)),
    "diph3-cn": lambda n: diph(n, "CN", N=3),
    "robin-steady": lambda n: mono(n, None, po.Robin(1.0, 1.0, 1.0)),
}
_CACHE = {}


def system(name, n):
    if (name, n) not in _CACHE:
        _CACHE[(name, n)] = SYSTEMS[name](n)
    return _CACHE[(name, n)]
