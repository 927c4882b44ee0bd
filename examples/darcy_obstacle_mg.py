"""Darcy flow past an impermeable disc, with and without the cell-aggregated multigrid preconditioner: the reference's 2-D Darcy
script (examples/2D/Darcy/DarcyFlow.jl) restated.  Pressure p solves -∇·(K ∇p) = 0 in the 4 x 4 box minus the disc of radius 1
about (2.01, 2.01), p = 10 on the top border, p = 20 on the bottom one, no condition on the two others, and no flow through the
disc: Neumann(0) on the body.  The steady system has no mass term, so the plain BiCGStab count grows with n.  `precond="mg"`
refuses a Neumann interface; `precond="mg-cell"` aggregates the bulk and interface unknowns of 2 x 2 cells together and serves it.
The script solves the pressure both ways, prints iterations, times and the hierarchy, then the Darcy velocity u = -K ∇p.  What a
Penguin.jl user changes: the level-set closure becomes the tagged body `Sphere(centre, radius, complement=True)`,
`solve_DarcyFlow!` is spelled `solve_DarcyFlow_b`, and `precond="mg-cell"` is a keyword the reference does not have.

    python examples/darcy_obstacle_mg.py [n=80]            (needs a GPU and the built library)
"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from penguin.jl_amd import (BorderConditions, Capacity, DarcyFlow, DiffusionOps, Dirichlet, Mesh, Neumann, Phase, Sphere,
                            solve_darcy_velocity, solve_DarcyFlow_b)

n = int(sys.argv[1]) if len(sys.argv) > 1 else 80

# Define the mesh and the body: fluid outside the disc
lx, ly = 4.0, 4.0
mesh = Mesh((n, n), (lx, ly), (0.0, 0.0))
radius, center = ly / 4, (lx / 2 + 0.01, ly / 2 + 0.01)
capacity = Capacity(Sphere(center, radius, complement=True), mesh)
operator = DiffusionOps(capacity)

# Boundary conditions for the pressure on two faces; the other faces have none.  The disc is impermeable
bc_p = BorderConditions({"top": Dirichlet(10.0), "bottom": Dirichlet(20.0)})
ic = Neumann(0.0)

# Source term and permeability
Fluide = Phase(capacity, operator, lambda x, y, z=0.0: 0.0, lambda x, y, z=0.0: 1.0)


def solve(**kwargs):
    solver = DarcyFlow(Fluide, bc_p, ic)
    t0 = time.perf_counter()
    solve_DarcyFlow_b(solver, reltol=1e-12, **kwargs)                  # (returns with the solution on the host)
    return solver, (time.perf_counter() - t0) * 1e3


plain, ms_plain = solve(precond=0)
mgc, ms_mgc = solve(precond="mg-cell")
info = mgc.mg_info("mg-cell")
rel = float(np.linalg.norm(mgc.x - plain.x) / np.linalg.norm(plain.x))
print(f"{n}² cells, {plain.system_info(0).n_own} unknowns, pressure between {mgc.x[mgc.x != 0].min():.4f} and {mgc.x.max():.4f}")
print(f"default options : {plain.ch[-1]['iters']:5d} iterations  {ms_plain:9.2f} ms  converged {plain.ch[-1]['converged']}")
print(f"mg-cell         : {mgc.ch[-1]['iters']:5d} iterations  {ms_mgc:9.2f} ms  converged {mgc.ch[-1]['converged']}"
      f"  (of which {info['setup_ms']:.2f} ms set-up)")
print(f"hierarchy: rows per level {info['rows']}, levels from {info['tail_level']} on run in the fused one-workgroup tail, "
      f"{info['bytes'] / 2 ** 20:.1f} MiB")
print(f"relative L2 distance of the two solutions: {rel:.2e}")

# Solve the velocity problem
u = solve_darcy_velocity(mgc, Fluide)
print(f"largest Darcy velocity component: {np.nanmax(np.abs(u)):.4f}")             # (cells without fluid carry no velocity)
