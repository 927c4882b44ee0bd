"""Poisson's equation outside a cylinder, with and without the multigrid preconditioner: -Δu = 1 in the 4 x 4 box minus the disc
of radius 0.5 about (2.01, 2.01), u = 0 on the disc and on the four borders, on an n² mesh (512² by default).  The steady system
has no mass term, so the plain BiCGStab iteration count grows with n; `precond="mg"` runs the same iteration right-preconditioned
with an aggregation multigrid V-cycle, whose count hardly moves.  The script solves the system both ways and prints iterations,
times, the hierarchy and how far apart the two solutions are.  What a Penguin.jl user changes: the level-set closure becomes the
tagged body `Sphere(centre, radius, complement=True)`, `solve_DiffusionSteadyMono!` is spelled `solve_DiffusionSteadyMono_b`, and
`precond="mg"` is a keyword the reference does not have.

    python examples/poisson_cylinder_mg.py [n=512]            (needs a GPU and the built library)
"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from penguin.jl_amd import (BorderConditions, Capacity, DiffusionOps, DiffusionSteadyMono, Dirichlet, Mesh, Phase, Sphere,
                            solve_DiffusionSteadyMono_b)

n = int(sys.argv[1]) if len(sys.argv) > 1 else 512

# Define the mesh and the body: fluid outside the cylinder
mesh = Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
capacity = Capacity(Sphere((2.01, 2.01), 0.5, complement=True), mesh)
operator = DiffusionOps(capacity)

# Source term, diffusion coefficient, boundary conditions
phase = Phase(capacity, operator, lambda x, y, z=0.0: 1.0, lambda x, y, z=0.0: 1.0)
borders = BorderConditions({k: Dirichlet(0.0) for k in ("left", "right", "bottom", "top")})


def solve(**kwargs):
    solver = DiffusionSteadyMono(phase, borders, Dirichlet(0.0))
    t0 = time.perf_counter()
    solve_DiffusionSteadyMono_b(solver, reltol=1e-12, **kwargs)        # (returns with the solution on the host)
    return solver, (time.perf_counter() - t0) * 1e3


plain, ms_plain = solve(precond=-1)
mg, ms_mg = solve(precond="mg")
info = mg.mg_info()
rel = float(np.linalg.norm(mg.x - plain.x) / np.linalg.norm(plain.x))
print(f"{n}² cells, {plain.system_info(0).n_own} unknowns, max u = {mg.x.max():.6f}")
print(f"plain BiCGStab : {plain.ch[-1]['iters']:5d} iterations  {ms_plain:9.2f} ms  converged {plain.ch[-1]['converged']}")
print(f"multigrid      : {mg.ch[-1]['iters']:5d} iterations  {ms_mg:9.2f} ms  converged {mg.ch[-1]['converged']}"
      f"  (of which {info['setup_ms']:.2f} ms set-up)")
print(f"hierarchy: rows per level {info['rows']}, levels from {info['tail_level']} on run in the fused one-workgroup tail, "
      f"{info['bytes'] / 2 ** 20:.1f} MiB")
print(f"relative L2 distance of the two solutions: {rel:.2e}")
