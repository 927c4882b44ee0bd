"""Heat conduction with a time step that does not shrink with the mesh, with and without the multigrid preconditioner of the time
loop: the reference's examples/2D/Diffusion/Heat_Nobody.jl / 3D/Diffusion/Heat.jl take Δt = 0.01 whatever the mesh, which on a fine
grid is hundreds of h².  Backward Euler and Crank-Nicolson are stable there, but the system of a step approaches the Poisson
system: the polynomial preconditioner of the default options is turned away and plain BiCGStab needs a number of products that
grows with n.  `precond="mg-step"` runs the cell-aggregated V-cycle inside the loop (one hierarchy per assembled matrix, built on
first use).  The script takes the same steps both ways and prints products per step, times and the hierarchies.  What a
Penguin.jl user changes: the level-set closure becomes the tagged body `Sphere(centre, radius, complement=True)`,
`solve_DiffusionUnsteadyMono!` is spelled `solve_DiffusionUnsteadyMono_b`, and `precond="mg-step"` is a keyword the reference does
not have.  At Δt of the order of h² the default options are the faster ones (README has the measured crossover).

    python examples/heat_large_step_mg.py [n=512] [steps=20] [scheme=CN]            (needs a GPU and the built library)
"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from penguin.jl_amd import (BorderConditions, Capacity, DiffusionOps, DiffusionUnsteadyMono, Dirichlet, Mesh, Phase, Sphere,
                            solve_DiffusionUnsteadyMono_b)

n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
scheme = sys.argv[3] if len(sys.argv) > 3 else "CN"

# Define the mesh and the body: fluid outside the heated cylinder
lx, ly = 4.0, 4.0
mesh = Mesh((n, n), (lx, ly), (0.0, 0.0))
radius, center = ly / 4, (lx / 2 + 0.01, ly / 2 + 0.01)
capacity = Capacity(Sphere(center, radius, complement=True), mesh)
operator = DiffusionOps(capacity)

# Boundary conditions: cold walls, the cylinder at T = 1
bc_b = BorderConditions({k: Dirichlet(0.0) for k in ("left", "right", "top", "bottom")})
bc = Dirichlet(1.0)

# No source, unit conductivity
Fluide = Phase(capacity, operator, lambda x, y, z=0.0: 0.0, lambda x, y, z=0.0: 1.0)

# The reference's step, and what it is in units of h²
Δt = 0.01
Tend = steps * Δt
M = (n + 1) ** 2
u0 = np.zeros(2 * M)
print(f"{n}² cells, Δt = {Δt} = {Δt / (lx / n) ** 2:.0f} h², {steps} steps, {scheme}")


def solve(**kwargs):
    solver = DiffusionUnsteadyMono(Fluide, bc_b, bc, Δt, u0, scheme)
    t0 = time.perf_counter()
    solve_DiffusionUnsteadyMono_b(solver, Fluide, Δt, Tend, bc_b, bc, scheme, save_states=False, reltol=1e-12, **kwargs)
    return solver, (time.perf_counter() - t0) * 1e3


plain, ms_plain = solve(precond=0)
mgs, ms_mgs = solve(precond="mg-step")
rel = float(np.linalg.norm(mgs.x - plain.x) / np.linalg.norm(plain.x))
for name, s, ms in (("default options", plain, ms_plain), ("mg-step", mgs, ms_mgs)):
    r = s.last_run
    print(f"{name:16s}: {r.steps} steps, {r.products / max(r.steps, 1):8.1f} products per step, {ms:9.2f} ms in all "
          f"(first solve included), {r.unconverged_steps} unconverged")
for which, info in zip(("constructor system", "run system"), mgs.mg_step_info()):
    if info["levels"]:
        print(f"hierarchy of the {which}: rows per level {info['rows']}, set-up {info['setup_ms']:.2f} ms, "
              f"{info['bytes'] / 2 ** 20:.1f} MiB")
print(f"relative L2 distance of the two final states: {rel:.2e}")
