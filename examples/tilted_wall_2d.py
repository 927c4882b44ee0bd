"""Heat conduction behind an inclined wall: the unit square, the wall 0.6 x + 0.8 y = 0.83 held at temperature 1, the fluid
below it starting cold.  Until the heat reaches the borders the temperature is erfc(distance to the wall / 2 sqrt(t)), which
the script prints next to the computed one.  What a Penguin.jl user changes: the level-set closure
`(x, y, _=0) -> 0.6x + 0.8y - 0.83` becomes the tagged body `Plane((0.6, 0.8), 0.83)`.

    python examples/tilted_wall_2d.py            (needs a GPU and the built library)
"""
import sys

import numpy as np
from scipy.special import erfc

sys.path.insert(0, ".")
from penguin.jl_amd import (BorderConditions, Capacity, DiffusionOps, DiffusionUnsteadyMono, Dirichlet, Mesh, Phase, Plane,
                            check_convergence, solve_DiffusionUnsteadyMono_b)

# Define the mesh
nx, ny = 64, 64
lx, ly = 1.0, 1.0
mesh = Mesh((nx, ny), (lx, ly), (0.0, 0.0))
h = lx / nx

# Define the body: fluid where normal . x - offset < 0
normal, offset = (0.6, 0.8), 0.83
body = Plane(normal, offset)                      # or Plane.through((0.25, 0.85), normal)

# Define the capacity and the operators
capacity = Capacity(body, mesh)
operator = DiffusionOps(capacity)
cut = capacity.cell_types == -1
print(f"{np.count_nonzero(cut)} cut cells, wall length {capacity.Γ.sum():.6f}, fluid area {capacity.V.sum():.6f}")

# Boundary conditions: the wall at 1, the analytic solution on the borders (border values are taken at mesh.centers, one
# spacing below the centres of the cells the unknowns belong to: hence x + h, y + h)
exact = lambda x, y, t: erfc((offset - normal[0] * np.asarray(x) - normal[1] * np.asarray(y)) / (2.0 * np.sqrt(t)))
bc_wall = Dirichlet(1.0)
with np.errstate(divide="ignore"):
    bc_b = BorderConditions({k: Dirichlet(lambda x, y, t: exact(x + h, y + h, t)) for k in ("left", "right", "top", "bottom")})

    # Source term, diffusion coefficient, phase, initial condition
    Fluide = Phase(capacity, operator, lambda x, y, z, t: 0.0, lambda x, y, z: 1.0)
    M = (nx + 1) * (ny + 1)
    u0 = np.concatenate([np.zeros(M), np.ones(M)])

    # Define the solver, solve
    dt, Tend = 0.25 * h ** 2, 0.02
    solver = DiffusionUnsteadyMono(Fluide, bc_b, bc_wall, dt, u0, "BE")
    solve_DiffusionUnsteadyMono_b(solver, Fluide, dt, Tend, bc_b, bc_wall, "BE", method="bicgstab")

t = len(solver.states) * dt
err = check_convergence(lambda x, y: exact(x, y, t), solver, capacity, 2)[2]
print(f"{len(solver.states)} states, t = {t:.5f}: volume-weighted L2 error against erfc = {err:.3e}")
T = solver.states[-1][:M].reshape(ny + 1, nx + 1)
Cw = capacity.C_ω
j = ny // 4
for i in range(0, nx, 8):
    q = j * (nx + 1) + i
    if capacity.V[q] > 0:
        print(f"  x = {Cw[q, 0]:.4f}  y = {Cw[q, 1]:.4f}   T = {T[j, i]:.6f}   erfc = {float(exact(Cw[q, 0], Cw[q, 1], t)):.6f}")
