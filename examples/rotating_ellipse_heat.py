"""Heat around an ellipse turning at constant rate (a stirrer), 2-D+t: a moving body no tagged kind expresses, written as the
reference's `body = (x, y, t) -> ...` and wrapped in DeviceFunction.  The closure is traced once; phi, its gradient and d phi / dt
are evaluated inside the space-time capacity kernels on every slab.

    python examples/rotating_ellipse_heat.py            (needs a GPU and the built library)

The program format repeats a subexpression every time it occurs and a program holds 96 instructions, so the rotation is written
with the double angle -- (X / a)^2 + (Y / b)^2 with (X, Y) = R(-w t)(x - c) expands to
p (dx^2 + dy^2) + q (cos 2wt (dx^2 - dy^2) + 2 sin 2wt dx dy), p, q = (1 / a^2 +- 1 / b^2) / 2 -- which keeps d phi / dt short.
"""
import sys

import numpy as np

sys.path.insert(0, ".")
from penguin.jl_amd import (BorderConditions, Capacity, DeviceFunction, DiffusionOps, Dirichlet, Mesh, MovingDiffusionUnsteadyMono,
                            Phase, SpaceTimeMesh, solve_MovingDiffusionUnsteadyMono_b)

# Define the mesh
nx, ny = 128, 128
lx, ly = 4.0, 4.0
mesh = Mesh((nx, ny), (lx, ly), (0.0, 0.0))

# Define the body: the fluid is OUTSIDE an ellipse with semi-axes a, b that turns at omega rad per unit time about (cx, cy)
a, b, omega, cx, cy = 1.1, 0.6, 2.0, 2.013, 1.968
p, q = 0.5 * (1.0 / a ** 2 + 1.0 / b ** 2), 0.5 * (1.0 / a ** 2 - 1.0 / b ** 2)


def ellipse(x, y, t):
    dx, dy = x - cx, y - cy
    return p * (dx * dx + dy * dy) + q * (np.cos(2.0 * omega * t) * (dx * dx - dy * dy) + 2.0 * np.sin(2.0 * omega * t) * dx * dy) - 1.0


body = DeviceFunction(ellipse, complement=True)

# Define the Space-Time mesh
dt = 0.5 * (lx / nx)
Tstart, Tend = 0.0, 40 * dt
STmesh = SpaceTimeMesh(mesh, [0.0, dt])

# Define the capacity and the operators
capacity = Capacity(body, STmesh)
operator = DiffusionOps(capacity)

# Boundary conditions (a hot stirrer in a cold box), source term, diffusion coefficient, phase
bc = Dirichlet(0.0)
bc1 = Dirichlet(1.0)
bc_b = BorderConditions({"left": bc, "right": bc, "top": bc, "bottom": bc})
f = lambda x, y, z, t: 0.0
K = lambda x, y, z: 1.0
Fluide = Phase(capacity, operator, f, K)

# Initial condition
M = (nx + 1) * (ny + 1)
u0 = np.concatenate([np.zeros(M), np.ones(M)])

# Define the solver, solve
solver = MovingDiffusionUnsteadyMono(Fluide, bc_b, bc1, dt, u0, mesh, "BE")
solve_MovingDiffusionUnsteadyMono_b(solver, Fluide, body, dt, Tstart, Tend, bc_b, bc1, mesh, "BE", method="bicgstab")

T = solver.states[-1][:M].reshape(ny + 1, nx + 1)
print(f"{len(solver.states)} states, the ellipse turned by {omega * Tend:.2f} rad; first slab: {capacity.spacetime_kernel_ms[1]} of "
      f"{nx * ny} cells went to the node loop, its capacity kernels took {capacity.kernel_ms:.2f} ms")
print("bulk temperature on the line y = cy, right of the ellipse:")
print(np.array2string(T[ny // 2, nx // 2 + 36:nx // 2 + 64:4], precision=4))
