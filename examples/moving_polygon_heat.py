"""Heat around a turning crystal (a hot six-lobed stirrer in a cold box), 2-D+t: a moving marker polygon through the public
prescribed-motion driver.  The body is a MovingFront, a callable t -> markers; every slab sends the markers at its two times to the
space-time capacity kernels, which move each marker on a straight line in between and measure the polygon itself -- no level set,
no program, any number of lobes.

    python examples/moving_polygon_heat.py            (needs a GPU and the built library)

Straight marker paths: a slab turns the crystal by omega dt = 0.03 rad here, so a chord replaces an arc of that angle and the
shape shrinks by about (omega dt)^2 / 4 = 2e-4 of its area in mid slab.  Take dt small against the turning rate.
"""
import sys

import numpy as np

sys.path.insert(0, ".")
from penguin.jl_amd import (BorderConditions, Capacity, DiffusionOps, Dirichlet, FrontTracker, Mesh, MovingDiffusionUnsteadyMono,
                            MovingFront, Phase, SpaceTimeMesh, create_crystal_b, solve_MovingDiffusionUnsteadyMono_b)

# Define the mesh
nx, ny = 128, 128
lx, ly = 4.0, 4.0
mesh = Mesh((nx, ny), (lx, ly), (0.0, 0.0))

# Define the body: the fluid is OUTSIDE a crystal of 240 markers that turns at omega rad per unit time about its centre
cx, cy, omega = 2.013, 1.968, 2.0
front = create_crystal_b(FrontTracker(), cx, cy, 0.9, 6, 0.3, 240)
body = MovingFront.rigid(front, angle=lambda t: omega * t, about=(cx, cy), complement=True)

# Define the Space-Time mesh
dt = 0.5 * (lx / nx)
Tstart, Tend = 0.0, 40 * dt
STmesh = SpaceTimeMesh(mesh, [0.0, dt])

# Define the capacity and the operators
capacity = Capacity(body, STmesh)
operator = DiffusionOps(capacity)

# Boundary conditions, source term, diffusion coefficient, phase
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
print(f"{len(solver.states)} states, the crystal turned by {omega * Tend:.2f} rad; first slab: {capacity.spacetime_kernel_ms[1]} of "
      f"{nx * ny} cells went to the node loop, its capacity kernels took {capacity.kernel_ms:.2f} ms, "
      f"the edge lookup {capacity.polygon_ms_parts['binning']:.2f} ms")
print("bulk temperature on the line y = cy, right of the crystal:")
print(np.array2string(T[ny // 2, nx // 2 + 40:nx // 2 + 64:4], precision=4))
