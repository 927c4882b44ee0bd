"""A vorticity ring spinning down inside a disc: stream function - vorticity flow in the unit square with fluid inside the circle
of radius 0.2 about the centre, no slip-through (ψ = 0) and ω = 0 on the circle.  The ring ω0 = cos(π r / R) drives an
azimuthal flow that viscosity (ν = 5e-3) damps; the script runs 40 steps of Δt = 5e-4 on a 96² mesh and prints the velocity
extrema, the enstrophy before and after, and what the two linear solves of a step cost.  What a Penguin.jl user changes: the
level-set closure becomes the tagged body `Sphere(centre, radius)`, and `run_StreamVorticity!` is spelled
`run_StreamVorticity_b`.

    python examples/stream_vorticity_circle.py [n=96] [steps=40]            (needs a GPU and the built library)
"""
import sys

import numpy as np

sys.path.insert(0, ".")
from penguin.jl_amd import BorderConditions, Capacity, Dirichlet, Mesh, Sphere, StreamVorticity, run_StreamVorticity_b

n = int(sys.argv[1]) if len(sys.argv) > 1 else 96
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40

# Define the mesh and the body: fluid inside the circle
mesh = Mesh((n, n), (1.0, 1.0), (0.0, 0.0))
centre, radius = (0.5, 0.5), 0.2
capacity = Capacity(Sphere(centre, radius), mesh)
M = (n + 1) ** 2

# Initial vorticity: a ring hugging the interface, zero outside the fluid
x, y = capacity.C_ω[:, 0], capacity.C_ω[:, 1]
r = np.hypot(x - centre[0], y - centre[1])
ω_bulk = np.where(capacity.V > 0, np.cos(np.pi * np.clip(r / radius, 0.0, 1.0)), 0.0)
ω0 = np.concatenate([ω_bulk, np.zeros(M)])

# Boundary conditions: ψ = 0 and ω = 0 on the circle and on the borders of the box
zero = Dirichlet(0.0)
borders = BorderConditions({k: zero for k in ("left", "right", "bottom", "top")})

ν, Δt = 5e-3, 5e-4
solver = StreamVorticity(capacity, ν, Δt, bc_stream=zero, bc_vorticity=zero, bc_stream_border=borders,
                         bc_vorticity_border=borders, ω0=ω0)

enstrophy = lambda ω: 0.5 * float(np.sum(capacity.V * ω[:M] ** 2))
e0 = enstrophy(solver.ω)
run_StreamVorticity_b(solver, steps, "BE", save_every=10)

u, v = solver.velocity
run = solver.last_run
print(f"t = {solver.time:.4f} after {run.steps} steps; {len(solver.states)} states kept (every 10th)")
print(f"velocity extrema with circular cut cells: |u|max = {np.abs(u).max():.6f}  |v|max = {np.abs(v).max():.6f}")
print(f"enstrophy {e0:.6e} -> {enstrophy(solver.ω):.6e}")
print(f"per step: {run.psi_products / run.steps:.1f} products in the Poisson solve, {run.omega_products / run.steps:.1f} in the "
      f"vorticity solve; {run.total_ms / run.steps:.2f} ms (ψ {run.psi_ms / run.steps:.2f}, velocity and convection operators "
      f"{run.velocity_ms / run.steps:.2f}, vorticity system {run.build_ms / run.steps:.2f}, its solve {run.omega_ms / run.steps:.2f})")
for st in solver.states:
    print(f"  state at t = {st.time:.4f}: max|ψ| = {np.abs(st.ψ).max():.4e}  max|ω| = {np.abs(st.ω).max():.4e}")
