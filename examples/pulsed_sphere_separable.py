"""A sphere heated by a sinusoidally pulsed source while its wall temperature is ramped up: time-dependent data that stay on
the device.  Source and wall value are written as `TimeSeparable` -- a sum of terms (spatial part) x (function of time) -- so
the solver sends the spatial parts to the GPU once and every time step costs a few scalars; written as plain closures
`f(x, y, z, t)` the same data send every step through Python and across PCIe (the script runs a few steps of that too and
prints both rates).

    python examples/pulsed_sphere_separable.py [n]            (needs a GPU and the built library; n = 64 by default)
"""
import math
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from penguin.jl_amd import (BorderConditions, Capacity, DiffusionOps, DiffusionUnsteadyMono, Dirichlet, Mesh, Phase, Sphere,
                            TimeSeparable, solve_DiffusionUnsteadyMono_b)

n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
mesh = Mesh((n, n, n), (4.0, 4.0, 4.0), (0.0, 0.0, 0.0))
capacity = Capacity(Sphere((2.01, 2.01, 2.01), 1.0), mesh)
operator = DiffusionOps(capacity)
M = (n + 1) ** 3
dt = 0.5 * (4.0 / n) ** 2
steps = 200
Tend = (steps - 0.5) * dt
omega = 2.0 * math.pi / (40.0 * dt)

# a Gaussian hot spot pulsed at omega on top of a steady uniform heating; the wall ramps from 0 to 1 over the first 100 steps
spot = lambda x, y, z: 5.0 * np.exp(-8.0 * ((x - 2.3) ** 2 + (y - 2.0) ** 2 + (z - 2.0) ** 2))
source = TimeSeparable([(spot, lambda t: math.sin(omega * t) ** 2), (0.2, lambda t: 1.0)])
wall = TimeSeparable([(1.0, lambda t: min(t / (100.0 * dt), 1.0))])
bc_b = BorderConditions({k: Dirichlet(0.0) for k in ("left", "right", "top", "bottom")})
u0 = np.zeros(2 * M)


def run(f, g, nsteps, save_states):
    phase = Phase(capacity, operator, f, lambda x, y, z: 1.0)
    solver = DiffusionUnsteadyMono(phase, bc_b, Dirichlet(g), dt, u0, "BE")
    t0 = time.perf_counter()
    solve_DiffusionUnsteadyMono_b(solver, phase, dt, (nsteps - 0.5) * dt, bc_b, Dirichlet(g), "CN", save_states=save_states)
    return solver, time.perf_counter() - t0


solver, secs = run(source, wall, steps, False)
print(f"{n}^3, {steps} steps with TimeSeparable data: time_data = {solver.time_data!r}, {steps / secs:.1f} steps/s "
      f"({solver.last_run.products / steps:.1f} products per step), max T = {np.abs(solver.x).max():.6f}")

# the same data as plain closures: the host-driven loop (a few steps are enough to see the rate)
few = 10
plain_f = lambda x, y, z, t: source(x, y, z, t)
plain_g = lambda x, y, z, t: wall(x, y, z, t)
host, secs_h = run(plain_f, plain_g, few, True)
dev, _ = run(source, wall, few, True)
diff = np.linalg.norm(dev.x - host.x) / np.linalg.norm(host.x)
print(f"{few} steps with the same data as plain closures: time_data = {host.time_data!r}, {few / secs_h:.1f} steps/s; "
      f"states of the two paths differ by {diff:.1e} (relative L2)")
