"""The heat problem of Schwartz & Colella in a sphere (the reference's BenchPhaseFlow Problem 5): the exact solution
phi = 4 / (5 pi (t+1)) exp(-r^2 / (5 (t+1))) of  phi_t = lap(phi) + f  needs the source

    f(x, y, z, t) = 4 (r^2 + 5 (t+1)) / (125 pi (t+1)^3) exp(-r^2 / (5 (t+1))),

which is not a sum of (function of space) x (function of time) for any number of terms, and neither is the exact solution the
sphere's surface is held at.  Written as plain closures they send every time step through Python and across PCIe; wrapped in
`DeviceFunction` each is traced once into a small program that a kernel evaluates at the cell centroids (the source) and at the
interface centroids (the surface value) every step, and the whole loop stays on the device.  The script starts from the exact
solution at t = 0, runs the mesh sequence, prints the errors in the reference's norms and the order of convergence, and times a
few steps of the plain closures for comparison.  (The reference's script holds the surface at the solution of the END time and
starts from a constant; its error does not fall with h.  Here the data follow the solution in time.)

    python examples/schwartz_colella_heat3d.py [n ...]        (needs a GPU and the built library; n = 32 48 64 by default)
"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from penguin.jl_amd import (BorderConditions, Capacity, DeviceFunction, DiffusionOps, DiffusionUnsteadyMono, Dirichlet, Mesh, Phase,
                            Sphere, check_convergence, solve_DiffusionUnsteadyMono_b)

sizes = [int(a) for a in sys.argv[1:]] or [32, 48, 64]
Tend, radius, centre = 0.1, 0.392, (0.5, 0.5, 0.5)


def exact(x, y, z, t):
    return 4.0 / (5.0 * np.pi * (t + 1.0)) * np.exp(-(x * x + y * y + z * z) / (5.0 * (t + 1.0)))


def source(x, y, z, t):
    r2 = x * x + y * y + z * z
    return 4.0 * (r2 + 5.0 * (t + 1.0)) / (125.0 * np.pi * (t + 1.0) ** 3) * np.exp(-r2 / (5.0 * (t + 1.0)))


def run(n, f, g, tend, save_states=False):
    mesh = Mesh((n, n, n), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    capacity = Capacity(Sphere(centre, radius), mesh)
    phase = Phase(capacity, DiffusionOps(capacity), f, lambda x, y, z: 1.0)
    bc_b = BorderConditions({k: Dirichlet(0.0) for k in ("left", "right", "top", "bottom", "forward", "backward")})
    bc_i = Dirichlet(g)
    M = (n + 1) ** 3
    Cw, Cg = capacity.C_ω, capacity.C_γ
    u0 = np.concatenate([exact(Cw[:, 0], Cw[:, 1], Cw[:, 2], 0.0), exact(Cg[:, 0], Cg[:, 1], Cg[:, 2], 0.0)])
    dt = 0.25 * (1.0 / n) ** 2
    solver = DiffusionUnsteadyMono(phase, bc_b, bc_i, dt, u0, "BE")
    t0 = time.perf_counter()
    solve_DiffusionUnsteadyMono_b(solver, phase, dt, tend, bc_b, bc_i, "CN", save_states=save_states)
    return solver, capacity, dt, time.perf_counter() - t0


f_dev, g_dev = DeviceFunction(source), DeviceFunction(exact)
print(f"the source as a program: {f_dev.program.n_ops} instructions, {f_dev.program.n_const} constants; the surface value: "
      f"{g_dev.program.n_ops} instructions")
hs, errs = [], []
for n in sizes:
    solver, capacity, dt, secs = run(n, f_dev, g_dev, Tend)
    steps = solver.last_run.steps
    _, _, err, err_full, err_cut, _ = check_convergence(lambda x, y, z: exact(x, y, z, Tend), solver, capacity, 2)
    hs.append(1.0 / n)
    errs.append(err)
    print(f"n = {n:3d}: time_data = {solver.time_data!r}, {steps} steps at {steps / secs:.0f} steps/s, L2 error {err:.3e} "
          f"(full cells {err_full:.3e}, cut cells {err_cut:.3e})")
for k in range(1, len(sizes)):
    print(f"order {sizes[k - 1]} -> {sizes[k]}: {np.log(errs[k - 1] / errs[k]) / np.log(hs[k - 1] / hs[k]):.2f}")

# the same data as plain closures: the host-driven loop (a few steps are enough to see the rate)
n, few = sizes[-1], 10
dt = 0.25 * (1.0 / n) ** 2
host, _, _, secs_h = run(n, source, exact, (few - 0.5) * dt, save_states=True)
dev, _, _, _ = run(n, f_dev, g_dev, (few - 0.5) * dt, save_states=True)
diff = np.linalg.norm(dev.x - host.x) / np.linalg.norm(host.x)
print(f"n = {n}: {few} steps with the plain closures: time_data = {host.time_data!r}, {few / secs_h:.1f} steps/s; the states of the "
      f"two paths differ by {diff:.1e} (relative L2)")
