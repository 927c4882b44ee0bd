"""Heat inside a torus -- a 3-D body no tagged kind can express: the level set is written inline, wrapped in DeviceFunction,
traced with its three derivatives and evaluated inside the capacity kernels (quadrature="height").

    python examples/torus_heat3d.py [n]

The torus (R = 1.2, r = 0.5, axis z, centre (2.03, 1.96, 2.07)) starts cold with its wall held at 1 (Dirichlet on the
interface); one backward-Euler step, then Crank-Nicolson.  The script prints the volume-averaged temperature as the heat
diffuses in, and the measured volume and surface against 2 pi^2 R r^2 and 4 pi^2 R r."""
import math
import sys

import numpy as np

sys.path.insert(0, ".")
import penguin.jl_amd as pj  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 48
R, r = 1.2, 0.5


def torus(x, y, z):
    return (np.sqrt((x - 2.03) ** 2 + (y - 1.96) ** 2) - R) ** 2 + (z - 2.07) ** 2 - r * r      # fluid where this is <= 0


pj.init(0)
mesh = pj.Mesh((n, n, n), (4.0, 4.0, 4.0), (0.0, 0.0, 0.0))
cap = pj.Capacity(pj.DeviceFunction(torus), mesh, quadrature="height")
print(f"volume {cap.V.sum():.12f}  (2 pi^2 R r^2 = {2 * math.pi ** 2 * R * r * r:.12f}),  surface {cap.Γ.sum():.9f}  "
      f"(4 pi^2 R r = {4 * math.pi ** 2 * R * r:.9f}),  {int((cap.cell_types == -1).sum())} cut cells, "
      f"capacity kernels {cap.kernel_ms:.3f} ms")

M = (n + 1) ** 3
phase = pj.Phase(cap, pj.DiffusionOps(cap), lambda x, y, z, t: 0.0, lambda x, y, z: 1.0)
bcb, wall = pj.BorderConditions({}), pj.Dirichlet(1.0)
dt = 0.25 * (4.0 / n) ** 2
u0 = np.concatenate([np.zeros(M), np.ones(M)])
solver = pj.DiffusionUnsteadyMono(phase, bcb, wall, dt, u0, "BE")
pj.solve_DiffusionUnsteadyMono_b(solver, phase, dt, 100 * dt, bcb, wall, "CN", reltol=1e-12)
V = cap.V
for k in (0, 24, 49, 99):
    if k < len(solver.states):
        print(f"t = {(k + 1) * dt:.5f}: mean temperature {float(np.dot(V, solver.states[k][:M]) / V.sum()):.6f}")
