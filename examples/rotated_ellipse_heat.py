"""Heat inside an ellipse turned by 0.5 rad -- a body no tagged kind can express: the level set is written inline, wrapped in
DeviceFunction, traced with its derivatives and evaluated inside the capacity kernels.

    python examples/rotated_ellipse_heat.py [n]

The ellipse (semi-axes 1.3 and 0.6, centre (2.01, 1.97)) starts cold with its wall held at 1; the script prints the
volume-averaged temperature as the heat diffuses in, and the measured area against pi a b."""
import math
import sys

import numpy as np

sys.path.insert(0, ".")
import penguin.jl_amd as pj  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
a, b, angle = 1.3, 0.6, 0.5
c, s = math.cos(angle), math.sin(angle)


def ellipse(x, y):
    X = c * (x - 2.01) + s * (y - 1.97)
    Y = c * (y - 1.97) - s * (x - 2.01)
    return (X / a) ** 2 + (Y / b) ** 2 - 1.0        # fluid where this is <= 0


pj.init(0)
mesh = pj.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
cap = pj.Capacity(pj.DeviceFunction(ellipse), mesh)
print(f"area {cap.V.sum():.12f}  (pi a b = {math.pi * a * b:.12f}),  perimeter {cap.Γ.sum():.9f},  "
      f"{int((cap.cell_types == -1).sum())} cut cells, capacity kernels {cap.kernel_ms:.3f} ms")

M = (n + 1) ** 2
phase = pj.Phase(cap, pj.DiffusionOps(cap), lambda x, y, z, t: 0.0, lambda x, y, z: 1.0)
bcb, wall = pj.BorderConditions({}), pj.Dirichlet(1.0)
dt = 0.25 * (4.0 / n) ** 2
u0 = np.concatenate([np.zeros(M), np.ones(M)])
solver = pj.DiffusionUnsteadyMono(phase, bcb, wall, dt, u0, "BE")
pj.solve_DiffusionUnsteadyMono_b(solver, phase, dt, 200 * dt, bcb, wall, "CN", reltol=1e-12)
V = cap.V
for k in (0, 49, 99, 199):
    if k < len(solver.states):
        print(f"t = {(k + 1) * dt:.5f}: mean temperature {float(np.dot(V, solver.states[k][:M]) / V.sum()):.6f}")
