"""Heat inside a disc given by MARKERS -- the set-up of the reference's benchmark/HeatFT.jl: a FrontTracker filled by
create_circle_b, Capacity(front, mesh), Robin exchange on the front, Dirichlet on the box.  The polygon of the markers is
measured inside the capacity kernels.

    python examples/heat_front_tracker.py [n]

The disc (radius 1 about (2.01, 2.01), max(500, 10 n) markers as in HeatFT.jl) starts at 270 in surroundings at 400; the script
prints the measured area and perimeter against the polygon's own, and the volume-averaged temperature as the heat comes in."""
import math
import sys

import numpy as np

sys.path.insert(0, ".")
import penguin.jl_amd as pj  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
radius, center = 1.0, (2.01, 2.01)

pj.init(0)
mesh = pj.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
front = pj.FrontTracker()
resolution = max(500, n * 10)
pj.create_circle_b(front, center[0], center[1], radius, resolution)
cap = pj.Capacity(front, mesh)
ms = cap.polygon_ms_parts
print(f"{resolution} markers: area {cap.V.sum():.12f}  (polygon {0.5 * resolution * radius ** 2 * math.sin(2 * math.pi / resolution):.12f}, "
      f"disc {math.pi * radius ** 2:.12f}),  perimeter {cap.Γ.sum():.9f}  (polygon {2 * resolution * radius * math.sin(math.pi / resolution):.9f}),  "
      f"{int((cap.cell_types == -1).sum())} cut cells, capacity kernels {cap.kernel_ms:.3f} ms + edge lookup {ms['binning']:.3f} ms")

M = (n + 1) ** 2
phase = pj.Phase(cap, pj.DiffusionOps(cap), lambda x, y, z, t: 0.0, lambda x, y, z: 1.0)
bc_boundary = pj.Robin(3.0, 1.0, 3.0 * 400)
bc0 = pj.Dirichlet(400.0)
bc_b = pj.BorderConditions({k: bc0 for k in ("left", "right", "top", "bottom")})
dt = 0.25 * (4.0 / n) ** 2
Tend = 0.1
u0 = np.concatenate([np.ones(M) * 270.0, np.zeros(M)])
solver = pj.DiffusionUnsteadyMono(phase, bc_b, bc_boundary, dt, u0, "BE")
pj.solve_DiffusionUnsteadyMono_b(solver, phase, dt, Tend, bc_b, bc_boundary, "CN", reltol=1e-12)
V = cap.V
steps = len(solver.states)
for k in sorted({0, steps // 4, steps // 2, steps - 1}):
    print(f"state {k + 1} of {steps}: mean temperature {float(np.dot(V, solver.states[k][:M]) / V.sum()):.6f}")
