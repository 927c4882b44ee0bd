"""Measurement of moving marker polygons: slabs per second of the prescribed-motion diffusion solver with the
capacities, the system and the solve rebuilt every slab, on the problem scripts/bench_moving_program.py measures (a disc growing
like 1 + 1.56 sqrt(t + 0.01) about the origin in [-8, 8]^2, fluid outside, Dirichlet(1) on the interface, Dirichlet(0) borders,
dt = h^2, BE, bicgstab, state handed over on the device), for

  sphere            MovingSphere(complement=True) with exact rates
  program disc      the same disc as DeviceFunction(lambda x, y, t: ..., complement=True)
  polygon M         the same disc as a MovingFront of M = 100, 1000, 10 000 markers on the circle (complement=True)
  crystal           the fluid outside a six-lobed crystal of 600 markers turning at 2 rad per unit time: a shape no program
                    expresses within 96 instructions

on n x n cells, n = 1024 and 2048.

    python scripts/bench_moving_polygon.py [out.json] [n ...]     (default: profiles/moving_polygon_bench.json, 1024 2048)

One warm-up solve of 2 slabs per body, then three timed solves of SLABS slabs per body, alternating; the median of slabs / s is
reported with the spread (max - min) / median.  For every body but the sphere one more capacity of the first slab is built alone
with the kernel timing on (pg_debug_spacetime_kernel_timing) and its six kernels are reported one by one -- for the polygons with
the time of the edge lookup and the wall time of the constructor, which holds the host's O(M^2) self-intersection tests at t0, mid
time and t1 -- with the number of cells the cheap pass left to the node loop and the number of CUT cells among them.  Every figure
is reported as found."""
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import penguin.jl_amd as pj
from penguin.jl_amd import moving
from penguin.jl_amd.build import source_hash

ARGS = sys.argv[1:]
OUT = ARGS[0] if ARGS else "profiles/moving_polygon_bench.json"
SIZES = [int(a) for a in ARGS[1:]] or [1024, 2048]
REPEATS, SLABS = 3, 8
C_GROW = 1.56


def radius(t):
    return 1.0 + C_GROW * np.sqrt(t + 0.01)


def disc(x, y, t):
    return np.sqrt(x * x + y * y) - (1.0 + C_GROW * np.sqrt(t + 0.01))


def polygon_disc(M):
    unit = pj.create_circle_b(pj.FrontTracker(), 0.0, 0.0, 1.0, M).polygon()
    return lambda: pj.MovingFront(lambda t: radius(t) * unit, complement=True)


def crystal():
    base = pj.create_crystal_b(pj.FrontTracker(), 0.0, 0.0, 2.0, 6, 0.3, 600)
    return pj.MovingFront.rigid(base, angle=lambda t: 2.0 * t, complement=True)


BODIES = {
    "sphere": lambda: pj.MovingSphere(lambda t: (0.0, 0.0), radius, complement=True, dcenter=lambda t: (0.0, 0.0),
                                      dradius=lambda t: 0.5 * C_GROW / np.sqrt(t + 0.01)),
    "program disc": lambda: pj.DeviceFunction(disc, complement=True),
    "polygon 100": polygon_disc(100),
    "polygon 1000": polygon_disc(1000),
    "polygon 10000": polygon_disc(10000),
    "crystal": crystal,
}


def solve(make, mesh, n, dt, slabs):
    body = make()
    M = (n + 1) ** 2
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in ("left", "right", "top", "bottom")})
    bc = pj.Dirichlet(1.0)
    cap0 = pj.Capacity(body, pj.SpaceTimeMesh(mesh, [0.0, dt]))
    ph = pj.Phase(cap0, pj.DiffusionOps(cap0), lambda x, y, z, t: 0.0, lambda x, y, z: 1.0)
    s = pj.MovingDiffusionUnsteadyMono(ph, bcb, bc, dt, np.concatenate([np.zeros(M), np.ones(M)]), mesh, "BE")
    t0 = time.perf_counter()
    pj.solve_MovingDiffusionUnsteadyMono_b(s, ph, body, dt, 0.0, (slabs - 0.5) * dt, bcb, bc, mesh, "BE", method="bicgstab",
                                           save_states=False)
    wall = time.perf_counter() - t0
    return slabs / wall, s.unconverged


def main():
    pj.init(0)
    out = {"source_hash": source_hash(), "device": pj.device_name(), "repeats": REPEATS, "slabs": SLABS, "sizes": {}}
    for n in SIZES:
        mesh = pj.Mesh((n, n), (16.0, 16.0), (-8.0, -8.0))
        dt = (16.0 / n) ** 2
        runs = {k: [] for k in BODIES}
        for make in BODIES.values():
            solve(make, mesh, n, dt, 2)
        for _ in range(REPEATS):
            for k, make in BODIES.items():
                runs[k].append(solve(make, mesh, n, dt, SLABS))
        res = {}
        for k, r in runs.items():
            sps = [x[0] for x in r]
            res[k] = {"slabs_per_s": statistics.median(sps), "spread": (max(sps) - min(sps)) / statistics.median(sps),
                      "slabs_per_s_all": sps, "unconverged": int(sum(x[1] for x in r))}
            moving.spacetime_kernel_timing(k != "sphere")
            t0 = time.perf_counter()
            cap = pj.Capacity(BODIES[k](), pj.SpaceTimeMesh(mesh, [0.0, dt]))
            res[k]["capacity_wall_ms"] = 1e3 * (time.perf_counter() - t0)
            moving.spacetime_kernel_timing(False)
            res[k]["capacity_kernel_ms"] = cap.kernel_ms
            if k != "sphere":
                ms, listed = cap.spacetime_kernel_ms
                res[k].update(kernel_ms_parts=ms, cells_left_to_the_list=listed, cut_cells=int((cap.cell_types == -1).sum()),
                              cells=n * n)
            if isinstance(cap.body, pj.MovingFront):
                res[k]["binning_ms"] = cap.polygon_ms_parts["binning"]
        for k in BODIES:
            if k != "sphere":
                res[k + " / sphere, capacity kernel ms"] = res[k]["capacity_kernel_ms"] / res["sphere"]["capacity_kernel_ms"]
                res["sphere / " + k + ", slabs per s"] = res["sphere"]["slabs_per_s"] / res[k]["slabs_per_s"]
        out["sizes"][str(n)] = res
        for k in BODIES:
            print(n, k, json.dumps(res[k]), flush=True)
        print(n, json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}), flush=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
