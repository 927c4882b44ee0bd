"""Measurement of traced level sets as bodies: capacity construction time of

  circle    a program circle, sqrt((x - 2.01)^2 + (y - 2.01)^2) - 1, against Sphere((2.01, 2.01), 1)
  ellipse   the rotated ellipse of the tests (semi-axes 1.3, 0.6, angle 0.5), which no tagged kind expresses: alone

on Mesh((n, n), (4, 4)), n = 1024 and 2048.

    python scripts/bench_levelset_capacity.py [out.json] [n ...]     (default: profiles/levelset_capacity_bench.json, 1024 2048)

One warm-up build per body, then three builds per body, alternating; the median is reported with the spread (max - min) /
median.  `kernel_ms` is the capacity's own event pair around its five kernels (classification, cut cells, sections, staggered
volumes and their cut boxes), `wall_ms` the constructor seen from Python (tracing, differentiation and the host-side gradient
check included).  `kernel_ms_parts` are the five kernels one by one, each between its own pair of events
(pg_capacity_kernel_ms_parts), from the build with the median `kernel_ms`.  Every figure is reported as found."""
import json
import math
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import penguin.jl_amd as pj
from penguin.jl_amd.build import source_hash

ARGS = sys.argv[1:]
OUT = ARGS[0] if ARGS else "profiles/levelset_capacity_bench.json"
SIZES = [int(a) for a in ARGS[1:]] or [1024, 2048]
REPEATS = 3


def rotated_ellipse(x, y):
    c, s = math.cos(0.5), math.sin(0.5)
    X = c * (x - 2.01) + s * (y - 1.97)
    Y = c * (y - 1.97) - s * (x - 2.01)
    return (X / 1.3) ** 2 + (Y / 0.6) ** 2 - 1.0


BODIES = {
    "sphere": lambda: pj.Sphere((2.01, 2.01), 1.0),
    "program circle": lambda: pj.DeviceFunction(lambda x, y: np.sqrt((x - 2.01) ** 2 + (y - 2.01) ** 2) - 1.0),
    "program rotated ellipse": lambda: pj.DeviceFunction(rotated_ellipse),
}


def build(make, mesh):
    t0 = time.perf_counter()
    cap = pj.Capacity(make(), mesh)
    wall = (time.perf_counter() - t0) * 1e3
    return cap.kernel_ms, wall, cap


def main():
    pj.init(0)
    out = {"source_hash": source_hash(), "device": pj.device_name(), "repeats": REPEATS, "sizes": {}}
    for n in SIZES:
        mesh = pj.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
        runs = {k: [] for k in BODIES}
        info = {}
        for k, make in BODIES.items():                       # warm-up, and what was built
            _, _, cap = build(make, mesh)
            info[k] = {"cut_cells": int((cap.cell_types == -1).sum()), "area": float(cap.V.sum()), "perimeter": float(cap.Γ.sum())}
        for _ in range(REPEATS):
            for k, make in BODIES.items():
                km, wall, cap = build(make, mesh)
                runs[k].append((km, wall, cap.kernel_ms_parts))
        res = {}
        for k, r in runs.items():
            km, wall = [x[0] for x in r], [x[1] for x in r]
            res[k] = dict(info[k], kernel_ms=statistics.median(km), kernel_ms_spread=(max(km) - min(km)) / statistics.median(km),
                          wall_ms=statistics.median(wall), kernel_ms_all=km, wall_ms_all=wall,
                          kernel_ms_parts=sorted(r, key=lambda x: x[0])[len(r) // 2][2])
        res["program circle / sphere, kernel_ms"] = res["program circle"]["kernel_ms"] / res["sphere"]["kernel_ms"]
        res["circle area difference"] = abs(res["program circle"]["area"] - res["sphere"]["area"])
        out["sizes"][str(n)] = res
        print(n, json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}), flush=True)
        for k in BODIES:
            print("   ", k, f"kernel {res[k]['kernel_ms']:.3f} ms  wall {res[k]['wall_ms']:.1f} ms  cut cells {res[k]['cut_cells']}  "
                  + " ".join(f"{q} {v:.3f}" for q, v in res[k]["kernel_ms_parts"].items()), flush=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
