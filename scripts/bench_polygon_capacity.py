"""Measurement of marker polygons as bodies: capacity construction time of

  polygon M   create_circle_b(2.01, 2.01, 1, M), M = 100, 1000, 10000
  sphere      Sphere((2.01, 2.01), 1)
  program     the program circle of section 23, sqrt((x - 2.01)^2 + (y - 2.01)^2) - 1

on Mesh((n, n), (4, 4)), n = 1024 and 2048.

    python scripts/bench_polygon_capacity.py [out.json] [n ...]     (default: profiles/polygon_capacity_bench.json, 1024 2048)

One warm-up build per body, then three builds per body, alternating; the median is reported with the spread (max - min) /
median.  `kernel_ms` is the capacity's own event pair around its five kernels, `kernel_ms_parts` the five one by one, each
between its own pair of events, from the build with the median `kernel_ms`; for a polygon `binning_ms` is the edge lookup (count,
scan, fill, order), which runs before the five and is outside `kernel_ms`.  `wall_ms` is the constructor seen from Python (for a
polygon: the O(M^2) self-intersection test on the host included).  No ratio is promised: every figure is reported as found."""
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import penguin.jl_amd as pj
from penguin.jl_amd.build import source_hash

ARGS = sys.argv[1:]
OUT = ARGS[0] if ARGS else "profiles/polygon_capacity_bench.json"
SIZES = [int(a) for a in ARGS[1:]] or [1024, 2048]
REPEATS = 3
MARKERS = (100, 1000, 10000)

BODIES = {f"polygon {M}": (lambda M=M: pj.create_circle_b(pj.FrontTracker(), 2.01, 2.01, 1.0, M)) for M in MARKERS}
BODIES["sphere"] = lambda: pj.Sphere((2.01, 2.01), 1.0)
BODIES["program circle"] = lambda: pj.DeviceFunction(lambda x, y: np.sqrt((x - 2.01) ** 2 + (y - 2.01) ** 2) - 1.0)


def build(make, mesh):
    body = make()
    t0 = time.perf_counter()
    cap = pj.Capacity(body, mesh)
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
                parts = cap.polygon_ms_parts if k.startswith("polygon") else cap.kernel_ms_parts
                runs[k].append((km, wall, parts))
        res = {}
        for k, r in runs.items():
            km, wall = [x[0] for x in r], [x[1] for x in r]
            mid = sorted(r, key=lambda x: x[0])[len(r) // 2][2]
            res[k] = dict(info[k], kernel_ms=statistics.median(km), kernel_ms_spread=(max(km) - min(km)) / statistics.median(km),
                          wall_ms=statistics.median(wall), kernel_ms_all=km, wall_ms_all=wall,
                          kernel_ms_parts={q: v for q, v in mid.items() if q != "binning"})
            if k.startswith("polygon"):
                b = [x[2]["binning"] for x in r]
                res[k]["binning_ms"] = statistics.median(b)
                res[k]["binning_ms_all"] = b
        out["sizes"][str(n)] = res
        for k in BODIES:
            print(n, k, f"kernel {res[k]['kernel_ms']:.3f} ms (spread {res[k]['kernel_ms_spread']:.2f})  "
                  + (f"binning {res[k]['binning_ms']:.3f} ms  " if "binning_ms" in res[k] else "")
                  + f"wall {res[k]['wall_ms']:.1f} ms  cut cells {res[k]['cut_cells']}  "
                  + " ".join(f"{q} {v:.3f}" for q, v in res[k]["kernel_ms_parts"].items()), flush=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
