"""Measurement of traced 3-D level sets as bodies: capacity construction time of

  sphere      a program sphere, sqrt((x - 2.01)^2 + (y - 1.97)^2 + (z - 2.03)^2) - 1, against Sphere with the same centre
  ellipsoid   an ellipsoid turned about two axes (semi-axes 1.4, 0.9, 1.1), which no tagged kind expresses: alone, 128^3
  torus       R = 1.2, r = 0.5, axis z: alone, 128^3

on Mesh((n, n, n), (4, 4, 4)), n = 64, 128, 256.

    python scripts/bench_levelset3d_capacity.py [out.json] [n ...]   (default: profiles/levelset3d_capacity_bench.json, 64 128 256)

One warm-up build per body, then three builds per body, alternating; the median is reported with the spread (max - min) /
median.  `kernel_ms` is the capacity's own event pair around its kernels, `wall_ms` the constructor seen from Python (tracing,
differentiation and the host-side gradient check included).  `kernel_ms_parts` are the five stages one by one, each between its
own pair of events (pg_capacity_kernel_ms_parts), from the build with the median `kernel_ms`; `classification_ms` is the sum of
the two stages that look at every cell (classify, stagger) and `quadrature_ms` the sum of the three that measure (cut cells,
sections, staggered cut boxes).  Every figure is reported as found: a program body is expected to lose against the closed form."""
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
OUT = ARGS[0] if ARGS else "profiles/levelset3d_capacity_bench.json"
SIZES = [int(a) for a in ARGS[1:]] or [64, 128, 256]
EXTRA_AT = 128
REPEATS = 3
C = (2.01, 1.97, 2.03)


def rotated_ellipsoid():
    ca, sa, cb, sb = math.cos(0.5), math.sin(0.5), math.cos(0.35), math.sin(0.35)
    m = (np.array([[1.0, 0.0, 0.0], [0.0, cb, sb], [0.0, -sb, cb]]) @ np.array([[ca, sa, 0.0], [-sa, ca, 0.0], [0.0, 0.0, 1.0]])) \
        / np.array((1.4, 0.9, 1.1))[:, None]
    k = m @ np.array((2.02, 1.97, 2.05))

    def phi(x, y, z):
        out = -1.0
        for i in range(3):
            u = float(m[i, 0]) * x + float(m[i, 1]) * y + float(m[i, 2]) * z - float(k[i])
            out = out + u * u
        return out
    return phi


def torus(x, y, z):
    return (np.sqrt((x - 2.03) ** 2 + (y - 1.96) ** 2) - 1.2) ** 2 + (z - 2.07) ** 2 - 0.25


BODIES = {
    "sphere": (lambda: pj.Sphere(C, 1.0), {}),
    "program sphere": (lambda: pj.DeviceFunction(lambda x, y, z: np.sqrt((x - C[0]) ** 2 + (y - C[1]) ** 2 + (z - C[2]) ** 2) - 1.0),
                       {"quadrature": "height"}),
}
EXTRA = {
    "program rotated ellipsoid": (lambda: pj.DeviceFunction(rotated_ellipsoid()), {"quadrature": "height"}),
    "program torus": (lambda: pj.DeviceFunction(torus), {"quadrature": "height"}),
}


def build(entry, mesh):
    make, kw = entry
    t0 = time.perf_counter()
    cap = pj.Capacity(make(), mesh, **kw)
    wall = (time.perf_counter() - t0) * 1e3
    return cap.kernel_ms, wall, cap


def main():
    pj.init(0)
    out = {"source_hash": source_hash(), "device": pj.device_name(), "repeats": REPEATS, "sizes": {}}
    for n in SIZES:
        mesh = pj.Mesh((n, n, n), (4.0, 4.0, 4.0), (0.0, 0.0, 0.0))
        bodies = dict(BODIES, **(EXTRA if n == EXTRA_AT else {}))
        runs = {k: [] for k in bodies}
        info = {}
        for k, entry in bodies.items():                      # warm-up, and what was built
            _, _, cap = build(entry, mesh)
            info[k] = {"cut_cells": int((cap.cell_types == -1).sum()), "volume": float(cap.V.sum()), "surface": float(cap.Γ.sum())}
        for _ in range(REPEATS):
            for k, entry in bodies.items():
                km, wall, cap = build(entry, mesh)
                runs[k].append((km, wall, cap.kernel_ms_parts))
        res = {}
        for k, r in runs.items():
            km, wall = [x[0] for x in r], [x[1] for x in r]
            parts = sorted(r, key=lambda x: x[0])[len(r) // 2][2]
            p = list(parts.values())
            res[k] = dict(info[k], kernel_ms=statistics.median(km), kernel_ms_spread=(max(km) - min(km)) / statistics.median(km),
                          wall_ms=statistics.median(wall), kernel_ms_all=km, wall_ms_all=wall, kernel_ms_parts=parts,
                          classification_ms=p[0] + p[3], quadrature_ms=p[1] + p[2] + p[4])
        res["program sphere / sphere, kernel_ms"] = res["program sphere"]["kernel_ms"] / res["sphere"]["kernel_ms"]
        res["sphere volume difference"] = abs(res["program sphere"]["volume"] - res["sphere"]["volume"])
        out["sizes"][str(n)] = res
        print(n, json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}), flush=True)
        for k in bodies:
            print("   ", k, f"kernel {res[k]['kernel_ms']:.3f} ms  wall {res[k]['wall_ms']:.1f} ms  cut cells {res[k]['cut_cells']}  "
                  f"classification {res[k]['classification_ms']:.3f}  quadrature {res[k]['quadrature_ms']:.3f}  "
                  + " ".join(f"{q} {v:.3f}" for q, v in res[k]["kernel_ms_parts"].items()), flush=True)
    with open(OUT, "w") as f:                                # one line per body
        sizes = ",\n".join("  %s: {\n%s\n  }" % (json.dumps(n), ",\n".join("   %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in r.items()))
                           for n, r in out["sizes"].items())
        head = "".join(" %s: %s,\n" % (json.dumps(k), json.dumps(out[k])) for k in ("source_hash", "device", "repeats"))
        f.write("{\n%s \"sizes\": {\n%s\n }\n}\n" % (head, sizes))


if __name__ == "__main__":
    main()
