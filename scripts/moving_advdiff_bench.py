"""Measurement of the prescribed-motion advection-diffusion path: slabs per second of solve_MovingAdvDiffusionUnsteadyMono! against
solve_MovingDiffusionUnsteadyMono! on the same translating body, same mesh, same slabs, one process.

    python scripts/moving_advdiff_bench.py [n=1024] [slabs=10] [scheme=BE] [state=host|device]
A disc of radius 2 translating at u = (2, 0) through a 16 x 16 box (fluid outside, as scripts/moving_bench.py's body),
Dirichlet(1) on the interface, Dirichlet(0) borders, Δt = h²; the advection-diffusion run has uₒ = uᵧ = (2, 0, 0) everywhere.
Each slab: space-time capacity, operators (DiffusionOps / ConvectionOps), moving solver, Krylov solve, and (state=host) the
state fetched to the host as the reference's push! does."""
import ctypes
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import penguin.jl_amd as pj
from penguin.jl_amd import _lib as L
from penguin.jl_amd import moving as mv

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
slabs = int(sys.argv[2]) if len(sys.argv) > 2 else 10
scheme = sys.argv[3] if len(sys.argv) > 3 else "BE"
DEVICE_STATE = len(sys.argv) > 4 and sys.argv[4] == "device"
pj.init(0)
lx = 16.0
mesh = pj.Mesh((n, n), (lx, lx), (-8.0, -8.0))
vx = 2.0
body = pj.MovingSphere(lambda t: (-1.0 + vx * t, 0.01), lambda t: 2.0, complement=True, dcenter=lambda t: (vx, 0.0),
                       dradius=lambda t: 0.0)
dt = (lx / n) ** 2
M = (n + 1) ** 2
uo = (np.full(2 * M, vx), np.zeros(2 * M), np.zeros(2 * M))
ug = np.concatenate([np.full(2 * M, vx), np.zeros(4 * M)])
bc = pj.Dirichlet(1.0)
bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in ("left", "right", "top", "bottom")})


def run(advdiff: bool):
    T = {"capacity_and_ops_s": 0.0, "create_solver_s": 0.0, "solve_s": 0.0, "state_fetch_s": 0.0}
    prev = [None]

    def slab(t, Ti, first=False):
        t0 = time.perf_counter()
        cap = pj.Capacity(body, pj.SpaceTimeMesh(mesh, [t, t + dt]))
        ph = pj.Phase(cap, pj.ConvectionOps(cap, uo, ug) if advdiff else pj.DiffusionOps(cap), 0.0, 1.0)
        L.check(L.lib().pg_device_synchronize())
        t1 = time.perf_counter()
        if first:
            s = (pj.MovingAdvDiffusionUnsteadyMono if advdiff else pj.MovingDiffusionUnsteadyMono)(ph, bcb, bc, dt, Ti, mesh, scheme)
        elif DEVICE_STATE:
            s = prev[0]
            mv._create_step(s, [ph], bcb, bc, dt, None, mesh, scheme, t, t, from_previous=True, advdiff=advdiff)
        else:
            s = pj.Solver("Unsteady", "Monophasic", "DiffusionAdvection" if advdiff else "Diffusion")
            s._nunk = 2 * M
            mv._create_step(s, [ph], bcb, bc, dt, Ti, mesh, scheme, t, t, advdiff=advdiff)
        L.check(L.lib().pg_device_synchronize())
        t2 = time.perf_counter()
        info = L.pg_step_info()
        opts = pj.api._krylov_opts("bicgstab", {})
        L.check(L.lib().pg_solver_initial_solve(s._h, ctypes.byref(opts), ctypes.byref(info)))
        L.check(L.lib().pg_device_synchronize())
        t3 = time.perf_counter()
        x = None if DEVICE_STATE else s._fetch_state(-1)
        prev[0] = s
        t4 = time.perf_counter()
        T["capacity_and_ops_s"] += t1 - t0
        T["create_solver_s"] += t2 - t1
        T["solve_s"] += t3 - t2
        T["state_fetch_s"] += t4 - t3
        assert info.converged
        return x, info.iters, s.system_info(0).n_own

    x, _, _ = slab(0.0, np.concatenate([np.zeros(M), np.ones(M)]), True)     # warm-up slab (first-use allocations)
    for k in T:
        T[k] = 0.0
    t_all = time.perf_counter()
    its, t = [], 0.0
    for _ in range(slabs):
        t += dt
        x, it, rows = slab(t, x)
        its.append(it)
    wall = time.perf_counter() - t_all
    out = {"slabs_per_s": slabs / wall, "ms_per_slab": wall / slabs * 1e3, "krylov_iters_per_slab": float(np.mean(its)),
           "rows_last_slab": int(rows), "per_slab_ms": {k: v * 1e3 / slabs for k, v in T.items()}}
    if x is None:
        x = prev[0]._fetch_state(-1)
    out["state_l2"] = float(np.linalg.norm(x))
    out["state_finite"] = bool(np.all(np.isfinite(x)))
    return out


res = {"what": "prescribed-motion mono, 2-D disc translating at (2, 0) (fluid outside), one space-time slab per step",
       "n": n, "cells": M, "scheme": scheme, "slabs": slabs,
       "state_between_slabs": "device" if DEVICE_STATE else "host (the reference's push!)",
       "MovingDiffusionUnsteadyMono": run(False), "MovingAdvDiffusionUnsteadyMono": run(True), "device": pj.device_name()}
res["advdiff_over_diffusion_rate"] = res["MovingAdvDiffusionUnsteadyMono"]["slabs_per_s"] / res["MovingDiffusionUnsteadyMono"]["slabs_per_s"]
print(json.dumps(res))
