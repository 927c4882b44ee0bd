"""Measurement of the 1-D liquid-motion (Stefan) path: time steps and Newton iterations per second of
solve_MovingLiquidDiffusionUnsteadyMono! on the one-phase benchmark shape (benchmark/Stefan_1d_1ph.jl:759-787: T₀ = 1, k = 1,
Ste = 1, lx = 10 x(0.1), x0 = 0.1, Tstart = 0.01, FluxJump(k, 0, ρL), Newton (20, 1e-12, 1e-12, 1), BE), fixed Δt.

    python scripts/liquid_bench.py [steps=40] [nx ...]          (default nx: 160 1280)

Δt = 0.5 (lx/160)² at every nx (the benchmark's Δt at nx = 160), so both sizes run the same number of steps.  Per nx: a
warm-up run of 2 steps, the timed run of `steps` steps (no device synchronisation besides the library's own), then a run of
the same length whose Newton iterations are split by host timers with a device synchronisation after each part: capacity
(the space-time Capacity), assembly (the moving solver of the rebuilt slab), solve, terms (pg_solver_stefan_terms).  The
timed run moves no state to the host until its end (save_states=False)."""
import json
import math
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import penguin.jl_amd as pj
from penguin.jl_amd import _lib as L
from penguin.jl_amd import liquid, moving

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
sizes = [int(a) for a in sys.argv[2:]] or [160, 1280]
pj.init(0)


def find_lambda():
    lo, hi = 1e-6, 5.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if mid * math.exp(mid * mid) * math.erf(mid) - 1.0 / math.sqrt(math.pi) > 0 else (mid, hi)
    return 0.5 * (lo + hi)


LAM = find_lambda()
pos = lambda t: 2 * LAM * math.sqrt(t)
lx, x0, t0 = 10.0 * pos(0.1), 0.1, 0.01
dt = 0.5 * (lx / 160) ** 2


def run(nx, nsteps):
    mesh = pj.Mesh((nx,), (lx,), (x0,))
    xi = pos(t0)
    cap = pj.Capacity(liquid._static(xi), pj.SpaceTimeMesh(mesh, [dt, 2 * dt]))
    ph = pj.Phase(cap, pj.DiffusionOps(cap), lambda x, y, z, t: 0.0, lambda x, y, z: 1.0)
    bcb = pj.BorderConditions({"bottom": pj.Dirichlet(1.0), "top": pj.Dirichlet(0.0)})
    ic = pj.InterfaceConditions(None, pj.FluxJump(1.0, 0.0, 1.0))
    u = np.array([1.0 - math.erf(x / (2 * math.sqrt(t0))) / math.erf(LAM) if x < xi else 0.0 for x in mesh.nodes[0]])
    s = pj.MovingLiquidDiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(0.0), dt, np.concatenate([u, u]), mesh, "BE")
    L.check(L.lib().pg_device_synchronize())
    t_start = time.perf_counter()
    s, res, xf_log, _ = pj.solve_MovingLiquidDiffusionUnsteadyMono_b(
        s, ph, xi, dt, t0, t0 + (nsteps - 1) * dt - 0.5 * dt, bcb, pj.Dirichlet(0.0), ic, mesh, "BE",
        Newton_params=(20, 1e-12, 1e-12, 1.0), adaptive_timestep=False, method="bicgstab", save_states=False)
    wall = time.perf_counter() - t_start
    iters = sum(len(v) for v in res.values())
    return wall, len(res), iters, xf_log[-1], s


def timed_split(nx, nsteps):
    """The same run with every part of a Newton iteration timed on the host behind a device synchronisation."""
    parts = {"capacity": 0.0, "assembly": 0.0, "solve": 0.0, "terms": 0.0}
    orig = (liquid._capacity, moving._create_step, moving._solve_current, liquid.stefan_terms)

    def timed(name, fn):
        def wrap(*a, **k):
            L.check(L.lib().pg_device_synchronize())
            t = time.perf_counter()
            out = fn(*a, **k)
            L.check(L.lib().pg_device_synchronize())
            parts[name] += time.perf_counter() - t
            return out
        return wrap

    liquid._capacity = timed("capacity", orig[0])
    moving._create_step = timed("assembly", orig[1])
    moving._solve_current = timed("solve", orig[2])
    liquid.stefan_terms = timed("terms", orig[3])
    try:
        _, nst, iters, _, _ = run(nx, nsteps)
    finally:
        liquid._capacity, moving._create_step, moving._solve_current, liquid.stefan_terms = orig
    return {k: v * 1e3 / iters for k, v in parts.items()}, iters


out = {"what": "solve_MovingLiquidDiffusionUnsteadyMono! on the benchmark/Stefan_1d_1ph.jl shape, BE, fixed dt",
       "dt": dt, "steps": steps, "device": pj.device_name(), "sizes": {}}
for nx in sizes:
    run(nx, 2)                                            # warm-up (first-use allocations, code objects)
    wall, nst, iters, xf, s = run(nx, steps)
    split, _ = timed_split(nx, steps)
    out["sizes"][str(nx)] = {
        "time_steps_per_s": nst / wall, "newton_iters_per_s": iters / wall, "mean_iters_per_step": iters / nst,
        "time_steps": nst, "newton_iters": iters, "ms_per_newton_iter": wall / iters * 1e3, "final_xf": xf,
        "rows": int(s.system_info(0).n_own), "per_iter_ms_synchronised": split}
print(json.dumps(out))
