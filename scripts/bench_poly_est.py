"""Measurement of precond="poly-est" (PG_PRECOND_POLY_EST): steps per second of the time loop with the
default options -- the plain BiCGStab loop on these systems, which is what the library did before the option existed -- against
the same loop with the polynomial preconditioner admitted on the estimated spectral disc.  Same solver family, same data, same
Krylov tolerance, one process, two solvers, windows alternating.

    python scripts/bench_poly_est.py [out.json] [workload ...]     (default: profiles/poly_est_bench.json c5 robin2048 diph3d128)

Workloads
  c5         config 5: 2-D diphasic 1024^2 (benchmark/Heat_2ph_2D.jl: box 8^2, disc r = 2, D = 1 / 2, He = 0.5, no borders),
             BE first solve then CN, Δt = 0.5 h²; also one window of 200 steps per path
  robin2048  monophasic 2048^2, fluid outside the disc r = 1 at (2.01, 2.01) of the 4 x 4 box, Robin(1, 1, 1) interface, four
             Dirichlet(0) borders, BE then CN
  diph3d128  3-D diphasic 128^3, the config-5 family with a sphere

5 warm-up steps, then REPEATS windows of 20 steps per path through pg_solver_run (the device-resident loop); the rate is that
of the median window, the spread (max - min) / median is reported.  Times are host clocks around work that ends in a device
synchronisation.  One more window per path runs with profiling on (HIP events around the SAMPLED product launches; not timed):
the profiler samples, so this is no count of the launches of a step; launches per step are derived instead: products + one vector
kernel per half-iteration + the step's start product and right-hand-side kernel.  The estimator's one-off cost, g_ritz, g_used and
Gershgorin's radius are recorded per matrix."""
import ctypes as C
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import penguin.jl_amd as pj
from penguin.jl_amd import _lib as L
from penguin.jl_amd.build import source_hash

ARGS = sys.argv[1:]
OUT = ARGS[0] if ARGS else "profiles/poly_est_bench.json"
WORKLOADS = ARGS[1:] or ["c5", "robin2048", "diph3d128"]
WARMUP, STEPS, REPEATS, LONG = 5, 20, 3, 200
KEYS = ("left", "right", "bottom", "top")
ZERO = 0.0


def sync():
    L.check(L.lib().pg_device_synchronize())


def diphasic(N, n):
    Lx = 8.0
    mesh = pj.Mesh((n,) * N, (Lx,) * N, (0.0,) * N)
    c1 = pj.Capacity(pj.Sphere((4.0,) * N, 2.0), mesh)
    c2 = pj.Capacity(pj.Sphere((4.0,) * N, 2.0, complement=True), mesh)
    keep = [pj.DiffusionOps(c1), pj.DiffusionOps(c2)]
    p1, p2 = pj.Phase(c1, keep[0], ZERO, 1.0), pj.Phase(c2, keep[1], ZERO, 2.0)
    ic = pj.InterfaceConditions(pj.ScalarJump(1.0, 0.5, 0.0), pj.FluxJump(1.0, 1.0, 0.0))
    M = (n + 1) ** N
    u0 = np.concatenate([np.ones(2 * M), np.zeros(2 * M)])
    dt = 0.5 * (Lx / n) ** 2
    return (lambda: pj.DiffusionUnsteadyDiph(p1, p2, pj.BorderConditions({}), ic, dt, u0, "BE")), keep + [p1, p2, c1, c2]


def robin(n):
    mesh = pj.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0, complement=True), mesh)
    op = pj.DiffusionOps(cap)
    ph = pj.Phase(cap, op, ZERO, 1.0)
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS})
    M = (n + 1) ** 2
    dt = 0.5 * (4.0 / n) ** 2
    return (lambda: pj.DiffusionUnsteadyMono(ph, bcb, pj.Robin(1.0, 1.0, 1.0), dt, np.ones(2 * M), "BE")), [op, ph, cap]


SPEC = {"c5": lambda: diphasic(2, 1024), "robin2048": lambda: robin(2048), "diph3d128": lambda: diphasic(3, 128)}


def opts_of(precond):
    return pj.api._krylov_opts("bicgstab", {"reltol": 1e-12, "precond": precond})


def window(s, opts, steps):
    run = L.pg_run_info()
    sync()
    t0 = time.perf_counter()
    L.check(L.lib().pg_solver_run(s._h, C.c_double(1e300), C.c_int32(L.PG_SCHEME["CN"]), C.byref(opts), C.c_int32(0), C.c_int64(steps),
                                  C.c_int32(0), C.byref(run)))
    sync()
    return time.perf_counter() - t0, run


def measure(name):
    make, keep = SPEC[name]()
    paths = {"default": (make(), opts_of(0)), "poly_est": (make(), opts_of("poly-est"))}
    first = {}
    for key, (s, o) in paths.items():
        info = L.pg_step_info()
        sync()
        t0 = time.perf_counter()
        L.check(L.lib().pg_solver_initial_solve(s._h, C.byref(o), C.byref(info)))
        sync()
        first[key] = dict(ms=(time.perf_counter() - t0) * 1e3, iters=info.iters, converged=bool(info.converged))
        window(s, o, WARMUP)
    wins = {k: [] for k in paths}
    runs = {k: [] for k in paths}
    for _ in range(REPEATS):
        for key, (s, o) in paths.items():
            t, run = window(s, o, STEPS)
            assert run.unconverged_steps == 0
            wins[key].append(t)
            runs[key].append(run)
    res = {}
    for key, (s, o) in paths.items():
        tot = REPEATS * STEPS
        med = statistics.median(wins[key])
        res[key] = dict(steps_per_s=STEPS / med, ms_per_step=1e3 * med / STEPS, windows_s=wins[key],
                        window_spread=(max(wins[key]) - min(wins[key])) / med,
                        products_per_step=sum(r.products for r in runs[key]) / tot, iters_per_step=sum(r.total_iters for r in runs[key]) / tot,
                        half_exits_per_step=sum(r.half_exits for r in runs[key]) / tot,
                        poly_degree_last=int(runs[key][-1].poly_degree), poly_xspace=int(runs[key][-1].poly_xspace),
                        first_solve=first[key], guess_states_kept=s.guess_info()["kept"])
    for x in res.values():
        # one launch per product (Horner step or closing product), one vector kernel per half-iteration, the step's start product
        # and right-hand-side kernel; unfolded scalar-phase launches and the extrapolation's fit kernel are not counted
        x["derived_launches_per_step"] = x["products_per_step"] + 2.0 * x["iters_per_step"] - x["half_exits_per_step"] + 2.0
    if name == "c5":
        for key, (s, o) in paths.items():
            t, run = window(s, o, LONG)
            res[key]["long_window"] = dict(steps=LONG, steps_per_s=LONG / t, ms_per_step=1e3 * t / LONG, products_per_step=run.products / LONG,
                                           unconverged=int(run.unconverged_steps))
    L.check(L.lib().pg_set_profiling(1))
    for key, (s, o) in paths.items():
        _, run = window(s, o, STEPS)
        res[key]["sampled_product_launches_per_step"] = (run.spmv_launches + run.spmv_lean_launches) / STEPS
    L.check(L.lib().pg_set_profiling(0))
    a, b = paths["default"][0], paths["poly_est"][0]
    si = b.system_info(1)
    est = {("constructor (BE)" if w == 0 else "run (CN)"): b.spectral_estimate(w, run=False) for w in (0, 1)}
    return dict(workload=name, rows=int(si.n_own), nnz=int(si.nnz), default=res["default"], poly_est=res["poly_est"],
                speedup_steps=res["poly_est"]["steps_per_s"] / res["default"]["steps_per_s"], estimate=est,
                state_rel_l2_between_paths=float(np.linalg.norm(b._fetch_state() - a._fetch_state()) / np.linalg.norm(a._fetch_state())))


pj.init(0)
out = dict(what="time loop with the default options (plain BiCGStab on these systems) against precond=\"poly-est\", one rank",
           warmup_steps=WARMUP, steps_per_window=STEPS, windows=REPEATS, reltol=1e-12, device=pj.device_name(),
           source_hash=source_hash(), config=pj.config_string(), results=[])
for name in WORKLOADS:
    r = measure(name)
    out["results"].append(r)
    print(json.dumps({k: r[k] for k in ("workload", "rows", "speedup_steps")}), f"default {r['default']['steps_per_s']:.1f} steps/s "
          f"{r['default']['products_per_step']:.1f} products, poly-est {r['poly_est']['steps_per_s']:.1f} steps/s "
          f"{r['poly_est']['products_per_step']:.1f} products (degree {r['poly_est']['poly_degree_last']})", flush=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
print(f"wrote {OUT}")
