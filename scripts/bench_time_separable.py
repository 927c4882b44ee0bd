"""Measurement of time-separable data (pj.TimeSeparable, DESIGN.md "Time-separable data"): steps per second of the unsteady
monophasic loop with a source φ(x) sin(ωt) and a uniform interface value g(t), three ways on the same problem, one process,
three solvers, windows alternating:

  host      the host-driven loop on the data as plain closures -- what every time-dependent closure takes, and the only path
            before TimeSeparable existed: per step both closures evaluated twice in Python on all M padded points, what
            changed uploaded (pg_solver_set_source, pg_solver_set_interface_value), pg_solver_step, the state downloaded.  The
            loop body below is the one of api.solve_DiffusionUnsteadyMono_b, statement for statement.
  device    the same data as TimeSeparable: spatial parts and coefficient table installed once, windows of pg_solver_run
  constant  the same problem with the data frozen at t = 0 (constant source φ(x) sin(ω Δt), constant g): pg_solver_run with
            quiet steps (folded start, extrapolated start) -- the ceiling

    python scripts/bench_time_separable.py [out.json] [workload ...]    (default: profiles/time_separable_bench.json, all six)

Workloads: heat inside a sphere / disc r = 1 at (2.01, ..) of the 4^N box, Dirichlet interface, four Dirichlet(0) borders,
Δt = 0.5 h², run scheme = constructor scheme: 3d128-BE, 3d128-CN, 3d256-BE, 3d256-CN, 2d2048-BE, 2d2048-CN.  reltol = 1e-12.
5 warm-up steps, then 3 windows of 20 steps per path, alternating; the rate is that of the median window, the spread
(max - min) / median is reported.  Times are host clocks around work that ends in a device synchronisation (host: the state
download).  Products per step come from pg_run_info; the host-driven loop steps through pg_solver_step, whose pg_step_info
carries iterations only: its products are not measured, its iterations are.  The combine kernel of the device path is timed
alone (pg_debug_td_combine_ms: 200 launches between two events) against (J + 2) · 8 · n_own bytes at 6.3 TB/s."""
import ctypes as C
import json
import math
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import penguin.jl_amd as pj
from penguin.jl_amd import _lib as L
from penguin.jl_amd import api
from penguin.jl_amd.build import source_hash

ARGS = sys.argv[1:]
OUT = ARGS[0] if ARGS else "profiles/time_separable_bench.json"
ALL = ["3d128-BE", "3d128-CN", "3d256-BE", "3d256-CN", "2d2048-BE", "2d2048-CN"]
WORKLOADS = ARGS[1:] or ALL
WARMUP, STEPS, REPEATS = 5, 20, 3
KEYS = ("left", "right", "bottom", "top")
STREAM_TBS = 6.3            # what a streaming kernel reaches on this chip


def sync():
    L.check(L.lib().pg_device_synchronize())


def problem(N, n):
    mesh = pj.Mesh((n,) * N, (4.0,) * N, (0.0,) * N)
    cap = pj.Capacity(pj.Sphere((2.01,) * N, 1.0), mesh)
    op = pj.DiffusionOps(cap)
    dt = 0.5 * (4.0 / n) ** 2
    om = 2.0 * math.pi / (20.0 * dt)                  # one period of the forcing per window
    phi = lambda x, y, z: 1.0 + 0.5 * x
    a_f = lambda t: math.sin(om * t)
    a_g = lambda t: 1.0 + 0.5 * math.sin(om * t)
    data = dict(
        host=((lambda x, y, z, t: (1.0 + 0.5 * x) * math.sin(om * t)), (lambda x, y, z, t: 1.0 + 0.5 * math.sin(om * t))),
        device=(pj.TimeSeparable([(phi, a_f)]), pj.TimeSeparable([(1.0, a_g)])),
        constant=((lambda x, y, z: (1.0 + 0.5 * x) * math.sin(om * dt)), 1.0))
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS})
    return cap, op, bcb, dt, data


class HostLoop:
    """The host-driven loop of api.solve_DiffusionUnsteadyMono_b, resumable window by window."""

    def __init__(self, s, phase, bc, dt, scheme, opts):
        self.s, self.phase, self.bc, self.dt, self.scheme, self.opts = s, phase, bc, dt, scheme, opts
        self.t, self.sent, self.iters = 0.0, api._UploadCache(), 0

    def window(self, steps):
        s, phase, bc, Δt, scheme, opts = self.s, self.phase, self.bc, self.dt, self.scheme, self.opts
        cap, M, sch = phase.capacity, s._ctx["M"], L.PG_SCHEME[scheme]
        info = L.pg_step_info()
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.t += Δt
            t = self.t
            fn = api._padded_field(api._eval(phase.source, cap._cw, t, 3), M)
            fn1 = api._padded_field(api._eval(phase.source, cap._cw, t + Δt, 3), M)
            zero = np.zeros(M)
            fn, fn1 = (fn if fn is not None else zero), (fn1 if fn1 is not None else zero)
            if self.sent.changed("f", fn, fn1):
                L.check(L.lib().pg_solver_set_source(s._h, 0, L.dptr(fn), L.dptr(fn1)))
            gn, gn1 = api._eval(bc.value, cap._cg, t, 3), api._eval(bc.value, cap._cg, t + Δt, 3)
            gn = np.full(M, gn) if isinstance(gn, float) else gn
            gn1 = np.full(M, gn1) if isinstance(gn1, float) else gn1
            if self.sent.changed("g", gn, gn1):
                L.check(L.lib().pg_solver_set_interface_value(s._h, L.dptr(gn), L.dptr(gn1)))
            L.check(L.lib().pg_solver_step(s._h, C.c_int32(sch), C.byref(opts), C.byref(info)))
            assert info.converged
            self.iters += info.iters
            s.x = s._fetch_state()
        return time.perf_counter() - t0


def run_window(s, opts, scheme, steps):
    run = L.pg_run_info()
    sync()
    t0 = time.perf_counter()
    L.check(L.lib().pg_solver_run(s._h, C.c_double(1e300), C.c_int32(L.PG_SCHEME[scheme]), C.byref(opts), C.c_int32(0), C.c_int64(steps),
                                  C.c_int32(0), C.byref(run)))
    sync()
    assert run.unconverged_steps == 0
    return time.perf_counter() - t0, run


def measure(name):
    N, n, scheme = int(name[0]), int(name[2:].split("-")[0]), name.split("-")[1]
    cap, op, bcb, dt, data = problem(N, n)
    M = (n + 1) ** N
    opts = api._krylov_opts("bicgstab", {"reltol": 1e-12})
    total = WARMUP + REPEATS * STEPS
    sol, phases, bcs = {}, {}, {}
    for key, (f, g) in data.items():
        phases[key] = pj.Phase(cap, op, f, 1.0)
        bcs[key] = pj.Dirichlet(g)
        s = pj.DiffusionUnsteadyMono(phases[key], bcb, bcs[key], dt, None, scheme)
        info = L.pg_step_info()
        L.check(L.lib().pg_solver_initial_solve(s._h, C.byref(opts), C.byref(info)))
        sol[key] = s
    f, g = data["device"]
    api._install_separable(sol["device"], api._TD_SOURCE, 0, api._separable_fields(f, cap._cw, 3, M), api._separable_table(f, dt, 1e300, total))
    api._install_separable(sol["device"], api._TD_INTERFACE, 0, api._separable_fields(g, cap._cg, 3, M), api._separable_table(g, dt, 1e300, total))
    host = HostLoop(sol["host"], phases["host"], bcs["host"], dt, scheme, opts)
    host.window(WARMUP)
    for key in ("device", "constant"):
        run_window(sol[key], opts, scheme, WARMUP)
    host.iters = 0
    wins = {k: [] for k in data}
    runs = {k: [] for k in ("device", "constant")}
    for _ in range(REPEATS):
        wins["host"].append(host.window(STEPS))
        print(f"  {name}: host window {wins['host'][-1]:.2f} s", flush=True)
        for key in ("device", "constant"):
            t, run = run_window(sol[key], opts, scheme, STEPS)
            wins[key].append(t)
            runs[key].append(run)
    tot = REPEATS * STEPS
    res = {}
    for key in data:
        med = statistics.median(wins[key])
        res[key] = dict(steps_per_s=STEPS / med, ms_per_step=1e3 * med / STEPS, windows_s=wins[key],
                        window_spread=(max(wins[key]) - min(wins[key])) / med)
    res["host"].update(iters_per_step=host.iters / tot, products_per_step="not measured (pg_step_info carries iterations only)")
    for key in ("device", "constant"):
        res[key].update(iters_per_step=sum(r.total_iters for r in runs[key]) / tot, products_per_step=sum(r.products for r in runs[key]) / tot)
    # the two time-dependent paths solve the same problem
    xh, xd = sol["host"]._fetch_state(), sol["device"]._fetch_state()
    ms, J, nbytes = C.c_double(0.0), C.c_int32(0), C.c_int64(0)
    L.check(L.lib().pg_debug_td_combine_ms(sol["device"]._h, C.c_int32(L.PG_SCHEME[scheme]), C.c_int32(200), C.byref(ms), C.byref(J),
                                           C.byref(nbytes)))
    floor_ms = nbytes.value / (STREAM_TBS * 1e12) * 1e3
    si = sol["device"].system_info(1)
    return dict(workload=name, N=N, n=n, scheme=scheme, M_padded=M, rows=int(si.n_own), dt=dt, **res,
                device_over_host=res["device"]["steps_per_s"] / res["host"]["steps_per_s"],
                device_over_constant=res["device"]["steps_per_s"] / res["constant"]["steps_per_s"],
                combine=dict(modes=J.value, bytes=nbytes.value, ms=ms.value, ms_at_6p3_TBs=floor_ms,
                             achieved_TBs=nbytes.value / (ms.value * 1e-3) / 1e12 if ms.value > 0 else None,
                             share_of_device_step=ms.value / res["device"]["ms_per_step"]),
                state_rel_l2_device_vs_host=float(np.linalg.norm(xd - xh) / np.linalg.norm(xh)))


pj.init(0)
out = dict(what="unsteady monophasic loop with a source phi(x) sin(wt) and a uniform interface value g(t): host-driven loop (plain "
                "closures) / device loop (TimeSeparable) / device loop with constant data, one rank",
           warmup_steps=WARMUP, steps_per_window=STEPS, windows=REPEATS, reltol=1e-12, device=pj.device_name(),
           source_hash=source_hash(), config=pj.config_string(), not_measured=[w for w in ALL if w not in WORKLOADS], results=[])
for name in WORKLOADS:
    r = measure(name)
    out["results"].append(r)
    print(json.dumps({k: r[k] for k in ("workload", "rows", "device_over_host", "device_over_constant")}),
          f"host {r['host']['steps_per_s']:.2f} steps/s (spread {r['host']['window_spread']:.2f}), device {r['device']['steps_per_s']:.1f} "
          f"(spread {r['device']['window_spread']:.2f}, {r['device']['products_per_step']:.1f} products), constant "
          f"{r['constant']['steps_per_s']:.1f} (spread {r['constant']['window_spread']:.2f}, {r['constant']['products_per_step']:.1f} products); "
          f"combine {r['combine']['ms'] * 1e3:.1f} us for {r['combine']['bytes'] / 1e6:.1f} MB = {r['combine']['achieved_TBs']:.2f} TB/s",
          flush=True)
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
print(f"wrote {OUT}")
