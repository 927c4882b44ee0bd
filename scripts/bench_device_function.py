"""Measurement of device functions (pj.DeviceFunction, DESIGN.md "Device functions"): steps per second of the unsteady monophasic
loop, one process, windows alternating, on the problem of scripts/bench_time_separable.py -- heat inside a sphere / disc r = 1 at
(2.01, ..) of the 4^N box, Dirichlet interface, four Dirichlet(0) borders, Δt = 0.5 h², reltol = 1e-12 -- with

  a  host      a source that is NOT separable (a Gaussian moving at constant speed) and g(t) as plain closures: the host-driven
               loop of api.solve_DiffusionUnsteadyMono_b, statement for statement -- the only path such data had
  b  program   the same closures as DeviceFunction: programs installed once, windows of pg_solver_run
  c  separable the separable datum of bench_time_separable.py, φ(x) sin(ωt) and g(t), as TimeSeparable
  d  sep-prog  that same datum written as a DeviceFunction: d / c is the price of evaluation against streaming modes
  p5           (3d128 only) the source of the reference's Schwartz-Colella heat problem as a DeviceFunction

    python scripts/bench_device_function.py [out.json] [workload ...]   (default: profiles/device_function_bench.json, all six)

Workloads: 3d128-BE, 3d128-CN, 3d256-BE, 3d256-CN, 2d2048-BE, 2d2048-CN.  5 warm-up steps, then 3 windows of 20 steps per path,
alternating; the rate is that of the median window, the spread (max - min) / median is reported.  The evaluation kernel of path
b is timed alone (pg_debug_td_eval_ms: 200 evaluations between two events) and reported in µs and as entries · instructions per
second.  Every ratio is reported as found."""
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
OUT = ARGS[0] if ARGS else "profiles/device_function_bench.json"
ALL = ["3d128-BE", "3d128-CN", "3d256-BE", "3d256-CN", "2d2048-BE", "2d2048-CN"]
WORKLOADS = ARGS[1:] or ALL
WARMUP, STEPS, REPEATS = 5, 20, 3
KEYS = ("left", "right", "bottom", "top")


def sync():
    L.check(L.lib().pg_device_synchronize())


def problem(N, n):
    mesh = pj.Mesh((n,) * N, (4.0,) * N, (0.0,) * N)
    cap = pj.Capacity(pj.Sphere((2.01,) * N, 1.0), mesh)
    op = pj.DiffusionOps(cap)
    dt = 0.5 * (4.0 / n) ** 2
    om = 2.0 * math.pi / (20.0 * dt)
    v = 0.5 / (65.0 * dt)                                   # the Gaussian crosses half a radius during the measurement
    gauss = lambda x, y, z, t: np.exp(-((x - 1.7 - v * t) ** 2 + (y - 2.0) ** 2 + (z - 2.0 * (N == 3)) ** 2) / 0.3)
    g_t = lambda x, y, z, t: 1.0 + 0.5 * np.sin(om * t)
    sep_f = lambda x, y, z, t: (1.0 + 0.5 * x) * np.sin(om * t)
    p5 = lambda x, y, z, t: 4.0 * (((x - 2.0) ** 2 + (y - 2.0) ** 2 + (z - 2.0) ** 2) + 5.0 * (t + 1.0)) / (125.0 * np.pi * (t + 1.0) ** 3) \
        * np.exp(-((x - 2.0) ** 2 + (y - 2.0) ** 2 + (z - 2.0) ** 2) / (5.0 * (t + 1.0)))
    data = dict(
        host=(gauss, g_t),
        program=(pj.DeviceFunction(gauss), pj.DeviceFunction(g_t)),
        separable=(pj.TimeSeparable([(lambda x, y, z: 1.0 + 0.5 * x, lambda t: math.sin(om * t))]),
                   pj.TimeSeparable([(1.0, lambda t: 1.0 + 0.5 * math.sin(om * t))])),
        sep_prog=(pj.DeviceFunction(sep_f), pj.DeviceFunction(g_t)))
    if N == 3 and n == 128:
        data["p5"] = (pj.DeviceFunction(p5), pj.DeviceFunction(g_t))
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS})
    return cap, op, bcb, dt, data


class HostLoop:
    """The host-driven loop of api.solve_DiffusionUnsteadyMono_b, resumable window by window."""

    def __init__(self, s, phase, bc, dt, scheme, opts):
        self.s, self.phase, self.bc, self.dt, self.scheme, self.opts = s, phase, bc, dt, scheme, opts
        self.t, self.sent = 0.0, api._UploadCache()

    def window(self, steps):
        s, phase, bc, Δt, opts = self.s, self.phase, self.bc, self.dt, self.opts
        cap, M, sch = phase.capacity, s._ctx["M"], L.PG_SCHEME[self.scheme]
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
    times = api._program_times(dt, 1e300, total)
    sol, phases, bcs = {}, {}, {}
    for key, (f, g) in data.items():
        phases[key] = pj.Phase(cap, op, f, 1.0)
        bcs[key] = pj.Dirichlet(g)
        s = pj.DiffusionUnsteadyMono(phases[key], bcb, bcs[key], dt, None, scheme)
        info = L.pg_step_info()
        L.check(L.lib().pg_solver_initial_solve(s._h, C.byref(opts), C.byref(info)))
        sol[key] = s
        if key == "separable":
            api._install_separable(s, api._TD_SOURCE, 0, api._separable_fields(f, cap._cw, 3, M), api._separable_table(f, dt, 1e300, total))
            api._install_separable(s, api._TD_INTERFACE, 0, api._separable_fields(g, cap._cg, 3, M), api._separable_table(g, dt, 1e300, total))
        elif key != "host":
            api._install_program(s, api._TD_SOURCE, 0, f, 3, times)
            api._install_program(s, api._TD_INTERFACE, 0, g, 3, times)
    host = HostLoop(sol["host"], phases["host"], bcs["host"], dt, scheme, opts)
    device_keys = [k for k in data if k != "host"]
    host.window(WARMUP)
    for key in device_keys:
        run_window(sol[key], opts, scheme, WARMUP)
    wins = {k: [] for k in data}
    runs = {k: [] for k in device_keys}
    for _ in range(REPEATS):
        wins["host"].append(host.window(STEPS))
        print(f"  {name}: host window {wins['host'][-1]:.2f} s", flush=True)
        for key in device_keys:
            t, run = run_window(sol[key], opts, scheme, STEPS)
            wins[key].append(t)
            runs[key].append(run)
    res = {}
    for key in data:
        med = statistics.median(wins[key])
        res[key] = dict(steps_per_s=STEPS / med, ms_per_step=1e3 * med / STEPS, windows_s=wins[key],
                        window_spread=(max(wins[key]) - min(wins[key])) / med)
    for key in device_keys:
        res[key]["products_per_step"] = sum(r.products for r in runs[key]) / (REPEATS * STEPS)
    kern = {}
    for key in [k for k in device_keys if k != "separable"]:
        ms, ne, ni = C.c_double(0.0), C.c_int64(0), C.c_int64(0)
        L.check(L.lib().pg_debug_td_eval_ms(sol[key]._h, C.c_int32(L.PG_SCHEME[scheme]), C.c_int32(200), C.byref(ms), C.byref(ne), C.byref(ni)))
        kern[key] = dict(us=ms.value * 1e3, entries=ne.value, instructions=ni.value,
                         entry_instructions_per_s=ni.value / (ms.value * 1e-3) if ms.value > 0 else None,
                         source_program_ops=int(data[key][0].program.n_ops), share_of_step=ms.value / res[key]["ms_per_step"])
    xh, xd = sol["host"]._fetch_state(), sol["program"]._fetch_state()
    return dict(workload=name, N=N, n=n, scheme=scheme, M_padded=M, rows=int(sol["program"].system_info(1).n_own), dt=dt, **res,
                program_over_host=res["program"]["steps_per_s"] / res["host"]["steps_per_s"],
                sep_prog_over_separable=res["sep_prog"]["steps_per_s"] / res["separable"]["steps_per_s"],
                eval_kernel=kern, state_rel_l2_program_vs_host=float(np.linalg.norm(xd - xh) / np.linalg.norm(xh)))


pj.init(0)
out = dict(what="unsteady monophasic loop: host-driven loop on plain closures (a) / the same closures as DeviceFunction (b) / "
                "TimeSeparable (c) / the separable datum as DeviceFunction (d) / the Schwartz-Colella source (3d128), one rank",
           warmup_steps=WARMUP, steps_per_window=STEPS, windows=REPEATS, reltol=1e-12, device=pj.device_name(),
           source_hash=source_hash(), config=pj.config_string(), not_measured=[w for w in ALL if w not in WORKLOADS], results=[])
for name in WORKLOADS:
    r = measure(name)
    out["results"].append(r)
    print(json.dumps({k: r[k] for k in ("workload", "rows", "program_over_host", "sep_prog_over_separable")}),
          " ".join(f"{k} {r[k]['steps_per_s']:.1f}/s (spread {r[k]['window_spread']:.2f})" for k in ("host", "program", "separable", "sep_prog")),
          "; eval kernel", {k: round(v["us"], 1) for k, v in r["eval_kernel"].items()}, "us", flush=True)
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
print(f"wrote {OUT}")
