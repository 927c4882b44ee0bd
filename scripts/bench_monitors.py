"""Measurement of monitors and the thinned state history (pj.Monitor ..., save_every; DESIGN.md "Monitors"): steps per second of
the unsteady monophasic loop with constant data, four ways on the same problem, one process, four solvers, windows alternating:

  a  per_step     pg_solver_step + a full-state download per step, and the observables reduced from each state with numpy (a
                  phase mean, the interface flux, two point values) -- the only way to a history before monitors existed; its
                  code is unchanged, so this is also the parent commit's figure.  Each state is dropped once it is reduced (a
                  script that keeps them pays their host memory on top: 20 states of 256^3 are 5.4 GB).
  b  monitors     windows of pg_solver_run with VolumeIntegral + InterfaceFlux + 2 probes installed; the window's own 20 rows of
                  the series are fetched at its end (pg_solver_get_monitor_series(row0, 20), inside the timed region)
  c  plain        windows of pg_solver_run with nothing installed -- the default path
  d  monitors_10  as b with save_every = 10: the two kept states are fetched and dropped at the end of every window

    python scripts/bench_monitors.py [--out profiles/monitors_bench.json] [--workloads 3d128-BE ...]
           [--device-loop-only] [--parent-json FILE] [--bench-before FILE] [--bench-after FILE]

--device-loop-only measures c alone and uses nothing the parent commit lacks: run from a checkout of the parent commit (this
file copied into it) it gives the parent's own device loop on the same box; --parent-json merges that file, and c must sit
inside the parent's window spread.  --bench-before / --bench-after: the JSON line of `python bench.py` on the parent commit and
on this one; its value and ms_per_step are recorded in the same file.

Workloads: heat inside a sphere / disc r = 1 at (2.01, ..) of the 4^N box, Dirichlet interface, four Dirichlet(0) borders,
constant source 1 + 0.5 x, Δt = 0.5 h², run scheme = constructor scheme: 3d128-BE, 3d128-CN, 3d256-BE, 3d256-CN, 2d2048-BE,
2d2048-CN.  reltol = 1e-12.  5 warm-up steps, then 3 windows of 20 steps per path, alternating; the rate is that of the median
window, the spread (max - min) / median is reported.  Times are host clocks around work that ends in a device synchronisation.
The evaluation kernel is timed alone (pg_debug_monitor_ms: 200 launches between two events) against the bytes it streams."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import penguin.jl_amd as pj
from penguin.jl_amd import _lib as L
from penguin.jl_amd import api
from penguin.jl_amd.build import source_hash

ALL = ["3d128-BE", "3d128-CN", "3d256-BE", "3d256-CN", "2d2048-BE", "2d2048-CN"]
ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/monitors_bench.json")
ap.add_argument("--workloads", nargs="*", default=ALL)
ap.add_argument("--device-loop-only", action="store_true")
ap.add_argument("--parent-json")
ap.add_argument("--bench-before")
ap.add_argument("--bench-after")
ARGS = ap.parse_args()
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
    ph = pj.Phase(cap, op, (lambda x, y, z: 1.0 + 0.5 * x), 1.0)
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS})
    return mesh, cap, ph, bcb, dt


def run_window(s, opts, scheme, steps, save_every=0, after=None):
    run = L.pg_run_info()
    sync()
    t0 = time.perf_counter()
    L.check(L.lib().pg_solver_run(s._h, C.c_double(1e300), C.c_int32(L.PG_SCHEME[scheme]), C.byref(opts), C.c_int32(0), C.c_int64(steps),
                                  C.c_int32(save_every), C.byref(run)))
    if after:
        after()
    sync()
    assert run.unconverged_steps == 0
    return time.perf_counter() - t0, run


def per_step_window(s, opts, scheme, steps, reduce):
    info = L.pg_step_info()
    sch = L.PG_SCHEME[scheme]
    sync()
    t0 = time.perf_counter()
    series = []
    for _ in range(steps):
        L.check(L.lib().pg_solver_step(s._h, C.c_int32(sch), C.byref(opts), C.byref(info)))
        assert info.converged
        s.x = s._fetch_state()
        series.append(reduce(s.x))
    return time.perf_counter() - t0, np.array(series)


def summary(wins):
    med = statistics.median(wins)
    return dict(steps_per_s=STEPS / med, ms_per_step=1e3 * med / STEPS, windows_s=wins, window_spread=(max(wins) - min(wins)) / med)


def measure(name):
    N, n, scheme = int(name[0]), int(name[2:].split("-")[0]), name.split("-")[1]
    mesh, cap, ph, bcb, dt = problem(N, n)
    M = (n + 1) ** N
    opts = api._krylov_opts("bicgstab", {"reltol": 1e-12})
    paths = ["plain"] if ARGS.device_loop_only else ["per_step", "monitors", "plain", "monitors_10"]
    sol = {}
    for key in paths:
        sol[key] = pj.DiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(1.0), dt, None, scheme)
    res = dict(workload=name, N=N, n=n, scheme=scheme, M_padded=M, dt=dt)
    if not ARGS.device_loop_only:
        centre = tuple(2.01 for _ in range(N))
        off = tuple(2.01 + (0.5 if d == 0 else 0.0) for d in range(N))
        mons = [pj.VolumeIntegral(cap), pj.InterfaceFlux(ph), pj.Probe(mesh, centre), pj.Probe(mesh, off)]
        W = api._monitor_weights(mons, 2 * M)
        for key in ("monitors", "monitors_10"):
            api._install_monitors(sol[key], mons)
        reduce = lambda x: [W[0] @ x, W[1] @ x, x[mons[2].cell], x[mons[3].cell]]
    info = L.pg_step_info()
    for key in paths:
        L.check(L.lib().pg_solver_initial_solve(sol[key]._h, C.byref(opts), C.byref(info)))

    series = {"monitors": [], "monitors_10": []}

    def fetch_series(key):
        def fetch():                     # the rows this window added, and only those
            K, rows = C.c_int32(0), C.c_int64(0)
            L.check(L.lib().pg_solver_monitor_info(sol[key]._h, C.byref(K), C.byref(rows), None, None))
            nr = min(rows.value, STEPS)
            vals, times = np.zeros((nr, K.value)), np.zeros(nr)
            L.check(L.lib().pg_solver_get_monitor_series(sol[key]._h, C.c_int64(rows.value - nr), C.c_int64(nr), L.dptr(vals), L.dptr(times)))
            series[key].append(vals)
        return fetch

    def fetch_kept():
        fetch_series("monitors_10")()
        sol["monitors_10"].states, sol["monitors_10"].state_steps = [], []
        api._fetch_kept_states(sol["monitors_10"], 10)

    def window(key, steps):
        if key == "per_step":
            return per_step_window(sol[key], opts, scheme, steps, reduce)
        if key == "monitors":
            return run_window(sol[key], opts, scheme, steps, 0, fetch_series(key))
        if key == "monitors_10":
            return run_window(sol[key], opts, scheme, steps, 10, fetch_kept)
        return run_window(sol[key], opts, scheme, steps)

    for key in paths:
        window(key, WARMUP)
    wins = {k: [] for k in paths}
    runs = {k: [] for k in paths}
    host_series = []
    for _ in range(REPEATS):
        for key in paths:
            t, extra = window(key, STEPS)
            wins[key].append(t)
            if key == "per_step":
                host_series.append(extra)
            else:
                runs[key].append(extra)
        print(f"  {name}: windows " + ", ".join(f"{k} {wins[k][-1] * 1e3:.1f} ms" for k in paths), flush=True)
    tot = REPEATS * STEPS
    for key in paths:
        res[key] = summary(wins[key])
        if key != "per_step":
            res[key].update(iters_per_step=sum(r.total_iters for r in runs[key]) / tot, products_per_step=sum(r.products for r in runs[key]) / tot)
    res["rows"] = int(sol["plain"].system_info(1).n_own)
    if not ARGS.device_loop_only:
        s = sol["monitors"]
        # the device series against the numpy reduction of the per-step path: the same problem, the same numbers
        dev = np.concatenate(series["monitors"][-REPEATS:])
        ref = np.concatenate(host_series)
        res["series_max_rel_diff_device_vs_numpy"] = float(np.max(np.abs(dev - ref) / np.maximum(np.abs(ref), 1e-300)))
        K, rows = C.c_int32(0), C.c_int64(0)
        sparse, stored = (C.c_int32 * 8)(), (C.c_int64 * 8)()
        L.check(L.lib().pg_solver_monitor_info(s._h, C.byref(K), C.byref(rows), sparse, stored))
        ms, nbytes = C.c_double(0.0), C.c_int64(0)
        L.check(L.lib().pg_solver_step(s._h, C.c_int32(L.PG_SCHEME[scheme]), C.byref(opts), C.byref(info)))    # (the state as z again)
        L.check(L.lib().pg_debug_monitor_ms(s._h, C.c_int32(200), C.byref(ms), C.byref(nbytes)))
        res["kernel"] = dict(sparse=list(sparse)[:K.value], stored=list(stored)[:K.value], bytes=nbytes.value, ms=ms.value,
                             ms_at_6p3_TBs=nbytes.value / (STREAM_TBS * 1e12) * 1e3,
                             achieved_TBs=nbytes.value / (ms.value * 1e-3) / 1e12 if ms.value > 0 else None,
                             share_of_plain_step=ms.value / res["plain"]["ms_per_step"])
        res["monitors_over_per_step"] = res["monitors"]["steps_per_s"] / res["per_step"]["steps_per_s"]
        res["monitors_over_plain"] = res["monitors"]["steps_per_s"] / res["plain"]["steps_per_s"]
        res["monitors_10_over_plain"] = res["monitors_10"]["steps_per_s"] / res["plain"]["steps_per_s"]
    return res


def load_bench_line(path):
    if not path:
        return None
    for line in reversed(open(path).read().splitlines()):
        line = line.strip()
        if line.startswith("{"):
            return json.loads(line)
    return None


pj.init(0)
out = dict(what="unsteady monophasic loop, constant data, one rank: (a) per-step branch with a state download per step and the "
                "observables reduced with numpy / (b) device loop with 4 monitors / (c) device loop, nothing installed / (d) as (b) "
                "with save_every = 10",
           warmup_steps=WARMUP, steps_per_window=STEPS, windows=REPEATS, reltol=1e-12, device=pj.device_name(),
           source_hash=source_hash(), config=pj.config_string(), device_loop_only=ARGS.device_loop_only,
           not_measured=[w for w in ALL if w not in ARGS.workloads], results=[])
if ARGS.parent_json:
    parent = json.load(open(ARGS.parent_json))
    out["parent_commit_device_loop"] = dict(source_hash=parent["source_hash"],
                                            results={r["workload"]: r["plain"] for r in parent["results"]})
for key, path in (("bench_py_parent_commit", ARGS.bench_before), ("bench_py_this_commit", ARGS.bench_after)):
    line = load_bench_line(path)
    if line is not None:
        out[key] = {k: line[k] for k in ("metric", "value", "unit", "steps", "warmup", "ms_per_step") if k in line}
for name in ARGS.workloads:
    r = measure(name)
    if ARGS.parent_json and name in out["parent_commit_device_loop"]["results"]:
        p = out["parent_commit_device_loop"]["results"][name]
        lo, hi = STEPS / max(p["windows_s"]), STEPS / min(p["windows_s"])
        r["plain_inside_parent_window_spread"] = bool(lo <= r["plain"]["steps_per_s"] <= hi)
        r["parent_plain_steps_per_s"] = p["steps_per_s"]
        r["parent_plain_window_range_steps_per_s"] = [lo, hi]
    out["results"].append(r)
    print(json.dumps({k: r[k] for k in r if not isinstance(r[k], dict)}), flush=True)
    for k in ("per_step", "monitors", "plain", "monitors_10"):
        if k in r:
            print(f"    {k}: {r[k]['steps_per_s']:.1f} steps/s (spread {r[k]['window_spread']:.2f})", flush=True)
    with open(ARGS.out, "w") as fh:
        json.dump(out, fh, indent=1)
print(f"wrote {ARGS.out}")
