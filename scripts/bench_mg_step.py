"""Measurement of precond="mg-step" (the cell-aggregated V-cycle inside the unsteady time loop) against the default options on
the same problem, at steps that do not shrink with the mesh (the reference's examples take Δt = 0.01 on every mesh).

    python scripts/bench_mg_step.py [out.json] [case ...]        (default: profiles/mg_step_bench.json, every case)

Method.  One solver per PROCESS: the driver starts a fresh child for every window, the two options in alternating order (default,
mg-step, default, ...), WINDOWS windows each.  A child builds the problem, runs the first solve and STEPS warm-up steps (code
objects, work vectors, the hierarchies and the loop's adaptive choices settle there), then times STEPS steps of pg_solver_run
between two device synchronisations.  Reported per case and option: the median window with the smallest and largest (spread),
products, iterations and unconverged solves per step, and for mg-step the set-up ms, rows per level and bytes of the hierarchies.
One more child per option runs the same window with profiling on and PG_PROFILE_SAMPLE=1 (HIP events around EVERY bracket; its
wall time is not used): launches per step as the library counts them -- the launches that apply Â with fused dots, and the
lean ones, where a V-cycle is bracketed as a whole and counts as ONE (its kernels are 6 x tail_level + 1, so a step of the option
launches about applications x (6 x tail_level + 3) + 4 kernels: `kernels_per_step_estimate`) -- and the mean time of a V-cycle,
from which the V-cycle's share of a step follows: share = ms per V-cycle x applications per step / ms per step.  `rel_l2_between_the_two` is taken on the final states of the
profiled children (the same number of steps from the same start).

Cases (box 4^N, Dirichlet(0) borders in 2-D, T = 0.2 at t = 0, interface value 1, source 1 + 0.3 x):
  cyl{n}-{be,cn}      outside the cylinder r = 1 about (2.01, 2.01), Dirichlet, Δt = 0.01: n = 512, 1024, 2048 (Δt / h² = 164, 655, 2621)
  sweep{r}-cn         the same at 1024², CN, Δt = r h²: r = 0.5, 8, 128, 2048 -- where the option starts to win
  sphere256-cn        inside the sphere r = 1 about (2.01, 2.01, 2.01), 256³, Dirichlet, Δt = 0.01 (Δt / h² = 41)
  robin1024-cn        the cylinder at 1024² with Robin(1, 1, 1), CN, Δt = 0.01
"""
import ctypes as C
import json
import statistics
import subprocess
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, ".")

STEPS = 20
WINDOWS = 3
RELTOL = 1e-12
KEYS = ("left", "right", "bottom", "top")
CHILD_LIMIT_S = 300


def cases():
    out = {}
    for n in (512, 1024, 2048):
        for sch in ("BE", "CN"):
            out[f"cyl{n}-{sch.lower()}"] = dict(N=2, n=n, scheme=sch, kind="dirichlet", dt=0.01)
    for r in (0.5, 8, 128, 2048):
        out[f"sweep{r}-cn"] = dict(N=2, n=1024, scheme="CN", kind="dirichlet", dt=r * (4.0 / 1024) ** 2)
    out["sphere256-cn"] = dict(N=3, n=256, scheme="CN", kind="dirichlet", dt=0.01)
    out["robin1024-cn"] = dict(N=2, n=1024, scheme="CN", kind="robin", dt=0.01)
    return out


def child(name, precond, profile):
    import os

    if profile:
        os.environ["PG_PROFILE_SAMPLE"] = "1"                      # (read once, when the library starts)
    import penguin.jl_amd as pj
    from penguin.jl_amd import _lib as L
    from penguin.jl_amd import api

    c = cases()[name]
    pj.init(0)
    N, n = c["N"], c["n"]
    mesh = pj.Mesh((n,) * N, (4.0,) * N, (0.0,) * N)
    body = pj.Sphere((2.01,) * N, 1.0, complement=(N == 2))
    cap = pj.Capacity(body, mesh)
    ph = pj.Phase(cap, pj.DiffusionOps(cap), lambda x, y, z=0.0: 1.0 + 0.3 * x, lambda x, y, z=0.0: 1.0)
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS} if N == 2 else {})
    bci = pj.Dirichlet(1.0) if c["kind"] == "dirichlet" else pj.Robin(1.0, 1.0, 1.0)
    M = (n + 1) ** N
    s = pj.DiffusionUnsteadyMono(ph, bcb, bci, c["dt"], np.concatenate([0.2 * np.ones(M), np.ones(M)]), c["scheme"])
    opts = api._krylov_opts("bicgstab", {"precond": precond if precond == "mg-step" else 0, "reltol": RELTOL})
    sch = L.PG_SCHEME[c["scheme"]]
    sync = lambda: L.check(L.lib().pg_device_synchronize())

    def run(steps, initial):
        info = L.pg_run_info()
        L.check(L.lib().pg_solver_run(s._h, C.c_double(1e300), C.c_int32(sch), C.byref(opts), C.c_int32(initial), C.c_int64(steps),
                                      C.c_int32(0), C.byref(info)))
        return info

    run(STEPS, 1)                                                  # the first solve and the warm-up
    if profile:
        L.check(L.lib().pg_set_profiling(1))
    sync()
    t0 = time.perf_counter()
    info = run(STEPS, 0)
    sync()
    ms = (time.perf_counter() - t0) * 1e3
    out = {"ms_per_step": ms / STEPS, "steps_per_s": STEPS / (ms * 1e-3), "products_per_step": info.products / STEPS,
           "iterations_per_step": info.total_iters / STEPS, "unconverged_steps": int(info.unconverged_steps),
           "worst_relres": info.worst_relres, "poly_degree": int(info.poly_degree), "unknowns": int(s.system_info(0).n_own),
           "dt_over_h2": c["dt"] / (4.0 / n) ** 2}
    if profile:
        out.update(launches_with_dots_per_step=info.spmv_launches / STEPS, lean_launches_per_step=info.spmv_lean_launches / STEPS,
                   ms_per_lean_launch=(info.spmv_lean_ms_total / info.spmv_lean_launches) if info.spmv_lean_launches else None,
                   ms_per_launch_with_dots=(info.spmv_ms_total / info.spmv_launches) if info.spmv_launches else None)
        x = s._fetch_state()
        idx = np.random.default_rng(7).integers(0, len(x), size=min(len(x), 20000))
        out["state_sample"] = [float(v) for v in x[idx]]
    if precond == "mg-step":
        h = s.mg_step_info()[0]
        out["hierarchy"] = {"setup_ms": h["setup_ms"], "rows": h["rows"], "nnz": h["nnz"], "tail_level": h["tail_level"],
                            "bytes": int(h["bytes"]), "kernels_per_vcycle": 6 * h["tail_level"] + 1}
    print("RESULT " + json.dumps(out), flush=True)


def spawn(name, precond, profile=False):
    try:
        r = subprocess.run([sys.executable, __file__, "--child", name, precond, "1" if profile else "0"], capture_output=True, text=True,
                           timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"{name} {precond}: a child ran into its time limit of {CHILD_LIMIT_S} s; nothing more is started")
    if r.returncode != 0:                                          # (a child that died: nothing more is started on the device)
        raise SystemExit(f"{name} {precond}: a child ended with status {r.returncode}; nothing more is started\n{r.stderr[-2000:]}")
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise SystemExit(f"{name} {precond}: a child printed no result\n{r.stdout[-2000:]}")


def measure(name):
    win = {"default": [], "mg-step": []}
    for _ in range(WINDOWS):                                       # alternating, a fresh process each
        for p in win:
            win[p].append(spawn(name, p))
    prof = {p: spawn(name, p, profile=True) for p in win}
    res = {"case": name, **cases()[name]}
    for p, ws in win.items():
        ms = [w["ms_per_step"] for w in ws]
        med = ws[ms.index(statistics.median(ms))]
        res[p] = dict(med, ms_windows=ms, ms_min=min(ms), ms_max=max(ms))
        pr = prof[p]
        res[p].update({k: pr[k] for k in ("launches_with_dots_per_step", "lean_launches_per_step", "ms_per_lean_launch",
                                          "ms_per_launch_with_dots")})
        res[p]["profile_sample"] = 1                              # (every bracket counted; a record with 3 counts every third)
        res["unknowns"], res["dt_over_h2"] = med["unknowns"], med["dt_over_h2"]
    a, b = np.array(prof["default"]["state_sample"]), np.array(prof["mg-step"]["state_sample"])
    res["rel_l2_between_the_two"] = float(np.linalg.norm(a - b) / np.linalg.norm(a))
    m = res["mg-step"]
    m["vcycle_share_of_a_step"] = m["ms_per_lean_launch"] * m["products_per_step"] / m["ms_per_step"]
    m["kernels_per_step_estimate"] = m["products_per_step"] * (m["hierarchy"]["kernels_per_vcycle"] + 2) + 4
    res["speedup"] = res["default"]["ms_per_step"] / m["ms_per_step"]
    return res


def main():
    args = [a for a in sys.argv[1:]]
    out = args[0] if args else "profiles/mg_step_bench.json"
    names = args[1:] or list(cases())
    try:
        with open(out) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {"steps_per_window": STEPS, "windows": WINDOWS, "reltol": RELTOL, "runs": []}
    if len(args) > 1 and args[1] == "--merge":                     # python scripts/bench_mg_step.py out.json --merge part.json ...
        for part in args[2:]:
            with open(part) as f:
                more = json.load(f)
            doc.update({k: v for k, v in more.items() if k != "runs"})
            doc["runs"] = [x for x in doc["runs"] if x["case"] not in {r["case"] for r in more["runs"]}] + more["runs"]
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print("wrote", out, "with", [r["case"] for r in doc["runs"]])
        return
    from penguin.jl_amd.build import source_hash

    doc["source_hash"] = source_hash()
    for name in names:
        r = measure(name)
        doc["runs"] = [x for x in doc["runs"] if x["case"] != name] + [r]
        d, m = r["default"], r["mg-step"]
        print(f"{name} (dt/h2 = {r['dt_over_h2']:.3g}, {r['unknowns']} unknowns): default {d['steps_per_s']:.1f} steps/s, "
              f"{d['products_per_step']:.1f} products/step; mg-step {m['steps_per_s']:.1f} steps/s, {m['products_per_step']:.1f} "
              f"V-cycles/step, share {m['vcycle_share_of_a_step']:.2f}, set-up {m['hierarchy']['setup_ms']:.1f} ms; "
              f"speedup {r['speedup']:.2f}", flush=True)
        with open(out, "w") as f:                                  # (after every case: a run cut short keeps what it measured)
            json.dump(doc, f, indent=1)
            f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            child(sys.argv[2], sys.argv[3], sys.argv[4] == "1")
    else:
        main()
