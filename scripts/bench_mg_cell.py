"""Measurement of the cell-aggregated multigrid preconditioner (precond="mg-cell") on the two steady systems it was added for,
against the default options (the behaviour before it existed), one process, the two alternating:

  darcy   Darcy flow past an impermeable disc: -Δp = 0 outside the disc r = 1 about (2.01, 2.01) in the 4 x 4 box, p = 10 / 20 on
          the top / bottom border, Neumann(0) on the disc (examples/darcy_obstacle_mg.py)
  robin   Poisson outside a cylinder: -Δu = 1 outside the disc r = 0.5, u = 0 on the four borders, Robin(1, 1, 0.5) on the disc

    python scripts/bench_mg_cell.py [out.json] [n ...]        (default: profiles/mg_cell_bench.json 512 768 1024)

Per case, size and option: iterations, ms per solve (median of WINDOWS windows, each one cold solve from zero to reltol 1e-12 on
a solver that has solved once before -- the hierarchy exists, its set-up is reported apart), convergence, and for "mg-cell" the
set-up ms, rows per level and device bytes of the hierarchy; the largest |x| of each path and the relative L2 distance of the two
solutions tell whether the two ended at the same state.  A default solve that does not converge within maxiter is recorded
as such, with no ratio.  Times are host clocks around work that ends in a device synchronisation."""
import json
import statistics
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, ".")
import penguin.jl_amd as pj
from penguin.jl_amd import _lib as L
from penguin.jl_amd.build import source_hash

ARGS = sys.argv[1:]
OUT = ARGS[0] if ARGS else "profiles/mg_cell_bench.json"
SIZES = [int(a) for a in ARGS[1:]] or [512, 768, 1024]
WINDOWS = 3
RELTOL = 1e-12
KEYS = ("left", "right", "bottom", "top")


def sync():
    L.check(L.lib().pg_device_synchronize())


def darcy(n):
    mesh = pj.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0, complement=True), mesh)
    ph = pj.Phase(cap, pj.DiffusionOps(cap), lambda x, y, z=0.0: 0.0, lambda x, y, z=0.0: 1.0)
    bcb = pj.BorderConditions({"top": pj.Dirichlet(10.0), "bottom": pj.Dirichlet(20.0)})
    return (lambda: pj.DarcyFlow(ph, bcb, pj.Neumann(0.0))), pj.solve_DarcyFlow_b, (cap, ph, bcb)


def robin(n):
    mesh = pj.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 0.5, complement=True), mesh)
    ph = pj.Phase(cap, pj.DiffusionOps(cap), lambda x, y, z=0.0: 1.0, lambda x, y, z=0.0: 1.0)
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS})
    return (lambda: pj.DiffusionSteadyMono(ph, bcb, pj.Robin(1.0, 1.0, 0.5))), pj.solve_DiffusionSteadyMono_b, (cap, ph, bcb)


def one_solve(solver, solve, precond):
    sync()
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)            # (an unconverged default solve is recorded, not warned about)
        solve(solver, reltol=RELTOL, precond=precond, warm_start=False)
    sync()
    return (time.perf_counter() - t0) * 1e3


def measure(case, n):
    make, solve, keep = {"darcy": darcy, "robin": robin}[case](n)
    paths = {"default": (make(), 0), "mg-cell": (make(), "mg-cell")}
    ms = {k: [] for k in paths}
    for k, (s, p) in paths.items():                                # warm-up: code objects, work vectors, the hierarchy
        one_solve(s, solve, p)
    for _ in range(WINDOWS):                                       # alternating windows
        for k, (s, p) in paths.items():
            ms[k].append(one_solve(s, solve, p))
    out = {"case": case, "n": n, "unknowns": int(paths["default"][0].system_info(0).n_own)}
    for k, (s, p) in paths.items():
        ch = s.ch[-1]
        out[k] = {"iterations": int(ch["iters"]), "converged": bool(ch["converged"]),
                  "relres": float(ch["resnorm"] / ch["bnorm"]) if ch["bnorm"] > 0 else float(ch["resnorm"]),
                  "ms_per_solve": statistics.median(ms[k]), "ms_windows": ms[k], "max_abs_x": float(np.abs(s.x).max())}
    info = paths["mg-cell"][0].mg_info("mg-cell")
    out["mg-cell"].update(setup_ms=info["setup_ms"], rows=info["rows"], nnz=info["nnz"], tail_level=info["tail_level"],
                          bytes=int(info["bytes"]))
    a, b = paths["default"][0].x, paths["mg-cell"][0].x
    out["rel_l2_between_the_two"] = float(np.linalg.norm(a - b) / np.linalg.norm(a))
    if out["default"]["converged"] and out["mg-cell"]["converged"]:
        out["speedup_ms"] = out["default"]["ms_per_solve"] / out["mg-cell"]["ms_per_solve"]
    else:
        out["speedup_ms"] = None
        out["note"] = "a path did not converge within maxiter: no ratio"
    return out


def main():
    pj.init(0)
    res = {"device": pj.device_name(), "source_hash": source_hash(), "reltol": RELTOL, "windows": WINDOWS, "runs": []}
    for case in ("darcy", "robin"):
        for n in SIZES:
            r = measure(case, n)
            res["runs"].append(r)
            d, m = r["default"], r["mg-cell"]
            print(f"{case} {n}^2: default {d['iterations']} iterations {d['ms_per_solve']:.2f} ms (converged {d['converged']}); "
                  f"mg-cell {m['iterations']} iterations {m['ms_per_solve']:.2f} ms, set-up {m['setup_ms']:.2f} ms, rows {m['rows']}, "
                  f"{m['bytes'] / 2 ** 20:.1f} MiB", flush=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
