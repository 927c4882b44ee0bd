"""Measurement of method=bicgstabl with l=2 and l=4 (PG_METHOD_BICGSTABL, DESIGN.md "BiCGStab(l)") against the default options, one
rank, one process, the paths alternating.

    python scripts/bench_bicgstabl.py [out.json] [case ...]     (default: profiles/bicgstabl_bench.json, every case)

Cases
  advdiff512, advdiff1024   steady advection-diffusion past a cylinder (fluid outside the disc r = 1 at (2.01, 2.01) of the 4 x 4
                            box, D = 1, f = 1, Dirichlet(1) on the cylinder, Dirichlet(0) borders) in uniform flow (1, 0.3) U and in
                            rigid rotation about the cylinder's centre, at cell Peclet number U h = 0.5, 2 and 8 (rotation: the
                            speed at r = 1).  Per path three cold solves (zero start, reltol 1e-12, at most MAXITER iterations),
                            the paths alternating: products and ms of the median solve, whether each solve converged, and the true
                            residual of the last state (computed on the host from the exported system).
  sv512                     the StreamVorticity cylinder run of scripts/bench_streamvorticity.py at 512^2: windows of SV_STEPS
                            steps, both solves of a step with the path's method; the vorticity solve's products and ms per step.
  heat256                   256^3 heat (sphere r = 1, BE first solve from zero), precond = -1: plain BiCGStab against BiCGStab(2),
                            ms per product -- a diffusion system, where nothing is to be gained -- next to the ratio the byte
                            counts of DESIGN.md predict.
Times are host clocks around work that ends in a device synchronisation."""
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
OUT = ARGS[0] if ARGS else "profiles/bicgstabl_bench.json"
CASES = ARGS[1:] or ["advdiff512", "advdiff1024", "sv512", "heat256"]
REPEATS, MAXITER, SV_WARMUP, SV_STEPS = 3, 20000, 2, 5
KEYS = ("left", "right", "bottom", "top")
PATHS = {"default": dict(method="bicgstab"), "l2": dict(method="bicgstabl", l=2), "l4": dict(method="bicgstabl", l=4)}


def sync():
    L.check(L.lib().pg_device_synchronize())


def opts_of(path, **kw):
    kw = dict(PATHS[path], reltol=1e-12, warm_start=False, **kw)
    return pj.api._krylov_opts(kw.pop("method"), kw)


def cold_solve(s, opts):
    """one solve of the constructor's system from zero -> (ms, pg_run_info)"""
    run = L.pg_run_info()
    sync()
    t0 = time.perf_counter()
    L.check(L.lib().pg_solver_run(s._h, C.c_double(0.0), C.c_int32(L.PG_SCHEME["BE"]), C.byref(opts), C.c_int32(1), C.c_int64(0),
                                  C.c_int32(0), C.byref(run)))
    sync()
    return (time.perf_counter() - t0) * 1e3, run


def alternate(solvers, opts):
    """REPEATS solves per path, the paths alternating -> per path the median solve"""
    ms = {k: [] for k in solvers}
    runs = {k: [] for k in solvers}
    for _ in range(REPEATS):
        for k, s in solvers.items():
            t, run = cold_solve(s, opts[k])
            ms[k].append(t)
            runs[k].append(run)
    out = {}
    for k in solvers:
        med = statistics.median(ms[k])
        r = runs[k][ms[k].index(med)]
        out[k] = dict(ms_per_solve=med, solves_ms=ms[k], products=int(r.products), iters=int(r.total_iters),
                      converged=[int(q.unconverged_steps) == 0 for q in runs[k]], relres=float(r.worst_relres))
    return out


def advdiff(n):
    mesh = pj.Mesh((n, n), (4.0, 4.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0, complement=True), mesh)
    M = (n + 1) ** 2
    h = 4.0 / n
    x, y = cap.C_ω[:, 0], cap.C_ω[:, 1]
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS})
    rows = []
    for flow in ("uniform", "rotation"):
        for pe in (0.5, 2.0, 8.0):
            U = pe / h
            u = [np.full(M, U), np.full(M, 0.3 * U)] if flow == "uniform" else [-U * (y - 2.01), U * (x - 2.01)]
            op = pj.ConvectionOps(cap, [np.ascontiguousarray(a) for a in u], np.zeros(2 * M))
            ph = pj.Phase(cap, op, 1.0, 1.0)
            solvers = {k: pj.AdvectionDiffusionSteadyMono(ph, bcb, pj.Dirichlet(1.0)) for k in PATHS}
            res = alternate(solvers, {k: opts_of(k, maxiter=MAXITER) for k in PATHS})
            si = solvers["default"].system_info(0)
            # the TRUE residual of every path's state on the exported preconditioned system, in the norm of the stopping test (the
            # plain loop reports its recurrence residual; BiCGStab(l) confirms the true one before it reports convergence)
            Ah, bh, idx = solvers["default"].system(2)
            Ah = Ah[:, : Ah.shape[0]].tocsr()
            S = solvers["default"].row_scaling(0)
            states = {k: solvers[k]._fetch_state() for k in PATHS}
            for k in PATHS:
                res[k]["true_relres"] = float(np.linalg.norm(S * (bh - Ah @ (states[k][idx] / S))) / np.linalg.norm(S * bh))
            for k in ("default", "l4"):
                res[k]["state_rel_l2_to_l2"] = float(np.linalg.norm(states[k] - states["l2"]) / np.linalg.norm(states["l2"]))
            rows.append(dict(case=f"advdiff{n}", flow=flow, cell_peclet=pe, rows=int(si.n_own), nnz=int(si.nnz), **res))
            print(rows[-1], flush=True)
    return rows


def stream_vorticity(n):
    def stream(x, y, t=0.0):
        return y
    mesh = pj.Mesh((n, n), (1.0, 1.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((0.5, 0.47), 0.15, complement=True), mesh)
    M = (n + 1) ** 2
    x, y = cap.C_ω[:, 0], cap.C_ω[:, 1]
    w0 = np.concatenate([20.0 * np.exp(-((x - 0.25) ** 2 + (y - 0.6) ** 2) / 0.01), np.zeros(M)])
    bs = pj.BorderConditions({k: pj.Dirichlet(stream) for k in KEYS})
    bw = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS})
    make = lambda: pj.StreamVorticity(cap, 1e-3, 0.32 / n, bc_stream=pj.Dirichlet(0.47), bc_stream_border=bs, bc_vorticity_border=bw, ω0=w0)
    svs = {k: make() for k in PATHS}
    kws = {k: dict(PATHS[k], reltol=1e-12) for k in PATHS}
    for k, sv in svs.items():
        pj.run_StreamVorticity_b(sv, SV_WARMUP, "BE", save_every=0, **kws[k])
    wins = {k: [] for k in PATHS}
    runs = {k: [] for k in PATHS}
    for _ in range(REPEATS):
        for k, sv in svs.items():
            sync()
            t0 = time.perf_counter()
            pj.run_StreamVorticity_b(sv, SV_STEPS, "BE", save_every=0, **kws[k])
            sync()
            wins[k].append(time.perf_counter() - t0)
            runs[k].append(sv.last_run)
    out = dict(case=f"sv{n}", steps_per_window=SV_STEPS)
    for k in PATHS:
        med = statistics.median(wins[k])
        r = runs[k][wins[k].index(med)]
        out[k] = dict(ms_per_step=1e3 * med / SV_STEPS, omega_ms_per_solve=r.omega_ms / SV_STEPS, omega_products_per_solve=r.omega_products / SV_STEPS,
                      psi_ms_per_solve=r.psi_ms / SV_STEPS, psi_products_per_solve=r.psi_products / SV_STEPS,
                      unconverged_solves=[int(q.unconverged) for q in runs[k]])
    print(out, flush=True)
    return [out]


def heat(n):
    mesh = pj.Mesh((n,) * 3, (4.0,) * 3)
    cap = pj.Capacity(pj.Sphere((2.01,) * 3, 1.0), mesh)
    ph = pj.Phase(cap, pj.DiffusionOps(cap), 0.0, 1.0)
    bcb = pj.BorderConditions({k: pj.Dirichlet(1.0) for k in KEYS})
    dt = 0.75 * (4.0 / n) ** 2
    paths = ("default", "l2")
    solvers = {k: pj.DiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(1.0), dt, None, "BE") for k in paths}
    res = alternate(solvers, {k: opts_of(k, precond=-1) for k in paths})
    si = solvers["default"].system_info(0)
    nrows, spmv_bytes = int(si.n_own), int(si.spmv_bytes)
    for k in paths:
        res[k]["ms_per_product"] = res[k]["ms_per_solve"] / res[k]["products"]
    # algorithmic bytes per product (DESIGN.md "BiCGStab(l)"): BiCGStab (2 B_spmv + 168 n) / 2; BiCGStab(l) B_spmv + (12 l + 48 + 32 / l) n
    l = 2
    predicted = (spmv_bytes + (12 * l + 48 + 32 / l) * nrows) / (spmv_bytes + 84 * nrows)
    out = dict(case=f"heat{n}", rows=nrows, spmv_bytes=spmv_bytes, **res,
               ms_per_product_ratio_l2_to_plain=res["l2"]["ms_per_product"] / res["default"]["ms_per_product"],
               predicted_ratio_from_bytes=predicted)
    print(out, flush=True)
    return [out]


pj.init(0)
results = []
for case in CASES:
    if case.startswith("advdiff"):
        results += advdiff(int(case[7:]))
    elif case.startswith("sv"):
        results += stream_vorticity(int(case[2:]))
    elif case.startswith("heat"):
        results += heat(int(case[4:]))
    else:
        raise SystemExit(f"unknown case {case}")
import torch

doc = dict(what="default options (BiCGStab, precond = 0, cold start) against method=bicgstabl with l=2 and l=4, one rank",
           repeats=REPEATS, maxiter=MAXITER, reltol=1e-12, device=torch.cuda.get_device_name(0), source_hash=source_hash(), results=results)
with open(OUT, "w") as f:
    json.dump(doc, f, indent=1)
print(f"wrote {OUT}")
