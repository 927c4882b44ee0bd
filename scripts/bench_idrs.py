"""Measurement of method=idrs with nshadow=4 and nshadow=8 (PG_METHOD_IDRS, DESIGN.md "IDR(s)") against the default options and
against method=bicgstabl with l=4, one rank.  ONE solver per process: the parent starts a child per (case, path), each under its
own time limit, the paths of a case in turn; a child builds its solver, runs REPEATS windows and prints one JSON line.

    python scripts/bench_idrs.py [out.json] [case ...]     (default: profiles/idrs_bench.json, every case)

Cases
  advdiff512, advdiff1024   steady advection-diffusion past a cylinder (fluid outside the disc r = 1 at (2.01, 2.01) of the 4 x 4
                            box, D = 1, f = 1, Dirichlet(1) on the cylinder, Dirichlet(0) borders) in uniform flow (1, 0.3) U and in
                            rigid rotation about the cylinder's centre, at cell Peclet number U h = 0.5, 2 and 8 (rotation: the
                            speed at r = 1).  Per path three cold solves (zero start, reltol 1e-12, at most MAXITER products):
                            products and ms of the median solve, whether each solve converged, and the TRUE residual of the last
                            state (computed on the host from the exported system) -- of the default path too, whatever it reports.
  sv512                     the StreamVorticity cylinder run of scripts/bench_streamvorticity.py at 512^2: windows of SV_STEPS
                            steps.  The C ABI takes ONE set of options for both solves of a step, so every path runs both solves
                            with its method and the two solves are reported apart: "the method on the vorticity solve only" is the
                            default path's psi time plus the path's omega time (sv_omega_only_ms_per_step, derived).
  heat256                   256^3 heat (sphere r = 1, BE first solve from zero), precond = -1: plain BiCGStab against IDR(4) and
                            IDR(8), ms per product -- a diffusion system, where nothing is to be gained -- next to the ratio the
                            byte counts of DESIGN.md predict.
Times are host clocks around work that ends in a device synchronisation."""
import json
import statistics
import subprocess
import sys
import time

REPEATS, MAXITER, SV_WARMUP, SV_STEPS = 3, 40000, 2, 5
CHILD_LIMIT = 240     # seconds, per child process
KEYS = ("left", "right", "bottom", "top")
PATHS = {"default": dict(method="bicgstab"), "l4": dict(method="bicgstabl", l=4), "s4": dict(method="idrs", nshadow=4),
         "s8": dict(method="idrs", nshadow=8)}


def child(spec):
    import ctypes as C

    import numpy as np

    sys.path.insert(0, ".")
    import penguin.jl_amd as pj
    from penguin.jl_amd import _lib as L

    pj.init(0)
    sync = lambda: L.check(L.lib().pg_device_synchronize())
    path = spec["path"]
    # maxiter in each method's own unit, the same cap in products: BiCGStab and BiCGStab(l) count two products per iteration
    cap = MAXITER if path in ("s4", "s8") else MAXITER // 2

    def opts_of(**kw):
        kw = dict(PATHS[path], reltol=1e-12, warm_start=False, **kw)
        return pj.api._krylov_opts(kw.pop("method"), kw)

    def cold_solves(s, opts):
        ms, runs = [], []
        for _ in range(REPEATS):
            run = L.pg_run_info()
            sync()
            t0 = time.perf_counter()
            L.check(L.lib().pg_solver_run(s._h, C.c_double(0.0), C.c_int32(L.PG_SCHEME["BE"]), C.byref(opts), C.c_int32(1), C.c_int64(0),
                                          C.c_int32(0), C.byref(run)))
            sync()
            ms.append((time.perf_counter() - t0) * 1e3)
            runs.append(run)
        med = statistics.median(ms)
        r = runs[ms.index(med)]
        return dict(ms_per_solve=med, solves_ms=ms, products=int(r.products), iters=int(r.total_iters),
                    converged=[int(q.unconverged_steps) == 0 for q in runs], relres=float(r.worst_relres))

    kind = spec["kind"]
    if kind == "advdiff":
        n, flow, pe = spec["n"], spec["flow"], spec["pe"]
        cap_ = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0, complement=True), pj.Mesh((n, n), (4.0, 4.0)))
        M = (n + 1) ** 2
        x, y = cap_.C_ω[:, 0], cap_.C_ω[:, 1]
        U = pe / (4.0 / n)
        u = [np.full(M, U), np.full(M, 0.3 * U)] if flow == "uniform" else [-U * (y - 2.01), U * (x - 2.01)]
        op = pj.ConvectionOps(cap_, [np.ascontiguousarray(a) for a in u], np.zeros(2 * M))
        s = pj.AdvectionDiffusionSteadyMono(pj.Phase(cap_, op, 1.0, 1.0), pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS}),
                                            pj.Dirichlet(1.0))
        res = cold_solves(s, opts_of(maxiter=cap))
        Ah, bh, idx = s.system(2)
        Ah = Ah[:, : Ah.shape[0]].tocsr()
        S = s.row_scaling(0)
        z = s._fetch_state()[idx] / S
        res["true_relres"] = float(np.linalg.norm(S * (bh - Ah @ z)) / np.linalg.norm(S * bh))
        si = s.system_info(0)
        res.update(rows=int(si.n_own), nnz=int(si.nnz))
    elif kind == "sv":
        n = spec["n"]

        def stream(x, y, t=0.0):
            return y
        cap_ = pj.Capacity(pj.Sphere((0.5, 0.47), 0.15, complement=True), pj.Mesh((n, n), (1.0, 1.0), (0.0, 0.0)))
        M = (n + 1) ** 2
        x, y = cap_.C_ω[:, 0], cap_.C_ω[:, 1]
        w0 = np.concatenate([20.0 * np.exp(-((x - 0.25) ** 2 + (y - 0.6) ** 2) / 0.01), np.zeros(M)])
        sv = pj.StreamVorticity(cap_, 1e-3, 0.32 / n, bc_stream=pj.Dirichlet(0.47),
                                bc_stream_border=pj.BorderConditions({k: pj.Dirichlet(stream) for k in KEYS}),
                                bc_vorticity_border=pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS}), ω0=w0)
        kw = dict(PATHS[path], reltol=1e-12)
        pj.run_StreamVorticity_b(sv, SV_WARMUP, "BE", save_every=0, **kw)
        wins, runs = [], []
        for _ in range(REPEATS):
            sync()
            t0 = time.perf_counter()
            pj.run_StreamVorticity_b(sv, SV_STEPS, "BE", save_every=0, **kw)
            sync()
            wins.append(time.perf_counter() - t0)
            runs.append(sv.last_run)
        med = statistics.median(wins)
        r = runs[wins.index(med)]
        res = dict(ms_per_step=1e3 * med / SV_STEPS, omega_ms_per_solve=r.omega_ms / SV_STEPS,
                   omega_products_per_solve=r.omega_products / SV_STEPS, psi_ms_per_solve=r.psi_ms / SV_STEPS,
                   psi_products_per_solve=r.psi_products / SV_STEPS, unconverged_solves=[int(q.unconverged) for q in runs],
                   worst_relres=float(r.worst_relres))
    else:
        n = spec["n"]
        cap_ = pj.Capacity(pj.Sphere((2.01,) * 3, 1.0), pj.Mesh((n,) * 3, (4.0,) * 3))
        ph = pj.Phase(cap_, pj.DiffusionOps(cap_), 0.0, 1.0)
        s = pj.DiffusionUnsteadyMono(ph, pj.BorderConditions({k: pj.Dirichlet(1.0) for k in KEYS}), pj.Dirichlet(1.0),
                                     0.75 * (4.0 / n) ** 2, None, "BE")
        res = cold_solves(s, opts_of(precond=-1))
        si = s.system_info(0)
        res.update(rows=int(si.n_own), spmv_bytes=int(si.spmv_bytes), ms_per_product=res["ms_per_solve"] / res["products"])
    print("RESULT " + json.dumps(res), flush=True)


def run_child(spec):
    """-> the child's result, or what became of it; a child that failed or ran out of time ends the whole measurement"""
    try:
        r = subprocess.run([sys.executable, __file__, "--child", json.dumps(spec)], capture_output=True, text=True, timeout=CHILD_LIMIT)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"child {spec} ran out of its {CHILD_LIMIT} s: nothing more is started")
    if r.returncode != 0:
        raise SystemExit(f"child {spec} failed with {r.returncode}: nothing more is started\n{r.stderr[-3000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def parent(out, cases):
    sys.path.insert(0, ".")
    from penguin.jl_amd.build import source_hash

    results = []

    def flush():
        doc = dict(what="default options (BiCGStab, precond = 0, cold start), method=bicgstabl l=4, method=idrs nshadow=4 and 8; one "
                        "rank, one solver per process", repeats=REPEATS, max_products=MAXITER, reltol=1e-12, source_hash=source_hash(),
                   results=results)
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)

    for case in cases:
        if case.startswith("advdiff"):
            n = int(case[7:])
            for flow in ("uniform", "rotation"):
                for pe in (0.5, 2.0, 8.0):
                    row = dict(case=case, flow=flow, cell_peclet=pe)
                    for path in PATHS:
                        row[path] = run_child(dict(kind="advdiff", n=n, flow=flow, pe=pe, path=path))
                    results.append(row)
                    print(row, flush=True)
                    flush()
        elif case.startswith("sv"):
            row = dict(case=case, steps_per_window=SV_STEPS)
            for path in PATHS:
                row[path] = run_child(dict(kind="sv", n=int(case[2:]), path=path))
            for path in PATHS:
                row[path]["sv_omega_only_ms_per_step"] = (row["default"]["ms_per_step"] - row["default"]["omega_ms_per_solve"]
                                                          + row[path]["omega_ms_per_solve"])
            results.append(row)
            print(row, flush=True)
            flush()
        elif case.startswith("heat"):
            row = dict(case=case)
            for path in ("default", "s4", "s8"):
                row[path] = run_child(dict(kind="heat", n=int(case[4:]), path=path))
            nrows, B = row["default"]["rows"], row["default"]["spmv_bytes"]
            for path, s in (("s4", 4), ("s8", 8)):
                # algorithmic bytes per product (DESIGN.md "IDR(s)"): IDR(s) B_spmv + 16 n (s^2 + 6 s + 3) / (s + 1); BiCGStab B_spmv + 84 n
                row[f"ms_per_product_ratio_{path}_to_plain"] = row[path]["ms_per_product"] / row["default"]["ms_per_product"]
                row[f"predicted_ratio_from_bytes_{path}"] = (B + 16.0 * nrows * (s * s + 6 * s + 3) / (s + 1)) / (B + 84.0 * nrows)
            results.append(row)
            print(row, flush=True)
            flush()
        else:
            raise SystemExit(f"unknown case {case}")
    print(f"wrote {out}")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--child":
        child(json.loads(sys.argv[2]))
    else:
        args = sys.argv[1:]
        parent(args[0] if args else "profiles/idrs_bench.json", args[1:] or ["advdiff512", "advdiff1024", "sv512", "heat256"])
