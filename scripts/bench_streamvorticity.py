"""Measurement of the stream function - vorticity solver: steps per second of StreamVorticity (ψ, ω, the velocity and the
convection operators stay on the device) against the same step composed from the public entry points that existed before it
(a new DiffusionSteadyMono per step, grad, ConvectionOps, AdvectionDiffusionUnsteadyMono: every state and velocity crosses
PCIe), same geometry, same data, same Krylov tolerance, one process, the two paths alternating.

    python scripts/bench_streamvorticity.py [out.json] [n ...]        (default: profiles/streamvorticity_bench.json 512 1024)
    python scripts/bench_streamvorticity.py --precond mg [out.json] [n ...]
                                                   (default: profiles/streamvorticity_mg_bench.json 512 1024)

With --precond the two alternating paths are StreamVorticity with the default options and StreamVorticity with that
preconditioner on the stream-function solve ("mg": the aggregation multigrid V-cycle; an integer: as pg_krylov_opts.precond):
steps/s, the ψ solve's ms, iterations and products per step, the hierarchy's set-up time, memory and levels.

Geometry of the test suite's shape C: flow past the cylinder r = 0.15 at (0.5, 0.47) in the unit box, ψ = y on the borders (a
uniform stream), ψ = 0.47 on the body, ω = 0 on borders and body, ω0 = 20 exp(-((x-0.25)² + (y-0.6)²)/0.01), ν = 1e-3,
Δt = 0.32 / n (1e-2 at n = 32: the same Courant number at every size), backward Euler.  5 warm-up steps, then REPEATS windows of
20 steps per path; the rate is that of the median window, the spread is reported.  Times are host clocks around work that
ends in a device synchronisation."""
import ctypes as C
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import penguin.jl_amd as pj
from penguin.jl_amd import _lib as L

ARGS = sys.argv[1:]
PRECOND = None
if "--precond" in ARGS:
    k = ARGS.index("--precond")
    PRECOND = ARGS[k + 1] if ARGS[k + 1] == "mg" else int(ARGS[k + 1])
    del ARGS[k:k + 2]
OUT = ARGS[0] if ARGS else ("profiles/streamvorticity_bench.json" if PRECOND is None else "profiles/streamvorticity_mg_bench.json")
SIZES = [int(a) for a in ARGS[1:]] or [512, 1024]
WARMUP, STEPS, REPEATS = 5, 20, 3
KEYS = ("left", "right", "bottom", "top")
SCHEME = "BE"


def stream(x, y, t=0.0):
    return y


def sync():
    L.check(L.lib().pg_device_synchronize())


def problem(n):
    mesh = pj.Mesh((n, n), (1.0, 1.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((0.5, 0.47), 0.15, complement=True), mesh)
    M = (n + 1) ** 2
    x, y = cap.C_ω[:, 0], cap.C_ω[:, 1]
    w0 = np.concatenate([20.0 * np.exp(-((x - 0.25) ** 2 + (y - 0.6) ** 2) / 0.01), np.zeros(M)])
    return dict(mesh=mesh, cap=cap, M=M, w0=w0, nu=1e-3, dt=0.32 / n,
                bs=pj.BorderConditions({k: pj.Dirichlet(stream) for k in KEYS}),
                bw=pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS}))


class Composed:
    """one step from the entry points a user had before StreamVorticity existed"""

    def __init__(self, P):
        self.P, self.op = P, pj.DiffusionOps(P["cap"])
        self.w = P["w0"].copy()
        self.psi, self.uv = None, None
        self.T = dict(psi_ms=0.0, velocity_ms=0.0, build_ms=0.0, omega_ms=0.0)
        self.products = [0, 0]

    def step(self):
        P, M, cap = self.P, self.P["M"], self.P["cap"]
        t0 = time.perf_counter()
        src = -self.w[:M]
        sp = pj.DiffusionSteadyMono(pj.Phase(cap, self.op, lambda x, y, z: src, 1.0), P["bs"], pj.Dirichlet(0.47))
        pj.solve_DiffusionSteadyMono_b(sp)
        self.psi = sp.x
        t1 = time.perf_counter()
        g = pj.grad(self.op, self.psi)
        u, v = np.ascontiguousarray(g[M:]), np.ascontiguousarray(-g[:M])
        cop = pj.ConvectionOps(cap, (u, v), np.concatenate([u, v]))
        self.uv = (u, v)
        sync()
        t2 = time.perf_counter()
        ph = pj.Phase(cap, cop, 0.0, P["nu"])
        sw = pj.AdvectionDiffusionUnsteadyMono(ph, P["bw"], pj.Dirichlet(0.0), P["dt"], self.w, SCHEME)
        sync()
        t3 = time.perf_counter()
        info = L.pg_step_info()
        opts = pj.api._krylov_opts("bicgstab", {})
        L.check(L.lib().pg_solver_initial_solve(sw._h, C.byref(opts), C.byref(info)))
        self.w = sw._fetch_state()
        t4 = time.perf_counter()
        for k, d in zip(self.T, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            self.T[k] += d * 1e3
        self.products[0] += sp.ch[-1]["iters"]
        self.products[1] += info.iters
        assert sp.ch[-1]["converged"] and info.converged


def measure(n):
    P = problem(n)
    new = pj.StreamVorticity(P["cap"], P["nu"], P["dt"], bc_stream=pj.Dirichlet(0.47), bc_stream_border=P["bs"],
                             bc_vorticity_border=P["bw"], ω0=P["w0"])
    old = Composed(P)
    pj.run_StreamVorticity_b(new, WARMUP, SCHEME, save_every=0)
    for _ in range(WARMUP):
        old.step()
    for k in old.T:
        old.T[k] = 0.0
    old.products = [0, 0]
    agree_after_warmup = float(np.linalg.norm(new.ω - old.w) / np.linalg.norm(old.w))
    win_new, win_old, runs = [], [], []
    for _ in range(REPEATS):
        sync()
        t0 = time.perf_counter()
        pj.run_StreamVorticity_b(new, STEPS, SCHEME, save_every=0)
        sync()
        win_new.append(time.perf_counter() - t0)
        runs.append(new.last_run)
        assert new.last_run.unconverged == 0
        t0 = time.perf_counter()
        for _ in range(STEPS):
            old.step()
        sync()
        win_old.append(time.perf_counter() - t0)
    tot = REPEATS * STEPS
    info = new.psi_solver.system_info(0)
    res_new = dict(steps_per_s=STEPS / statistics.median(win_new), windows_s=win_new,
                   psi_products_per_step=sum(r.psi_products for r in runs) / tot,
                   omega_products_per_step=sum(r.omega_products for r in runs) / tot,
                   psi_iters_per_step=sum(r.psi_iters for r in runs) / tot, omega_iters_per_step=sum(r.omega_iters for r in runs) / tot,
                   per_step_ms=dict(psi_solve=sum(r.psi_ms for r in runs) / tot, velocity_and_convection=sum(r.velocity_ms for r in runs) / tot,
                                    omega_solver_construction=sum(r.build_ms for r in runs) / tot, omega_solve=sum(r.omega_ms for r in runs) / tot))
    res_old = dict(steps_per_s=STEPS / statistics.median(win_old), windows_s=win_old,
                   psi_iters_per_step=old.products[0] / tot, omega_iters_per_step=old.products[1] / tot,
                   per_step_ms=dict(psi_solver_construction_solve_and_download=old.T["psi_ms"] / tot,
                                    grad_and_convection_ops=old.T["velocity_ms"] / tot,
                                    omega_solver_construction=old.T["build_ms"] / tot, omega_solve_and_download=old.T["omega_ms"] / tot))
    return dict(n=n, cells=P["M"], rows_per_system=int(info.n_own), dt=P["dt"], scheme=SCHEME, StreamVorticity=res_new, composed_from_public_entry_points=res_old,
                speedup=res_new["steps_per_s"] / res_old["steps_per_s"], omega_rel_l2_between_paths_after_warmup=agree_after_warmup,
                omega_rel_l2_between_paths_at_end=float(np.linalg.norm(new.ω - old.w) / np.linalg.norm(old.w)),
                state_finite=bool(np.all(np.isfinite(new.ω)) and np.all(np.isfinite(new.ψ))))


def _sv_result(win, runs, tot):
    return dict(steps_per_s=STEPS / statistics.median(win), windows_s=win,
                psi_products_per_step=sum(r.psi_products for r in runs) / tot,
                omega_products_per_step=sum(r.omega_products for r in runs) / tot,
                psi_iters_per_step=sum(r.psi_iters for r in runs) / tot, omega_iters_per_step=sum(r.omega_iters for r in runs) / tot,
                per_step_ms=dict(psi_solve=sum(r.psi_ms for r in runs) / tot, velocity_and_convection=sum(r.velocity_ms for r in runs) / tot,
                                 omega_solver_construction=sum(r.build_ms for r in runs) / tot, omega_solve=sum(r.omega_ms for r in runs) / tot))


def measure_precond(n):
    """default options against --precond on the ψ solve: two StreamVorticity solvers on the same problem, windows alternating"""
    P = problem(n)
    make = lambda: pj.StreamVorticity(P["cap"], P["nu"], P["dt"], bc_stream=pj.Dirichlet(0.47), bc_stream_border=P["bs"],
                                      bc_vorticity_border=P["bw"], ω0=P["w0"])
    plain, pre = make(), make()
    pj.run_StreamVorticity_b(plain, WARMUP, SCHEME, save_every=0)
    pj.run_StreamVorticity_b(pre, WARMUP, SCHEME, save_every=0, precond=PRECOND)
    agree_after_warmup = float(np.linalg.norm(pre.ω - plain.ω) / np.linalg.norm(plain.ω))
    win = {"plain": [], "pre": []}
    runs = {"plain": [], "pre": []}
    for _ in range(REPEATS):
        for key, sv, kw in (("plain", plain, {}), ("pre", pre, {"precond": PRECOND})):
            sync()
            t0 = time.perf_counter()
            pj.run_StreamVorticity_b(sv, STEPS, SCHEME, save_every=0, **kw)
            sync()
            win[key].append(time.perf_counter() - t0)
            runs[key].append(sv.last_run)
            assert sv.last_run.unconverged == 0
    tot = REPEATS * STEPS
    info = pre.psi_solver.system_info(0)
    a, b = _sv_result(win["plain"], runs["plain"], tot), _sv_result(win["pre"], runs["pre"], tot)
    spread = lambda w: (max(w) - min(w)) / statistics.median(w)
    out = dict(n=n, cells=P["M"], rows_per_system=int(info.n_own), dt=P["dt"], scheme=SCHEME, precond=PRECOND, default_options=a,
               with_precond=b, speedup_steps=b["steps_per_s"] / a["steps_per_s"],
               speedup_psi_solve=a["per_step_ms"]["psi_solve"] / b["per_step_ms"]["psi_solve"],
               window_spread=dict(default_options=spread(win["plain"]), with_precond=spread(win["pre"])),
               omega_rel_l2_between_paths_after_warmup=agree_after_warmup,
               omega_rel_l2_between_paths_at_end=float(np.linalg.norm(pre.ω - plain.ω) / np.linalg.norm(plain.ω)),
               psi_rel_l2_between_paths_at_end=float(np.linalg.norm(pre.ψ - plain.ψ) / np.linalg.norm(plain.ψ)),
               state_finite=bool(np.all(np.isfinite(pre.ω)) and np.all(np.isfinite(pre.ψ))))
    if PRECOND == "mg":
        out["hierarchy"] = pre.psi_solver.mg_info()
    return out


pj.init(0)
if PRECOND is not None:
    from penguin.jl_amd.build import source_hash

    res = dict(what="stream function - vorticity step, flow past a cylinder (shape C of tests/test_gpu_streamvorticity.py), one rank: "
                    "default options against --precond on the stream-function solve",
               warmup_steps=WARMUP, steps_per_window=STEPS, windows=REPEATS, reltol=1e-12, device=pj.device_name(),
               config=pj.config_string(), source_hash=source_hash(), sizes=[])
    for n in SIZES:
        res["sizes"].append(measure_precond(n))
        print(json.dumps(res["sizes"][-1]), flush=True)
        with open(OUT, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    sys.exit(0)
res = dict(what="stream function - vorticity step, flow past a cylinder (shape C of tests/test_gpu_streamvorticity.py), one rank",
           warmup_steps=WARMUP, steps_per_window=STEPS, windows=REPEATS, reltol=1e-12, device=pj.device_name(),
           config=pj.config_string(), sizes=[])
for n in SIZES:
    res["sizes"].append(measure(n))
    print(json.dumps(res["sizes"][-1]), flush=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
