"""One child process of tests/test_gpu_residual_truth.py: the loop's variants are chosen by PG_* variables that are read once
per process, so every setting runs in a process of its own (started by the test with subprocess.run and a timeout).

    python scripts/residual_truth_child.py first                                    first solves from zero, capped solves
    python scripts/residual_truth_child.py warm --expect full|gamma|compact [...]   warm steps of the time loop

The child builds its cases, steps them with pg_solver_initial_solve / pg_solver_step, and after EVERY solve downloads the
system the solver iterated on (Â, b̂: pg_solver_get_system_csr 2 / 3), the weights ds of its convergence test and the state,
and holds the step info against them with tests/residual_truth.check_step.  Next to each device solve it runs the oracle's
restatement of the same iteration on the same exported system from the same start (oracle/krylov_c): its iterations
(it_ref) and its own recurrence-against-truth gap (gap_ratio, what the checker's constant c is derived from).

pg_step_info carries neither the products of a solve nor its degree nor whether it ended at a half step.  A TWIN solver,
built like the first, takes the same solves in lockstep through pg_solver_run (the first solve: do_initial with no step; a
step: max_steps = 1), whose pg_run_info does: products, poly_degree, half_exits.  The loop is bitwise reproducible, and the
child holds the twin to that -- its iterations and its ||r|| / ||b|| must equal the checked solve's exactly -- so the
figures are those of the solve checked: `products` of check_step is the device's own count, `degree` and `half_exit` of
the JSON are what the device ran.  It stops at
the first failing check or non-zero status -- nothing more is started on the device after an error -- and prints ONE JSON
line of what it saw: per case n_own, n_c, the paths taken, iterations, figures.  Exit status 0 and "ok": true, or 1 and
"error".
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import penguin.jl_amd as pj                      # noqa: E402
from oracle import krylov_c                      # noqa: E402
from penguin.jl_amd import _lib as L             # noqa: E402
from penguin.jl_amd import api                   # noqa: E402
from tests import residual_truth as rt           # noqa: E402

KEYS = ("left", "right", "top", "bottom")
RELTOLS = (1e-6, 1e-9)
RAMP = lambda t: 1.0 + 0.5 * t                   # the Dirichlet interface value of the "closure" / "separable" data


class Case:
    """a solver with its time step, schemes and (mono, Dirichlet interface) the handle for per-step interface data"""

    def __init__(self, name, data="const"):
        self.name, self.data = name, data
        self.sch0, self.sch = "BE", "CN"
        self.poly = name.startswith("ball3d")             # Gershgorin admits the polynomial: checked in first_solve
        rng = np.random.default_rng(11)
        if name in ("ball3d", "ball3d_odd"):
            # ball3d has n_own = 967 and 245 remaining rows; 13 x 12 x 11 has 901 and 222 (both n_own odd), 13 x 12 x 10 has 804
            # and 192: an odd and an even count of each kind
            n = (12, 12, 12) if name == "ball3d" else (13, 12, 10)
            mesh = pj.Mesh(n, (4.0,) * 3)
            cap = pj.Capacity(pj.Sphere((2.01, 2.01, 2.01), 1.0), mesh)
            self.M = int(np.prod([v + 1 for v in n]))
            g = {"const": 1.0, "closure": (lambda x, y, z, t: RAMP(t)), "separable": pj.TimeSeparable([(1.0, RAMP)])}[data]
            self.dt = 0.75 * (4.0 / max(n)) ** 2
            ph = pj.Phase(cap, pj.DiffusionOps(cap), 0.0, 1.0)
            bcb = pj.BorderConditions({k: pj.Dirichlet(1.0) for k in KEYS})
            self.s = pj.DiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(g), self.dt, np.zeros(2 * self.M), self.sch0)
            self.keep = (mesh, cap, ph, bcb)
        elif name == "disc2d_robin":
            n = (24, 20)
            mesh = pj.Mesh(n, (4.0, 4.0))
            cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0), mesh)
            self.M = 25 * 21
            self.dt = 0.4 * (4.0 / 24) ** 2
            ph = pj.Phase(cap, pj.DiffusionOps(cap), 0.0, 1.0)
            bcb = pj.BorderConditions({k: pj.Dirichlet(1.0) for k in KEYS})
            u0 = np.concatenate([rng.uniform(0.0, 1.0, self.M), np.zeros(self.M)])
            self.s = pj.DiffusionUnsteadyMono(ph, bcb, pj.Robin(1.0, 0.4, 0.7), self.dt, u0, self.sch0)
            self.keep = (mesh, cap, ph, bcb)
        elif name == "diph2d":
            n = (20, 20)
            mesh = pj.Mesh(n, (4.0, 4.0))
            c1, c2 = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0), mesh), pj.Capacity(pj.Sphere((2.01, 2.01), 1.0, complement=True), mesh)
            self.M = 21 * 21
            self.dt = 0.4 * (4.0 / 20) ** 2
            p1, p2 = pj.Phase(c1, pj.DiffusionOps(c1), 0.0, 1.0), pj.Phase(c2, pj.DiffusionOps(c2), 0.0, 2.0)
            ic = pj.InterfaceConditions(pj.ScalarJump(1.0, 0.8, 0.1), pj.FluxJump(1.0, 2.0, 0.0))
            bcb = pj.BorderConditions({k: pj.Dirichlet(0.3) for k in KEYS})
            u0 = np.concatenate([np.ones(self.M), np.ones(self.M), np.zeros(self.M), np.zeros(self.M)])
            self.s = pj.DiffusionUnsteadyDiph(p1, p2, bcb, ic, self.dt, u0, self.sch0)
            self.keep = (mesh, c1, c2, p1, p2, ic, bcb)
        elif name == "cg2d":                                # tests/test_gpu_parity.py test_cg_method_on_symmetric_problem
            n = (20, 20)
            mesh = pj.Mesh(n, (4.0, 4.0))
            cap = pj.Capacity(pj.Sphere((2.0, 2.0), 10.0), mesh)
            self.M = 21 * 21
            self.dt = 0.25 * (4.0 / 20) ** 2
            self.sch = "BE"
            ph = pj.Phase(cap, pj.DiffusionOps(cap), 0.0, 1.0)
            u0 = np.concatenate([np.random.default_rng(5).uniform(0.0, 1.0, self.M), np.zeros(self.M)])
            self.s = pj.DiffusionUnsteadyMono(ph, pj.BorderConditions({}), pj.Dirichlet(1.0), self.dt, u0, self.sch0)
            self.keep = (mesh, cap, ph)
        else:
            raise ValueError(name)
        self.t = 0.0
        self.steps = 0

    def install(self, nsteps):
        """separable data: the table of the steps to come, once"""
        if self.data == "separable":
            api._clear_separable(self.s, 1)
            api._install_separable(self.s, api._TD_INTERFACE, 0, np.ones((1, self.M)), api._separable_table([RAMP], self.dt, 1e300, nsteps))

    def before_step(self):
        """closure data: what the host-driven loop sends before a step (g at t and t + Δt, t already advanced)"""
        self.t += self.dt
        if self.data == "closure":
            gn, gn1 = np.full(self.M, RAMP(self.t)), np.full(self.M, RAMP(self.t + self.dt))
            L.check(L.lib().pg_solver_set_interface_value(self.s._h, L.dptr(gn), L.dptr(gn1)))


def opts_of(method="bicgstab", **kw):
    return api._krylov_opts(method, kw)


def twin_solve(twin, o, initial):
    """the same solve on the twin, through pg_solver_run: its pg_run_info"""
    run = L.pg_run_info()
    if not initial:
        twin.before_step()
    L.check(L.lib().pg_solver_run(twin.s._h, C.c_double(1e300), C.c_int32(L.PG_SCHEME[twin.sch]), C.byref(o), C.c_int32(1 if initial else 0),
                                  C.c_int64(0 if initial else 1), C.c_int32(0), C.byref(run)))
    return run


def products_of(method, info, run, restart=20):
    """products with the matrix inside the solve: the device's own count (pg_run_info.products of the twin) for BiCGStab --
    (2 iters - half exit) x degree --, BiCGStab(l) and IDR(s); CG: one per iteration; GMRES, which reports none: one per
    Arnoldi step and one true residual per cycle, iters // restart + 1 cycles"""
    if method == "cg":
        return int(info.iters)
    if method == "gmres":
        return int(info.iters) + int(info.iters) // restart + 1
    return int(run.products)


def exported(s, which):
    Ah, bh, idx = s.system(which)
    n = Ah.shape[0]
    Ah = Ah[:, :n].tocsr()
    return Ah, bh.copy(), idx, s.row_scaling(which & 1).copy()


def check_solve(case, which, info, run, reltol, method, y_start, label, want_ref=True, maxiter=0):
    """(a)-(d) of this solve, and the restatement next to it.  run: the twin's pg_run_info of the same solve; y_start: the
    start of the restatement (None: zero)."""
    s = case.s
    relres = info.resnorm / info.bnorm if info.bnorm > 0 else 0.0
    if run.total_iters != info.iters or run.worst_relres != relres or run.unconverged_steps != 1 - info.converged:
        raise rt.ResidualMismatch(f"{label}: the twin's solve is not this one: {run.total_iters} iterations, relres {run.worst_relres!r}, "
                                  f"{run.unconverged_steps} unconverged against {info.iters}, {relres!r}, converged {info.converged}")
    m = int(run.poly_degree)
    Ah, bh, idx, ds = exported(s, which)
    x = s._fetch_state()
    y = x[idx] / ds
    t = rt.truth(Ah, bh, ds, y)
    prod = products_of(method, info, run)
    delta, tol = t.delta(prod), t.tol(reltol)
    rec = {"label": label, "iters": int(info.iters), "converged": int(info.converged), "relres": relres,
           "res_true_rel": t.res / t.bnorm, "delta_over_tol": delta / tol, "products": prod, "degree": m,
           "half_exit": int(run.half_exits), "res_gap_over_delta": abs(info.resnorm - t.res) / delta,
           "bnorm_err_over_bound": abs(info.bnorm - t.bnorm) / (2.0 * t.n * rt.U * t.bnorm)}
    rt.check_step(info, t, reltol, 0.0, prod, label=label)
    if want_ref and method in ("bicgstab", "cg"):
        if method == "cg":
            xr, it_ref, res_ref = krylov_c.solve(Ah, bh, "cg", reltol=reltol, maxiter=maxiter or 10000)
            nmv, tr = it_ref, rt.truth(Ah, bh, np.ones(t.n), xr)
        else:
            g = min(max(float(s.system_info(which).gershgorin), 0.05), 0.95)
            xr, it_ref, res_ref, nmv = krylov_c.solve_poly(Ah, bh, m, g, x0=y_start, weights=ds, reltol=reltol, maxiter=maxiter or 10000)
            tr = rt.truth(Ah, bh, ds, xr)
        rec.update(it_ref=int(it_ref), gap_ratio=rt.gap_ratio(res_ref, tr, nmv), ref_delta_over_tol=tr.delta(nmv) / tr.tol(reltol))
        if not tr.delta(nmv) <= rt.VACUITY * tr.tol(reltol):
            raise rt.ResidualMismatch(f"{label}: (d) fails on the restatement: delta / tol = {tr.delta(nmv) / tr.tol(reltol):.3e}")
    return rec, (Ah, bh, idx, ds, y)


def first_solve(name, reltol, method="bicgstab", precond=-1, maxiter=0, **kw):
    case, twin = Case(name), Case(name)
    s = case.s
    si = s.system_info(2)
    if case.poly and not si.neumann_ok:
        raise rt.ResidualMismatch(f"{name}: the polynomial is not admitted on this system (gershgorin {si.gershgorin})")
    info = L.pg_step_info()
    o = opts_of(method, reltol=reltol, precond=precond, maxiter=maxiter, **kw)
    L.check(L.lib().pg_solver_initial_solve(s._h, C.byref(o), C.byref(info)))
    mname = {L.PG_METHOD["bicgstabl"]: "bicgstabl", L.PG_METHOD_IDRS: "idrs", L.PG_METHOD["gmres"]: "gmres", L.PG_METHOD["cg"]: "cg"}.get(o.method, "bicgstab")
    run = twin_solve(twin, o, True)
    want = precond if precond >= 2 else 0
    if mname == "bicgstab" and run.poly_degree != want:
        raise rt.ResidualMismatch(f"{name}: the first solve ran degree {run.poly_degree}, {want} asked for")
    rec, _ = check_solve(case, 2, info, run, reltol, mname, None, f"{name} first {mname} precond={precond} reltol={reltol:g} maxiter={maxiter}",
                         maxiter=maxiter)
    rec.update(n_own=int(si.n_own), method=mname, reltol=reltol)
    return rec


def run_first(out):
    recs = []
    out["solves"] = recs
    sizes = {}
    for name in ("ball3d", "ball3d_odd", "disc2d_robin", "diph2d"):
        for reltol in RELTOLS:
            for precond in ((-1, 2, 5) if name.startswith("ball3d") else (-1,)):
                r = first_solve(name, reltol, precond=precond)
                recs.append(r)
                sizes[name] = r["n_own"]
                if not r["converged"]:
                    raise rt.ResidualMismatch(f"{r['label']}: not converged")
                if name.startswith("ball3d") and abs(r["iters"] - r["it_ref"]) > 1:
                    raise rt.ResidualMismatch(f"{r['label']}: {r['iters']} iterations, the restatement takes {r['it_ref']}")
                if name == "ball3d" and precond in (-1, 5):
                    # capped one below what the solve needed: not converged, (b) and (c) hold -- so the uncapped solve stopped
                    # at its first chance
                    c = first_solve(name, reltol, precond=precond, maxiter=r["iters"] - 1)
                    c["capped"] = True
                    recs.append(c)
                    if c["converged"] != 0 or c["iters"] != r["iters"] - 1:
                        raise rt.ResidualMismatch(f"{c['label']}: converged {c['converged']} after {c['iters']} of {r['iters']} iterations")
    out["n_own"] = sizes
    if (sizes["ball3d"] + sizes["ball3d_odd"]) % 2 != 1:
        raise rt.ResidualMismatch(f"the two ball3d shapes do not give an odd and an even n_own: {sizes}")
    for reltol in RELTOLS:
        recs.append(first_solve("cg2d", reltol, method="cg"))
    recs.append(first_solve("ball3d", 1e-9, method="gmres", restart=20))
    recs.append(first_solve("ball3d_odd", 1e-9, method="bicgstabl", l=2))
    recs.append(first_solve("ball3d_odd", 1e-6, method="idrs", nshadow=4))
    for r in recs[-5:]:
        if not r["converged"]:
            raise rt.ResidualMismatch(f"{r['label']}: not converged")


def snapped(y_prev, Ah, bh, rows):
    y0 = y_prev.copy()
    y0[rows] = bh[rows] / Ah.diagonal()[rows]
    return y0


def run_warm(out, a):
    cases = {}
    out["cases"] = cases
    cfg = dict(kv.split("=", 1) for kv in pj.config_string().split() if "=" in kv)
    out["config"] = {k: cfg.get(k) for k in ("guess_states", "guess_depth") if k in cfg}
    for name in a.cases.split(","):
        for data in a.data.split(","):
            if data != "const" and not name.startswith("ball3d"):
                continue
            for reltol in ((1e-9,) if a.one_reltol else RELTOLS):
                key = f"{name}/{data}/{reltol:g}"
                cases[key] = {}
                warm_case(name, data, reltol, a, cases[key])
    # the half-step exit is one of the places the reported (r,r)_W comes from: it must have been taken -- and, where steps of
    # the compact loop were quiet (rows within the noise threshold: the 1e-9 cases with constant data), on a quiet step too
    out["half_exits"] = sum(c["half_exits"] for c in cases.values())
    out["quiet_half_exits"] = sum(c["quiet_half_exits"] for c in cases.values())
    if out["half_exits"] == 0:
        raise rt.ResidualMismatch("no solve of this setting ended at a half step")
    if a.expect == "compact" and not a.iters and out["quiet_half_exits"] == 0:
        raise rt.ResidualMismatch("no quiet step of this setting ended at a half step")
    if a.expect == "compact":
        nc = [v["n_c"] for k, v in cases.items() if k.startswith("ball3d/")][:1] + [v["n_c"] for k, v in cases.items() if k.startswith("ball3d_odd/")][:1]
        out["n_c"] = nc
        if len(nc) == 2 and sum(nc) % 2 != 1:
            raise rt.ResidualMismatch(f"the two ball3d shapes do not give an odd and an even remaining-row count: {nc}")


def warm_case(name, data, reltol, a, res):
    case, twin = Case(name, data), Case(name, data)
    s = case.s
    lib = L.lib()
    precond = a.degree if case.poly else -1
    o = opts_of("bicgstab", reltol=reltol, precond=precond)
    sch = L.PG_SCHEME[case.sch]
    info = L.pg_step_info()
    L.check(lib.pg_solver_initial_solve(s._h, C.byref(o), C.byref(info)))
    rec0, (_, _, idx, ds0, y) = check_solve(case, 2, info, twin_solve(twin, o, True), reltol, "bicgstab", None,
                                            f"{name}/{data} first reltol={reltol:g}")
    x_prev = s._fetch_state()
    case.install(a.steps)
    twin.install(a.steps)
    res.update({"first": rec0, "steps": [], "n_own": int(s.system_info(0).n_own)})
    relres, unconv, kept_max, moved, moved_steps = [], 0, 0, 0.0, []
    red = None
    for k in range(a.steps):
        case.before_step()
        L.check(lib.pg_solver_step(s._h, C.c_int32(sch), C.byref(o), C.byref(info)))
        run1 = twin_solve(twin, o, False)
        si = s.system_info(3)
        m = int(run1.poly_degree)
        Ah, bh, idx, ds = exported(s, 3)
        if k == 0:
            # which path this process takes, against the host's own reduction of the exported matrix
            li = s.system_info(7)
            n_w = int(si.n_omega)
            compact = bool(si.loop_is_compact)
            rd = rt.restrict_diag(Ah.indptr, Ah.indices, Ah.data, Ah.shape[0], Ah.shape[0])
            rg = rt.restrict_gamma(Ah.indptr, Ah.indices, Ah.data, n_w)
            gamma = (not compact) and int(li.rows_matrix) < int(si.n_own)
            res.update(loop_is_compact=int(compact), gamma_elim=int(gamma), rows_matrix=int(li.rows_matrix), n_c=int(rd["n_c"]),
                       n_e_host=int(rd["n_e"]), n_gamma_host=int(rg["n_e"]) if rg else 0, degree=m)
            path = "compact" if compact else ("gamma" if gamma else "full")
            want = a.expect if case.poly else "full"           # (no polynomial, no compact system; Robin / diphasic: no identity rows)
            if name == "diph2d" and path != "full":
                raise rt.ResidualMismatch(f"{name}: the diphasic system does not keep the full system: {path}")
            if path != want:
                raise rt.ResidualMismatch(f"{name}/{data}: the loop took the {path} path, {want} expected")
            res["path"] = path
            if path != "full":
                red = rd if compact else rg
                if int(li.rows_matrix) != red["n_c"] or int(si.n_own) - int(li.rows_matrix) != red["n_e"]:
                    raise rt.ResidualMismatch(f"{name}: the loop leaves {int(si.n_own) - int(li.rows_matrix)} rows out, the host {red['n_e']}")
                # the matrix the loop multiplies by IS the full one restricted: entry for entry, values bitwise
                rt.same_matrix(L.loop_system_csr(s._h, 7), red, f"{name} {path} loop matrix")
                res["loop_matrix_checked"] = {"rows": red["n_c"], "nnz": int(red["rowptr"][-1]), "coupling_rows": int(red["wg_rows"].size),
                                              "coupling_nnz": int(red["wg_ptr"][-1])}
        y_prev = x_prev[idx] / ds
        y_start = snapped(y_prev, Ah, bh, red["elist"]) if red is not None else y_prev
        rec, _ = check_solve(case, 3, info, run1, reltol, "bicgstab", y_start, f"{name}/{data} step {k + 1} reltol={reltol:g}",
                             want_ref=not a.guess)
        x = s._fetch_state()
        if red is not None:
            moved_steps.append(float(np.max(np.abs(x[idx][red["elist"]] - x_prev[idx][red["elist"]]))))
            moved = max(moved_steps)
        if a.guess:
            rec["guess_kept"] = s.guess_info()["kept"]
            rec["guess_states"] = len(s.guess_info()["offsets"])
            kept_max = max(kept_max, rec["guess_kept"])
        if a.iters and abs(rec["iters"] - rec["it_ref"]) > 1:
            raise rt.ResidualMismatch(f"{rec['label']}: {rec['iters']} iterations, the restatement on the full system takes {rec['it_ref']}")
        if not rec["converged"]:
            unconv += 1
        relres.append(info.resnorm / info.bnorm if info.bnorm > 0 else 0.0)
        res["steps"].append(rec)
        x_prev = x
    res["eliminated_rows_moved_by"] = moved
    res["eliminated_rows_moved_by_step"] = moved_steps
    # steps in which the rows left out did not move at all: the compact loop's steps with unchanged data, whose start phase is
    # folded into the right-hand-side kernel and which queue no coupling launch (a row that does move there sends the step to
    # the full system)
    quiet = [k for k, v in enumerate(moved_steps) if k >= 1 and v == 0.0] if (res["path"] == "compact" and data == "const") else []
    res["quiet_steps"] = len(quiet)
    # ... and those among them that ended at a half step: the residual reported is then (s,s)_W plus what the rows that stayed hold
    res["quiet_half_exits"] = sum(res["steps"][k]["half_exit"] for k in quiet)
    res["half_exits"] = sum(r["half_exit"] for r in res["steps"])
    if data != "const" and res["path"] != "full" and not moved > 0.0:
        raise rt.ResidualMismatch(f"{name}/{data}: the rows alone on their diagonal did not move although their datum changes every step")
    if a.guess:
        res["guess_kept_max"] = kept_max
        if res["path"] == "compact" and kept_max == 0:
            raise rt.ResidualMismatch(f"{name}: PG_GUESS_ALWAYS=1 and no older state was kept in {a.steps} steps")
    # the same steps in one call on a fresh solver: the run's totals describe the very solves checked above
    if data != "closure":
        c2 = Case(name, data)
        L.check(lib.pg_solver_initial_solve(c2.s._h, C.byref(o), C.byref(info)))
        c2.install(a.steps)
        run = L.pg_run_info()
        L.check(lib.pg_solver_run(c2.s._h, C.c_double(1e300), C.c_int32(sch), C.byref(o), C.c_int32(0), C.c_int64(a.steps), C.c_int32(0),
                                  C.byref(run)))
        res["run"] = {"steps": int(run.steps), "total_iters": int(run.total_iters), "worst_relres": run.worst_relres,
                      "unconverged_steps": int(run.unconverged_steps), "poly_degree": int(run.poly_degree), "half_exits": int(run.half_exits),
                      "products": int(run.products), "poly_f32_chains": int(run.poly_f32_chains), "guess_states_read": int(run.guess_states_read)}
        res["stepwise"] = {"worst_relres": max(relres), "unconverged_steps": unconv, "total_iters": sum(r["iters"] for r in res["steps"]),
                           "products": sum(r["products"] for r in res["steps"]), "half_exits": res["half_exits"]}
        if run.steps != a.steps or run.worst_relres != max(relres) or run.unconverged_steps != unconv:
            raise rt.ResidualMismatch(f"{name}/{data}: run totals {res['run']} differ from the stepwise run's {res['stepwise']}")
        if run.total_iters != res["stepwise"]["total_iters"] or run.products != res["stepwise"]["products"] or run.half_exits != res["half_exits"]:
            raise rt.ResidualMismatch(f"{name}/{data}: run counts {res['run']} against the stepwise run's {res['stepwise']}")
        if case.poly and res["path"] != "full" and run.poly_degree != precond:
            raise rt.ResidualMismatch(f"{name}/{data}: degree {run.poly_degree} in the last solve, {precond} asked for")
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["first", "warm"])
    p.add_argument("--expect", choices=["full", "gamma", "compact"], default="compact")
    p.add_argument("--cases", default="ball3d,ball3d_odd,disc2d_robin,diph2d")
    p.add_argument("--data", default="const")
    p.add_argument("--steps", type=int, default=4)
    p.add_argument("--degree", type=int, default=5)
    p.add_argument("--guess", action="store_true", help="PG_GUESS_ALWAYS=1: older states must be kept; no restatement (another start)")
    p.add_argument("--iters", action="store_true", help="hold every warm step's iterations to the restatement's")
    p.add_argument("--one-reltol", action="store_true")
    a = p.parse_args()
    out = {"mode": a.mode, "args": vars(a), "ok": False}
    status = 0
    try:
        pj.init(0)
        if a.mode == "first":
            run_first(out)
        else:
            run_warm(out, a)
        out["ok"] = True
    except Exception as e:                       # (nothing more runs on the device: the process ends here)
        out["error"] = f"{type(e).__name__}: {e}"
        status = 1
    print(json.dumps(out))
    return status


if __name__ == "__main__":
    sys.exit(main())
