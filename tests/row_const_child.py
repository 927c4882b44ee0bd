"""One child process of tests/test_gpu_row_const.py.  PG_ROW_CONST is read once per process, so the test runs every case twice
-- the compact loop's kernels taking the constants of uniform groups of rows from their arguments (1) or streaming them for
every row (0) -- in fresh processes and compares what the two print and save.

    python tests/row_const_child.py --case CASE --steps N --out DIR

Cases (a sphere of radius 1 centred at 2.01 in a box of side 4, Dirichlet everywhere, as tests/step_head_child.py):
  sphere128         128^3: chords of up to 64 rows, uniform groups and broken ones side by side in one wave
  sphere128_jump    the interface value changes before steps 7 and 8 (as step_head_child's sphere3d_jump)
  sphere128_source  a source constant in space and different in every step (TimeSeparable): bconst is one value along the
                    rows of a step and another one in the next
  sphere128_fsteps  a source constant in space and in time for 5 steps, another constant from step 6 on (sent by
                    pg_solver_set_source): the bconst mark is built, goes stale, and is built again
  sphere40          40^3: no chord has 16 rows in a line that start at a multiple of 16 -- no group qualifies
  disc768           768^2: long runs, a partial last group

The child takes the first solve (BE) and N Crank-Nicolson steps, one pg_solver_run call each, reads pg_solver_guess_info after
every step, with what pg_debug_row_const_bconst says about the bconst mark, and pg_solver_row_const_info at the end, and
saves the state after the last step and the exported right-hand side b̂ (system 3) to DIR.  Floating-point figures travel as
hex strings: the test compares bits.  ONE JSON line; exit status 0 and "ok": true, or 1 and "error".
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
from penguin.jl_amd import _lib as L             # noqa: E402
from penguin.jl_amd import api                   # noqa: E402

KEYS = ("left", "right", "top", "bottom")
JUMP_BEFORE_STEP, JUMP_FROM, JUMP_TO = 7, 1.0, 1.25
FSTEP_BEFORE_STEP, FSTEP_FROM, FSTEP_TO = 6, 0.3, 0.7
SIZES = {"sphere128": (128,) * 3, "sphere128_jump": (128,) * 3, "sphere128_source": (128,) * 3, "sphere128_fsteps": (128,) * 3,
         "sphere40": (40,) * 3, "disc768": (768, 768)}


def source_of(case, dt):
    if case == "sphere128_source":
        return pj.TimeSeparable([(1.0, lambda t: 0.25 + t / (10.0 * dt))])     # (another value in every step)
    if case == "sphere128_fsteps":
        return FSTEP_FROM
    return 0.0


def build(case):
    n = SIZES[case]
    mesh = pj.Mesh(n, (4.0,) * len(n))
    cap = pj.Capacity(pj.Sphere((2.01,) * len(n), 1.0), mesh)
    M = int(np.prod([v + 1 for v in n]))
    dt = 0.75 * (4.0 / max(n)) ** 2
    src = source_of(case, dt)
    ph = pj.Phase(cap, pj.DiffusionOps(cap), src, 1.0)
    bcb = pj.BorderConditions({k: pj.Dirichlet(1.0) for k in KEYS})
    s = pj.DiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(1.0), dt, np.zeros(2 * M), "BE")
    return s, M, dt, src, (mesh, cap, ph, bcb)


def one_solve(s, o, initial):
    run = L.pg_run_info()
    L.check(L.lib().pg_solver_run(s._h, C.c_double(1e300), C.c_int32(L.PG_SCHEME["CN"]), C.byref(o), C.c_int32(1 if initial else 0),
                                  C.c_int64(0 if initial else 1), C.c_int32(0), C.byref(run)))
    return {"iters": int(run.total_iters), "products": int(run.products), "degree": int(run.poly_degree),
            "half_exits": int(run.half_exits), "unconverged": int(run.unconverged_steps), "relres": float(run.worst_relres).hex(),
            "states_read": int(run.guess_states_read)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--case", required=True, choices=sorted(SIZES))
    p.add_argument("--steps", type=int, required=True)
    p.add_argument("--out", required=True)
    a = p.parse_args()
    out = {"case": a.case, "ok": False}
    status = 0
    try:
        pj.init(0)
        out["config"] = dict(kv.split("=", 1) for kv in pj.config_string().split() if "=" in kv)
        s, M, dt, src, keep = build(a.case)
        o = api._krylov_opts("bicgstab", {"reltol": 1e-9})
        out["first"] = one_solve(s, o, True)
        if a.case == "sphere128_source":       # (as the drivers do: spatial parts and coefficient table once, after the first solve)
            cap = keep[1]
            api._install_separable(s, api._TD_SOURCE, 0, api._separable_fields(src, cap._cw, 3, M),
                                   api._separable_table(src, dt, 1e300, a.steps))
        steps = []
        for k in range(1, a.steps + 1):
            if a.case == "sphere128_jump" and k in (JUMP_BEFORE_STEP, JUMP_BEFORE_STEP + 1):
                g0, g1 = np.full(M, JUMP_FROM if k == JUMP_BEFORE_STEP else JUMP_TO), np.full(M, JUMP_TO)
                L.check(L.lib().pg_solver_set_interface_value(s._h, L.dptr(g0), L.dptr(g1)))
            if a.case == "sphere128_fsteps" and k in (FSTEP_BEFORE_STEP, FSTEP_BEFORE_STEP + 1):
                f0, f1 = np.full(M, FSTEP_FROM if k == FSTEP_BEFORE_STEP else FSTEP_TO), np.full(M, FSTEP_TO)
                L.check(L.lib().pg_solver_set_source(s._h, 0, L.dptr(f0), L.dptr(f1)))
            rec = one_solve(s, o, False)
            gi = s.guess_info()
            rec["guess"] = {"kept": int(gi["kept"]), "offsets": [int(v) for v in gi["offsets"]],
                            "coef": [float(v).hex() for v in gi["coef"]],
                            "rr": [float(gi["rr_plain"]).hex(), float(gi["rr_taken"]).hex()]}
            rec["bmark"] = s.row_const_bconst_info()      # (did this step's launch take a bconst mark, how many groups it marks)
            steps.append(rec)
        out["steps"] = steps
        out["row_const"] = s.row_const_info()
        si = s.system_info(3)
        out["n_own"], out["loop_is_compact"] = int(si.n_own), int(si.loop_is_compact)
        _, bhat, _ = s.system(3)
        np.save(Path(a.out) / "state.npy", s._fetch_state())
        np.save(Path(a.out) / "bhat.npy", np.asarray(bhat))
        out["ok"] = True
    except Exception as e:                       # (nothing more runs on the device: the process ends here)
        out["error"] = f"{type(e).__name__}: {e}"
        status = 1
    print(json.dumps(out))
    return status


if __name__ == "__main__":
    sys.exit(main())
