"""One child process of tests/test_gpu_step_head_fused.py.  PG_STEP_FUSE is read once per process, so the test runs every case
twice -- the fit inside the right-hand-side launch (1) or as a launch of its own (0) -- in fresh
processes and compares what the two print and save.

    python tests/step_head_child.py --case sphere3d|sphere3d_jump|disc2d --steps N --out DIR

The child takes the first solve (BE) and N Crank-Nicolson steps, one pg_solver_run call each (its pg_run_info carries the
iterations, the products and the degree of that solve), reads pg_solver_guess_info after every step, and saves the state after
the last step and the exported right-hand side b̂ (system 3) to DIR.  Floating-point figures travel as hex strings: the test
compares bits.  sphere3d_jump changes the interface value between steps 6 and 7: step 7 is sent (old value at t, new value at
t + Δt), step 8 (new, new) -- two steps with changed data (coupling launch, block-row tables rebuilt); under Crank-Nicolson
the interface rows then rest at the new value, and the steps after them are quiet again.  ONE JSON line; exit status 0 and "ok": true, or 1 and "error".
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


def build(case):
    if case in ("sphere3d", "sphere3d_jump"):
        n, ext, centre = (40, 40, 40), (4.0,) * 3, (2.01,) * 3
    elif case == "disc2d":
        n, ext, centre = (768, 768), (4.0, 4.0), (2.01, 2.01)
    else:
        raise ValueError(case)
    mesh = pj.Mesh(n, ext)
    cap = pj.Capacity(pj.Sphere(centre, 1.0), mesh)
    M = int(np.prod([v + 1 for v in n]))
    dt = 0.75 * (4.0 / max(n)) ** 2
    ph = pj.Phase(cap, pj.DiffusionOps(cap), 0.0, 1.0)
    bcb = pj.BorderConditions({k: pj.Dirichlet(1.0) for k in KEYS})
    s = pj.DiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(1.0), dt, np.zeros(2 * M), "BE")
    return s, M, (mesh, cap, ph, bcb)


def one_solve(s, o, initial):
    run = L.pg_run_info()
    L.check(L.lib().pg_solver_run(s._h, C.c_double(1e300), C.c_int32(L.PG_SCHEME["CN"]), C.byref(o), C.c_int32(1 if initial else 0),
                                  C.c_int64(0 if initial else 1), C.c_int32(0), C.byref(run)))
    return {"iters": int(run.total_iters), "products": int(run.products), "degree": int(run.poly_degree),
            "half_exits": int(run.half_exits), "unconverged": int(run.unconverged_steps), "relres": float(run.worst_relres).hex(),
            "states_read": int(run.guess_states_read)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--case", required=True)
    p.add_argument("--steps", type=int, required=True)
    p.add_argument("--out", required=True)
    a = p.parse_args()
    out = {"case": a.case, "ok": False}
    status = 0
    try:
        pj.init(0)
        out["config"] = dict(kv.split("=", 1) for kv in pj.config_string().split() if "=" in kv)
        s, M, keep = build(a.case)
        o = api._krylov_opts("bicgstab", {"reltol": 1e-9})
        out["first"] = one_solve(s, o, True)
        steps = []
        for k in range(1, a.steps + 1):
            if a.case == "sphere3d_jump" and k in (JUMP_BEFORE_STEP, JUMP_BEFORE_STEP + 1):
                g0, g1 = np.full(M, JUMP_FROM if k == JUMP_BEFORE_STEP else JUMP_TO), np.full(M, JUMP_TO)
                L.check(L.lib().pg_solver_set_interface_value(s._h, L.dptr(g0), L.dptr(g1)))
            rec = one_solve(s, o, False)
            gi = s.guess_info()
            rec["guess"] = {"kept": int(gi["kept"]), "offsets": [int(v) for v in gi["offsets"]],
                            "coef": [float(v).hex() for v in gi["coef"]],
                            "rr": [float(gi["rr_plain"]).hex(), float(gi["rr_taken"]).hex()]}
            steps.append(rec)
        out["steps"] = steps
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
