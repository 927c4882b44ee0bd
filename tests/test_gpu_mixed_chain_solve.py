"""The mixed-precision Horner chain inside the time loop (pg_krylov.hip), on the benchmark's shape at 64^3:
sphere r = 1 at (2.01, 2.01, 2.01) in the 4^3 box, Dirichlet data, Δt = 0.75 h², backward Euler for the first solve, then 12
Crank-Nicolson steps through pg_solver_run with the default options -- in a child process per setting, because the switches are
read from the environment once per process:

    PG_POLY_F32=0                        today's all-fp64 chain
    PG_POLY_F32=1                        the mixed chain, tail from the reduction each solve needs (twice: reproducibility)
    PG_POLY_F32=1 PG_POLY_F32_TAIL=0     the shortest tail there is (the hand-over launch alone) forced on every solve

Checked: every solve converges in every run (a forced short tail may cost second applications; it must not end unconverged);
every state is within TOL_T of the oracle's direct solve FROM THE PREVIOUS STATE OF THE SAME RUN (one LU factorisation of the
oracle's Crank-Nicolson matrix serves every step of every run: the matrix does not change); the two default runs agree bit for
bit; the run info reports fp32 launches, chains and tails with PG_POLY_F32=1 and exactly none with =0; and with =0 the final
state is bit for bit the all-fp64 loop's.  The commit before the mixed chain gave, with this file's child (sha256 over the
float64 bytes of the state after step 12, and the --dump-outputs style figures):

    sha256 10c60daa76c73d566b7d23424e9b26f9ad19c0ce2a69c588d53f7458ca093038
    n 549250  nonzero 40644  l2 173.2211640100048  max_abs 1.0000000000000004  sum 32794.75210657847

and the chain, switched off, reproduced it.  Since then the all-fp64 loop itself has moved in its last bits: on a step with
unchanged data a row alone on its diagonal whose correction is within the noise threshold stays where it is, so that the
residual the solve reports is the state's (pg_solver.hip k_rhs_init_c; tests/test_gpu_residual_truth.py), where it used to
move without the rows coupled to it hearing of it.  The pin is the all-fp64 state with that in:

    sha256 dd1aed62d089b44ef72d9066a9c0f8d2a2907f6b9ae2fa7035dfbbfbf6d0e23b
    n 549250  nonzero 40644  l2 173.2211640100048  max_abs 1.0000000000000007  sum 32794.75210657847

The solves run to reltol = 1e-13, as every comparison at TOL_T in tests/test_gpu_parity.py does (the environment's defaults
otherwise).

The reference.  At 64^3 the oracle's direct solve alone is not good to TOL_T = 1e-10: SuperLU's solution of the step's system
lies 6.7e-11 (relative L2) from the solution of that very system, and a one-ulp perturbation of the right-hand side moves the
solution by 3.4e-11 (both measured on the CPU with the oracle's own capacities; two rounds of iterative refinement with the
residual in long double bring the correction down to 2e-17).  Held against the unrefined solve, the all-fp64 chain with
PG_POLY_F32=0 -- bit for bit the previous commit's states -- misses TOL_T itself: 1.69e-10 at step 1 with reltol = 1e-13, 1.0012e-10
at step 2 with reltol = 1e-12 (and 1.0012e-10 there with the mixed chain and with the forced tail: the three agree to four digits
because the distance is the reference's error).  So the oracle's direct solve is refined REFINE times with an extended-precision
residual before anything is held against it: the reference gets better, the bound stays TOL_T.
"""
import hashlib
import json
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from oracle import penguin_oracle as po
from tests.common import oracle_capacity_from_product, rel_l2
from tests.test_gpu_parity import HEAT_BORDERS, TOL_T

pytestmark = pytest.mark.gpu

N, STEPS = 64, 12
RELTOL = 1e-13      # what every TOL_T comparison of tests/test_gpu_parity.py solves to (module docstring)
REFINE = 2          # rounds of iterative refinement of the oracle's direct solve (module docstring)
DT = 0.75 * (4.0 / N) ** 2
ROOT = pathlib.Path(__file__).resolve().parents[1]
# state after step 12 of the all-fp64 run (module docstring)
FP64_STATE_SHA256 = "dd1aed62d089b44ef72d9066a9c0f8d2a2907f6b9ae2fa7035dfbbfbf6d0e23b"

_RUNS, _ORACLE = {}, {}


def summary(x):
    """the figures bench.py --dump-outputs writes about a state, and a hash of its bytes"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    return {"sha256": hashlib.sha256(x.tobytes()).hexdigest(), "n": int(x.size), "l2": float(np.linalg.norm(x)),
            "max_abs": float(np.max(np.abs(x))), "sum": float(np.sum(x)), "nonzero": int(np.count_nonzero(x))}


def child(out, reltol=RELTOL):
    """the run itself (in the child process): states 0 .. STEPS and the run info to `out`.npz"""
    import ctypes as C

    import penguin.jl_amd as pj
    from penguin.jl_amd import _lib as L
    from penguin.jl_amd.api import _krylov_opts

    pj.init(0)
    mesh = pj.Mesh((N,) * 3, (4.0,) * 3)
    cap = pj.Capacity(pj.Sphere((2.01,) * 3, 1.0), mesh)
    bcb = pj.BorderConditions({k: pj.Dirichlet(1.0) for k in HEAT_BORDERS})
    s = pj.DiffusionUnsteadyMono(pj.Phase(cap, pj.DiffusionOps(cap), 0.0, 1.0), bcb, pj.Dirichlet(1.0), DT, None, "BE")
    opts = _krylov_opts("bicgstab", {"reltol": reltol})
    run = L.pg_run_info()
    L.check(L.lib().pg_solver_run(s._h, C.c_double(1e30), C.c_int32(L.PG_SCHEME["CN"]), C.byref(opts), C.c_int32(1),
                                  C.c_int64(STEPS), C.c_int32(1), C.byref(run)))
    nstates = C.c_int64(0)
    L.check(L.lib().pg_solver_num_states(s._h, C.byref(nstates)))
    assert nstates.value == STEPS + 1, nstates.value
    states = np.stack([s._fetch_state(k) for k in range(STEPS + 1)])
    info = {k: getattr(run, k) for k, _ in L.pg_run_info._fields_}
    np.savez(out, states=states, info=json.dumps(info), config=pj.config_string(), summary=json.dumps(summary(states[-1])))
    print("child ok", json.dumps(summary(states[-1])))


def _run(tag, env, tmp_path_factory):
    if tag not in _RUNS:
        out = tmp_path_factory.mktemp("mixed_chain") / f"{tag}.npz"
        env = dict(env)
        reltol = float(env.pop("reltol", RELTOL))
        code = f"import sys; sys.path.insert(0, '.'); import tests.test_gpu_mixed_chain_solve as t; t.child({str(out)!r}, {reltol!r})"
        base = {k: v for k, v in os.environ.items() if k not in ("PG_POLY_F32", "PG_POLY_F32_TAIL")}
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env={**base, **env}, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "child ok" in r.stdout, (env, r.stdout[-2000:], r.stderr[-4000:])
        z = np.load(out)
        _RUNS[tag] = {"states": z["states"], "info": json.loads(str(z["info"])), "config": str(z["config"])}
    return _RUNS[tag]


ENVS = {"f64": {"PG_POLY_F32": "0"}, "mixed": {"PG_POLY_F32": "1"}, "mixed_again": {"PG_POLY_F32": "1"},
        "forced": {"PG_POLY_F32": "1", "PG_POLY_F32_TAIL": "0"},
        # the library's default tolerance, which the bench runs at: the tail rule chooses shorter tails there ("reltol" is not an
        # environment variable: _run hands it to the child)
        "mixed_default_reltol": {"PG_POLY_F32": "1", "reltol": "1e-12"}}


def _oracle(pj):
    """the oracle's systems of the problem, on the product's capacities, each factorised once: (phase, border conditions,
    reduced index set and LU of the constructor's BE matrix and of the loop's CN matrix)"""
    if not _ORACLE:
        M = (N + 1) ** 3
        omesh = po.Mesh((N,) * 3, (4.0,) * 3)
        cap = pj.Capacity(pj.Sphere((2.01,) * 3, 1.0), pj.Mesh((N,) * 3, (4.0,) * 3))
        ocap = oracle_capacity_from_product(cap, omesh)
        oph = po.Phase(ocap, po.make_diffusion_ops(ocap), lambda x, y, z, t: 0.0, lambda x, y, z: 1.0)
        obcb = po.BorderConditions({k: po.Dirichlet(1.0) for k in HEAT_BORDERS})
        _ORACLE.update(M=M, oph=oph, obcb=obcb, omesh=omesh, lu={})
    return _ORACLE


def _oracle_solve(pj, scheme, Ti, t):
    """the oracle's direct solve of one step of `scheme` from the state Ti (diffusion.jl:243-265, 286-294), the LU of the
    step's reduced matrix kept: the matrix is the same in every step"""
    o = _oracle(pj)
    oph, bci = o["oph"], po.Dirichlet(1.0)
    if scheme not in o["lu"]:
        o["lu"][scheme] = {"A": po.A_mono_unstead_diff(oph.operator, oph.capacity, oph.Diffusion_coeff, bci, DT, scheme)}
    e = o["lu"][scheme]
    b = po.b_mono_unstead_diff(oph.operator, oph.source, oph.Diffusion_coeff, oph.capacity, bci, Ti, DT, t, scheme)
    A, b = po.BC_border_mono(e["A"], b, o["obcb"], o["omesh"], t=t)
    if "solve" not in e:
        Ar, _, idx = po.remove_zero_rows_cols(A, b)
        Ar = Ar.tocsr()
        Ar.sort_indices()
        assert np.all(np.diff(Ar.indptr) > 0)
        e.update(Ar=Ar, idx=idx, solve=spla.splu(Ar.tocsc()).solve)
    Ar, br, ld = e["Ar"], b[e["idx"]], np.longdouble
    assert np.finfo(ld).nmant >= 63
    xr = e["solve"](br)
    for _ in range(REFINE):      # residual in extended precision, correction through the same factors
        res = br.astype(ld) - np.add.reduceat(Ar.data.astype(ld) * xr[Ar.indices].astype(ld), Ar.indptr[:-1])
        xr = xr + e["solve"](res.astype(np.float64))
    x = np.zeros(2 * o["M"])
    x[e["idx"]] = xr
    return x


@pytest.mark.parametrize("tag", ["f64", "mixed", "forced", "mixed_default_reltol"])
def test_every_solve_converges_and_every_state_matches_the_oracles_step(pj, tag, tmp_path_factory):
    r = _run(tag, ENVS[tag], tmp_path_factory)
    info, states = r["info"], r["states"]
    print(tag, {k: info[k] for k in ("total_iters", "products", "half_exits", "unconverged_steps", "worst_relres", "poly_f32_launches",
                                     "poly_f32_chains", "poly_f32_tail_sum")})
    assert info["steps"] == STEPS and info["unconverged_steps"] == 0, info
    M = (N + 1) ** 3
    worst = rel_l2(states[0], _oracle_solve(pj, "BE", np.zeros(2 * M), 0.0))
    assert worst <= TOL_T, ("first solve", worst)
    for k in range(1, STEPS + 1):
        e = rel_l2(states[k], _oracle_solve(pj, "CN", states[k - 1], k * DT))
        worst = max(worst, e)
        assert e <= TOL_T, (tag, k, e)
    print(tag, "largest distance to the oracle's step:", worst)


def test_fp32_launches_are_reported_when_on_and_none_when_off(pj, tmp_path_factory):
    off, on, forced = (_run(t, ENVS[t], tmp_path_factory) for t in ("f64", "mixed", "forced"))
    assert "poly_f32=0" in off["config"] and "poly_f32=1" in on["config"] and "poly_f32_tail=0" in forced["config"]
    for k in ("poly_f32_launches", "poly_f32_timed", "poly_f32_chains", "poly_f32_tail_sum"):
        assert off["info"][k] == 0, (k, off["info"][k])
    assert off["info"]["poly_f32_ms_total"] == 0.0
    for r in (on, forced):
        i = r["info"]
        assert i["poly_f32_launches"] > 0 and i["poly_f32_chains"] > 0, i
        assert i["poly_f32_tail_sum"] >= i["poly_f32_chains"], i                 # (every tail has its hand-over launch)
        assert i["poly_f32_launches"] >= 3 * i["poly_f32_chains"], i             # (two fp32 stores and the hand-over at least)
    f = forced["info"]
    assert f["poly_f32_tail_sum"] == f["poly_f32_chains"], f                     # (the forced tail is the hand-over alone)


def test_mixed_runs_are_bitwise_reproducible(pj, tmp_path_factory):
    a, b = _run("mixed", ENVS["mixed"], tmp_path_factory), _run("mixed_again", ENVS["mixed_again"], tmp_path_factory)
    assert a["info"]["total_iters"] == b["info"]["total_iters"] and a["info"]["products"] == b["info"]["products"]
    assert a["info"]["poly_f32_tail_sum"] == b["info"]["poly_f32_tail_sum"]
    assert np.array_equal(a["states"].view(np.uint64), b["states"].view(np.uint64))


def test_switched_off_the_state_is_the_fp64_loops_bit_for_bit(pj, tmp_path_factory):
    r = _run("f64", ENVS["f64"], tmp_path_factory)
    got = summary(r["states"][-1])
    print(got)
    assert got["sha256"] == FP64_STATE_SHA256, got
