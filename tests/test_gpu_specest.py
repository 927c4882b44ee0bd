"""precond="poly-est" (PG_PRECOND_POLY_EST) on the GPU: the spectral estimate of csrc/pg_specest.hip against the numpy restatement
(tests/specest_reference.py) on the matrix the library iterates on, the admission of the polynomial preconditioner where
Gershgorin refuses it, parity of the runs it changes with the oracle's direct solves and with the default-options runs, and
what the option refuses.

Shapes: the config-5 diphasic family at 32^2 and 64^2 (BE first solve + 4 CN steps), a monophasic Robin(1,1,1) and Neumann(0)
interface at 32^2 with four Dirichlet borders, diphasic 12^3 -- the smallest with cut cells of every kind and a few hundred rows
per Arnoldi step.  Nothing here reads a file outside the tree."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import penguin_oracle as po
from penguin.jl_amd import _lib as L
from tests import specest_reference as sr
from tests.common import oracle_capacity_from_product, rel_l2

pytestmark = pytest.mark.gpu

KEYS2 = ("left", "right", "top", "bottom")
ZERO = lambda x, y, z, t: 0.0
CASES = ["diph32", "diph64", "robin32", "neumann32", "diph3d12"]
_RUNS, _REF = {}, {}


def _const(v):
    return lambda x, y, z: v


def _build(pj, case):
    """(make: () -> product solver, solve: (solver, steps, **kw) -> solver, oracle: steps -> states, scheme)"""
    if case.startswith("diph"):
        N, n = (3, 12) if case == "diph3d12" else (2, int(case[4:]))
        Lx = 8.0
        M = (n + 1) ** N
        mesh, omesh = pj.Mesh((n,) * N, (Lx,) * N, (0.0,) * N), po.Mesh((n,) * N, (Lx,) * N, (0.0,) * N)
        c1 = pj.Capacity(pj.Sphere((4.0,) * N, 2.0), mesh)
        c2 = pj.Capacity(pj.Sphere((4.0,) * N, 2.0, complement=True), mesh)
        p1, p2 = pj.Phase(c1, pj.DiffusionOps(c1), ZERO, _const(1.0)), pj.Phase(c2, pj.DiffusionOps(c2), ZERO, _const(2.0))
        ic = pj.InterfaceConditions(pj.ScalarJump(1.0, 0.5, 0.0), pj.FluxJump(1.0, 1.0, 0.0))
        bcb = pj.BorderConditions({})
        u0 = np.concatenate([np.ones(M), np.ones(M), np.zeros(M), np.zeros(M)])
        dt = 0.5 * (Lx / n) ** 2

        def make():
            return pj.DiffusionUnsteadyDiph(p1, p2, bcb, ic, dt, u0, "BE")

        def solve(s, steps, **kw):
            return pj.solve_DiffusionUnsteadyDiph_b(s, p1, p2, dt, steps * dt, bcb, ic, "CN", time_independent=True, **kw)

        def oracle(steps):
            o1, o2 = oracle_capacity_from_product(c1, omesh), oracle_capacity_from_product(c2, omesh)
            q1 = po.Phase(o1, po.make_diffusion_ops(o1), ZERO, _const(1.0))
            q2 = po.Phase(o2, po.make_diffusion_ops(o2), ZERO, _const(2.0))
            oic = po.InterfaceConditions(po.ScalarJump(1.0, 0.5, 0.0), po.FluxJump(1.0, 1.0, 0.0))
            so = po.DiffusionUnsteadyDiph(q1, q2, po.BorderConditions({}), oic, dt, u0, "BE")
            po.solve_DiffusionUnsteadyDiph(so, q1, q2, dt, steps * dt, po.BorderConditions({}), oic, "CN", method="\\")
            return so.states

        return make, solve, oracle
    n = 32
    M = (n + 1) ** 2
    mesh, omesh = pj.Mesh((n, n), (4.0, 4.0)), po.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0, complement=True), mesh)      # fluid outside the disc, up to the borders
    ph = pj.Phase(cap, pj.DiffusionOps(cap), ZERO, _const(1.0))
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS2})
    bc, obc = (pj.Robin(1.0, 1.0, 1.0), po.Robin(1.0, 1.0, 1.0)) if case == "robin32" else (pj.Neumann(0.0), po.Neumann(0.0))
    u0 = np.ones(2 * M)
    dt = 0.5 * (4.0 / n) ** 2

    def make():
        return pj.DiffusionUnsteadyMono(ph, bcb, bc, dt, u0, "BE")

    def solve(s, steps, **kw):
        return pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, steps * dt, bcb, bc, "CN", time_independent=True, **kw)

    def oracle(steps):
        oc = oracle_capacity_from_product(cap, omesh)
        oph = po.Phase(oc, po.make_diffusion_ops(oc), ZERO, _const(1.0))
        obcb = po.BorderConditions({k: po.Dirichlet(0.0) for k in KEYS2})
        so = po.DiffusionUnsteadyMono(oph, obcb, obc, dt, u0, "BE")
        po.solve_DiffusionUnsteadyMono(so, oph, dt, steps * dt, obcb, obc, "CN", method="\\")
        return so.states

    return make, solve, oracle


def _one_more_step(s, precond):
    """one step of the run system through pg_solver_run: the run info has the degree of its solve"""
    run = L.pg_run_info()
    opts = L.pg_krylov_opts(L.PG_METHOD["bicgstab"], 1e-12, 0.0, 0, 4, 1, 0, precond)
    L.check(L.lib().pg_solver_run(s._h, C.c_double(1e300), C.c_int32(L.PG_SCHEME["CN"]), C.byref(opts), C.c_int32(0), C.c_int64(1),
                                  C.c_int32(0), C.byref(run)))
    assert run.unconverged_steps == 0
    return run


def run(pj, case):
    """BE first solve + 4 CN steps with the default options and with "poly-est" (+ one step each for the run info), once"""
    if case not in _RUNS:
        make, solve, oracle = _build(pj, case)
        out = {"oracle": oracle(4), "alive": (make, solve)}     # (a solver does not own its operators: they live as long as it does)
        for key, precond in (("default", 0), ("est", "poly-est")):
            s = make()
            solve(s, 4, reltol=1e-12, precond=precond)
            out[key] = s
            out[key + "_states"] = [np.array(x) for x in s.states]
            out[key + "_run"] = _one_more_step(s, L.PG_PRECOND_POLY_EST if key == "est" else 0)
        _RUNS[case] = out
    return _RUNS[case]


def krylov_matrix(s, which):
    """Â of system `which` (0 constructor, 1 run) as the library iterates on it: pg_solver_get_system_csr(2 / 3)"""
    rowptr, col, val = L.loop_system_csr(s._h, 2 + which)
    n = rowptr.size - 1
    return sp.csr_matrix((val, col, rowptr), shape=(n, n))


def reference(pj, case, which):
    """the restatement on the downloaded Â, float64 and long double; g_true from dense eigvals at 32^2"""
    if (case, which) not in _REF:
        A = krylov_matrix(run(pj, case)["est"], which)
        e64, e80 = sr.estimate(A, L.PG_SPECEST_MARGIN), sr.estimate(A, L.PG_SPECEST_MARGIN, dtype=np.longdouble)
        g_true = float(np.max(np.abs(np.linalg.eigvals(A.toarray()) - 1.0))) if A.shape[0] <= 2500 else None
        _REF[(case, which)] = (e64, e80, g_true)
    return _REF[(case, which)]


# ------------------------------------------------------------------------------------ 1. the estimator against the restatement
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("which", [0, 1])
def test_the_estimate_matches_the_restatement(pj, case, which):
    """Hessenberg matrix entry by entry over the first 10 columns and g_ritz, both within 10 x what the restatement itself moves
    by between float64 and long double on that system (floor 1e-12): the bar of an application in tests/test_gpu_multigrid.py.
    (Arnoldi loses agreement between roundings column by column; the converged extremes do not.)"""
    s = run(pj, case)["est"]
    e = s.spectral_estimate(which)
    H = L.debug_specest_hessenberg(s._h, which)
    e64, e80, g_true = reference(pj, case, which)
    assert e["steps"] == sr.STEPS == e64["steps"] and H.shape == (sr.STEPS + 1, sr.STEPS)
    tol_h = max(10.0 * np.max(np.abs(e64["H"][:, :10] - e80["H"][:, :10])), 1e-12)
    tol_g = max(10.0 * abs(e64["g_ritz"] - e80["g_ritz"]), 1e-12)
    dh, dg = np.max(np.abs(H[:, :10] - e64["H"][:, :10])), abs(e["g_ritz"] - e64["g_ritz"])
    print(f"{case} which {which}: |H - H_ref| over 10 columns {dh:.2e} (bar {tol_h:.2e}), |g_ritz - ref| {dg:.2e} (bar {tol_g:.2e}), "
          f"g_ritz {e['g_ritz']:.5f}, g_used {e['g_used']:.5f}, g_true {g_true}, Gershgorin {e['gershgorin']:.1f}, {e['estimate_ms']:.2f} ms")
    assert dh <= tol_h
    assert dg <= tol_g
    assert e["margin"] == L.PG_SPECEST_MARGIN and e["g_used"] == pytest.approx(e["g_ritz"] + e["margin"], abs=1e-15)
    assert e["admitted"] == int(e["g_used"] < 0.95) == int(e64["admitted"])
    assert e["ritz_re_min"] == pytest.approx(e64["re_min"], abs=1e-6) and e["ritz_re_max"] == pytest.approx(e64["re_max"], abs=1e-6)
    if g_true is not None:
        assert g_true <= e["g_used"]


@pytest.mark.parametrize("case", ["diph32", "robin32"])
def test_two_estimates_are_bitwise_equal(pj, case):
    """no atomics: two solvers of the same system, estimated in one process, give the same bits"""
    make, _, _ = _build(pj, case)
    a, b = make(), make()
    Ha, Hb = L.debug_specest_hessenberg(a._h, 0), L.debug_specest_hessenberg(b._h, 0)
    assert Ha.shape == Hb.shape == (sr.STEPS + 1, sr.STEPS)
    assert np.array_equal(Ha.view(np.uint64), Hb.view(np.uint64))
    assert a.spectral_estimate(0)["g_ritz"] == b.spectral_estimate(0)["g_ritz"]


# ------------------------------------------------------------------------------------ 2. new ground
@pytest.mark.parametrize("case", CASES)
def test_gershgorin_refuses_and_the_estimate_admits(pj, case):
    r = run(pj, case)
    for which in (0, 1):
        assert r["default"].system_info(which).neumann_ok == 0 and r["est"].system_info(which).neumann_ok == 0
        e = r["est"].spectral_estimate(which, run=False)           # (the solves have run it)
        assert e["steps"] == sr.STEPS and e["admitted"] == 1 and e["gershgorin_admits"] == 0 and e["gershgorin"] >= 0.95
        assert r["default"].spectral_estimate(which, run=False)["steps"] == 0      # the default run estimates nothing
    assert r["default_run"].poly_degree == 0 and r["default_run"].poly_xspace == 0
    print(f"{case}: degree {r['est_run'].poly_degree}, {r['est_run'].products} products in the step (default: {r['default_run'].products})")
    assert r["est_run"].poly_degree >= 2 and r["est_run"].poly_xspace == 1


# ------------------------------------------------------------------------------------ 3. parity
@pytest.mark.parametrize("case", CASES)
def test_parity_with_the_oracle_and_with_the_default_run(pj, case):
    """against the oracle's direct solves at the bar tests/test_gpu_parity.py holds the same systems to under default options
    (1e-9: diphasic and Robin / Neumann cut cells), and against the default-options run at 1e-10: both stop at reltol = 1e-12 in
    the units of x"""
    r = run(pj, case)
    assert len(r["est_states"]) == len(r["default_states"]) == len(r["oracle"]) == 5
    for k, (a, d, o) in enumerate(zip(r["est_states"], r["default_states"], r["oracle"])):
        print(f"{case} state {k}: vs oracle {rel_l2(a, o):.2e} (default {rel_l2(d, o):.2e}), vs default {rel_l2(a, d):.2e}")
        assert rel_l2(a, o) <= 1e-9
        assert rel_l2(a, d) <= 1e-10


# ------------------------------------------------------------------------------------ 4. a system Gershgorin admits
def test_on_a_system_gershgorin_admits_it_is_the_default_solve(pj):
    n = 32
    M = (n + 1) ** 2
    mesh = pj.Mesh((n, n), (4.0, 4.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0, complement=True), mesh)
    ph = pj.Phase(cap, pj.DiffusionOps(cap), ZERO, _const(1.0))
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS2})
    dt = 0.5 * (4.0 / n) ** 2
    got = {}
    for precond in (0, "poly-est"):
        s = pj.DiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(1.0), dt, np.zeros(2 * M), "BE")
        pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 6 * dt, bcb, pj.Dirichlet(1.0), "CN", reltol=1e-12, precond=precond, log=True)
        assert s.system_info(0).neumann_ok == 1 and s.system_info(1).neumann_ok == 1
        got[precond] = s
    a, b = got[0], got["poly-est"]
    assert [c["iters"] for c in a.ch] == [c["iters"] for c in b.ch]
    assert len(a.states) == len(b.states) == 7
    for x, y in zip(a.states, b.states):
        assert np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64))
    for which in (0, 1):
        assert b.spectral_estimate(which, run=False)["steps"] == 0          # no estimate ran as a side effect of the solves


# ------------------------------------------------------------------------------------ 5. not admitted
def test_a_steady_system_is_not_admitted_and_converges_plain(pj):
    n = 32
    mesh, omesh = pj.Mesh((n, n), (4.0, 4.0)), po.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0, complement=True), mesh)
    one = lambda x, y, z=0.0: 1.0
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS2})
    s = pj.DiffusionSteadyMono(pj.Phase(cap, pj.DiffusionOps(cap), one, one), bcb, pj.Robin(1.0, 1.0, 1.0))
    pj.solve_DiffusionSteadyMono_b(s, reltol=1e-13, precond="poly-est")
    assert s.ch[-1]["converged"]
    e = s.spectral_estimate(0, run=False)
    print(f"steady Robin 32^2: g_ritz {e['g_ritz']:.4f}, g_used {e['g_used']:.4f}")
    assert e["steps"] == sr.STEPS and e["admitted"] == 0 and e["g_used"] >= 0.95
    oc = oracle_capacity_from_product(cap, omesh)
    so = po.DiffusionSteadyMono(po.Phase(oc, po.make_diffusion_ops(oc), one, one),
                                po.BorderConditions({k: po.Dirichlet(0.0) for k in KEYS2}), po.Robin(1.0, 1.0, 1.0))
    po.solve_DiffusionSteadyMono(so, method="\\")
    assert rel_l2(s.x, so.x) <= 1e-9


# ------------------------------------------------------------------------------------ 6. refusals
def _mono24(pj):
    n = 24
    mesh = pj.Mesh((n, n), (4.0, 4.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0, complement=True), mesh)
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS2})
    return n, mesh, cap, bcb


def test_refused_on_a_moving_solver(pj):
    n = 16
    mesh = pj.Mesh((n, n), (4.0, 4.0))
    body = pj.MovingSphere(lambda t: (2.01, 2.01), lambda t: 0.8 + 0.5 * t, complement=True)
    dt = 0.5 * (4.0 / n) ** 2
    cap = pj.Capacity(body, pj.SpaceTimeMesh(mesh, [0.0, dt]))
    ph = pj.Phase(cap, pj.DiffusionOps(cap), ZERO, _const(1.0))
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS2})
    u0 = np.concatenate([np.zeros((n + 1) ** 2), np.ones((n + 1) ** 2)])
    s = pj.MovingDiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(1.0), dt, u0, mesh, "BE")
    with pytest.raises(pj.PenguinHipError, match="moving-body"):
        pj.solve_MovingDiffusionUnsteadyMono_b(s, ph, body, dt, 0.0, 2 * dt, bcb, pj.Dirichlet(1.0), mesh, "BE", method="bicgstab",
                                               precond="poly-est")


def test_refused_on_a_convection_system(pj):
    from tests.test_gpu_parity import _velocity_fields

    n, mesh, cap, bcb = _mono24(pj)
    M = (n + 1) ** 2
    u, ug = _velocity_fields(cap, 2, M)
    ph = pj.Phase(cap, pj.ConvectionOps(cap, u, ug), ZERO, _const(1.0))
    dt = 0.25 * (4.0 / n) ** 2
    s = pj.AdvectionDiffusionUnsteadyMono(ph, bcb, pj.Robin(1.0, 0.5, 1.0), dt, np.zeros(2 * M), "BE")
    with pytest.raises(pj.PenguinHipError, match="ConvectionOps"):
        pj.solve_AdvectionDiffusionUnsteadyMono_b(s, ph, dt, 2 * dt, bcb, pj.Robin(1.0, 0.5, 1.0), "BE", precond="poly-est")


@pytest.mark.parametrize("method,word", [("cg", "CG"), ("gmres", "GMRES")])
def test_refused_with_cg_and_gmres(pj, method, word):
    n, mesh, cap, bcb = _mono24(pj)
    M = (n + 1) ** 2
    ph = pj.Phase(cap, pj.DiffusionOps(cap), ZERO, _const(1.0))
    dt = 0.5 * (4.0 / n) ** 2
    s = pj.DiffusionUnsteadyMono(ph, bcb, pj.Robin(1.0, 1.0, 1.0), dt, np.zeros(2 * M), "BE")
    with pytest.raises(pj.PenguinHipError, match=word):
        pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 2 * dt, bcb, pj.Robin(1.0, 1.0, 1.0), "BE", method=method, precond="poly-est")
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 2 * dt, bcb, pj.Robin(1.0, 1.0, 1.0), "BE", precond="poly-est")   # the same solver serves BiCGStab
    assert np.isfinite(s.x).all() and s.spectral_estimate(0, run=False)["admitted"] == 1


def test_refused_on_a_virtual_rank_run_and_multigrid_is_undisturbed(pj):
    """2 virtual ranks: refused by the entry point with the one-rank condition, before a rank starts; the same configuration then
    runs with precond = 0.  A "mg-cell" solve on the same process gives the same bits before and after all of this file's
    "poly-est" solves and refusals."""
    n, mesh, cap, bcb = _mono24(pj)
    one = lambda x, y, z=0.0: 1.0

    def mg_solve():
        s = pj.DiffusionSteadyMono(pj.Phase(cap, pj.DiffusionOps(cap), one, one), bcb, pj.Robin(1.0, 1.0, 0.5))
        pj.solve_DiffusionSteadyMono_b(s, reltol=1e-12, precond="mg-cell")
        assert s.ch[-1]["converged"]
        return np.array(s.x)

    before = mg_solve()
    lib = L.lib()
    nn, LL = np.array([16, 16], dtype=np.int64), np.array([4.0, 4.0])
    params = np.array([2.01, 2.01, 1.0])
    keys = np.array([L.PG_KEY[k] for k in KEYS2], dtype=np.int32)
    x = np.zeros(2 * 17 * 17)
    outs = [np.zeros(2, dtype=np.int64) for _ in range(4)]

    def vrun():
        return lib.pg_debug_run_virtual_ranks(2, 2, L.iptr(nn), L.dptr(LL), L.PG_BODY_BALL, L.dptr(params), len(params), C.c_double(1.0),
                                              C.c_double(1.0), len(keys), keys.ctypes.data_as(L.c_i32_p), C.c_double(0.04), 0, 0,
                                              C.c_int64(2), L.dptr(x), *(L.iptr(o) for o in outs))

    try:
        L.check(lib.pg_debug_set_virtual_rank_precond(L.PG_PRECOND_POLY_EST))
        with pytest.raises(pj.PenguinHipError, match="one rank"):
            L.check(vrun())
    finally:
        L.check(lib.pg_debug_set_virtual_rank_precond(0))
    L.check(vrun())
    assert outs[0].sum() > 0 and np.isfinite(x).all() and x.any()
    # a "poly-est" run in between
    make, solve, _ = _build(pj, "robin32")
    solve(make(), 2, reltol=1e-12, precond="poly-est")
    after = mg_solve()
    assert np.array_equal(before.view(np.uint64), after.view(np.uint64))


# ------------------------------------------------------------------------------------ 7. the extrapolated start stays on
def test_the_extrapolated_start_stays_on_with_the_option(pj):
    """The plain warm path's start (k_rhs_init<KH>) is the start of these solves whatever iterates afterwards: after enough
    steps on the diphasic 64^2 system with the option, older states are kept -- where the policy of the default run keeps them."""
    cfg = dict(kv.split("=", 1) for kv in pj.config_string().split() if "=" in kv)
    make, solve, _ = _build(pj, "diph64")
    kept = {}
    for precond in (0, "poly-est"):
        s = make()
        solve(s, 24, reltol=1e-12, precond=precond, save_states=False)
        last = _one_more_step(s, L.PG_PRECOND_POLY_EST if precond == "poly-est" else 0)
        kept[precond] = s.guess_info()["kept"]
        assert (last.poly_degree >= 2) == (precond == "poly-est")
        print(f"precond = {precond!r}: {kept[precond]} older states kept after 25 steps, {last.products} products in the last step, "
              f"{s.system_info(1).spmv_bytes} bytes per product")
    if int(cfg["guess_states"]) > 0 and int(cfg["poly"]) != 0:
        assert kept["poly-est"] > 0
