"""`method = idrs, nshadow = ...` on the device (pg_idrs.hip): IDR(s) against the oracle's direct solves (TOL_T), against its numpy
restatement tests/idrs_reference.py on the SAME preconditioned system (the state after one, two and three cycles), its product
counts at cell Peclet number 12.5 against BiCGStab's, its counting rules, its breakdown paths, its start from a previous state,
its refusals and its reproducibility."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from oracle import penguin_oracle as po
from penguin.jl_amd import _lib as L
from tests.common import oracle_capacity_from_product, rel_l2
from tests.idrs_reference import idrs_ref
from tests.test_gpu_bicgstabl import _first_solve, _heat_pair, _peclet_solver, _poisson_pair, _shared
from tests.test_gpu_parity import HEAT_BORDERS, TOL_T, _mono_pair, _velocity_fields

pytestmark = pytest.mark.gpu

SHADOWS = (2, 4, 8)
RELTOL = 1e-13
IDRS = 4     # PG_METHOD_IDRS


def _opts(method, s=0, reltol=RELTOL, maxiter=0, precond=0, warm=0):
    return L.pg_krylov_opts(method, reltol, 0.0, maxiter, 4, warm, s, precond)


def _scaled_system(s):
    """The system the device iterates on, Â = B⁻¹SAS and b̂, the row scaling S and the active index set."""
    Ah, bh, _ = s.system(2)
    _, _, idx = s.system(0)
    return Ah[:, : Ah.shape[0]].tocsr(), bh, s.row_scaling(0), idx


def _true_relres(s, x):
    """||b̂ - Â z||_W / ||b̂||_W of a fetched state x = S z, recomputed on the host."""
    Ah, bh, S, idx = _scaled_system(s)
    return np.linalg.norm(S * (bh - Ah @ (x[idx] / S))) / np.linalg.norm(S * bh)


# The rounding of one host evaluation of the residual, relative to the tolerance it is compared with: eps * (entries per row)
# * |Â||z| / |b̂| ~ 1e-15 against reltol >= 1e-13 -- a recomputed residual may exceed the device's by a few per cent, no more.
RECOMPUTED = 1.05


# ------------------------------------------------------------------------------------ parity with the oracle's direct solves
@pytest.mark.parametrize("ns", SHADOWS)
@pytest.mark.parametrize("scheme", ["BE", "CN"])
def test_heat_matches_direct_solves(pj, scheme, ns):
    ((s, ph, bcb, bci), (so, oph, obcb, obci)), dt = _heat_pair(pj)

    def direct():
        po.solve_DiffusionUnsteadyMono(so, oph, dt, 5 * dt, obcb, obci, scheme, method="\\")
        return [a.copy() for a in so.states]
    ref = _shared(("heat", scheme), direct)
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 5 * dt, bcb, bci, scheme, method="idrs", nshadow=ns, reltol=RELTOL, log=True)
    assert len(s.states) == len(ref)
    for a, b in zip(s.states, ref):
        assert rel_l2(a, b) <= TOL_T
    assert all(c["isconverged"] for c in s.ch) and s.unconverged == 0


@pytest.mark.parametrize("ns", SHADOWS)
def test_robin_3d_matches_direct_solves(pj, ns):
    n = 12
    M = (n + 1) ** 3
    u0 = np.concatenate([np.random.default_rng(11).uniform(0.0, 1.0, M), np.random.default_rng(12).uniform(0.0, 1.0, M)])
    dt = 0.5 * (4.0 / n) ** 2
    keys = ("left", "right", "top", "bottom", "forward", "backward")
    (s, ph, bcb, bci), (so, oph, obcb, obci) = _mono_pair(
        pj, 3, n, 4.0, (2.03, 1.98, 2.01), 1.1, pj.Robin(1.0, 0.5, 0.3), po.Robin(1.0, 0.5, 0.3),
        {k: pj.Dirichlet(0.2) for k in keys}, {k: po.Dirichlet(0.2) for k in keys}, dt, u0, "BE")

    def direct():
        po.solve_DiffusionUnsteadyMono(so, oph, dt, 3 * dt, obcb, obci, "CN", method="\\")
        return so.x.copy()
    ref = _shared("robin3d", direct)
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 3 * dt, bcb, bci, "CN", method="idrs", nshadow=ns, reltol=RELTOL)
    assert s.unconverged == 0 and rel_l2(s.x, ref) <= TOL_T


@pytest.mark.parametrize("ns", SHADOWS)
def test_diphasic_matches_direct_solves(pj, ns):
    n, Lx, c, r = 24, 8.0, (4.0, 4.0), 2.0
    M = (n + 1) ** 2
    mesh, omesh = pj.Mesh((n, n), (Lx, Lx), (0.0, 0.0)), po.Mesh((n, n), (Lx, Lx), (0.0, 0.0))
    cap1, cap2 = pj.Capacity(pj.Sphere(c, r), mesh), pj.Capacity(pj.Sphere(c, r, complement=True), mesh)
    f = lambda x, y, z, t: 0.0
    D1, D2 = (lambda x, y, z: 1.0), (lambda x, y, z: 2.0)
    p1, p2 = pj.Phase(cap1, pj.DiffusionOps(cap1), f, D1), pj.Phase(cap2, pj.DiffusionOps(cap2), f, D2)
    ic = pj.InterfaceConditions(pj.ScalarJump(1.0, 0.5, 0.0), pj.FluxJump(1.0, 1.0, 0.0))
    bcb = pj.BorderConditions({})
    u0 = np.concatenate([np.ones(M), np.ones(M), np.zeros(M), np.zeros(M)])
    dt = 0.5 * (Lx / n) ** 2
    s = pj.DiffusionUnsteadyDiph(p1, p2, bcb, ic, dt, u0, "BE")

    def direct():
        oc1, oc2 = oracle_capacity_from_product(cap1, omesh), oracle_capacity_from_product(cap2, omesh)
        q1, q2 = po.Phase(oc1, po.make_diffusion_ops(oc1), f, D1), po.Phase(oc2, po.make_diffusion_ops(oc2), f, D2)
        oic = po.InterfaceConditions(po.ScalarJump(1.0, 0.5, 0.0), po.FluxJump(1.0, 1.0, 0.0))
        so = po.DiffusionUnsteadyDiph(q1, q2, po.BorderConditions({}), oic, dt, u0, "BE")
        po.solve_DiffusionUnsteadyDiph(so, q1, q2, dt, 5 * dt, po.BorderConditions({}), oic, "CN", method="\\")
        return so.x.copy()
    ref = _shared("diph", direct)
    pj.solve_DiffusionUnsteadyDiph_b(s, p1, p2, dt, 5 * dt, bcb, ic, "CN", method="idrs", nshadow=ns, reltol=RELTOL)
    assert s.unconverged == 0 and rel_l2(s.x, ref) <= TOL_T


@pytest.mark.parametrize("ns", SHADOWS)
def test_steady_poisson_matches_direct_solve(pj, ns):
    s, so = _poisson_pair(pj)

    def direct():
        po.solve_DiffusionSteadyMono(so, method="\\")
        return so.x.copy()
    ref = _shared("poisson", direct)
    pj.solve_DiffusionSteadyMono_b(s, method="idrs", nshadow=ns, reltol=RELTOL)
    assert s.ch[-1]["converged"] and s.unconverged == 0 and rel_l2(s.x, ref) <= TOL_T


@pytest.mark.parametrize("ns", SHADOWS)
def test_advection_diffusion_matches_direct_solves(pj, ns):
    """The velocity fields of test_advection_diffusion_mono_matches_oracle: steady, and unsteady (BE first solve, CN steps)."""
    n, N = 24, 2
    M = (n + 1) ** 2
    mesh, omesh = pj.Mesh((n, n), (4.0, 4.0)), po.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0), mesh)
    u, ug = _velocity_fields(cap, N, M)
    op = pj.ConvectionOps(cap, u, ug)
    f, D = (lambda x, y, z=0.0: 1.0 + 0.2 * x), (lambda x, y, z=0.0: 0.5 + 0.1 * y)
    ft = lambda x, y, z, t: 1.0 + 0.2 * x
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in HEAT_BORDERS})
    dt = 0.25 * (4.0 / n) ** 2
    u0 = np.concatenate([np.zeros(M), np.ones(M)])

    def direct():
        ocap = oracle_capacity_from_product(cap, omesh)
        oop = po.make_convection_ops(ocap, u, ug)
        obcb = po.BorderConditions({k: po.Dirichlet(0.0) for k in HEAT_BORDERS})
        so = po.AdvectionDiffusionSteadyMono(po.Phase(ocap, oop, f, D), obcb, po.Dirichlet(1.0))
        po.solve_system(so, method="\\")
        opht = po.Phase(ocap, oop, ft, D)
        suo = po.AdvectionDiffusionUnsteadyMono(opht, obcb, po.Robin(1.0, 0.5, 1.0), dt, u0, "BE")
        po.solve_AdvectionDiffusionUnsteadyMono(suo, opht, dt, 5 * dt, obcb, po.Robin(1.0, 0.5, 1.0), "CN", method="\\")
        return so.x.copy(), [a.copy() for a in suo.states]
    x_steady, states = _shared("advdiff", direct)
    s = pj.AdvectionDiffusionSteadyMono(pj.Phase(cap, op, f, D), bcb, pj.Dirichlet(1.0))
    pj.solve_AdvectionDiffusionSteadyMono_b(s, method="idrs", nshadow=ns, reltol=RELTOL)
    assert s.ch[-1]["converged"] and s.unconverged == 0 and rel_l2(s.x, x_steady) <= TOL_T
    pht = pj.Phase(cap, op, ft, D)
    su = pj.AdvectionDiffusionUnsteadyMono(pht, bcb, pj.Robin(1.0, 0.5, 1.0), dt, u0, "BE")
    pj.solve_AdvectionDiffusionUnsteadyMono_b(su, pht, dt, 5 * dt, bcb, pj.Robin(1.0, 0.5, 1.0), "CN", method="idrs", nshadow=ns,
                                              reltol=RELTOL)
    assert su.unconverged == 0 and len(su.states) == len(states)
    for a, b in zip(su.states, states):
        assert rel_l2(a, b) <= TOL_T


def test_stream_vorticity_step_with_idrs_for_both_solves(pj):
    """One step on the disc case (shape B) of the stage tests of tests/test_gpu_streamvorticity.py, held to their bars."""
    from tests.test_gpu_streamvorticity import RELTOL as SV_RELTOL, TOL, _build, _check_system as sv_check_system
    s, so, _ = _build(pj, "B")
    M = s._M
    t, w_n = s.time, s.ω.copy()
    pj.step_StreamVorticity_b(s, "BE", method="idrs", nshadow=4, reltol=SV_RELTOL)
    psi, (u, v), w_np1 = s.ψ, s.velocity, s.ω
    e_psi = rel_l2(psi, so.poisson(w_n, t))
    g = po.grad(so.op, psi)
    ou, ov = g[M:], -g[:M]
    assert np.allclose(u, ou, rtol=1e-12, atol=1e-12 * np.abs(ou).max())
    assert np.allclose(v, ov, rtol=1e-12, atol=1e-12 * np.abs(ov).max())
    osys = so.omega_system(u, v, w_n, t, "BE")
    sv_check_system(s.omega_solver, osys)
    po.solve_system(osys, method="\\")
    e_w = rel_l2(w_np1, osys.x)
    print(f"psi {e_psi:.2e} omega {e_w:.2e}")
    assert s.unconverged == 0 and e_psi <= TOL and e_w <= TOL


# ------------------------------------------------------------------------------------ the algebra, insensitive to chaos
@pytest.mark.parametrize("ns", (1, 2, 4, 8))
@pytest.mark.parametrize("case", ["heat", "poisson"])
def test_state_after_one_two_three_cycles_is_the_restatements(pj, case, ns):
    """maxiter = s + 1, 2 (s + 1), 3 (s + 1): one, two and three cycles from zero on the device's own system.  The yardstick is what
    the order of summation is worth: the relative L2 difference between the float64 restatement and the same restatement with
    longdouble sums.  The device may differ from the float64 restatement by 10 x that (the margin the multigrid tests give a
    different order of summation), floor 64 * 2^-53.  Total product counts are NOT compared: they move by up to 27 % under a
    one-ulp perturbation of b (tests/golden/idrs_products.json)."""
    for cycles in (1, 2, 3):
        s = _heat_pair(pj)[0][0][0] if case == "heat" else _poisson_pair(pj)[0]
        cap = cycles * (ns + 1)
        Ah, bh, S, idx = _scaled_system(s)
        z64, i64_ = idrs_ref(Ah, bh, s=ns, reltol=RELTOL, weights=S, maxiter=cap)
        zld, _ = idrs_ref(Ah, bh, s=ns, reltol=RELTOL, weights=S, maxiter=cap, long_sums=True)
        run, x = _first_solve(s, _opts(IDRS, ns, maxiter=cap))
        yard = rel_l2(z64, zld)
        diff = rel_l2(x[idx] / S, z64)
        bound = max(10.0 * yard, 64.0 * 2.0 ** -53)
        print(f"{case} s={ns} cycles={cycles}: yardstick {yard:.2e} device {diff:.2e} bound {bound:.2e} iters {run.total_iters}/{i64_['iters']}")
        if i64_["converged"]:
            # (heat with s = 8 meets the tolerance inside its third cycle: both end there, and the states are still compared)
            assert i64_["iters"] <= cap and run.unconverged_steps == 0
        else:
            assert run.total_iters == i64_["iters"] == cap and run.unconverged_steps == 1
        assert diff <= bound, (case, ns, cycles, diff, yard)


# ------------------------------------------------------------------------------------ cell Peclet number 12.5
@pytest.mark.parametrize("kind", ["uniform", "rotation"])
def test_peclet_12_needs_fewer_products_than_bicgstab(pj, kind):
    """32^2, uniform flow (100, 30) and rigid rotation of amplitude 100: IDR(4) and IDR(8) converge with the true residual meeting
    the test and need fewer products than plain BiCGStab (precond = -1) on the same system (the restatement: 200 / 200 against
    474, 240 / 196 against 8306)."""
    s = _peclet_solver(pj, 32, kind)
    A, b, idx = s.system(0)
    direct = spla.spsolve(A[:, : len(idx)].tocsc(), b)
    plain, x_plain = _first_solve(s, _opts(L.PG_METHOD["bicgstab"], reltol=1e-12, precond=-1))
    print(kind, "BiCGStab products", plain.products, "unconverged", plain.unconverged_steps)
    for ns in (4, 8):
        si = _peclet_solver(pj, 32, kind)
        run, x = _first_solve(si, _opts(IDRS, ns, reltol=1e-12))
        true = _true_relres(si, x)
        print(kind, f"IDR({ns}) products", run.products, "iters", run.total_iters, "reported", run.worst_relres, "true", true,
              "error", rel_l2(x[idx], direct))
        assert run.unconverged_steps == 0
        assert run.worst_relres <= 1e-12 and true <= RECOMPUTED * 1e-12
        assert run.products < plain.products
        assert rel_l2(x[idx], direct) <= 1e-9


# ------------------------------------------------------------------------------------ fails without the feature
def test_method_4_through_the_abi(pj):
    s = _heat_pair(pj, 16)[0][0][0]
    run, x = _first_solve(s, _opts(IDRS, 2))
    assert run.unconverged_steps == 0 and run.total_iters > 0 and np.all(np.isfinite(x)) and np.abs(x).max() > 0


def test_restart_0_runs_s_8_and_9_is_refused(pj):
    run0, x0 = _first_solve(_heat_pair(pj, 16)[0][0][0], _opts(IDRS, 0))
    run8, x8 = _first_solve(_heat_pair(pj, 16)[0][0][0], _opts(IDRS, 8))
    assert run0.unconverged_steps == 0 and run0.total_iters == run8.total_iters and np.array_equal(x0, x8)
    with pytest.raises(Exception, match="more than 8"):
        _first_solve(_heat_pair(pj, 16)[0][0][0], _opts(IDRS, 9))


@pytest.mark.parametrize("ns", (1, 2, 4, 8))
def test_products_are_iters_plus_restarts_plus_confirmations(pj, ns):
    """A zero start on a well-conditioned system: no restart, one confirmation -- products = iters + 1, the restatement's count
    of confirmations.  (The + 1 of a start from a previous state: test_second_steady_solve_needs_one_product.)"""
    s = _heat_pair(pj)[0][0][0]
    Ah, bh, S, _ = _scaled_system(s)
    _, info = idrs_ref(Ah, bh, s=ns, reltol=RELTOL, weights=S)
    run, _ = _first_solve(s, _opts(IDRS, ns))
    extra = run.products - run.total_iters
    print(ns, "device", run.total_iters, run.products, "restatement", info["iters"], info["products"])
    assert run.unconverged_steps == 0 and 1 <= extra <= 4
    assert extra == info["confirmations"] + info["restarts"]


@pytest.mark.parametrize("ns,cap", [(2, 1), (2, 4), (4, 7), (8, 13)])
def test_maxiter_caps_iters_exactly(pj, ns, cap):
    """In the middle of a cycle and at its ω step alike: no update of x starts at iters >= maxiter; no confirmation is spent."""
    s = _heat_pair(pj)[0][0][0]
    run, x = _first_solve(s, _opts(IDRS, ns, maxiter=cap))
    assert run.total_iters == cap and run.products == cap and run.unconverged_steps == 1
    assert np.all(np.isfinite(x)) and np.abs(x).max() > 0


@pytest.mark.parametrize("ns", [2, 8])
def test_bitwise_reproducible(pj, ns):
    out = []
    for _ in range(2):
        run, x = _first_solve(_peclet_solver(pj), _opts(IDRS, ns, reltol=1e-12))
        out.append((int(run.total_iters), int(run.products), x))
    assert out[0][0] == out[1][0] > 0 and out[0][1] == out[1][1]
    assert np.array_equal(out[0][2], out[1][2])


# ------------------------------------------------------------------------------------ breakdown paths, nothing provoked
def test_more_shadow_vectors_than_the_system_likes(pj):
    """Poisson 8^2 (a few dozen unknowns) with s = 8: the Sonneveld spaces shrink to nothing within a few cycles."""
    s, so = _poisson_pair(pj, 8)
    po.solve_DiffusionSteadyMono(so, method="\\")
    run, x = _first_solve(s, _opts(IDRS, 8))
    _, _, idx = s.system(0)
    print("unknowns", len(idx), "iters", run.total_iters, "products", run.products)
    assert run.unconverged_steps == 0 and np.all(np.isfinite(x))
    assert rel_l2(s._fetch_state(), so.x) <= TOL_T


def test_idr1_returns_a_finite_state_and_an_honest_flag(pj):
    """IDR(1) on the uniform-flow system at cell Peclet number 12.5 stagnates in the restatement (restarts, then gives up).
    Whatever the device meets: the state is finite and `converged` agrees with the residual recomputed on the host."""
    s = _peclet_solver(pj, 32, "uniform")
    run, x = _first_solve(s, _opts(IDRS, 1, reltol=1e-12, maxiter=3000))
    true = _true_relres(s, x)
    print("converged", run.unconverged_steps == 0, "iters", run.total_iters, "products", run.products, "reported", run.worst_relres,
          "true", true)
    assert np.all(np.isfinite(x))
    if run.unconverged_steps == 0:
        assert true <= RECOMPUTED * 1e-12
    else:
        assert true > 1e-12


def test_a_wrong_state_never_passes_as_converged(pj):
    """64^2 rigid rotation of amplitude 100, the near-singular system on which recurrence residuals drift from true ones
    (tests/test_bicgstabl_reference.py).  Whatever the device's iteration meets on its own (equilibrated) system: a solve
    reported converged has the true residual it reports and the direct solve's state."""
    s = _peclet_solver(pj, 64, "rotation")
    A, b, idx = s.system(0)
    direct = spla.spsolve(A[:, : len(idx)].tocsc(), b)
    run, x = _first_solve(s, _opts(IDRS, 4, maxiter=4000))
    assert np.all(np.isfinite(x))
    true = _true_relres(s, x)
    print("converged", run.unconverged_steps == 0, "iters", run.total_iters, "reported", run.worst_relres, "true", true,
          "error", rel_l2(x[idx], direct))
    if run.unconverged_steps == 0:
        assert run.worst_relres <= RELTOL and true <= 1.5 * RELTOL
        assert rel_l2(x[idx], direct) <= TOL_T


# ------------------------------------------------------------------------------------ warm start
def _run_steps(s, opts, scheme, steps):
    run = L.pg_run_info()
    L.check(L.lib().pg_solver_run(s._h, C.c_double(1e30), C.c_int32(L.PG_SCHEME[scheme]), C.byref(opts), C.c_int32(0),
                                  C.c_int64(steps), C.c_int32(0), C.byref(run)))
    return run, s._fetch_state().copy()


def test_time_steps_start_from_the_previous_state(pj):
    """Heat 24^2, BE first solve and 8 CN steps: with warm_start the steps start from the previous state -- the same states as from
    zero and as the oracle's direct solves, in fewer products over steps 3 .. 8."""
    out = {}
    for warm in (0, 1):
        ((s, ph, bcb, bci), (so, oph, obcb, obci)), dt = _heat_pair(pj)
        opts = _opts(IDRS, 4, warm=warm)
        first, _ = _first_solve(s, opts)
        r2, x2 = _run_steps(s, opts, "CN", 2)
        r8, x8 = _run_steps(s, opts, "CN", 6)
        assert first.unconverged_steps == 0 and r2.unconverged_steps == 0 and r8.unconverged_steps == 0
        assert r2.steps == 2 and r8.steps == 6
        out[warm] = (int(r8.products), x2, x8)

    def direct():
        po.solve_DiffusionUnsteadyMono(so, oph, dt, 8 * dt, obcb, obci, "CN", method="\\")
        return [a.copy() for a in so.states]
    ref = _shared(("heat8", "CN"), direct)
    assert len(ref) >= 9
    print("products over steps 3 .. 8: cold", out[0][0], "warm", out[1][0])
    for warm in (0, 1):
        assert rel_l2(out[warm][1], ref[2]) <= TOL_T and rel_l2(out[warm][2], ref[8]) <= TOL_T
    assert rel_l2(out[1][2], out[0][2]) <= TOL_T
    assert out[1][0] < out[0][0]


def test_second_steady_solve_needs_one_product(pj):
    """The stream-function system of a StreamVorticity (Poisson 24^2, shape B) solved twice with unchanged data: the second solve
    starts from the first one's solution, finds its true residual below the tolerance and ends without an update of x --
    products = 0 iters + 0 restarts + 0 confirmations + 1 (the product with the start), within the two the start may cost."""
    from tests.test_gpu_streamvorticity import _build
    s, so, _ = _build(pj, "B")
    psi1 = pj.solve_StreamVorticity_b(s, method="idrs", nshadow=4, reltol=1e-12).copy()
    info = L.pg_step_info()
    opts = _opts(IDRS, 4, reltol=1e-12, warm=1)
    L.check(L.lib().pg_streamvort_solve_stream(s._h, C.byref(opts), C.byref(info)))
    s._touch()
    assert info.converged == 1 and info.iters == 0
    assert info.resnorm <= 1e-12 * info.bnorm
    assert rel_l2(s.ψ, psi1) == 0.0 and rel_l2(psi1, so.poisson(s.ω, s.time)) <= TOL_T
    # from zero the same solve takes its products again
    cold = _opts(IDRS, 4, reltol=1e-12, warm=0)
    L.check(L.lib().pg_streamvort_solve_stream(s._h, C.byref(cold), C.byref(info)))
    assert info.converged == 1 and info.iters > 4


# ------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_condition(pj):
    ((s, ph, bcb, bci), _), dt = _heat_pair(pj, 16)
    with pytest.raises(Exception, match="more than 8"):
        pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, dt, bcb, bci, "BE", method="idrs", nshadow=9)
    for precond in (8, "poly-est", "mg-step"):
        with pytest.raises(Exception, match=r"refused: .*IDR\(s\)"):
            pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, dt, bcb, bci, "BE", method="idrs", nshadow=2, precond=precond)
    # an unsteady solver that refused keeps working afterwards with defaults
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 2 * dt, bcb, bci, "BE", reltol=RELTOL)
    assert s.unconverged == 0 and np.all(np.isfinite(s.x)) and np.abs(s.x).max() > 0
    for precond in ("mg", "mg-cell"):
        sp, _ = _poisson_pair(pj, 16)
        with pytest.raises(Exception, match=r"refused: .*IDR\(s\)"):
            pj.solve_DiffusionSteadyMono_b(sp, method="idrs", nshadow=2, precond=precond)
    with pytest.raises(Exception, match=r"IDR\(s\) refused: .*one rank"):
        L.check(L.lib().pg_debug_set_virtual_rank_method(C.c_int32(IDRS), C.c_int32(2)))


def test_nshadow_selects_the_method_and_the_bare_name_stays_bicgstab(pj):
    runs = {}
    for key, kw in (("bare", dict(method="idrs")), ("s4", dict(method="idrs", nshadow=4)), ("bicgstab", dict(method="bicgstab"))):
        s = _peclet_solver(pj)
        pj.solve_AdvectionDiffusionSteadyMono_b(s, reltol=1e-12, **kw)
        runs[key] = (s.ch[-1]["iters"], s.x.copy())
    assert runs["bare"][0] == runs["bicgstab"][0] and np.array_equal(runs["bare"][1], runs["bicgstab"][1])   # bit-identical
    assert runs["s4"][0] != runs["bare"][0]

    def idrs():   # stands in for IterativeSolvers.idrs: only the name crosses the boundary
        raise AssertionError
    s = _peclet_solver(pj)
    pj.solve_AdvectionDiffusionSteadyMono_b(s, method=idrs, nshadow=4, reltol=1e-12)
    assert s.ch[-1]["iters"] == runs["s4"][0] and np.array_equal(s.x, runs["s4"][1])
