"""`method = bicgstabl, l = ...` on the device (pg_bicgstabl.hip): BiCGStab(l) against the oracle's direct solves (TOL_T), against
its numpy restatement tests/bicgstabl_reference.py on the SAME preconditioned system (iteration counts), its counting, its
refusals, its reproducibility and the confirmation of the true residual."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from oracle import penguin_oracle as po
from penguin.jl_amd import _lib as L
from tests.bicgstabl_reference import bicgstabl_ref
from tests.common import oracle_capacity_from_product, rel_l2
from tests.test_gpu_parity import HEAT_BORDERS, TOL_T, _mono_pair, _velocity_fields

pytestmark = pytest.mark.gpu

ELLS = (1, 2, 4)
RELTOL = 1e-13
_oracle = {}     # direct solves of the oracle, computed once and shared between the cases of a parametrised test (read only)


def _shared(key, make):
    if key not in _oracle:
        _oracle[key] = make()
    return _oracle[key]


def _heat_pair(pj, n=24, scheme0="BE"):
    M = (n + 1) ** 2
    u0 = np.concatenate([np.zeros(M), np.ones(M)])
    dt = 0.25 * (4.0 / n) ** 2
    return _mono_pair(pj, 2, n, 4.0, (2.01, 2.01), 1.0, pj.Dirichlet(1.0), po.Dirichlet(1.0),
                      {k: pj.Dirichlet(0.0) for k in HEAT_BORDERS}, {k: po.Dirichlet(0.0) for k in HEAT_BORDERS}, dt, u0, scheme0), dt


def _poisson_pair(pj, n=24):
    mesh, omesh = pj.Mesh((n, n), (4.0, 4.0), (0.0, 0.0)), po.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((2.0, 2.0), 1.0), mesh)
    ocap = oracle_capacity_from_product(cap, omesh)
    f = lambda x, y, z, t=0.0: 4.0
    D = lambda x, y, z: 1.0
    ph, oph = pj.Phase(cap, pj.DiffusionOps(cap), f, D), po.Phase(ocap, po.make_diffusion_ops(ocap), f, D)
    return (pj.DiffusionSteadyMono(ph, pj.BorderConditions({}), pj.Dirichlet(0.0)),
            po.DiffusionSteadyMono(oph, po.BorderConditions({}), po.Dirichlet(0.0)))


def _peclet_solver(pj, n=32, kind="uniform"):
    """Steady advection-diffusion inside the disc r = 1 at (2.01, 2.01): uniform flow (100, 30) or rigid rotation of amplitude
    100 -- cell Peclet number 12.5 at 32^2."""
    M = (n + 1) ** 2
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0), pj.Mesh((n, n), (4.0, 4.0)))
    x, y = cap.C_ω[:, 0], cap.C_ω[:, 1]
    u = [np.full(M, 100.0), np.full(M, 30.0)] if kind == "uniform" else [-100.0 * (y - 2.01), 100.0 * (x - 2.01)]
    op = pj.ConvectionOps(cap, [np.ascontiguousarray(a) for a in u], np.zeros(2 * M))
    one = lambda x, y, z=0.0: 1.0
    return pj.AdvectionDiffusionSteadyMono(pj.Phase(cap, op, one, one),
                                           pj.BorderConditions({k: pj.Dirichlet(0.0) for k in HEAT_BORDERS}), pj.Dirichlet(1.0))


def _first_solve(s, opts):
    """The constructor system's solve through the C ABI -> (pg_run_info, state)."""
    run = L.pg_run_info()
    L.check(L.lib().pg_solver_run(s._h, C.c_double(0.0), C.c_int32(L.PG_SCHEME["BE"]), C.byref(opts), C.c_int32(1), C.c_int64(0),
                                  C.c_int32(0), C.byref(run)))
    return run, s._fetch_state().copy()


def _opts(method, l=0, reltol=RELTOL, maxiter=0, precond=0):
    return L.pg_krylov_opts(method, reltol, 0.0, maxiter, 4, 0, l, precond)


def _restatement(s, l, **kw):
    Ah, bh, _ = s.system(2)
    Ah = Ah[:, : Ah.shape[0]].tocsr()
    return bicgstabl_ref(Ah, bh, l=l, reltol=kw.pop("reltol", RELTOL), weights=s.row_scaling(0), **kw)


# ------------------------------------------------------------------------------------ parity with the oracle's direct solves
@pytest.mark.parametrize("l", ELLS)
@pytest.mark.parametrize("scheme", ["BE", "CN"])
def test_heat_matches_direct_solves(pj, scheme, l):
    ((s, ph, bcb, bci), (so, oph, obcb, obci)), dt = _heat_pair(pj)

    def direct():
        po.solve_DiffusionUnsteadyMono(so, oph, dt, 5 * dt, obcb, obci, scheme, method="\\")
        return [a.copy() for a in so.states]
    ref = _shared(("heat", scheme), direct)
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 5 * dt, bcb, bci, scheme, method="bicgstabl", l=l, reltol=RELTOL, log=True)
    assert len(s.states) == len(ref)
    for a, b in zip(s.states, ref):
        assert rel_l2(a, b) <= TOL_T
    assert all(c["isconverged"] for c in s.ch) and s.unconverged == 0


@pytest.mark.parametrize("l", ELLS)
def test_robin_3d_matches_direct_solves(pj, l):
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
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 3 * dt, bcb, bci, "CN", method="bicgstabl", l=l, reltol=RELTOL)
    assert s.unconverged == 0 and rel_l2(s.x, ref) <= TOL_T


@pytest.mark.parametrize("l", ELLS)
def test_diphasic_matches_direct_solves(pj, l):
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
    pj.solve_DiffusionUnsteadyDiph_b(s, p1, p2, dt, 5 * dt, bcb, ic, "CN", method="bicgstabl", l=l, reltol=RELTOL)
    assert s.unconverged == 0 and rel_l2(s.x, ref) <= TOL_T


@pytest.mark.parametrize("l", ELLS)
def test_steady_poisson_matches_direct_solve(pj, l):
    s, so = _poisson_pair(pj)

    def direct():
        po.solve_DiffusionSteadyMono(so, method="\\")
        return so.x.copy()
    ref = _shared("poisson", direct)
    pj.solve_DiffusionSteadyMono_b(s, method="bicgstabl", l=l, reltol=RELTOL)
    assert s.ch[-1]["converged"] and rel_l2(s.x, ref) <= TOL_T


@pytest.mark.parametrize("l", ELLS)
def test_advection_diffusion_matches_direct_solves(pj, l):
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
    pj.solve_AdvectionDiffusionSteadyMono_b(s, method="bicgstabl", l=l, reltol=RELTOL)
    assert s.ch[-1]["converged"] and rel_l2(s.x, x_steady) <= TOL_T
    pht = pj.Phase(cap, op, ft, D)
    su = pj.AdvectionDiffusionUnsteadyMono(pht, bcb, pj.Robin(1.0, 0.5, 1.0), dt, u0, "BE")
    pj.solve_AdvectionDiffusionUnsteadyMono_b(su, pht, dt, 5 * dt, bcb, pj.Robin(1.0, 0.5, 1.0), "CN", method="bicgstabl", l=l,
                                              reltol=RELTOL)
    assert su.unconverged == 0 and len(su.states) == len(states)
    for a, b in zip(su.states, states):
        assert rel_l2(a, b) <= TOL_T


def test_stream_vorticity_step_with_l2_for_both_solves(pj):
    """One step on the disc case (shape B) of the stage tests of tests/test_gpu_streamvorticity.py, held to their bars."""
    from tests.test_gpu_streamvorticity import RELTOL as SV_RELTOL, TOL, _build, _check_system as sv_check_system
    s, so, _ = _build(pj, "B")
    M = s._M
    t, w_n = s.time, s.ω.copy()
    pj.step_StreamVorticity_b(s, "BE", method="bicgstabl", l=2, reltol=SV_RELTOL)
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
    assert e_psi <= TOL and e_w <= TOL


# ------------------------------------------------------------------------------------ the same iteration as the restatement
@pytest.mark.parametrize("l", ELLS)
@pytest.mark.parametrize("case", ["heat", "poisson"])
def test_same_iteration_as_the_restatement(pj, case, l):
    """iters within 2 of tests/bicgstabl_reference.py on the constructor's preconditioned system (the allowance
    tests/test_gpu_gmres.py gives GMRES), weights = the row scaling S."""
    s = _heat_pair(pj)[0][0][0] if case == "heat" else _poisson_pair(pj)[0]
    _, info = _restatement(s, l)
    run, _ = _first_solve(s, _opts(L.PG_METHOD["bicgstabl"], l))
    print(case, l, "device iters", run.total_iters, "products", run.products, "restatement", info["iters"], info["products"])
    assert info["converged"] and run.unconverged_steps == 0
    assert abs(run.total_iters - info["iters"]) <= 2, (run.total_iters, info["iters"])


def test_peclet_12_needs_no_more_products_than_bicgstab(pj):
    """32^2 uniform flow (100, 30), cell Peclet number 12.5.  The restatement's count on the row-scaled system moves by 6 products
    under a one-ulp perturbation of b (tests/golden/bicgstabl_products.json), so the counts of device and restatement are not
    compared here: BiCGStab(2) needs no more products than plain BiCGStab on the device, and both reach the direct solve."""
    s = _peclet_solver(pj)
    A, b, idx = s.system(0)
    direct = spla.spsolve(A[:, : len(idx)].tocsc(), b)
    plain, x_plain = _first_solve(s, _opts(L.PG_METHOD["bicgstab"], reltol=1e-12, precond=-1))
    two, x_two = _first_solve(_peclet_solver(pj), _opts(L.PG_METHOD["bicgstabl"], 2, reltol=1e-12))
    print("products: BiCGStab", plain.products, "BiCGStab(2)", two.products)
    assert two.unconverged_steps == 0 and plain.unconverged_steps == 0
    assert two.products <= plain.products
    assert rel_l2(x_two[idx], direct) <= 1e-9 and rel_l2(x_plain[idx], direct) <= 1e-9


# ------------------------------------------------------------------------------------ fails without the feature
def test_method_3_through_the_abi(pj):
    s = _heat_pair(pj, 16)[0][0][0]
    run, x = _first_solve(s, _opts(3, 2))
    assert run.unconverged_steps == 0 and run.total_iters > 0 and np.all(np.isfinite(x))


def test_l_selects_the_method_and_the_bare_name_stays_bicgstab(pj):
    runs = {}
    for key, kw in (("bare", dict(method="bicgstabl")), ("l2", dict(method="bicgstabl", l=2)), ("bicgstab", dict(method="bicgstab"))):
        s = _peclet_solver(pj)
        pj.solve_AdvectionDiffusionSteadyMono_b(s, reltol=1e-12, **kw)
        runs[key] = (s.ch[-1]["iters"], s.x.copy())
    assert runs["bare"][0] == runs["bicgstab"][0] and np.array_equal(runs["bare"][1], runs["bicgstab"][1])   # bit-identical
    assert runs["l2"][0] != runs["bare"][0]

    def bicgstabl():   # stands in for IterativeSolvers.bicgstabl: only the name crosses the boundary
        raise AssertionError
    s = _peclet_solver(pj)
    pj.solve_AdvectionDiffusionSteadyMono_b(s, method=bicgstabl, l=2, reltol=1e-12)
    assert s.ch[-1]["iters"] == runs["l2"][0] and np.array_equal(s.x, runs["l2"][1])


# ------------------------------------------------------------------------------------ reproducibility, counting, caps
@pytest.mark.parametrize("l", [2, 4])
def test_bitwise_reproducible(pj, l):
    out = []
    for _ in range(2):
        run, x = _first_solve(_peclet_solver(pj), _opts(3, l, reltol=1e-12))
        out.append((int(run.total_iters), int(run.products), x))
    assert out[0][0] == out[1][0] > 0 and out[0][1] == out[1][1]
    assert np.array_equal(out[0][2], out[1][2])


def test_maxiter_caps_bicg_substeps(pj):
    """maxiter = 3, l = 2: the second outer iteration starts at iters = 2 < 3 and ends at 4; unconverged; no confirmation."""
    s = _heat_pair(pj)[0][0][0]
    _, info = _restatement(s, 2, maxiter=3)
    assert info["iters"] == 4 and not info["converged"]
    run, x = _first_solve(s, _opts(3, 2, maxiter=3))
    assert run.total_iters == 4 and run.unconverged_steps == 1 and run.products == 8
    assert np.all(np.isfinite(x))


@pytest.mark.parametrize("l", ELLS)
def test_products_are_two_per_substep_plus_confirmations(pj, l):
    s = _heat_pair(pj)[0][0][0]
    _, info = _restatement(s, l)
    run, _ = _first_solve(s, _opts(3, l))
    confirmations = run.products - 2 * run.total_iters
    assert run.unconverged_steps == 0 and 1 <= confirmations <= 4
    assert confirmations == info["confirmations"]


# ------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_condition(pj):
    ((s, ph, bcb, bci), _), dt = _heat_pair(pj, 16)
    with pytest.raises(Exception, match="more than 8"):
        pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, dt, bcb, bci, "BE", method="bicgstabl", l=9)
    with pytest.raises(Exception, match=r"BiCGStab\(l\)"):
        pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, dt, bcb, bci, "BE", method="bicgstabl", l=2, precond=8)
    with pytest.raises(Exception, match=r"BiCGStab\(l\)"):
        pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, dt, bcb, bci, "BE", method="bicgstabl", l=2, precond="poly-est")
    # an unsteady solver that refused keeps working afterwards with defaults
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 2 * dt, bcb, bci, "BE", reltol=RELTOL)
    assert s.unconverged == 0 and np.all(np.isfinite(s.x)) and np.abs(s.x).max() > 0
    for precond in ("mg", "mg-cell"):
        sp, _ = _poisson_pair(pj, 16)
        with pytest.raises(Exception, match=r"BiCGStab\(l\)"):
            pj.solve_DiffusionSteadyMono_b(sp, method="bicgstabl", l=2, precond=precond)
    with pytest.raises(Exception, match="one rank"):
        L.check(L.lib().pg_debug_set_virtual_rank_method(C.c_int32(3), C.c_int32(2)))


# ------------------------------------------------------------------------------------ true-residual confirmation
def test_a_wrong_state_never_passes_as_converged(pj):
    """64^2 rigid rotation of amplitude 100: on the row-scaled system of this geometry the restatement's recurrence residual meets
    the test while the true residual is O(1) (tests/test_bicgstabl_reference.py).  Whatever the device's iteration meets on its
    own (equilibrated) system: a solve reported converged has the true residual it reports and the direct solve's state."""
    s = _peclet_solver(pj, 64, "rotation")
    A, b, idx = s.system(0)
    direct = spla.spsolve(A[:, : len(idx)].tocsc(), b)
    Ah, bh, _ = s.system(2)
    Ah = Ah[:, : Ah.shape[0]].tocsr()
    S = s.row_scaling(0)
    run, x = _first_solve(s, _opts(3, 4, maxiter=4000))
    assert np.all(np.isfinite(x))
    true_rel = np.linalg.norm(S * (bh - Ah @ (x[idx] / S))) / np.linalg.norm(S * bh)
    print("converged", run.unconverged_steps == 0, "iters", run.total_iters, "reported", run.worst_relres, "true", true_rel,
          "error", rel_l2(x[idx], direct))
    if run.unconverged_steps == 0:
        assert run.worst_relres <= RELTOL and true_rel <= 1.5 * RELTOL
        assert rel_l2(x[idx], direct) <= TOL_T


def test_a_steady_solver_keeps_its_phase(pj):
    """The handle of a steady solver points into its phase's capacity and operators; the helpers above return the solver alone."""
    s = _peclet_solver(pj)
    assert isinstance(s._ctx["phase"], pj.Phase) and isinstance(s._ctx["phase"].operator, pj.ConvectionOps)
    sp, _ = _poisson_pair(pj, 16)
    assert isinstance(sp._ctx["phase"], pj.Phase)
