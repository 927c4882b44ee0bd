"""`method = IterativeSolvers.gmres` (the default of solve_system!, src/solver.jl:158) on the device: restarted GMRES of
pg_gmres.hip against the oracle's direct solve (<= 1e-10 rel-L2, the north star's bar) and against the oracle's own
GMRES restatement on the SAME preconditioned system (iteration counts); then, below, against the numpy restatement of the DEVICE
algorithm (tests/gmres_reference.py): the state after one, two and three cycles, the weighted acceptance on a small box, the unit
of maxiter, the edges and data that is not finite."""
import numpy as np
import pytest

from oracle import penguin_oracle as po
from penguin.jl_amd import _lib as L
from tests.common import oracle_capacity_from_product, rel_l2
from tests.gmres_reference import gmres_dev_ref
from tests.test_gpu_bicgstabl import _first_solve, _heat_pair, _peclet_solver, _poisson_pair, _shared
from tests.test_gpu_idrs import RECOMPUTED, _run_steps, _scaled_system, _true_relres
from tests.test_gpu_parity import HEAT_BORDERS, TOL_T, _mono_pair, _velocity_fields

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scheme0,scheme,restart", [("BE", "BE", 0), ("BE", "CN", 0), ("CN", "CN", 4)])
def test_gmres_heat_monophasic(pj, scheme0, scheme, restart):
    """test/solver/diffusion_test.jl:57-80 shape with method=gmres; restart=4 forces several restart cycles."""
    n = 24
    M = (n + 1) ** 2
    u0 = np.concatenate([np.zeros(M), np.ones(M)])
    dt = 0.25 * (4.0 / n) ** 2
    (s, ph, bcb, bci), (so, oph, obcb, obci) = _mono_pair(
        pj, 2, n, 4.0, (2.01, 2.01), 1.0, pj.Dirichlet(1.0), po.Dirichlet(1.0),
        {k: pj.Dirichlet(0.0) for k in HEAT_BORDERS}, {k: po.Dirichlet(0.0) for k in HEAT_BORDERS}, dt, u0, scheme0)
    # the constructor's preconditioned system, before any solve: what the first GMRES solve iterates on
    Ah, bh, _ = s.system(2)
    Ah = Ah[:, : Ah.shape[0]].tocsr()
    kw = {"restart": restart} if restart else {}
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 5 * dt, bcb, bci, scheme, method="gmres", reltol=1e-13, log=True, **kw)
    po.solve_DiffusionUnsteadyMono(so, oph, dt, 5 * dt, obcb, obci, scheme, method="\\")
    assert len(s.states) == len(so.states)
    for a, b in zip(s.states, so.states):
        assert rel_l2(a, b) <= TOL_T
    assert all(c["isconverged"] for c in s.ch)
    # same iteration as the oracle's GMRES (modified Gram-Schmidt there, CGS2 here) on the same system, with the same
    # acceptance rule: the true residual in the units of x at the restarts (weights = the row scaling S)
    _, it_ref, _ = po.gmres_ref(Ah, bh, reltol=1e-13, restart=restart or 20, weights=s.row_scaling(0))
    assert abs(s.ch[0]["iters"] - it_ref) <= 2, (s.ch[0]["iters"], it_ref)


def test_gmres_robin_3d(pj):
    """Robin interface in 3-D (non-trivial cell blocks, non-symmetric system)."""
    n = 12
    M = (n + 1) ** 3
    rng = np.random.default_rng(11)
    u0 = np.concatenate([rng.uniform(0.0, 1.0, M), rng.uniform(0.0, 1.0, M)])
    dt = 0.5 * (4.0 / n) ** 2
    keys = ("left", "right", "top", "bottom", "forward", "backward")
    (s, ph, bcb, bci), (so, oph, obcb, obci) = _mono_pair(
        pj, 3, n, 4.0, (2.03, 1.98, 2.01), 1.1, pj.Robin(1.0, 0.5, 0.3), po.Robin(1.0, 0.5, 0.3),
        {k: pj.Dirichlet(0.2) for k in keys}, {k: po.Dirichlet(0.2) for k in keys}, dt, u0, "BE")
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 3 * dt, bcb, bci, "CN", method="gmres", reltol=1e-13, restart=30)
    po.solve_DiffusionUnsteadyMono(so, oph, dt, 3 * dt, obcb, obci, "CN", method="\\")
    assert rel_l2(s.x, so.x) <= TOL_T


def test_gmres_callable_named_like_iterativesolvers(pj):
    """A callable whose name is `gmres` (the way the reference passes IterativeSolvers.gmres) selects GMRES; maxiter caps
    the total number of inner iterations (IterativeSolvers' meaning) and an unconverged solve is reported as such."""
    def gmres():   # stands in for IterativeSolvers.gmres
        raise AssertionError("never called: only its name crosses the boundary")

    n = 16
    M = (n + 1) ** 2
    u0 = np.concatenate([np.zeros(M), np.ones(M)])
    dt = 0.25 * (4.0 / n) ** 2
    (s, ph, bcb, bci), _ = _mono_pair(
        pj, 2, n, 4.0, (2.01, 2.01), 1.0, pj.Dirichlet(1.0), po.Dirichlet(1.0),
        {k: pj.Dirichlet(0.0) for k in HEAT_BORDERS}, {k: po.Dirichlet(0.0) for k in HEAT_BORDERS}, dt, u0, "BE")
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, dt, bcb, bci, "BE", method=gmres, reltol=1e-14, maxiter=3, log=True)
    assert s.ch[0]["iters"] == 3 and not s.ch[0]["isconverged"]


def test_gmres_steady_poisson(pj):
    """Steady diffusion with gmres: no mass term, so the restart length matters (test/convergence_test.jl:30-70 shape)."""
    n = 24
    mesh, omesh = pj.Mesh((n, n), (4.0, 4.0), (0.0, 0.0)), po.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    from tests.common import oracle_capacity_from_product
    cap = pj.Capacity(pj.Sphere((2.0, 2.0), 1.0), mesh)
    ocap = oracle_capacity_from_product(cap, omesh)
    op, oop = pj.DiffusionOps(cap), po.make_diffusion_ops(ocap)
    f = lambda x, y, z, t=0.0: 4.0
    D = lambda x, y, z: 1.0
    ph, oph = pj.Phase(cap, op, f, D), po.Phase(ocap, oop, f, D)
    s = pj.DiffusionSteadyMono(ph, pj.BorderConditions({}), pj.Dirichlet(0.0))
    so = po.DiffusionSteadyMono(oph, po.BorderConditions({}), po.Dirichlet(0.0))
    pj.solve_DiffusionSteadyMono_b(s, method="gmres", reltol=1e-13, restart=60)
    po.solve_DiffusionSteadyMono(so, method="\\")
    assert rel_l2(s.x, so.x) <= TOL_T


def test_gmres_256_cubed_matches_bicgstab(pj):
    """BASELINE config 3 (256^3 sphere, benchmark/Heat3D.jl shape) with the reference's DEFAULT method (gmres,
    src/solver/diffusion.jl:268): at this size the rows are 400 apart in scale and the un-weighted Givens estimate would
    stop two to three digits early in the units of T; accepted on the weighted true residual at the restarts, GMRES(20)
    ends at the state BiCGStab reaches to the north star's 1e-10."""
    n = 256
    mesh = pj.Mesh((n,) * 3, (4.0,) * 3)
    cap = pj.Capacity(pj.Sphere((2.01,) * 3, 1.0), mesh)
    keys = ("left", "right", "top", "bottom")
    dt = 0.75 * (4.0 / n) ** 2
    states = {}
    for method in ("gmres", "bicgstab"):
        ph = pj.Phase(cap, pj.DiffusionOps(cap), 0.0, 1.0)
        bcb = pj.BorderConditions({k: pj.Dirichlet(1.0) for k in keys})
        s = pj.DiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(1.0), dt, None, "BE")
        pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 1e30, bcb, pj.Dirichlet(1.0), "CN", save_states=False, max_steps=2,
                                         method=method, reltol=1e-12, log=True)
        assert s.unconverged == 0
        assert all(c["isconverged"] for c in s.ch)
        states[method] = s.x
        if method == "gmres":
            assert max(c["iters"] for c in s.ch) > 20                      # several restart cycles: the restart verdicts ran
    assert float(np.max(states["bicgstab"])) > 0.5
    assert rel_l2(states["gmres"], states["bicgstab"]) <= TOL_T


# ====================================================================================== the device's own algebra
# What follows holds pg_gmres.hip to tests/gmres_reference.py gmres_dev_ref -- the numpy restatement of the device algorithm (CGS2 in
# groups of 8, the Givens estimate that only ends a cycle, acceptance on the weighted true residual, the lowered inner tolerance,
# maxiter in Arnoldi steps) -- on the device's own exported system, as tests/test_gpu_idrs.py does for IDR(s).
RELTOL = 1e-13
GMRES = L.PG_METHOD["gmres"]


def _opts(restart=0, reltol=RELTOL, abstol=0.0, maxiter=0, precond=0):
    return L.pg_krylov_opts(GMRES, reltol, abstol, maxiter, 4, 0, restart, precond)


def _restatement(s, restart=0, reltol=RELTOL, **kw):
    Ah, bh, S, idx = _scaled_system(s)
    z, info = gmres_dev_ref(Ah, bh, restart=restart, reltol=reltol, weights=S, **kw)
    return z, info, S, idx


# ------------------------------------------------------------------------------------ 1. state after one, two, three cycles
@pytest.mark.parametrize("restart", (1, 7, 8, 9, 16, 17, 20))
@pytest.mark.parametrize("case", ["heat", "poisson"])
def test_state_after_one_two_three_cycles_is_the_restatements(pj, case, restart):
    """maxiter = restart, 2 restart, 3 restart: one, two and three cycles from zero on the device's own system, at the boundaries of
    the groups of 8 basis vectors (one, two and three launches per pass, tails of 1).  The yardstick is what the order of summation is
    worth: the relative L2 difference between the float64 restatement and the same restatement with longdouble sums.  The device may
    differ from the float64 restatement by 10 x that, floor 64 * 2^-53 (the bound of the IDR(s) test of the same name)."""
    for cycles in (1, 2, 3):
        s = _heat_pair(pj)[0][0][0] if case == "heat" else _poisson_pair(pj)[0]
        cap = cycles * restart
        z64, i64_, S, idx = _restatement(s, restart, maxiter=cap)
        zld, _, _, _ = _restatement(s, restart, maxiter=cap, long_sums=True)
        run, x = _first_solve(s, _opts(restart, maxiter=cap))
        yard = rel_l2(z64, zld)
        diff = rel_l2(x[idx] / S, z64)
        bound = max(10.0 * yard, 64.0 * 2.0 ** -53)
        print(f"{case} restart={restart} cycles={cycles}: yardstick {yard:.2e} device {diff:.2e} bound {bound:.2e} "
              f"iters {run.total_iters}/{i64_['iters']}")
        if i64_["converged"]:
            assert i64_["iters"] <= cap and run.total_iters <= cap and run.unconverged_steps == 0
        else:
            assert run.total_iters == i64_["iters"] == cap and run.unconverged_steps == 1
        assert diff <= bound, (case, restart, cycles, diff, yard)


# ------------------------------------------------------------------------------------ 2. direct-solve parity where GMRES had none
def test_gmres_diphasic_matches_direct_solves(pj):
    """The diphasic heat case of tests/test_gpu_idrs.py (the oracle's solve is shared with it)."""
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
    pj.solve_DiffusionUnsteadyDiph_b(s, p1, p2, dt, 5 * dt, bcb, ic, "CN", method="gmres", reltol=RELTOL)
    assert s.unconverged == 0 and rel_l2(s.x, ref) <= TOL_T


def test_gmres_advection_diffusion_matches_direct_solves(pj):
    """The steady and the unsteady advection-diffusion case of tests/test_gpu_idrs.py (non-symmetric; the oracle's solves are shared
    with it).  The steady system has no mass term: restart 60, as test_gmres_steady_poisson."""
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
    pj.solve_AdvectionDiffusionSteadyMono_b(s, method="gmres", reltol=RELTOL, restart=60)
    assert s.ch[-1]["converged"] and s.unconverged == 0 and rel_l2(s.x, x_steady) <= TOL_T
    pht = pj.Phase(cap, op, ft, D)
    su = pj.AdvectionDiffusionUnsteadyMono(pht, bcb, pj.Robin(1.0, 0.5, 1.0), dt, u0, "BE")
    pj.solve_AdvectionDiffusionUnsteadyMono_b(su, pht, dt, 5 * dt, bcb, pj.Robin(1.0, 0.5, 1.0), "CN", method="gmres", reltol=RELTOL)
    assert su.unconverged == 0 and len(su.states) == len(states)
    for a, b in zip(su.states, states):
        assert rel_l2(a, b) <= TOL_T


# ------------------------------------------------------------------------------------ 3. the weighted rule on a small box
BOX = 0.04       # the box of the issue; on the device's exported system (with its B⁻¹) the restatement still reports lowered >= 1
BOX_RELTOL = 1e-10


def _box_pair(pj, box=BOX):
    """Heat BE on box x box, 16^2, disc r = box / 4 at 0.5025 box, dt = 0.25 h^2, interface Dirichlet(1), borders Dirichlet(0): rows
    1 / h apart in scale -- the Givens estimate meets reltol while the residual in the units of x does not."""
    n = 16
    M = (n + 1) ** 2
    u0 = np.concatenate([np.zeros(M), np.ones(M)])
    dt = 0.25 * (box / n) ** 2
    return _mono_pair(pj, 2, n, box, (0.5025 * box, 0.5025 * box), 0.25 * box, pj.Dirichlet(1.0), po.Dirichlet(1.0),
                      {k: pj.Dirichlet(0.0) for k in HEAT_BORDERS}, {k: po.Dirichlet(0.0) for k in HEAT_BORDERS}, dt, u0, "BE")


def _box_direct(so):
    def direct():
        po.solve_system(so, method="\\")
        return so.x.copy()
    return _shared(("box", BOX), direct)


@pytest.mark.parametrize("restart", [20, 5])
def test_weighted_rule_on_a_small_box(pj, restart):
    (s, _, _, _), (so, _, _, _) = _box_pair(pj)
    z, info, S, idx = _restatement(s, restart, BOX_RELTOL)
    print(f"box {BOX} restart {restart}: S in [{S.min():.3g}, {S.max():.3g}] restatement iters {info['iters']} cycles {info['cycles']} "
          f"lowered {info['lowered']}")
    assert info["converged"] and info["lowered"] >= 1          # the case reaches the tolerance-lowering branch
    run, x = _first_solve(s, _opts(restart, BOX_RELTOL))
    true = _true_relres(s, x)
    print(f"device iters {run.total_iters} unconverged {run.unconverged_steps} reported {run.worst_relres:.3e} true {true:.3e}")
    assert run.unconverged_steps == 0
    assert run.worst_relres <= BOX_RELTOL and true <= RECOMPUTED * BOX_RELTOL
    assert abs(run.total_iters - info["iters"]) <= 2, (run.total_iters, info["iters"])
    assert rel_l2(x, _box_direct(so)) <= TOL_T


# ------------------------------------------------------------------------------------ 4. maxiter caps iterations, and only iterations
def test_maxiter_is_charged_what_ran_on_the_small_box(pj):
    """Restart 20: the Givens estimate ends the first cycle early, and the cycle is charged the steps that ran.  maxiter = the
    restatement's uncapped count converges; one below ends unconverged at exactly maxiter iterations."""
    restart = 20
    s = _box_pair(pj)[0][0]
    _, free, _, _ = _restatement(s, restart, BOX_RELTOL)
    _, below, _, _ = _restatement(s, restart, BOX_RELTOL, maxiter=free["iters"] - 1)
    assert free["converged"] and free["cycles"] >= 2 and free["iters"] < free["cycles"] * restart    # a cycle was cut short
    print(f"restatement: uncapped {free['iters']} iterations in {free['cycles']} cycles, lowered {free['lowered']}; "
          f"maxiter {free['iters'] - 1}: converged {below['converged']} at {below['iters']}")
    assert not below["converged"] and below["iters"] == free["iters"] - 1
    run, x = _first_solve(s, _opts(restart, BOX_RELTOL, maxiter=free["iters"]))
    print(f"device, maxiter {free['iters']}: iters {run.total_iters} unconverged {run.unconverged_steps}")
    assert run.unconverged_steps == 0 and run.total_iters <= free["iters"]
    assert _true_relres(s, x) <= RECOMPUTED * BOX_RELTOL
    s1 = _box_pair(pj)[0][0]
    run1, _ = _first_solve(s1, _opts(restart, BOX_RELTOL, maxiter=free["iters"] - 1))
    print(f"device, maxiter {free['iters'] - 1}: iters {run1.total_iters} unconverged {run1.unconverged_steps}")
    assert run1.unconverged_steps == 1 and run1.total_iters == free["iters"] - 1


@pytest.mark.parametrize("restart", [7, 9])
def test_maxiter_caps_iters_exactly(pj, restart):
    """maxiter = 1, restart, restart + 1 (a second cycle of one step) on heat 24^2, which needs more than 20 iterations: that many
    iterations, unconverged, a finite state -- as the restatement has it.  (Restart 20 is no case: the solve converges at its
    20th iteration.)"""
    for cap in (1, restart, restart + 1):
        s = _heat_pair(pj)[0][0][0]
        _, info, _, _ = _restatement(s, restart, maxiter=cap)
        assert info["iters"] == cap and not info["converged"]
        run, x = _first_solve(s, _opts(restart, maxiter=cap))
        assert run.total_iters == cap and run.unconverged_steps == 1, (cap, run.total_iters)
        assert np.all(np.isfinite(x)) and np.abs(x).max() > 0


# ------------------------------------------------------------------------------------ 5. edges
def test_zero_right_hand_side(pj):
    """u0 = 0, every border and the interface Dirichlet(0), f = 0: b = 0 -- converged at once, x = 0, a finite reported residual."""
    n = 16
    M = (n + 1) ** 2
    dt = 0.25 * (4.0 / n) ** 2
    (s, ph, bcb, bci), _ = _mono_pair(pj, 2, n, 4.0, (2.01, 2.01), 1.0, pj.Dirichlet(0.0), po.Dirichlet(0.0),
                                      {k: pj.Dirichlet(0.0) for k in HEAT_BORDERS}, {k: po.Dirichlet(0.0) for k in HEAT_BORDERS},
                                      dt, np.zeros(2 * M), "BE")
    _, bh, _, _ = _scaled_system(s)
    assert np.all(bh == 0.0)
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, dt, bcb, bci, "BE", method="gmres", reltol=RELTOL, log=True)
    assert s.unconverged == 0 and s.ch[0]["isconverged"] and s.ch[0]["iters"] == 0
    assert np.isfinite(s.ch[0]["resnorm"]) and s.ch[0]["resnorm"] == 0.0
    assert np.all(s.x == 0.0)
    run, x = _first_solve(_mono_pair(pj, 2, n, 4.0, (2.01, 2.01), 1.0, pj.Dirichlet(0.0), po.Dirichlet(0.0),
                                     {k: pj.Dirichlet(0.0) for k in HEAT_BORDERS}, {k: po.Dirichlet(0.0) for k in HEAT_BORDERS},
                                     dt, np.zeros(2 * M), "BE")[0][0], _opts())
    assert run.unconverged_steps == 0 and run.total_iters == 0 and np.isfinite(run.worst_relres) and np.all(x == 0.0)


def test_restart_beyond_the_system_is_one_cycle(pj):
    """Poisson 8^2 (a few dozen unknowns) with restart = 200: m is cut to n, one cycle of at most n steps reaches the direct solve."""
    s, so = _poisson_pair(pj, 8)
    po.solve_DiffusionSteadyMono(so, method="\\")
    _, info, _, idx = _restatement(s, 200)
    run, x = _first_solve(s, _opts(200))
    print("unknowns", len(idx), "iters", run.total_iters, "restatement", info["iters"], "cycles", info["cycles"])
    assert len(idx) < 200 and info["cycles"] == 1 and info["converged"]
    assert run.unconverged_steps == 0 and 0 < run.total_iters <= len(idx) and abs(run.total_iters - info["iters"]) <= 2
    assert rel_l2(s._fetch_state(), so.x) <= TOL_T


def test_restart_1_converges(pj):
    ((s, ph, bcb, bci), (so, oph, obcb, obci)), dt = _heat_pair(pj, 16)
    _, info, _, _ = _restatement(s, 1)
    run, x = _first_solve(s, _opts(1))
    po.solve_system(so, method="\\")
    print("GMRES(1): device", run.total_iters, "restatement", info["iters"])
    assert info["converged"] and run.unconverged_steps == 0 and abs(run.total_iters - info["iters"]) <= 2
    assert _true_relres(s, x) <= RECOMPUTED * RELTOL and rel_l2(x, so.x) <= TOL_T


def test_abstol_alone_decides(pj):
    """reltol = 0: accepted on ||S r|| <= abstol -- the residual recomputed on the host meets it, and a looser abstol needs fewer
    iterations."""
    out = {}
    for abstol in (1e-4, 1e-9):
        s = _heat_pair(pj)[0][0][0]
        Ah, bh, S, idx = _scaled_system(s)
        run, x = _first_solve(s, _opts(5, reltol=0.0, abstol=abstol))
        res = np.linalg.norm(S * (bh - Ah @ (x[idx] / S)))
        _, info, _, _ = _restatement(s, 5, 0.0, abstol=abstol)
        print(f"abstol {abstol:g}: ||S r|| {res:.3e} iters {run.total_iters} restatement {info['iters']}")
        assert run.unconverged_steps == 0 and res <= RECOMPUTED * abstol
        assert info["converged"] and abs(run.total_iters - info["iters"]) <= 2
        out[abstol] = int(run.total_iters)
    assert 0 < out[1e-4] < out[1e-9]


def test_bitwise_reproducible(pj):
    out = []
    for _ in range(2):
        run, x = _first_solve(_peclet_solver(pj), _opts(20, reltol=1e-12))
        out.append((int(run.total_iters), x))
    assert out[0][0] == out[1][0] > 20 and np.array_equal(out[0][1], out[1][1])


def test_precond_0_and_minus_1_are_the_same_plain_iteration(pj):
    """GMRES runs plain: the polynomial preconditioner's switch changes nothing, bit for bit."""
    out = []
    for precond in (0, -1):
        run, x = _first_solve(_heat_pair(pj)[0][0][0], _opts(precond=precond))
        assert run.unconverged_steps == 0
        out.append((int(run.total_iters), x))
    assert out[0][0] == out[1][0] > 0 and np.array_equal(out[0][1], out[1][1])


# ------------------------------------------------------------------------------------ 6. data that is not finite
def test_a_nan_in_the_state_is_never_converged_and_never_handed_back(pj):
    """Heat 16^2 with one NaN in an active bulk entry of u0: the right-hand side is not finite, the solve ends unconverged with a
    zero state (as BiCGStab(l) does: never NaN), and the solver works on from it -- one more BE step from T = 0 is the first solve
    of a solver built on u0 = 0, which the oracle solves directly."""
    n = 16
    M = (n + 1) ** 2
    ((s0, _, _, _), _), dt = _heat_pair(pj, n)
    _, _, idx = s0.system(0)
    bulk = idx[idx < M]
    u0 = np.concatenate([np.zeros(M), np.ones(M)])
    u0[bulk[len(bulk) // 2]] = np.nan
    (s, ph, bcb, bci), _ = _mono_pair(pj, 2, n, 4.0, (2.01, 2.01), 1.0, pj.Dirichlet(1.0), po.Dirichlet(1.0),
                                      {k: pj.Dirichlet(0.0) for k in HEAT_BORDERS}, {k: po.Dirichlet(0.0) for k in HEAT_BORDERS},
                                      dt, u0, "BE")
    run, x = _first_solve(s, _opts(maxiter=40))
    print("NaN in u0: iters", run.total_iters, "unconverged", run.unconverged_steps, "finite", bool(np.all(np.isfinite(x))),
          "max |x|", float(np.nanmax(np.abs(x))) if np.any(np.isfinite(x)) else None)
    assert run.unconverged_steps == 1 and run.total_iters <= 40
    assert np.all(np.isfinite(x)) and np.all(x == 0.0)
    again, x1 = _run_steps(s, _opts(), "BE", 1)
    assert again.unconverged_steps == 0 and again.steps == 1 and np.all(np.isfinite(x1)) and np.abs(x1).max() > 0
    (_, _, _, _), (so, _, _, _) = _mono_pair(pj, 2, n, 4.0, (2.01, 2.01), 1.0, pj.Dirichlet(1.0), po.Dirichlet(1.0),
                                            {k: pj.Dirichlet(0.0) for k in HEAT_BORDERS}, {k: po.Dirichlet(0.0) for k in HEAT_BORDERS},
                                            dt, np.zeros(2 * M), "BE")
    po.solve_system(so, method="\\")
    assert rel_l2(x1, so.x) <= TOL_T
