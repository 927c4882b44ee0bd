"""The branches the time loop takes when a solve does NOT go as planned: a row that counts as solved moves behind the loop's
back (S_MOVED), the polynomial preconditioner stagnates (in a first solve and on the compact system), a solve stops at
maxiter, a solve is done before it starts (zero data, a steady field).  Each of them hands back a state the caller trusts,
so each is held to the oracle's direct solve at the north star's bar: the oracle is FED with the product's previous state
(its constructor with the run scheme; its first solve is then the expected next state), or runs alongside from the start.

The debug entry points are called through raw ctypes, as _spmv_compare of test_gpu_parity.py does."""
import ctypes as C
import os
import pathlib
import subprocess
import sys
import warnings

import numpy as np
import pytest

from oracle import penguin_oracle as po
from penguin.jl_amd import _lib as L
from penguin.jl_amd import api as _api
from tests.common import oracle_capacity_from_product, rel_l2
from tests.test_gpu_parity import HEAT_BORDERS, TOL_T, _mono_pair

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parents[1]
RELTOL = 1e-13


# ------------------------------------------------------------------------------------ the common small problem
class _Problem:
    """Monophasic heat problem with constant data, built once with the product and wrapped for the oracle."""

    def __init__(self, pj, N, n, centre, value, T0=None):
        self.pj, self.n, self.M = pj, n, (n + 1) ** N
        self.dt = 0.75 * (4.0 / n) ** 2
        mesh, omesh = pj.Mesh((n,) * N, (4.0,) * N), po.Mesh((n,) * N, (4.0,) * N)
        cap = pj.Capacity(pj.Sphere(centre, 1.0), mesh)
        ocap = oracle_capacity_from_product(cap, omesh)
        self.ph = pj.Phase(cap, pj.DiffusionOps(cap), 0.0, 1.0)
        self.oph = po.Phase(ocap, po.make_diffusion_ops(ocap), lambda x, y, z, t: 0.0, lambda x, y, z: 1.0)
        self.bcb = pj.BorderConditions({k: pj.Dirichlet(value) for k in HEAT_BORDERS})
        self.obcb = po.BorderConditions({k: po.Dirichlet(value) for k in HEAT_BORDERS})
        self.bci, self.obci = pj.Dirichlet(value), po.Dirichlet(value)
        self.T0 = np.zeros(2 * self.M) if T0 is None else T0

    def solver(self):
        """the product's solver (backward-Euler constructor), not yet solved"""
        return self.pj.DiffusionUnsteadyMono(self.ph, self.bcb, self.bci, self.dt, self.T0, "BE")

    def oracle_next(self, x_prev, scheme):
        """the oracle's step from x_prev: its constructor with the run scheme, its first (direct) solve"""
        so = po.DiffusionUnsteadyMono(self.oph, self.obcb, self.obci, self.dt, x_prev, scheme)
        po.solve_system(so, method="\\")
        return so.x


_cache = {}


def _p32(pj):
    """P32: 3-D, n = 32, L = 4, Sphere((2.01, 2.01, 2.01), 1), Dirichlet(1) on borders and interface, T0 = 0, f = 0, D = 1,
    dt = 0.75 (4/32)^2 -- the compact loop is active and the data are non-zero (scaling a zero moves nothing)."""
    if "p32" not in _cache:
        _cache["p32"] = _Problem(pj, 3, 32, (2.01, 2.01, 2.01), 1.0)
    return _cache["p32"]


def _first(s, **kw):
    info = L.pg_step_info()
    opts = _api._krylov_opts(kw.pop("method", "bicgstab"), {"reltol": RELTOL, **kw})
    L.check(L.lib().pg_solver_initial_solve(s._h, C.byref(opts), C.byref(info)))
    _api._step_info_check(s, info, "the first solve")
    s._initial_done = True
    return info, s._fetch_state()


def _step(s, scheme, **kw):
    """one pg_solver_step with the host layer's bookkeeping of unconverged solves; -> (info, state)"""
    info = L.pg_step_info()
    opts = _api._krylov_opts(kw.pop("method", "bicgstab"), {"reltol": RELTOL, **kw})
    L.check(L.lib().pg_solver_step(s._h, C.c_int32(L.PG_SCHEME[scheme]), C.byref(opts), C.byref(info)))
    _api._step_info_check(s, info, "a time-step solve")
    s._have_run = True
    return info, s._fetch_state()


def _held(tag, x, ref, missed):
    e = rel_l2(x, ref)
    print(f"{tag}: rel-L2 {e:.3e}")
    if not e <= TOL_T:
        missed.append((tag, e))


def _child(code, env):
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, '.'); import penguin.jl_amd as pj; pj.init(0); "
                        "import tests.test_gpu_recovery as t\n" + code + "\nprint('recovery ok')\n"], cwd=ROOT,
                       env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "recovery ok" in r.stdout, (env, r.stdout[-3000:], r.stderr[-4000:])
    print(r.stdout[-3000:])


# ------------------------------------------------------------------------------------ 1. a solved row moves anyway
def _moved_row_sequence(pj, scheme, steps=4):
    """First solve, four steps (2-4 quiet; `steps`: more of them), then every row alone on its diagonal is scaled by 1.5 behind the loop's back: the
    next (quiet) step starts from a residual that lacks the coupling to the moved rows, notices (S_MOVED) and finishes on the
    full system.  That step and the three after it (QuietGuard has reset the snapshot; no stale product, no stale kept
    state) against the oracle's steps from the kicked state.  -> the number of older states the kicked step's start reads."""
    P = _p32(pj)
    s = P.solver()
    _first(s)
    for _ in range(steps):
        info, x = _step(s, scheme)
        assert info.converged == 1
    assert s.system_info(1).loop_is_compact == 1
    guess = s.guess_info()
    print(f"moved row, {scheme}: the extrapolated start before the kick: {guess}")
    L.check(L.lib().pg_debug_scale_diagonal_rows(s._h, C.c_double(1.5)))
    xk = s._fetch_state()
    assert np.max(np.abs(xk - x)) >= 0.4            # the kick is material: boundary values 1 -> 1.5
    missed, ref = [], xk
    for k in range(4):
        info, x = _step(s, scheme)
        assert info.converged == 1, k
        ref = P.oracle_next(ref, scheme)            # k = 0: the oracle's step from the kicked state; then its continuation
        _held(f"moved row, {scheme}, step {k} after the kick ({info.iters} iterations)", x, ref, missed)
    assert not missed, missed
    assert s.unconverged == 0
    return len(guess["offsets"])


@pytest.mark.parametrize("scheme", ["CN", "BE"])
def test_a_moved_row_in_a_quiet_step_is_caught_and_the_step_finished_on_the_full_system(pj, scheme):
    """Measured on an MI355X: CN <= 1.6e-12, BE <= 3.5e-13 on the four steps.  With the net switched off (moved_unseen = false
    in a scratch build) the step after the kick ends at rel-L2 4.2e-2 (CN) / 5.2e-2 (BE) of the oracle's, and the three after
    it stay at 1e-2 ... 5.5e-2."""
    _moved_row_sequence(pj, scheme)


def test_a_moved_row_meets_an_extrapolated_deferred_start():
    """The same sequences with PG_GUESS_ALWAYS=1 (read once per process: a child): the quiet steps start from an extrapolation
    of older states whose forming is deferred to the solve's first update of x (xguess) -- and the moved rows meet that.
    Whether the fit takes older states is its own decision: after four steps it does for BE (two states) and not yet for CN,
    so CN runs once more with twelve steps before the kick, and at least one of the kicked steps must have read older states."""
    _child("read = [t._moved_row_sequence(pj, 'CN'), t._moved_row_sequence(pj, 'BE'), t._moved_row_sequence(pj, 'CN', 12)]\n"
           "print('older states read by the kicked steps:', read)\nassert max(read) >= 1, read", {"PG_GUESS_ALWAYS": "1"})


# ------------------------------------------------------------------------------------ 3. the polynomial stagnates
def _set_give_up(iterations):
    L.check(L.lib().pg_debug_set_poly_give_up(C.c_int32(iterations)))


def _robin_disc(pj):
    """2-D 64^2, L = 4, disc (2.01, 2.01) of radius 1, Dirichlet(0) borders, Robin(1, 0.3, 1) interface, f = 1"""
    n = 64
    mesh, omesh = pj.Mesh((n, n), (4.0, 4.0)), po.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0), mesh)
    ocap = oracle_capacity_from_product(cap, omesh)
    f, D = (lambda x, y, z=0.0, t=0.0: 1.0), (lambda x, y, z=0.0: 1.0)
    ph, oph = pj.Phase(cap, pj.DiffusionOps(cap), f, D), po.Phase(ocap, po.make_diffusion_ops(ocap), f, D)
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in HEAT_BORDERS})
    obcb = po.BorderConditions({k: po.Dirichlet(0.0) for k in HEAT_BORDERS})
    return n, ph, oph, bcb, obcb, pj.Robin(1.0, 0.3, 1.0), po.Robin(1.0, 0.3, 1.0)


def test_stagnation_verdict_in_a_first_solve_continues_with_the_plain_iteration(pj):
    """krylov_solve's own fallback: with the give-up point at one iteration a polynomial-preconditioned first solve (which
    needs at least 3) is declared stagnated at its first poll, the plain iteration continues from the iterate reached --
    x0 == x in k_bicg_init -- and the matrix keeps the verdict.  check_every = 1: the first batch is one iteration.

    The solve is the FIRST solve of an unsteady problem on the disc (backward Euler, dt = 0.75 h^2, T0 = 0, Dirichlet(1)
    interface, degree 2), not the steady Robin problem on it: a steady system has no mass term, its Gershgorin radius is 1
    and the polynomial is never admitted on it (test_polynomial_preconditioner_is_admitted_and_follows_the_host_restatement
    pins that; the unsteady system with the Robin rows is not admitted either: radius 13.1), so the hook has nothing
    to act on there -- which the second half of this test holds the steady Robin problem to."""
    n, ph, oph, bcb, obcb, bci, obci = _robin_disc(pj)
    M, dt = (n + 1) ** 2, 0.75 * (4.0 / n) ** 2
    mk = lambda: pj.DiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(1.0), dt, np.zeros(2 * M), "BE")
    so = po.DiffusionUnsteadyMono(oph, obcb, po.Dirichlet(1.0), dt, np.zeros(2 * M), "BE")
    po.solve_system(so, method="\\")
    plain = mk()
    assert plain.system_info(0).neumann_ok == 1
    info0, x0 = _first(plain, check_every=1, precond=2)
    assert info0.converged == 1 and info0.iters >= 3, (info0.converged, info0.iters)
    assert plain.system_info(0).neumann_ok == 1
    assert rel_l2(x0, so.x) <= TOL_T
    s = mk()
    _set_give_up(1)
    try:
        info, x = _first(s, check_every=1, precond=2)
    finally:
        _set_give_up(0)
    e = rel_l2(x, so.x)
    print(f"first solve after the stagnation verdict: rel-L2 {e:.3e}, {info.iters} iterations (undisturbed: {info0.iters})")
    assert e <= TOL_T, e
    assert info.converged == 1 and s.unconverged == 0
    assert info.iters > info0.iters                           # the plain iteration took over
    assert s.system_info(0).neumann_ok == 0                   # the matrix keeps the verdict
    # the steady problem on the same disc: not admitted, so the same hook changes nothing and the state is the oracle's
    sto = po.DiffusionSteadyMono(oph, obcb, obci)
    po.solve_DiffusionSteadyMono(sto, method="\\")
    its = []
    for give_up in (0, 1):
        st = pj.DiffusionSteadyMono(ph, bcb, bci)
        assert st.system_info(0).neumann_ok == 0 and st.system_info(0).gershgorin >= 0.95
        _set_give_up(give_up)
        try:
            pj.solve_DiffusionSteadyMono_b(st, reltol=RELTOL, check_every=1)
        finally:
            _set_give_up(0)
        assert st.ch[-1]["converged"] and st.ch[-1]["iters"] >= 3 and rel_l2(st.x, sto.x) <= TOL_T, (give_up, st.ch, rel_l2(st.x, sto.x))
        its.append(st.ch[-1]["iters"])
    assert its[0] == its[1], its


def test_stagnation_verdict_on_the_compact_system_resolves_on_the_full_one(pj):
    """The compact loop's fallback: three quiet Crank-Nicolson steps, then a step whose polynomial is declared stagnated at the
    first poll (give-up point 1; degree 2 and check_every = 1, so that the first batch is one iteration of 4 products where
    the solve needs about 30: it cannot be done by then).  krylov_solve returns poly_degree = -1, do_step drops the compact
    system and solves again on the full one from the state reached; afterwards the loop is the plain iteration on the full
    system.  Measured on an MI355X: 9.8e-13 on that step, 1.1e-12 on the two after it.  With poly_degree == -1 treated as
    solved (a scratch build) that step ends at rel-L2 1.9e-3 of the oracle's."""
    P = _p32(pj)
    s = P.solver()
    _first(s)
    for _ in range(4):                       # the first CN step builds the run matrix, the next three are quiet
        info, x = _step(s, "CN")
    assert s.system_info(1).loop_is_compact == 1 and s.system_info(1).neumann_ok == 1
    missed = []
    _set_give_up(1)
    try:
        info, x1 = _step(s, "CN", precond=2, check_every=1)
    finally:
        _set_give_up(0)
    _held(f"step with the stagnation verdict ({info.iters} iterations)", x1, P.oracle_next(x, "CN"), missed)
    assert not missed, missed
    assert info.converged == 1
    assert s.system_info(1).loop_is_compact == 0 and s.system_info(1).neumann_ok == 0
    x = x1
    for k in range(2):
        info, x1 = _step(s, "CN")
        assert info.converged == 1
        _held(f"plain step {k} on the full system ({info.iters} iterations)", x1, P.oracle_next(x, "CN"), missed)
        x = x1
    assert not missed, missed
    assert s.unconverged == 0


# ------------------------------------------------------------------------------------ 4. a step that stops at maxiter
def _cg_problem(pj):
    """the shape of test_cg_method_on_symmetric_problem: a body covering the box, no border rows -- V + dt GᵀWꜝG, SPD"""
    n = 20
    M = (n + 1) ** 2
    u0 = np.concatenate([np.random.default_rng(5).uniform(0.0, 1.0, M), np.zeros(M)])
    dt = 0.25 * (4.0 / n) ** 2
    (s, ph, bcb, bci), (so, oph, obcb, obci) = _mono_pair(
        pj, 2, n, 4.0, (2.0, 2.0), 10.0, pj.Dirichlet(1.0), po.Dirichlet(1.0), {}, {}, dt, u0, "BE")

    def oracle_next(x_prev, scheme):
        o = po.DiffusionUnsteadyMono(oph, obcb, obci, dt, x_prev, scheme)
        po.solve_system(o, method="\\")
        return o.x
    return s, oracle_next


# (the capped BiCGStab step runs the polynomial at degree 2: two iterations are then 8 products of the ~30 the solve needs.
#  At the loop's own degree two iterations are four applications of a polynomial ONE of which usually suffices: the cap
#  would not bind and there would be no unconverged step to look at.)
@pytest.mark.parametrize("method,capped", [("bicgstab", {"precond": 2}), ("cg", {})])
def test_a_step_that_stops_at_maxiter_is_reported_and_the_loop_recovers(pj, method, capped):
    if method == "cg":
        s, oracle_next = _cg_problem(pj)
    else:
        P = _p32(pj)
        s, oracle_next = P.solver(), P.oracle_next
    _first(s, method=method)
    for _ in range(2):
        info, x = _step(s, "CN", method=method)
        assert info.converged == 1
    if method == "bicgstab":
        assert s.system_info(1).loop_is_compact == 1
    assert s.unconverged == 0
    with pytest.warns(RuntimeWarning, match="did not converge"):
        info, x = _step(s, "CN", method=method, maxiter=2, reltol=1e-14, **capped)
    assert info.converged == 0 and info.iters == 2, (info.converged, info.iters)
    assert s.unconverged == 1 and np.all(np.isfinite(x))
    missed = []
    for k in range(2):                       # k = 0 starts from the unconverged state
        info, x1 = _step(s, "CN", method=method)
        assert info.converged == 1, k
        _held(f"{method}: step {k} after the unconverged one ({info.iters} iterations)", x1, oracle_next(x, "CN"), missed)
        x = x1
    assert not missed, missed
    assert s.unconverged == 1
    # the run form reports the same thing
    opts = _api._krylov_opts(method, {"maxiter": 2, "reltol": 1e-14, **capped})
    run = L.pg_run_info()
    L.check(L.lib().pg_solver_run(s._h, C.c_double(1e300), C.c_int32(L.PG_SCHEME["CN"]), C.byref(opts), C.c_int32(0), C.c_int64(3),
                                  C.c_int32(0), C.byref(run)))
    assert run.steps == 3 and run.unconverged_steps == 3 and run.worst_relres > 0.0, (run.steps, run.unconverged_steps, run.worst_relres)
    assert np.all(np.isfinite(s._fetch_state()))


# ------------------------------------------------------------------------------------ 5. done at the start
def _zero_mono(pj):
    n = 16
    M = (n + 1) ** 3
    (s, *_), _ = _mono_pair(pj, 3, n, 4.0, (2.01, 2.01, 2.01), 1.0, pj.Dirichlet(0.0), po.Dirichlet(0.0),
                            {k: pj.Dirichlet(0.0) for k in HEAT_BORDERS}, {k: po.Dirichlet(0.0) for k in HEAT_BORDERS},
                            0.75 * (4.0 / n) ** 2, np.zeros(2 * M), "BE", f=lambda x, y, z, t: 0.0)
    return s, 2 * M


def _zero_diph(pj):
    """config 5's shape at 32^2 (test_diphasic_heat_2d) with nothing in it"""
    n, Lx, c, r = 32, 8.0, (4.0, 4.0), 2.0
    M = (n + 1) ** 2
    mesh = pj.Mesh((n, n), (Lx, Lx), (0.0, 0.0))
    cap1, cap2 = pj.Capacity(pj.Sphere(c, r), mesh), pj.Capacity(pj.Sphere(c, r, complement=True), mesh)
    p1, p2 = pj.Phase(cap1, pj.DiffusionOps(cap1), 0.0, 1.0), pj.Phase(cap2, pj.DiffusionOps(cap2), 0.0, 2.0)
    ic = pj.InterfaceConditions(pj.ScalarJump(1.0, 0.5, 0.0), pj.FluxJump(1.0, 1.0, 0.0))
    s = pj.DiffusionUnsteadyDiph(p1, p2, pj.BorderConditions({}), ic, 0.5 * (Lx / n) ** 2, np.zeros(4 * M), "BE")
    s._keep = (mesh, cap1, cap2, p1, p2)
    return s, 4 * M


@pytest.mark.parametrize("shape,method", [("mono", "bicgstab"), ("mono", "cg"), ("mono", "gmres"), ("diph", "bicgstab"),
                                          ("diph", "gmres")])
def test_zero_data_give_zero_states_without_an_iteration(pj, shape, method):
    """T0 = 0, every boundary value 0, f = 0: the right-hand side is zero, (r,r)_W = 0 <= tol^2 = 0 in derive(PH_INIT) /
    derive(PH_CG_INIT) and beta == 0.0 at the GMRES start -- every solve is done before it starts, and no 0/0 of the
    recurrences is ever formed."""
    s, nunk = (_zero_mono if shape == "mono" else _zero_diph)(pj)
    zero = np.zeros(nunk)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        info, x = _first(s, method=method)
        assert np.array_equal(x, zero) and info.converged == 1 and info.iters == 0, (info.converged, info.iters)
        for k in range(3):
            info, x = _step(s, "CN", method=method)
            assert np.array_equal(x, zero) and info.converged == 1 and info.iters == 0, (k, info.converged, info.iters)
    assert s.unconverged == 0


def _steady_field_sequence(pj):
    """P32 with T0 = 1: the constant 1 solves the discrete system with Dirichlet(1) everywhere (the gradient of a constant
    vanishes), so nothing ever changes -- after the first few the solves meet the tolerance at their start (no product, the
    branch that switches the deferred forming of an extrapolated start off)."""
    if "steady" not in _cache:
        base = _p32(pj)
        P = _Problem(pj, 3, 32, (2.01, 2.01, 2.01), 1.0, T0=np.ones(2 * base.M))
        so = po.DiffusionUnsteadyMono(P.oph, P.obcb, P.obci, P.dt, P.T0, "BE")
        po.solve_DiffusionUnsteadyMono(so, P.oph, P.dt, 1e300, P.obcb, P.obci, "CN", method="\\", max_steps=12)
        _cache["steady"] = (P, so.states)
    P, ref = _cache["steady"]
    assert len(ref) == 13
    s = P.solver()
    info, x = _first(s)
    states, its = [x], [info.iters]
    for _ in range(12):
        info, x = _step(s, "CN")
        states.append(x)
        its.append(info.iters)
    _, _, idx = s.system(1)
    worst = max(rel_l2(a, b) for a, b in zip(states, ref))
    dev = max(float(np.max(np.abs(a[idx] - 1.0))) for a in states)
    print(f"steady field: worst rel-L2 {worst:.3e}, max |x - 1| {dev:.3e}, iterations {its}")
    assert worst <= TOL_T, worst
    assert dev <= 1e-12, dev
    assert s.unconverged == 0
    assert s.system_info(1).loop_is_compact == 1


def test_a_steady_field_stays_put(pj):
    _steady_field_sequence(pj)


def test_a_steady_field_stays_put_under_the_extrapolated_start():
    _child("t._steady_field_sequence(pj)", {"PG_GUESS_ALWAYS": "1"})
