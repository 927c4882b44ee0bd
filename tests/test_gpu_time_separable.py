"""Time-separable data on the GPU: sources, interface values and border values of the form Σ φ_k(x) a_k(t) (pj.TimeSeparable)
keep the time loop on the device -- spatial parts and a coefficient table installed once, one streaming kernel per step.  Every
state against the oracle's direct solves given the SAME objects, against the product's own host-driven loop given the same data
as plain closures, the refusals of the raw C ABI, and the combine kernel alone against k_bconst fed from the host."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import penguin_oracle as po
from penguin.jl_amd import _lib as L
from penguin.jl_amd import api
from tests.common import oracle_capacity_from_product, rel_l2
from tests.test_gpu_parity import HEAT_BORDERS, TOL_T, _mono_pair, _velocity_fields

pytestmark = pytest.mark.gpu

X = lambda x, *_: x
COSX = lambda x, *_: np.cos(x)


def _case1_data(pj):
    f = pj.TimeSeparable([(1.0, lambda t: 1.0), (X, lambda t: t), (COSX, lambda t: math.sin(40.0 * t))])
    g = pj.TimeSeparable([(COSX, lambda t: 1.0 + t)])
    bv = pj.TimeSeparable([(lambda x, *_: 0.5 * x, lambda t: 1.0), (1.0, lambda t: t)])
    return f, g, bv


def _case1_pair(pj, scheme0, f, g, bv, n=24, r=1.7):
    M = (n + 1) ** 2
    D = lambda x, y, z: 1.0 + 0.3 * x + 0.1 * y
    u0 = np.concatenate([0.2 * np.ones(M), np.ones(M)])
    dt = 0.4 * (4.0 / n) ** 2
    pair = _mono_pair(pj, 2, n, 4.0, (2.01, 2.01), r, pj.Dirichlet(g), po.Dirichlet(g),
                      {k: pj.Dirichlet(bv) for k in HEAT_BORDERS}, {k: po.Dirichlet(bv) for k in HEAT_BORDERS}, dt, u0, scheme0,
                      f=f, D=D)
    return pair, dt


_CASE1 = {}


def _case1(pj, scheme0, scheme):
    """The oracle's states and the device path's (per-step branch) of case 1, computed once per pair of schemes."""
    key = (scheme0, scheme)
    if key not in _CASE1:
        f, g, bv = _case1_data(pj)
        ((s, ph, bcb, bci), (so, oph, obcb, obci)), dt = _case1_pair(pj, scheme0, f, g, bv)
        pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 6 * dt, bcb, bci, scheme, reltol=1e-13)
        po.solve_DiffusionUnsteadyMono(so, oph, dt, 6 * dt, obcb, obci, scheme, method="\\")
        _CASE1[key] = dict(time_data=s.time_data, states=[x.copy() for x in s.states], oracle=[np.array(x) for x in so.states],
                           info=_td_info(s), dt=dt)
    return _CASE1[key]


def _td_info(s):
    terms = (C.c_int32 * 4)()
    nrows, cursor = C.c_int64(-1), C.c_int64(-1)
    L.check(L.lib().pg_solver_time_data_info(s._h, terms, C.byref(nrows), C.byref(cursor)))
    return list(terms), nrows.value, cursor.value


SCHEMES = [("BE", "BE"), ("BE", "CN"), ("CN", "CN")]


@pytest.mark.parametrize("scheme0,scheme", SCHEMES)
def test_mono_2d_device_loop_matches_the_oracle(pj, scheme0, scheme):
    """Case 1: three source terms with different a_k, interface value cos(x)(1 + t), border value 0.5 x + t."""
    c = _case1(pj, scheme0, scheme)
    assert c["time_data"] == "device"
    assert c["info"] == ([3, 0, 1, 2], 6, 6)               # terms per slot, table rows, every row consumed
    assert len(c["states"]) == len(c["oracle"]) == 7
    errs = [rel_l2(a, b) for a, b in zip(c["states"], c["oracle"])]
    print("mono 2-D", scheme0, scheme, "rel L2 against the oracle per state:", errs)
    assert max(errs) <= TOL_T


@pytest.mark.parametrize("scheme0,scheme", SCHEMES)
def test_mono_2d_device_loop_matches_the_host_driven_loop(pj, scheme0, scheme):
    """The same data wrapped in plain lambdas take the host-driven loop; and pg_solver_run (save_states=False) takes 6 steps to
    the same final state as the per-step branch."""
    c = _case1(pj, scheme0, scheme)
    f, g, bv = _case1_data(pj)
    fl, gl, bl = (lambda x, y, z, t: f(x, y, z, t)), (lambda x, y, z, t: g(x, y, z, t)), (lambda x, y, t: bv(x, y, t))
    ((s, ph, bcb, bci), _), dt = _case1_pair(pj, scheme0, fl, gl, bl)
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 6 * dt, bcb, bci, scheme, reltol=1e-13)
    assert s.time_data == "host"
    assert len(s.states) == len(c["states"])
    errs = [rel_l2(a, b) for a, b in zip(c["states"], s.states)]
    print("mono 2-D", scheme0, scheme, "rel L2 device loop against host-driven loop per state:", errs)
    assert max(errs) <= TOL_T
    # the other device branch: the whole loop in one call
    ((s2, ph2, bcb2, bci2), _), dt = _case1_pair(pj, scheme0, f, g, bv)
    pj.solve_DiffusionUnsteadyMono_b(s2, ph2, dt, 6 * dt, bcb2, bci2, scheme, reltol=1e-13, save_states=False)
    assert s2.time_data == "device" and s2.last_run.steps == 6
    e = rel_l2(s2.x, c["states"][-1])
    print("pg_solver_run against the per-step branch:", e)
    assert e <= TOL_T
    assert rel_l2(s2.x, c["oracle"][-1]) <= TOL_T


@pytest.mark.parametrize("scheme", ["BE", "CN"])
def test_late_switch_reaches_the_solve_at_the_right_step(pj, scheme):
    """A source that switches on after 3.5 Δt and an interface coefficient that changes once at 5.5 Δt: an off-by-one in the
    table's rows shows as a state that differs from the oracle's."""
    n = 20
    M = (n + 1) ** 2
    dt = 0.4 * (4.0 / n) ** 2
    f = pj.TimeSeparable([(2.0, lambda t: 1.0 if t > 3.5 * dt else 0.0)])
    g = pj.TimeSeparable([(1.0, lambda t: 1.0 if t < 5.5 * dt else 1.5)])
    bv = pj.TimeSeparable([(X, lambda t: t)])
    u0 = np.concatenate([0.1 * np.ones(M), np.ones(M)])
    borders = lambda mod, v: {k: mod.Dirichlet(v) for k in HEAT_BORDERS}
    (s, ph, bcb, bci), (so, oph, obcb, obci) = _mono_pair(
        pj, 2, n, 4.0, (2.01, 2.01), 1.6, pj.Dirichlet(g), po.Dirichlet(g), borders(pj, bv), borders(po, bv), dt, u0, scheme, f=f)
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 8 * dt, bcb, bci, scheme, reltol=1e-13)
    po.solve_DiffusionUnsteadyMono(so, oph, dt, 8 * dt, obcb, obci, scheme, method="\\")
    assert s.time_data == "device"
    assert len(s.states) == len(so.states)
    errs = [rel_l2(a, b) for a, b in zip(s.states, so.states)]
    print("late switch", scheme, errs)
    assert max(errs) <= TOL_T
    # and the late data did matter: the last state differs from a run that keeps the early data
    f0 = pj.TimeSeparable([(2.0, lambda t: 0.0)])
    g0 = pj.TimeSeparable([(1.0, lambda t: 1.0)])
    (s0, ph0, bcb0, bci0), _ = _mono_pair(
        pj, 2, n, 4.0, (2.01, 2.01), 1.6, pj.Dirichlet(g0), po.Dirichlet(g0), borders(pj, bv), borders(po, bv), dt, u0, scheme, f=f0)
    pj.solve_DiffusionUnsteadyMono_b(s0, ph0, dt, 8 * dt, bcb0, bci0, scheme, reltol=1e-13)
    assert s0.time_data == "device"
    assert rel_l2(s0.x, s.x) > 1e-3


def _diph_pair(pj, n, f1, f2, scheme0, conv=False):
    Lx, c, r = 8.0, (4.0, 4.0), 2.0
    M = (n + 1) ** 2
    mesh, omesh = pj.Mesh((n, n), (Lx, Lx), (0.0, 0.0)), po.Mesh((n, n), (Lx, Lx), (0.0, 0.0))
    cap1, cap2 = pj.Capacity(pj.Sphere(c, r), mesh), pj.Capacity(pj.Sphere(c, r, complement=True), mesh)
    oc1, oc2 = oracle_capacity_from_product(cap1, omesh), oracle_capacity_from_product(cap2, omesh)
    D1, D2 = (lambda x, y, z: 1.0), (lambda x, y, z: 2.0)
    p1, p2 = pj.Phase(cap1, pj.DiffusionOps(cap1), f1, D1), pj.Phase(cap2, pj.DiffusionOps(cap2), f2, D2)
    q1, q2 = po.Phase(oc1, po.make_diffusion_ops(oc1), f1, D1), po.Phase(oc2, po.make_diffusion_ops(oc2), f2, D2)
    ic = pj.InterfaceConditions(pj.ScalarJump(1.0, 0.5, 0.0), pj.FluxJump(1.0, 1.0, 0.0))
    oic = po.InterfaceConditions(po.ScalarJump(1.0, 0.5, 0.0), po.FluxJump(1.0, 1.0, 0.0))
    bcb, obcb = pj.BorderConditions({}), po.BorderConditions({})
    u0 = np.concatenate([np.ones(M), np.ones(M), np.zeros(M), np.zeros(M)])
    dt = 0.5 * (Lx / n) ** 2
    s = pj.DiffusionUnsteadyDiph(p1, p2, bcb, ic, dt, u0, scheme0)
    so = po.DiffusionUnsteadyDiph(q1, q2, obcb, oic, dt, u0, scheme0)
    return (s, p1, p2, bcb, ic), (so, q1, q2, obcb, oic), dt


@pytest.mark.parametrize("scheme0,scheme", [("BE", "BE"), ("BE", "CN")])
def test_diphasic_separable_sources_in_both_phases(pj, scheme0, scheme):
    f1 = pj.TimeSeparable([(1.0, lambda t: 1.0 + t), (X, lambda t: math.sin(3.0 * t))])
    f2 = pj.TimeSeparable([(lambda x, y, *_: 0.5 + 0.1 * y, lambda t: math.cos(2.0 * t))])
    (s, p1, p2, bcb, ic), (so, q1, q2, obcb, oic), dt = _diph_pair(pj, 16, f1, f2, scheme0)
    pj.solve_DiffusionUnsteadyDiph_b(s, p1, p2, dt, 5 * dt, bcb, ic, scheme, reltol=1e-13)
    po.solve_DiffusionUnsteadyDiph(so, q1, q2, dt, 5 * dt, obcb, oic, scheme, method="\\")
    assert s.time_data == "device"
    assert _td_info(s) == ([2, 1, 0, 0], 5, 5)
    assert len(s.states) == len(so.states)
    errs = [rel_l2(a, b) for a, b in zip(s.states, so.states)]
    print("diph", scheme0, scheme, errs)
    assert max(errs) <= TOL_T
    # the whole loop in one call
    (s2, p1, p2, bcb, ic), _, dt = _diph_pair(pj, 16, f1, f2, scheme0)
    pj.solve_DiffusionUnsteadyDiph_b(s2, p1, p2, dt, 5 * dt, bcb, ic, scheme, reltol=1e-13, save_states=False)
    assert s2.time_data == "device" and s2.last_run.steps == 5
    assert rel_l2(s2.x, so.x) <= TOL_T


def test_mono_3d_cn(pj):
    n = 12
    M = (n + 1) ** 3
    f = pj.TimeSeparable([(lambda x, y, z: 1.0 + 0.2 * x * z, lambda t: 1.0 + 5.0 * t), (1.0, lambda t: math.sin(8.0 * t))])
    g = pj.TimeSeparable([(lambda x, y, z: np.cos(x) + 0.1 * z, lambda t: 1.0 + t)])
    bv = pj.TimeSeparable([(lambda x, y, z: 0.5 * x + 0.25 * z, lambda t: 1.0), (1.0, lambda t: t)])
    u0 = np.concatenate([0.2 * np.ones(M), np.ones(M)])
    dt = 0.5 * (4.0 / n) ** 2
    (s, ph, bcb, bci), (so, oph, obcb, obci) = _mono_pair(
        pj, 3, n, 4.0, (2.01, 2.01, 2.01), 1.3, pj.Dirichlet(g), po.Dirichlet(g), {k: pj.Dirichlet(bv) for k in HEAT_BORDERS},
        {k: po.Dirichlet(bv) for k in HEAT_BORDERS}, dt, u0, "CN", f=f)
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 4 * dt, bcb, bci, "CN", reltol=1e-13)
    po.solve_DiffusionUnsteadyMono(so, oph, dt, 4 * dt, obcb, obci, "CN", method="\\")
    assert s.time_data == "device"
    errs = [rel_l2(a, b) for a, b in zip(s.states, so.states)]
    print("mono 3-D CN", errs)
    assert len(s.states) == len(so.states) and max(errs) <= TOL_T


def test_advection_diffusion_mono_be_with_a_separable_source(pj):
    n, N = 16, 2
    M = (n + 1) ** 2
    mesh, omesh = pj.Mesh((n, n), (4.0, 4.0)), po.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0), mesh)
    ocap = oracle_capacity_from_product(cap, omesh)
    u, ug = _velocity_fields(cap, N, M)
    op, oop = pj.ConvectionOps(cap, u, ug), po.make_convection_ops(ocap, u, ug)
    f = pj.TimeSeparable([(lambda x, *_: 1.0 + 0.2 * x, lambda t: 1.0 + 20.0 * t), (1.0, lambda t: math.sin(30.0 * t))])
    D = lambda x, y, z=0.0: 0.5 + 0.1 * y
    ph, oph = pj.Phase(cap, op, f, D), po.Phase(ocap, oop, f, D)
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in HEAT_BORDERS})
    obcb = po.BorderConditions({k: po.Dirichlet(0.0) for k in HEAT_BORDERS})
    dt = 0.25 * (4.0 / n) ** 2
    u0 = np.concatenate([np.zeros(M), np.ones(M)])
    s = pj.AdvectionDiffusionUnsteadyMono(ph, bcb, pj.Robin(1.0, 0.5, 1.0), dt, u0, "BE")
    so = po.AdvectionDiffusionUnsteadyMono(oph, obcb, po.Robin(1.0, 0.5, 1.0), dt, u0, "BE")
    pj.solve_AdvectionDiffusionUnsteadyMono_b(s, ph, dt, 5 * dt, bcb, pj.Robin(1.0, 0.5, 1.0), "BE", reltol=1e-13)
    po.solve_AdvectionDiffusionUnsteadyMono(so, oph, dt, 5 * dt, obcb, po.Robin(1.0, 0.5, 1.0), "BE", method="\\")
    assert s.time_data == "device"
    errs = [rel_l2(a, b) for a, b in zip(s.states, so.states)]
    print("advection-diffusion BE", errs)
    assert len(s.states) == len(so.states) and max(errs) <= TOL_T


def test_one_plain_closure_sends_the_whole_call_to_the_host_loop(pj):
    f, _, _ = _case1_data(pj)
    g = lambda x, y, z, t: np.cos(x) * (1.0 + t)
    ((s, ph, bcb, bci), (so, oph, obcb, obci)), dt = _case1_pair(pj, "BE", f, g, 0.25)
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 4 * dt, bcb, bci, "CN", reltol=1e-13)
    po.solve_DiffusionUnsteadyMono(so, oph, dt, 4 * dt, obcb, obci, "CN", method="\\")
    assert s.time_data == "host"
    assert _td_info(s) == ([0, 0, 0, 0], 0, 0)
    errs = [rel_l2(a, b) for a, b in zip(s.states, so.states)]
    assert len(s.states) == len(so.states) and max(errs) <= TOL_T
    # constant data: neither
    s, ph, bcb, bci, dt = _product_mono(pj, 16, 1.2)
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 2 * dt, bcb, bci, "BE", reltol=1e-13)
    assert s.time_data is None


def _product_mono(pj, n, r):
    """A monophasic BE solver of the product alone, constant data."""
    M = (n + 1) ** 2
    mesh = pj.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), r), mesh)
    ph = pj.Phase(cap, pj.DiffusionOps(cap), lambda x, y, z: 1.0, lambda x, y, z: 1.0)
    bcb, bci = pj.BorderConditions({k: pj.Dirichlet(0.25) for k in HEAT_BORDERS}), pj.Dirichlet(0.5)
    dt = 0.4 * (4.0 / n) ** 2
    return pj.DiffusionUnsteadyMono(ph, bcb, bci, dt, np.concatenate([0.2 * np.ones(M), np.ones(M)]), "BE"), ph, bcb, bci, dt


def _last_error():
    buf = C.create_string_buffer(4096)
    L.lib().pg_last_error(buf, 4096)
    return buf.value.decode("utf-8", "replace")


def test_refusals_through_the_raw_abi(pj):
    lib = L.lib()
    s, ph, bcb, bci, dt = _product_mono(pj, 16, 1.2)
    M = 17 * 17
    opts = api._krylov_opts("bicgstab", {"reltol": 1e-12})
    info = L.pg_step_info()
    modes = np.ones((9, M))
    table = np.ones((2, 2, 9))
    sep = lambda sol, which, K, nrows: lib.pg_solver_set_separable(sol._h, C.c_int32(which), C.c_int32(0), C.c_int32(K), L.dptr(modes),
                                                                   C.c_int64(nrows), L.dptr(table))
    # before the first solve the constructor's system is the host's
    assert sep(s, 0, 1, 2) != 0 and "pg_solver_initial_solve" in _last_error()
    L.check(lib.pg_solver_initial_solve(s._h, C.byref(opts), C.byref(info)))
    # K = 9
    assert sep(s, 0, 9, 2) != 0
    assert "more than 8 terms" in _last_error()
    assert _td_info(s) == ([0, 0, 0, 0], 0, 0)
    # a step past the table: two rows, the third step fails and says so, the state stays what the second step left
    assert sep(s, 0, 1, 2) == 0
    assert _td_info(s) == ([1, 0, 0, 0], 2, 0)
    for _ in range(2):
        L.check(lib.pg_solver_step(s._h, C.c_int32(0), C.byref(opts), C.byref(info)))
    x2 = s._fetch_state()
    assert _td_info(s) == ([1, 0, 0, 0], 2, 2)
    assert lib.pg_solver_step(s._h, C.c_int32(0), C.byref(opts), C.byref(info)) != 0
    msg = _last_error()
    assert "past the last row" in msg and "2 rows" in msg
    assert np.array_equal(s._fetch_state(), x2)
    # pg_solver_set_source on that slot clears it, and the loop goes on with the host's data
    f = np.full(M, 1.0)
    L.check(lib.pg_solver_set_source(s._h, 0, L.dptr(f), L.dptr(f)))
    assert _td_info(s) == ([0, 0, 0, 0], 0, 0)
    L.check(lib.pg_solver_step(s._h, C.c_int32(0), C.byref(opts), C.byref(info)))
    # a steady solver
    mesh = pj.Mesh((16, 16), (4.0, 4.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.2), mesh)
    st = pj.DiffusionSteadyMono(pj.Phase(cap, pj.DiffusionOps(cap), lambda x, y, z: 1.0, lambda x, y, z: 1.0),
                                pj.BorderConditions({k: pj.Dirichlet(0.0) for k in HEAT_BORDERS}), pj.Dirichlet(0.0))
    assert sep(st, 0, 1, 2) != 0
    assert "steady solver" in _last_error()
    # PG_TD_INTERFACE on a diphasic solver
    (sd, p1, p2, bcbd, ic), _, dtd = _diph_pair(pj, 16, lambda x, y, z, t: 0.0, lambda x, y, z, t: 0.0, "BE")
    L.check(lib.pg_solver_initial_solve(sd._h, C.byref(opts), C.byref(info)))
    assert sep(sd, 1, 1, 2) != 0
    assert "diphasic" in _last_error()
    assert sep(sd, 0, 1, 2) == 0                                  # (its sources are welcome)
    # unknown slot
    assert sep(s, 3, 1, 2) != 0 and "which" in _last_error()


def _host_data(ts, coords, t, M, nspace=3):
    v = api._eval(ts, coords, t, nspace)
    return np.full(M, v) if isinstance(v, float) else v


# sizes whose n_own is odd: the combine kernel moves two rows per access and one thread takes the odd last row
@pytest.mark.parametrize("N,n,c,r", [(2, 19, (2.01, 2.01), 1.5), (3, 9, (2.01, 2.01, 2.3), 1.3)])      # n_own = 323, 643
@pytest.mark.parametrize("scheme", ["BE", "CN"])
def test_combine_kernel_alone_against_k_bconst_fed_from_the_host(pj, N, n, c, r, scheme):
    """One step with the table cursor at row 0: the right-hand side of the run system, b = mass∘x + bconst, with bconst from the
    combine against bconst from k_bconst after pg_solver_set_source / _interface_value / _border_values with the same data
    evaluated on the host at the same two times.  Both start from the same state (the first solve), so b differs by the
    rounding of the two forms alone: <= 1e-12 max|b|, the bar of _check_system."""
    lib = L.lib()
    M = (n + 1) ** N
    f = pj.TimeSeparable([(lambda x, *_: 1.0 + 0.3 * x, lambda t: 1.0 + 7.0 * t), (COSX, lambda t: math.sin(40.0 * t)), (0.5, lambda t: t * t)])
    g = pj.TimeSeparable([(COSX, lambda t: 1.0 + t), (lambda x, y, *_: 0.2 * y, lambda t: math.cos(9.0 * t))])
    bv = pj.TimeSeparable([(lambda x, *_: 0.5 * x, lambda t: 1.0), (1.0, lambda t: 3.0 * t)])
    u0 = np.concatenate([0.2 * np.ones(M), np.ones(M)])
    dt = 0.4 * (4.0 / n) ** 2
    opts = api._krylov_opts("bicgstab", {"reltol": 1e-13})
    info = L.pg_step_info()
    sch = L.PG_SCHEME[scheme]
    b = {}
    for path in ("device", "host"):
        (s, ph, bcb, bci), _ = _mono_pair(pj, N, n, 4.0, c, r, pj.Dirichlet(g), po.Dirichlet(g), {k: pj.Dirichlet(bv) for k in HEAT_BORDERS},
                                          {k: po.Dirichlet(bv) for k in HEAT_BORDERS}, dt, u0, scheme, f=f)
        cap, mesh = ph.capacity, ph.capacity.mesh
        L.check(lib.pg_solver_initial_solve(s._h, C.byref(opts), C.byref(info)))
        t = 0.0 + dt
        if path == "device":
            table = lambda ts: api._separable_table(ts, dt, 3 * dt)
            api._install_separable(s, api._TD_SOURCE, 0, api._separable_fields(f, cap._cw, 3, M), table(f))
            api._install_separable(s, api._TD_INTERFACE, 0, api._separable_fields(g, cap._cg, 3, M), table(g))
            modes, coefs = api._separable_border(bcb, mesh)
            api._install_separable(s, api._TD_BORDER, 0, modes, table(coefs))
            assert _td_info(s) == ([3, 0, 2, 2], 3, 0)
        else:
            L.check(lib.pg_solver_set_source(s._h, 0, L.dptr(_host_data(f, cap._cw, t, M)), L.dptr(_host_data(f, cap._cw, t + dt, M))))
            L.check(lib.pg_solver_set_interface_value(s._h, L.dptr(_host_data(g, cap._cg, t, M)), L.dptr(_host_data(g, cap._cg, t + dt, M))))
            L.check(lib.pg_solver_set_border_values(s._h, L.dptr(api._border_values(bcb, mesh, t))))
        L.check(lib.pg_solver_step(s._h, C.c_int32(sch), C.byref(opts), C.byref(info)))
        s._have_run = True
        _, b[path], idx = s.system(1)
        if path == "device":
            assert _td_info(s)[2] == 1
            assert len(idx) % 2 == 1, f"n_own = {len(idx)}: choose a size with an odd number of rows"
    scale = np.max(np.abs(b["host"]))
    err = np.max(np.abs(b["device"] - b["host"]))
    print(f"combine alone N={N} n={n} {scheme}: n_own = {len(b['host'])}, max|b| = {scale:.3e}, max diff = {err:.3e}")
    assert scale > 0 and err <= 1e-12 * scale
