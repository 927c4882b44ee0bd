"""Device functions on the GPU (pj.DeviceFunction, pg_solver_set_program): a closure traced into a postfix program that a
kernel evaluates every step at the reference's points.  The evaluator alone on points against a long-double interpretation of
the same bytecode; the right-hand side after one step against k_bconst fed from the host with the same closure; every state
against the oracle's direct solves and against the product's own host-driven loop on the same closure; the two device branches
bit for bit; table discipline and the refusals of the raw C ABI."""
import ctypes as C

import numpy as np
import pytest

from oracle import penguin_oracle as po
from penguin.jl_amd import _lib as L
from penguin.jl_amd import api, devfn
from tests.common import oracle_capacity_from_product, rel_l2
from tests.device_function_cases import (EPS, all_opcodes_program, depth16_program, erf_ld, erfc_ld, full_length_program, raw_program,
                                         worst_rel_error)
from tests.test_gpu_parity import HEAT_BORDERS, TOL_T, _mono_pair, _velocity_fields

pytestmark = pytest.mark.gpu


def _last_error():
    buf = C.create_string_buffer(4096)
    L.lib().pg_last_error(buf, 4096)
    return buf.value.decode("utf-8", "replace")


def _device_eval(prog, pts, t):
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    out = np.full(len(pts), np.nan)
    L.check(L.lib().pg_debug_program_eval(C.byref(prog), C.c_int64(len(pts)), L.dptr(pts), C.c_double(t), L.dptr(out)))
    return out


def _host_eval(prog, pts, t):
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    out = np.full(len(pts), np.nan)
    L.check(L.lib().pg_program_eval_host(C.byref(prog), C.c_int64(len(pts)), L.dptr(pts), C.c_double(t), L.dptr(out)))
    return out


def _info(s):
    progs, entries = (C.c_int32 * 4)(), (C.c_int64 * 4)()
    nrows, cursor = C.c_int64(-1), C.c_int64(-1)
    L.check(L.lib().pg_solver_program_info(s._h, progs, entries, C.byref(nrows), C.byref(cursor)))
    return list(progs), list(entries), nrows.value, cursor.value


# ------------------------------------------------------------------------------------ 1. the evaluator on points
PROGRAMS = {
    "const": lambda: raw_program([("CONST", 0)], [0.3]),
    "t_only": lambda: devfn.DeviceFunction(lambda x, y, z, t: (t + 1.0) * t / 3.0 + np.sqrt(t)).program,
    "ninety_six": full_length_program,
    "depth_16": depth16_program,
    "every_opcode": all_opcodes_program,
}
_POINTS = np.random.default_rng(5).uniform(0.5, 1.5, size=(1000, 3))      # away from every zero and cancellation of the programs
_T = 0.375


@pytest.mark.parametrize("npts", [1, 63, 64, 65, 255, 256, 257, 1000])
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_evaluator_on_points_against_long_double(pj, name, npts):
    """Bar: on the same points, 4 x the worst relative error of the HOST float64 interpreter (pg_program_eval_host) against the
    long-double interpretation of the same bytecode -- device libm results may differ from glibc's by an ulp or two per call --
    and never less than nothing: where the host is exact (a constant, comparisons) the device has to be exact too."""
    prog = PROGRAMS[name]()
    if name == "ninety_six":
        assert prog.n_ops == 96
    pts = _POINTS[:npts]
    ref = devfn.interpret(prog, pts, _T, dtype=np.longdouble, erf_fn=erf_ld, erfc_fn=erfc_ld)
    host = _host_eval(prog, pts, _T)
    dev = _device_eval(prog, pts, _T)
    e_host, e_dev = worst_rel_error(host, ref), worst_rel_error(dev, ref)
    print(f"evaluator {name} npts={npts}: n_ops={prog.n_ops} host err {e_host:.3e} device err {e_dev:.3e} (bar {4 * e_host:.3e})")
    assert np.all(np.isfinite(dev))
    assert e_host <= 64 * EPS, "the reference itself left its own bar: inputs too close to a cancellation"
    assert e_dev <= 4 * e_host


# ------------------------------------------------------------------------------------ 2. the right-hand side after one step
def F_SRC(x, y, z, t):
    return (1.0 + 0.3 * x) * np.exp(-0.1 * ((x - 2.0) ** 2 + (y - 2.0) ** 2 + z * z) / (t + 1.0)) / (t + 1.0)


def G_INT(x, y, z, t):
    return 1.5 + np.cos(x) * np.exp(-t) + 0.1 * z


def B_2D(x, y, t):
    return 0.5 + 0.25 * x + np.sqrt(y + 1.0) * (t + 0.5)


def B_3D(x, y, z, t):
    return 0.5 + 0.25 * x + np.sqrt(y + 1.0) * (t + 0.5) + 0.1 * z


def _host_err_of(df, coords, times, nspace):
    """The host interpreter's worst relative error against long double at these points and times."""
    prog = df.program_for(nspace)
    pts = np.zeros((len(coords), 3))
    pts[:, :coords.shape[1]] = coords
    return max(worst_rel_error(_host_eval(prog, pts, t), devfn.interpret(prog, pts, t, dtype=np.longdouble, erf_fn=erf_ld,
                                                                        erfc_fn=erfc_ld)) for t in times)


def _host_data(fn, coords, t, M, nspace=3):
    v = api._eval(fn, coords, t, nspace)
    return np.full(M, v) if isinstance(v, float) else v


@pytest.mark.parametrize("N,n,c,r,scheme", [(2, 24, (2.01, 2.01), 1.7, "BE"), (2, 24, (2.01, 2.01), 1.7, "CN"),
                                            (2, 19, (2.01, 2.01), 1.5, "BE"), (2, 19, (2.01, 2.01), 1.5, "CN"),     # n_own = 323
                                            (3, 9, (2.01, 2.01, 2.3), 1.3, "CN"),                                  # n_own = 643
                                            (3, 12, (2.01, 2.01, 2.01), 1.3, "CN")])
def test_right_hand_side_after_one_step_against_k_bconst_fed_from_the_host(pj, N, n, c, r, scheme):
    """b = mass∘x + bconst of the first step of the run system: bconst from the programs against bconst from k_bconst after
    pg_solver_set_source / _interface_value / _border_values with the same closures evaluated by numpy at the same two times.
    A third solver fed zero data gives b without the data terms: the data terms are checked to be no larger than max|b|, which
    is what lets the bar be taken relative to max|b|.  Bar: the evaluator's bar (4 ε_host, ε_host
    the host interpreter's error against long double at these very points) plus the numpy side's own ε_host, times the number of
    evaluations the scheme adds (1 BE, 2 CN), plus ten roundings (five products and sums on either side)."""
    lib = L.lib()
    M = (n + 1) ** N
    f, g = pj.DeviceFunction(F_SRC), pj.DeviceFunction(G_INT)
    bv = pj.DeviceFunction(B_2D if N == 2 else B_3D)
    u0 = np.concatenate([0.2 * np.ones(M), np.ones(M)])
    dt = 0.4 * (4.0 / n) ** 2
    opts = api._krylov_opts("bicgstab", {"reltol": 1e-13})
    info = L.pg_step_info()
    sch = L.PG_SCHEME[scheme]
    b, eps_host = {}, 0.0
    for path in ("device", "host", "none"):
        (s, ph, bcb, bci), _ = _mono_pair(pj, N, n, 4.0, c, r, pj.Dirichlet(g), po.Dirichlet(g), {k: pj.Dirichlet(bv) for k in HEAT_BORDERS},
                                          {k: po.Dirichlet(bv) for k in HEAT_BORDERS}, dt, u0, scheme, f=f)
        cap, mesh = ph.capacity, ph.capacity.mesh
        L.check(lib.pg_solver_initial_solve(s._h, C.byref(opts), C.byref(info)))
        t = 0.0 + dt
        if path == "none":
            zero = np.zeros(M)
            L.check(lib.pg_solver_set_source(s._h, 0, L.dptr(zero), L.dptr(zero)))
            L.check(lib.pg_solver_set_interface_value(s._h, L.dptr(zero), L.dptr(zero)))
            L.check(lib.pg_solver_set_border_values(s._h, L.dptr(np.zeros(len(mesh._border_arrays()[2])))))
        elif path == "device":
            times = api._program_times(dt, 3 * dt, None)
            assert np.array_equal(times[0], [t, t + dt])
            api._install_program(s, api._TD_SOURCE, 0, f, 3, times)
            api._install_program(s, api._TD_INTERFACE, 0, g, 3, times)
            static, progs = api._program_border(bcb, mesh, False)
            assert np.all(static == 0.0) and len(progs) == 4
            L.check(lib.pg_solver_set_border_values(s._h, L.dptr(static)))
            for kval, df in progs:
                api._install_program(s, api._TD_BORDER, 0, df, N, times, key=kval)
            progs_n, entries, nrows, cursor = _info(s)
            assert progs_n == [1, 0, 1, 4] and nrows == 3 and cursor == 0 and min(entries[0], entries[2], entries[3]) > 0
            _, pos, _ = mesh._border_arrays()
            eps_host = max(_host_err_of(f, cap.C_ω, (t, t + dt), 3), _host_err_of(g, cap.C_γ, (t, t + dt), 3),
                           _host_err_of(bv, pos, (t,), N))
        else:
            L.check(lib.pg_solver_set_source(s._h, 0, L.dptr(_host_data(f, cap._cw, t, M)), L.dptr(_host_data(f, cap._cw, t + dt, M))))
            L.check(lib.pg_solver_set_interface_value(s._h, L.dptr(_host_data(g, cap._cg, t, M)), L.dptr(_host_data(g, cap._cg, t + dt, M))))
            L.check(lib.pg_solver_set_border_values(s._h, L.dptr(api._border_values(bcb, mesh, t))))
        L.check(lib.pg_solver_step(s._h, C.c_int32(sch), C.byref(opts), C.byref(info)))
        s._have_run = True
        _, b[path], idx = s.system(1)
    scale = np.max(np.abs(b["host"]))
    err = np.max(np.abs(b["device"] - b["host"])) / scale
    bar = (2 if scheme == "CN" else 1) * 5 * eps_host + 10 * EPS
    print(f"rhs alone N={N} n={n} {scheme}: n_own = {len(b['host'])}, max|b| = {scale:.3e}, eps_host = {eps_host:.3e}, "
          f"max diff / max|b| = {err:.3e} (bar {bar:.3e})")
    data = np.max(np.abs(b["host"] - b["none"]))
    assert 0 < data <= scale, (data, scale)
    assert err <= bar


def test_a_border_list_shorter_than_one_wave_and_a_key_without_cells(pj):
    """8 x 8 cells: every border key has fewer than 64 fixed rows.  A program on one key changes that key's rows alone; a key the
    2-D mesh does not have (forward) lists nothing and launches nothing."""
    lib = L.lib()
    n, N = 8, 2
    M = (n + 1) ** 2
    bv = pj.DeviceFunction(B_2D)
    u0 = np.concatenate([0.2 * np.ones(M), np.ones(M)])
    dt = 0.4 * (4.0 / n) ** 2
    opts = api._krylov_opts("bicgstab", {"reltol": 1e-13})
    info = L.pg_step_info()
    b = {}
    for path in ("device", "host"):
        borders = {k: pj.Dirichlet(bv if k == "left" else 0.25) for k in HEAT_BORDERS}
        (s, ph, bcb, bci), _ = _mono_pair(pj, N, n, 4.0, (2.01, 2.01), 1.2, pj.Dirichlet(1.0), po.Dirichlet(1.0), borders,
                                          {k: po.Dirichlet(0.25) for k in HEAT_BORDERS}, dt, u0, "BE")
        mesh = ph.capacity.mesh
        L.check(lib.pg_solver_initial_solve(s._h, C.byref(opts), C.byref(info)))
        if path == "device":
            times = api._program_times(dt, 2 * dt, None)
            static, progs = api._program_border(bcb, mesh, False)
            assert [k for k, _ in progs] == [L.PG_KEY["left"]]
            L.check(lib.pg_solver_set_border_values(s._h, L.dptr(static)))
            api._install_program(s, api._TD_BORDER, 0, bv, N, times, key=L.PG_KEY["forward"])
            progs_n, entries, _, _ = _info(s)
            assert progs_n == [0, 0, 0, 1] and entries[3] == 0, (progs_n, entries)      # the key without cells, alone: no entry
            api._install_program(s, api._TD_BORDER, 0, bv, N, times, key=progs[0][0])
            progs_n, entries, _, _ = _info(s)
            assert progs_n == [0, 0, 0, 2] and 0 < entries[3] < 64, entries
        else:
            L.check(lib.pg_solver_set_border_values(s._h, L.dptr(api._border_values(bcb, mesh, dt))))
        L.check(lib.pg_solver_step(s._h, C.c_int32(0), C.byref(opts), C.byref(info)))
        s._have_run = True
        _, b[path], _ = s.system(1)
    scale = np.max(np.abs(b["host"]))
    err = np.max(np.abs(b["device"] - b["host"])) / scale
    print(f"short border list: {entries[3]} entries, max diff / max|b| = {err:.3e}")
    assert err <= 5 * 4 * EPS + 10 * EPS       # (sqrt, products and sums only: ε_host is a few roundings)


# ------------------------------------------------------------------------------------ 3. states
def _case1_pair(pj, scheme0, f, g, bv, n=24, r=1.7, N=2, c=(2.01, 2.01)):
    M = (n + 1) ** N
    D = lambda x, y, z: 1.0 + 0.3 * x + 0.1 * y
    u0 = np.concatenate([0.2 * np.ones(M), np.ones(M)])
    dt = 0.4 * (4.0 / n) ** 2
    pair = _mono_pair(pj, N, n, 4.0, c, r, pj.Dirichlet(g), po.Dirichlet(g), {k: pj.Dirichlet(bv) for k in HEAT_BORDERS},
                      {k: po.Dirichlet(bv) for k in HEAT_BORDERS}, dt, u0, scheme0, f=f, D=D)
    return pair, dt


_CASE1 = {}


def _case1(pj, scheme0, scheme):
    """The oracle's states, the device loop's (per-step branch) and the host-driven loop's on the same closures, once."""
    key = (scheme0, scheme)
    if key not in _CASE1:
        f, g, bv = pj.DeviceFunction(F_SRC), pj.DeviceFunction(G_INT), pj.DeviceFunction(B_2D)
        ((s, ph, bcb, bci), (so, oph, obcb, obci)), dt = _case1_pair(pj, scheme0, f, g, bv)
        pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 6 * dt, bcb, bci, scheme, reltol=1e-13)
        po.solve_DiffusionUnsteadyMono(so, oph, dt, 6 * dt, obcb, obci, scheme, method="\\")
        ((sh, phh, bcbh, bcih), _), dt = _case1_pair(pj, scheme0, F_SRC, G_INT, B_2D)
        pj.solve_DiffusionUnsteadyMono_b(sh, phh, dt, 6 * dt, bcbh, bcih, scheme, reltol=1e-13)
        _CASE1[key] = dict(time_data=s.time_data, host_time_data=sh.time_data, states=[x.copy() for x in s.states],
                           oracle=[np.array(x) for x in so.states], host=[x.copy() for x in sh.states], info=_info(s), dt=dt)
    return _CASE1[key]


SCHEMES = [("BE", "BE"), ("BE", "CN"), ("CN", "CN")]


def _against_host_loop(what, s, sh):
    """The device run `s` against the host-driven loop `sh` on the same closures, unwrapped: state for state at the suite's bar."""
    assert s.time_data == "device" and sh.time_data == "host"
    errs = [rel_l2(a, b) for a, b in zip(s.states, sh.states)]
    print(what, "rel L2 against the host-driven loop per state:", errs)
    assert len(s.states) == len(sh.states) and max(errs) <= TOL_T


@pytest.mark.parametrize("scheme0,scheme", SCHEMES)
def test_mono_2d_states_against_the_oracle_and_the_host_driven_loop(pj, scheme0, scheme):
    c = _case1(pj, scheme0, scheme)
    assert c["time_data"] == "device" and c["host_time_data"] == "host"
    assert c["info"][0] == [1, 0, 1, 4] and c["info"][2:] == (6, 6)
    assert len(c["states"]) == len(c["oracle"]) == len(c["host"]) == 7
    errs = [rel_l2(a, b) for a, b in zip(c["states"], c["oracle"])]
    errs_h = [rel_l2(a, b) for a, b in zip(c["states"], c["host"])]
    print("mono 2-D", scheme0, scheme, "rel L2 against the oracle per state:", errs)
    print("mono 2-D", scheme0, scheme, "rel L2 against the host-driven loop per state:", errs_h)
    assert max(errs) <= TOL_T and max(errs_h) <= TOL_T


@pytest.mark.parametrize("scheme0,scheme", SCHEMES)
def test_run_and_per_step_branch_agree_bit_for_bit_and_runs_repeat(pj, scheme0, scheme):
    """pg_solver_run (save_states=False) against the per-step branch, and the same run twice: no atomics anywhere, the same bits."""
    c = _case1(pj, scheme0, scheme)
    finals = []
    for _ in range(2):
        f, g, bv = pj.DeviceFunction(F_SRC), pj.DeviceFunction(G_INT), pj.DeviceFunction(B_2D)
        ((s, ph, bcb, bci), _), dt = _case1_pair(pj, scheme0, f, g, bv)
        pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 6 * dt, bcb, bci, scheme, reltol=1e-13, save_states=False)
        assert s.time_data == "device" and s.last_run.steps == 6
        finals.append(s.x.copy())
    assert np.array_equal(finals[0], finals[1])
    assert np.array_equal(finals[0], c["states"][-1])


@pytest.mark.parametrize("scheme", ["BE", "CN"])
def test_late_switch_reaches_the_solve_at_the_right_step(pj, scheme):
    """A source that switches on after 3.5 Δt (a comparison and a select): an off-by-one in the table's rows shows against the oracle."""
    n = 20
    M = (n + 1) ** 2
    dt = 0.4 * (4.0 / n) ** 2
    plain = (lambda x, y, z, t: pj.dev.select(t > 3.5 * dt, 2.0 + 0.1 * x, 0.0), lambda x, y, z, t: pj.dev.select(t < 5.5 * dt, 1.0, 1.5),
             lambda x, y, t: x * t)
    f, g, bv = (pj.DeviceFunction(fn) for fn in plain)
    u0 = np.concatenate([0.1 * np.ones(M), np.ones(M)])
    borders = lambda mod, v: {k: mod.Dirichlet(v) for k in HEAT_BORDERS}
    (s, ph, bcb, bci), (so, oph, obcb, obci) = _mono_pair(
        pj, 2, n, 4.0, (2.01, 2.01), 1.6, pj.Dirichlet(g), po.Dirichlet(g), borders(pj, bv), borders(po, bv), dt, u0, scheme, f=f)
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 8 * dt, bcb, bci, scheme, reltol=1e-13)
    po.solve_DiffusionUnsteadyMono(so, oph, dt, 8 * dt, obcb, obci, scheme, method="\\")
    assert s.time_data == "device" and len(s.states) == len(so.states)
    errs = [rel_l2(a, b) for a, b in zip(s.states, so.states)]
    print("late switch", scheme, errs)
    assert max(errs) <= TOL_T
    (sh, phh, bcbh, bcih), _ = _mono_pair(pj, 2, n, 4.0, (2.01, 2.01), 1.6, pj.Dirichlet(plain[1]), po.Dirichlet(plain[1]),
                                          borders(pj, plain[2]), borders(po, plain[2]), dt, u0, scheme, f=plain[0])
    pj.solve_DiffusionUnsteadyMono_b(sh, phh, dt, 8 * dt, bcbh, bcih, scheme, reltol=1e-13)
    _against_host_loop(f"late switch {scheme}", s, sh)
    f0 = pj.DeviceFunction(lambda x, y, z, t: 0.0 * t)
    (s0, ph0, bcb0, bci0), _ = _mono_pair(
        pj, 2, n, 4.0, (2.01, 2.01), 1.6, pj.Dirichlet(g), po.Dirichlet(g), borders(pj, bv), borders(po, bv), dt, u0, scheme, f=f0)
    pj.solve_DiffusionUnsteadyMono_b(s0, ph0, dt, 8 * dt, bcb0, bci0, scheme, reltol=1e-13)
    assert s0.time_data == "device" and rel_l2(s0.x, s.x) > 1e-3      # the late data did matter


def test_mono_3d_cn(pj):
    n = 12
    f, g, bv = pj.DeviceFunction(F_SRC), pj.DeviceFunction(G_INT), pj.DeviceFunction(B_3D)
    ((s, ph, bcb, bci), (so, oph, obcb, obci)), dt = _case1_pair(pj, "CN", f, g, bv, n=n, r=1.3, N=3, c=(2.01, 2.01, 2.01))
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 4 * dt, bcb, bci, "CN", reltol=1e-13)
    po.solve_DiffusionUnsteadyMono(so, oph, dt, 4 * dt, obcb, obci, "CN", method="\\")
    assert s.time_data == "device"
    errs = [rel_l2(a, b) for a, b in zip(s.states, so.states)]
    print("mono 3-D CN", errs)
    assert len(s.states) == len(so.states) and max(errs) <= TOL_T
    ((sh, phh, bcbh, bcih), _), dt = _case1_pair(pj, "CN", F_SRC, G_INT, B_3D, n=n, r=1.3, N=3, c=(2.01, 2.01, 2.01))
    pj.solve_DiffusionUnsteadyMono_b(sh, phh, dt, 4 * dt, bcbh, bcih, "CN", reltol=1e-13)
    _against_host_loop("mono 3-D CN", s, sh)


def _diph_pair(pj, n, f1, f2, scheme0):
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
def test_diphasic_sources_of_both_phases(pj, scheme0, scheme):
    plain = (lambda x, y, z, t: 1.0 + t + x * np.sin(3.0 * t), lambda x, y, z, t: (0.5 + 0.1 * y) * np.cos(2.0 * t))
    f1, f2 = pj.DeviceFunction(plain[0]), pj.DeviceFunction(plain[1])
    (s, p1, p2, bcb, ic), (so, q1, q2, obcb, oic), dt = _diph_pair(pj, 16, f1, f2, scheme0)
    pj.solve_DiffusionUnsteadyDiph_b(s, p1, p2, dt, 5 * dt, bcb, ic, scheme, reltol=1e-13)
    po.solve_DiffusionUnsteadyDiph(so, q1, q2, dt, 5 * dt, obcb, oic, scheme, method="\\")
    assert s.time_data == "device"
    progs, entries, nrows, cursor = _info(s)
    assert progs == [1, 1, 0, 0] and entries[0] > 0 and entries[1] > 0 and (nrows, cursor) == (5, 5)
    errs = [rel_l2(a, b) for a, b in zip(s.states, so.states)]
    print("diph", scheme0, scheme, errs)
    assert len(s.states) == len(so.states) and max(errs) <= TOL_T
    (s2, p1, p2, bcb, ic), _, dt = _diph_pair(pj, 16, f1, f2, scheme0)
    pj.solve_DiffusionUnsteadyDiph_b(s2, p1, p2, dt, 5 * dt, bcb, ic, scheme, reltol=1e-13, save_states=False)
    assert s2.time_data == "device" and s2.last_run.steps == 5
    assert np.array_equal(s2.x, s.states[-1])
    (sh, p1, p2, bcb, ic), _, dt = _diph_pair(pj, 16, plain[0], plain[1], scheme0)
    pj.solve_DiffusionUnsteadyDiph_b(sh, p1, p2, dt, 5 * dt, bcb, ic, scheme, reltol=1e-13)
    _against_host_loop(f"diph {scheme0} {scheme}", s, sh)


def test_advection_diffusion_mono_be(pj):
    n, N = 16, 2
    M = (n + 1) ** 2
    mesh, omesh = pj.Mesh((n, n), (4.0, 4.0)), po.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0), mesh)
    ocap = oracle_capacity_from_product(cap, omesh)
    u, ug = _velocity_fields(cap, N, M)
    op, oop = pj.ConvectionOps(cap, u, ug), po.make_convection_ops(ocap, u, ug)
    plain = lambda x, y, z, t: (1.0 + 0.2 * x) * (1.0 + 20.0 * t) + np.sin(30.0 * t)
    f = pj.DeviceFunction(plain)
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
    phh = pj.Phase(cap, op, plain, D)
    sh = pj.AdvectionDiffusionUnsteadyMono(phh, bcb, pj.Robin(1.0, 0.5, 1.0), dt, u0, "BE")
    pj.solve_AdvectionDiffusionUnsteadyMono_b(sh, phh, dt, 5 * dt, bcb, pj.Robin(1.0, 0.5, 1.0), "BE", reltol=1e-13)
    _against_host_loop("advection-diffusion BE", s, sh)


def test_darcy_flow_unsteady_with_a_pressure_ramp_on_one_border(pj):
    n = 16
    M = (n + 1) ** 2
    mesh, omesh = pj.Mesh((n, n), (4.0, 4.0)), po.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0, complement=True), mesh)
    ocap = oracle_capacity_from_product(cap, omesh)
    zero, zero_o = (lambda x, y, z=0.0: 0.0), (lambda x, y, z=0.0, t=0.0: 0.0)      # (the oracle calls its source with t)
    one = lambda x, y, z=0.0: 1.0
    plain = lambda x, y, t: 10.0 + np.minimum(4.0 * t, 3.0) + 0.5 * y
    ramp = pj.DeviceFunction(plain)
    ph, oph = pj.Phase(cap, pj.DiffusionOps(cap), zero, one), po.Phase(ocap, po.make_diffusion_ops(ocap), zero_o, one)
    bcb = pj.BorderConditions({"left": pj.Dirichlet(ramp), "right": pj.Dirichlet(20.0)})
    obcb = po.BorderConditions({"left": po.Dirichlet(ramp), "right": po.Dirichlet(20.0)})
    dt = 0.5 * (4.0 / n) ** 2
    p0 = np.linspace(10.0, 20.0, 2 * M)
    s = pj.DarcyFlowUnsteady(ph, bcb, pj.Neumann(0.0), dt, p0, "BE")
    pj.solve_DarcyFlowUnsteady_b(s, ph, dt, 4 * dt, bcb, pj.Neumann(0.0), "BE", reltol=1e-13)
    so = po.DiffusionUnsteadyMono(oph, obcb, po.Neumann(0.0), dt, p0, "BE")
    po.solve_DiffusionUnsteadyMono(so, oph, dt, 4 * dt, obcb, po.Neumann(0.0), "BE", method="\\")
    assert s.time_data == "device" and _info(s)[0] == [0, 0, 0, 1]
    errs = [rel_l2(a, b) for a, b in zip(s.states, so.states)]
    print("DarcyFlowUnsteady:", errs)
    assert len(s.states) == len(so.states) == 5 and max(errs) <= TOL_T
    bcbh = pj.BorderConditions({"left": pj.Dirichlet(plain), "right": pj.Dirichlet(20.0)})
    sh = pj.DarcyFlowUnsteady(ph, bcbh, pj.Neumann(0.0), dt, p0, "BE")
    pj.solve_DarcyFlowUnsteady_b(sh, ph, dt, 4 * dt, bcbh, pj.Neumann(0.0), "BE", reltol=1e-13)
    _against_host_loop("DarcyFlowUnsteady", s, sh)


def test_mixed_call_separable_source_program_interface_and_border(pj):
    f = pj.TimeSeparable([(1.0, lambda t: 1.0), (lambda x, *_: x, lambda t: t)])
    g, bv = pj.DeviceFunction(G_INT), pj.DeviceFunction(B_2D)
    ((s, ph, bcb, bci), (so, oph, obcb, obci)), dt = _case1_pair(pj, "BE", f, g, bv)
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 5 * dt, bcb, bci, "CN", reltol=1e-13)
    po.solve_DiffusionUnsteadyMono(so, oph, dt, 5 * dt, obcb, obci, "CN", method="\\")
    assert s.time_data == "device" and _info(s)[0] == [0, 0, 1, 4]
    terms = (C.c_int32 * 4)()
    L.check(L.lib().pg_solver_time_data_info(s._h, terms, None, None))
    assert list(terms) == [2, 0, 0, 0]
    errs = [rel_l2(a, b) for a, b in zip(s.states, so.states)]
    print("mixed call", errs)
    assert len(s.states) == len(so.states) and max(errs) <= TOL_T
    ((sh, phh, bcbh, bcih), _), dt = _case1_pair(pj, "BE", lambda x, y, z, t: 1.0 + x * t, G_INT, B_2D)      # (f, written out)
    pj.solve_DiffusionUnsteadyMono_b(sh, phh, dt, 5 * dt, bcbh, bcih, "CN", reltol=1e-13)
    _against_host_loop("mixed call", s, sh)


# ------------------------------------------------------------------------------------ 4. loop behaviour
def test_monitors_save_every_and_mg_step_on_a_device_function_run(pj):
    c = _case1(pj, "BE", "BE")
    f, g, bv = pj.DeviceFunction(F_SRC), pj.DeviceFunction(G_INT), pj.DeviceFunction(B_2D)
    ((s, ph, bcb, bci), _), dt = _case1_pair(pj, "BE", f, g, bv)
    w = np.random.default_rng(3).uniform(0.5, 1.5, size=len(c["states"][0]))
    mon = pj.Monitor(w, name="weighted sum")
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 6 * dt, bcb, bci, "BE", reltol=1e-13, monitors=[mon], save_every=2, save_states=False)
    assert s.time_data == "device" and s.state_steps == [0, 2, 4, 6] and s.monitor_series.shape == (7, 1)
    for k, x in zip(s.state_steps, s.states):
        assert np.array_equal(x, c["states"][k])
    want = np.array([np.dot(w, x) for x in c["states"]])      # (positive weights and states: nothing cancels)
    assert np.allclose(s.monitor_series[:, 0], want, rtol=1e-12, atol=0.0)
    ((s2, ph2, bcb2, bci2), _), dt = _case1_pair(pj, "BE", f, g, bv)
    pj.solve_DiffusionUnsteadyMono_b(s2, ph2, dt, 6 * dt, bcb2, bci2, "BE", reltol=1e-12, precond="mg-step")
    assert s2.time_data == "device" and s2.unconverged == 0
    errs = [rel_l2(a, b) for a, b in zip(s2.states, c["oracle"])]
    print("mg-step on a DeviceFunction run:", errs)
    assert max(errs) <= TOL_T


# ------------------------------------------------------------------------------------ 5. table discipline and refusals
def _product_mono(pj, n, r):
    M = (n + 1) ** 2
    mesh = pj.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), r), mesh)
    ph = pj.Phase(cap, pj.DiffusionOps(cap), lambda x, y, z: 1.0, lambda x, y, z: 1.0)
    bcb, bci = pj.BorderConditions({k: pj.Dirichlet(0.25) for k in HEAT_BORDERS}), pj.Dirichlet(0.5)
    dt = 0.4 * (4.0 / n) ** 2
    return pj.DiffusionUnsteadyMono(ph, bcb, bci, dt, np.concatenate([0.2 * np.ones(M), np.ones(M)]), "BE"), ph, bcb, bci, dt


def test_table_discipline_and_refusals_through_the_raw_abi(pj):
    lib = L.lib()
    s, ph, bcb, bci, dt = _product_mono(pj, 16, 1.2)
    M = 17 * 17
    opts = api._krylov_opts("bicgstab", {"reltol": 1e-12})
    info = L.pg_step_info()
    prog = pj.DeviceFunction(F_SRC).program
    times = np.array([[dt, 2 * dt], [2 * dt, 3 * dt]])
    put = lambda sol, which, p=prog, phase=0, nrows=2: lib.pg_solver_set_program(sol._h, C.c_int32(which), C.c_int32(phase), C.byref(p),
                                                                                   C.c_int64(nrows), L.dptr(times))
    # before the first solve the constructor's system is the host's
    assert put(s, 0) != 0 and "pg_solver_initial_solve" in _last_error()
    L.check(lib.pg_solver_initial_solve(s._h, C.byref(opts), C.byref(info)))
    # an invalid program is refused with the validator's message, and nothing is installed
    bad = raw_program([("VAR", 0), ("ADD", 0)], [])
    assert put(s, 0, bad) != 0 and "invalid program" in _last_error() and "underflow" in _last_error()
    assert put(s, 0, prog, 0, 0) != 0 and "table row" in _last_error()
    assert _info(s) == ([0, 0, 0, 0], [0, 0, 0, 0], 0, 0)
    # a step past the table: two rows, the third step fails and says so, the state stays what the second step left
    assert put(s, 0) == 0
    assert _info(s)[0] == [1, 0, 0, 0] and _info(s)[2:] == (2, 0)
    for _ in range(2):
        L.check(lib.pg_solver_step(s._h, C.c_int32(0), C.byref(opts), C.byref(info)))
    x2 = s._fetch_state()
    assert _info(s)[2:] == (2, 2)
    assert lib.pg_solver_step(s._h, C.c_int32(0), C.byref(opts), C.byref(info)) != 0
    msg = _last_error()
    assert "past the last row" in msg and "2 rows" in msg
    assert np.array_equal(s._fetch_state(), x2)
    # installing rewinds the cursor; separable terms and a program replace one another in a slot
    assert put(s, 0) == 0 and _info(s)[2:] == (2, 0)
    modes, table = np.ones((1, M)), np.ones((2, 2, 1))
    L.check(lib.pg_solver_set_separable(s._h, C.c_int32(0), C.c_int32(0), C.c_int32(1), L.dptr(modes), C.c_int64(2), L.dptr(table)))
    assert _info(s)[0] == [0, 0, 0, 0]
    assert put(s, 0) == 0
    terms = (C.c_int32 * 4)()
    L.check(lib.pg_solver_time_data_info(s._h, terms, None, None))
    assert list(terms) == [0, 0, 0, 0] and _info(s)[0] == [1, 0, 0, 0]
    # pg_solver_set_source on that slot clears it, and the loop goes on with the host's data; pg_solver_clear_separable too
    f = np.full(M, 1.0)
    L.check(lib.pg_solver_set_source(s._h, 0, L.dptr(f), L.dptr(f)))
    assert _info(s) == ([0, 0, 0, 0], [0, 0, 0, 0], 0, 0)
    L.check(lib.pg_solver_step(s._h, C.c_int32(0), C.byref(opts), C.byref(info)))
    assert put(s, 1) == 0 and put(s, 2) == 0 and _info(s)[0] == [0, 0, 1, 1]
    L.check(lib.pg_solver_set_interface_value(s._h, L.dptr(f), L.dptr(f)))
    assert _info(s)[0] == [0, 0, 0, 1]
    L.check(lib.pg_solver_clear_separable(s._h, C.c_int32(2), C.c_int32(0)))
    assert _info(s)[0] == [0, 0, 0, 0]
    assert put(s, 2) == 0
    _, _, key = ph.capacity.mesh._border_arrays()
    L.check(lib.pg_solver_set_border_values(s._h, L.dptr(np.zeros(len(key)))))
    assert _info(s)[0] == [0, 0, 0, 0]
    # unknown slot, a source of a phase the solver has not
    assert put(s, 3) != 0 and "which" in _last_error()
    assert put(s, 0, prog, 1) != 0 and "phase" in _last_error()
    assert lib.pg_solver_set_border_program(s._h, C.c_int32(9), C.byref(prog), C.c_int64(2), L.dptr(times)) != 0 and "PG_KEY" in _last_error()
    # a steady solver
    mesh = pj.Mesh((16, 16), (4.0, 4.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.2), mesh)
    st = pj.DiffusionSteadyMono(pj.Phase(cap, pj.DiffusionOps(cap), lambda x, y, z: 1.0, lambda x, y, z: 1.0),
                                pj.BorderConditions({k: pj.Dirichlet(0.0) for k in HEAT_BORDERS}), pj.Dirichlet(0.0))
    assert put(st, 0) != 0 and "steady solver" in _last_error()
    # PG_TD_INTERFACE on a diphasic solver; its sources are welcome
    (sd, p1, p2, bcbd, ic), _, dtd = _diph_pair(pj, 16, lambda x, y, z, t: 0.0, lambda x, y, z, t: 0.0, "BE")
    L.check(lib.pg_solver_initial_solve(sd._h, C.byref(opts), C.byref(info)))
    assert put(sd, 1) != 0 and "diphasic" in _last_error()
    assert put(sd, 0, prog, 1) == 0


def test_a_solver_behind_a_communicator_is_refused():
    """The one-rank refusal (`ctx().nranks == 1 && !ctx().comm`) through its communicator half: a 1-rank RCCL communicator on one
    GPU, in a fresh child process (the library is initialised once per process), as tests/test_gpu_rccl.py does.  The child
    installs through both entry points after the first solve and checks message and emptiness itself.  (The virtual-rank half
    builds its solvers inside pg_debug_run_virtual_ranks: no handle of one reaches the ABI from outside.)"""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    env = {**os.environ, "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    r = subprocess.run([sys.executable, str(root / "scripts" / "device_function_rank_refusal.py")], cwd=root, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "one rank only" in r.stdout


def test_moving_and_stefan_solvers_are_refused(pj):
    from tests.test_gpu_liquid import _hip_cap

    lib = L.lib()
    prog = pj.DeviceFunction(F_SRC).program
    times = np.array([[0.1, 0.2]])
    put = lambda sol: lib.pg_solver_set_program(sol._h, C.c_int32(0), C.c_int32(0), C.byref(prog), C.c_int64(1), L.dptr(times))
    one = lambda x, y, z: 1.0
    mesh = pj.Mesh((16, 16), (4.0, 4.0), (0.0, 0.0))
    cen, rad = (lambda t: (2.01 + 0.8 * t, 1.97 - 0.5 * t)), (lambda t: 1.0 + 0.4 * t)
    body = pj.MovingSphere(cen, rad, False, dcenter=lambda t: (0.8, -0.5), dradius=lambda t: 0.4)
    cap0 = pj.Capacity(body, pj.SpaceTimeMesh(mesh, [0.0, 0.05]))
    phm = pj.Phase(cap0, pj.DiffusionOps(cap0), lambda x, y, z, t=0.0: 0.0, one)
    bcbm = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in HEAT_BORDERS})
    sm = pj.MovingDiffusionUnsteadyMono(phm, bcbm, pj.Dirichlet(1.0), 0.05, np.ones(2 * 17 * 17), mesh, "BE")
    assert put(sm) != 0 and "moving-body" in _last_error()
    nx = 32
    mesh1 = pj.Mesh((nx,), (1.0,), (0.0,))
    M, dt, t0 = nx + 1, 0.005, 0.01
    c1 = _hip_cap(pj, mesh1, 0.4513, 0.4702, t0, t0 + dt, False)
    c2 = _hip_cap(pj, mesh1, 0.4513, 0.4702, t0, t0 + dt, False, True)
    src = lambda x, y, z, t: 0.3
    p1, p2 = pj.Phase(c1, pj.DiffusionOps(c1), src, one), pj.Phase(c2, pj.DiffusionOps(c2), src, one)
    ic = pj.InterfaceConditions(pj.ScalarJump(1.0, 1.0, 0.0), pj.FluxJump(1.0, 1.0, 2.0))
    bcb = pj.BorderConditions({"bottom": pj.Dirichlet(1.0), "top": pj.Dirichlet(-0.5)})
    ss = pj.MovingLiquidDiffusionUnsteadyDiph(p1, p2, bcb, ic, dt, np.ones(4 * M), mesh1, "BE")
    assert put(ss) != 0 and "Stefan" in _last_error()


def test_one_plain_closure_sends_the_whole_call_to_the_host_loop(pj):
    f, bv = pj.DeviceFunction(F_SRC), pj.DeviceFunction(B_2D)
    ((s, ph, bcb, bci), (so, oph, obcb, obci)), dt = _case1_pair(pj, "BE", f, G_INT, bv)
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 3 * dt, bcb, bci, "CN", reltol=1e-13)
    po.solve_DiffusionUnsteadyMono(so, oph, dt, 3 * dt, obcb, obci, "CN", method="\\")
    assert s.time_data == "host" and _info(s)[0] == [0, 0, 0, 0]
    errs = [rel_l2(a, b) for a, b in zip(s.states, so.states)]
    assert len(s.states) == len(so.states) and max(errs) <= TOL_T
    # a TimeSeparable on one border and a DeviceFunction on another do not fit the one border slot: the host loop, and it says so
    borders = {k: pj.Dirichlet(bv if k == "left" else pj.TimeSeparable([(1.0, lambda t: t)])) for k in HEAT_BORDERS}
    M = 25 * 25
    (s, ph, bcb, bci), _ = _mono_pair(pj, 2, 24, 4.0, (2.01, 2.01), 1.7, pj.Dirichlet(1.0), po.Dirichlet(1.0), borders,
                                      {k: po.Dirichlet(0.0) for k in HEAT_BORDERS}, dt, np.concatenate([0.2 * np.ones(M), np.ones(M)]), "BE")
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 2 * dt, bcb, bci, "BE", reltol=1e-13)
    assert s.time_data == "host"
