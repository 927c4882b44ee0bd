"""GPU tests of moving traced level sets: Capacity(DeviceFunction(lambda x, y, t: ...), SpaceTimeMesh(...)) through
pg_capacity_create_spacetime_program.

* capacities against the numpy restatement of the slab rule on the host build of the same header
  (tests/spacetime_program_reference.py), with the bars stated there; B and W against the restatement taken at the product's C_ω;
* the disc and the 1-D wall as programs against MovingSphere / MovingHalfSpace through the product;
* analytic checks no restatement shares; bitwise repeatability;
* the four moving drivers fed to the oracle's literal algebra on the product's capacities, 1 + 4 slabs, 1e-10;
* every refusal of the entry."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import penguin_oracle as po
from oracle import spacetime as ost
from tests import levelset_cases as lc
from tests import spacetime_program_reference as sr
from tests.common import rel_l2
from tests.test_gpu_moving import _oracle_cap

pytestmark = pytest.mark.gpu
TOL_T = 1e-10
T0, DT = sr.T0, sr.DT


@functools.lru_cache(maxsize=None)
def _hostlib():
    return sr.build_host_lib()


def _product(pj, name, nq, t0=T0, t1=T0 + DT):
    fn, comp, n, L, x0 = sr.CASES[name]
    panels, order = sr.RULES[nq]
    mesh = pj.Mesh(n, L, x0)
    body = pj.DeviceFunction(fn, complement=comp)
    return pj.Capacity(body, pj.SpaceTimeMesh(mesh, [t0, t1]), time_panels=panels, time_order=order), body


# ------------------------------------------------------------------------------------ capacities against the restatement
# nq = 3: fewer nodes than the two face lanes plus one; 64: one node per lane; 80: the strided second pass of the node loop
@pytest.mark.parametrize("name,nq", [("ellipse", 3), ("ellipse", 64), ("ellipse", 80), ("ellipse_complement", 64),
                                     ("superellipse", 64), ("wavy_wall", 64), ("approaching_discs", 64), ("wall", 3), ("wall", 64), ("wall", 80)])
def test_capacities_match_the_restatement(pj, name, nq):
    fn, comp, n, L, x0 = sr.CASES[name]
    cap, body = _product(pj, name, nq)
    assert isinstance(cap, pj.SpaceTimeCapacity) and cap.body is body
    N, omesh = len(n), po.Mesh(n, L, x0)
    M = int(np.prod(omesh.ext))
    tau, wt = sr.time_rule(T0, T0 + DT, *sr.RULES[nq])
    assert len(tau) == nq
    # one run of the restatement: V, A, Γ, the types and the centroids are its own, B and W are taken at the product's C_ω
    ref = sr.slab_capacity(sr.HostMovingBody(_hostlib(), fn, N, comp), omesh, T0, T0 + DT, tau, wt, C_w=cap.C_ω_st)
    assert np.array_equal(cap.cell_types, ref.cell_types[:M])
    assert set(cap.cell_types) == {0.0, 1.0, -1.0}
    assert np.array_equal(np.flatnonzero(cap.Γ > 0), np.flatnonzero(ref.G[:M] > 0))
    sr.check(name, sr.Layer(cap, N, M), sr.Layer(ref, N, M), x0, L, n, DT, nq, what="gpu ")
    assert len(cap.A_st) == N + 1 and all(len(a) == 2 * M for a in cap.A_st)
    _, listed = cap.spacetime_kernel_ms
    ncut = int(np.count_nonzero(cap.cell_types == -1.0))
    assert ncut <= listed < int(np.prod(n))                           # the cheap pass did finish cells, and lost no cut cell


# ------------------------------------------------------------------------------------ against the closed-form kinds, through the product
def test_program_wall_against_moving_half_space(pj):
    """1-D: every quantity within 4 units (roots are bracketed to 2 ulp at each end), types identical"""
    fn, _, n, L, x0 = sr.CASES["wall"]
    mesh = pj.Mesh(n, L, x0)
    st = pj.SpaceTimeMesh(mesh, [T0, T0 + DT])
    a = pj.Capacity(pj.DeviceFunction(fn), st)
    b = pj.Capacity(pj.MovingHalfSpace(0, sr.WALL_POS, 1.0, dposition=sr.WALL_DPOS), st)
    assert np.array_equal(a.cell_types, b.cell_types)
    M = n[0] + 1
    r = sr.slab_ratios(sr.Layer(a, 1, M), sr.Layer(b, 1, M), x0, L, n, DT)
    print("[spacetime-program gpu wall vs MovingHalfSpace] " + "  ".join(f"{q} {r[q]:.3g}/4" for q in sr.QUANTITIES))
    assert all(r[q] <= 4.0 for q in sr.QUANTITIES), r


def test_program_disc_against_moving_sphere(pj):
    """2-D: the bars DESIGN.md section 23 records for Sphere (tests/levelset_cases.py "circle"), doubled; types identical"""
    fn, _, n, L, x0 = sr.CASES["disc"]
    mesh = pj.Mesh(n, L, x0)
    st = pj.SpaceTimeMesh(mesh, [T0, T0 + DT])
    a = pj.Capacity(pj.DeviceFunction(fn), st)
    b = pj.Capacity(pj.MovingSphere(sr.DISC_CEN, sr.DISC_RAD, False, dcenter=sr.DISC_DCEN, dradius=sr.DISC_DRAD), st)
    assert np.array_equal(a.cell_types, b.cell_types)
    M = int(np.prod([k + 1 for k in n]))
    sr.check("disc vs MovingSphere", sr.Layer(a, 2, M), sr.Layer(b, 2, M), x0, L, n, DT, 64, source=lc.BARS["circle"], what="gpu ")


# ------------------------------------------------------------------------------------ analytic checks
def test_rigid_rotation_keeps_the_area(pj):
    cap, _ = _product(pj, "ellipse", 64)
    area = np.pi * 1.1 * 0.6
    assert abs(cap.Vn_1.sum() - area) <= 1e-12 * area and abs(cap.Vn.sum() - area) <= 1e-12 * area


def test_growing_disc_volume_is_the_exact_integral(pj):
    """r(t) = 0.8 + 0.3 t: the integrand pi r^2 is a quadratic, the 16 x 4 rule integrates it exactly"""
    n, L, x0 = sr.MESH_B
    cap = pj.Capacity(pj.DeviceFunction(sr.growing_disc), pj.SpaceTimeMesh(pj.Mesh(n, L, x0), [T0, T0 + DT]))
    r0, r1 = 0.8 + 0.3 * T0, 0.8 + 0.3 * (T0 + DT)
    exact = np.pi * (r1 ** 3 - r0 ** 3) / 0.9
    assert abs(cap.V.sum() - exact) <= 1e-12 * exact


def test_faces_of_consecutive_slabs_and_two_builds_are_bitwise_equal(pj):
    t1 = T0 + DT
    a, _ = _product(pj, "ellipse", 64, T0, t1)
    b, _ = _product(pj, "ellipse", 64, t1, t1 + DT)
    assert np.array_equal(a.Vn, b.Vn_1) and np.count_nonzero((a.Vn > 0) & (a.Vn < a.Vn.max())) > 10
    c, _ = _product(pj, "ellipse", 64, T0, t1)
    for f in ("V", "Γ", "cell_types", "Vn_1", "Vn", "C_ω_st", "C_γ_st"):
        assert np.array_equal(getattr(a, f), getattr(c, f)), f
    for f in ("A", "B", "W"):
        assert all(np.array_equal(p, q) for p, q in zip(getattr(a, f), getattr(c, f))), f


# ------------------------------------------------------------------------------------ solves
HEAT_KEYS = ("left", "right", "top", "bottom")
F_SRC = lambda x, y, z, t: 0.3 + 0.2 * x + 0.5 * t
D_VAR = lambda x, y, z: 1.0 + 0.1 * x
G_INT = lambda x, y, z=0.0: 1.0 + 0.2 * x + 0.3 * y
B_VAL = lambda *a: 0.2 + 0.1 * a[-1]


def _compare_states(s, so, what):
    assert len(s.states) == len(so.states) == 5 and s.unconverged == 0
    nact = set()
    for k, (x, xo) in enumerate(zip(s.states, so.states)):
        assert np.array_equal(np.flatnonzero(x != 0.0), np.flatnonzero(xo != 0.0)), f"{what}: active set of state {k}"
        print(f"[spacetime-program solve {what}] state {k}: rel L2 {rel_l2(x, xo):.3e}")
        nact.add(int(np.count_nonzero(xo)))
    for k, (x, xo) in enumerate(zip(s.states, so.states)):
        assert rel_l2(x, xo) <= TOL_T, f"{what} state {k}: {rel_l2(x, xo):.2e}"
    return nact


@pytest.mark.parametrize("scheme", ["BE", "CN"])
def test_rotating_ellipse_mono_matches_the_oracle(pj, scheme):
    """the oracle's literal blocks and direct solves on the capacities the product computed, 1 + 4 slabs; the programs are traced
    once for the whole solve"""
    n, L, x0 = sr.MESH_A
    mesh, omesh = pj.Mesh(n, L, x0), po.Mesh(n, L, x0)
    M = int(np.prod(omesh.ext))
    calls = []

    def fn(x, y, t):
        calls.append(1)
        return sr.rotating_ellipse()(x, y, t)
    body = pj.DeviceFunction(fn)
    bc, obc = pj.Dirichlet(G_INT), po.Dirichlet(G_INT)
    bcb = pj.BorderConditions({k: pj.Dirichlet(B_VAL) for k in HEAT_KEYS})
    obcb = po.BorderConditions({k: po.Dirichlet(B_VAL) for k in HEAT_KEYS})
    Ti = np.random.default_rng(7).random(2 * M)
    cap0 = pj.Capacity(body, pj.SpaceTimeMesh(mesh, [0.0, DT]))
    ph = pj.Phase(cap0, pj.DiffusionOps(cap0), F_SRC, D_VAR)
    s = pj.MovingDiffusionUnsteadyMono(ph, bcb, bc, DT, Ti, mesh, scheme)
    pj.solve_MovingDiffusionUnsteadyMono_b(s, ph, body, DT, 0.0, 3.5 * DT, bcb, bc, mesh, scheme, method="bicgstab", reltol=1e-14)
    assert len(calls) == 1
    ocap0 = _oracle_cap(cap0, omesh, 0.0, DT)
    oph = po.Phase(ocap0, po.make_diffusion_ops(ocap0), F_SRC, D_VAR)
    so = ost.MovingDiffusionUnsteadyMono(oph, obcb, obc, DT, Ti, omesh, scheme)
    ost.solve_MovingDiffusionUnsteadyMono(
        so, oph, None, DT, 0.0, 3.5 * DT, obcb, obc, omesh, scheme,
        capacity_fn=lambda t0, t1: _oracle_cap(pj.Capacity(body, pj.SpaceTimeMesh(mesh, [t0, t1])), omesh, t0, t1))
    _compare_states(s, so, f"ellipse mono {scheme}")


def _diphasic(pj, mesh_spec, scheme, what, bar):
    """The ellipse and its complement, 1 + 4 slabs, as tests/test_gpu_moving.py::test_moving_diphasic_steps_match_oracle has it: the
    oracle's literal blocks on the product's capacities, every slab from the product's previous state, with its probe `sens` -- how
    far the ORACLE's own direct solution moves when its matrix entries move by one rounding error -- and the componentwise
    backward error of the product's state in the oracle's system.  bar(sens) is the bar of a state."""
    import scipy.sparse.linalg as spla
    n, L, x0 = mesh_spec
    mesh, omesh = pj.Mesh(n, L, x0), po.Mesh(n, L, x0)
    M = int(np.prod(omesh.ext))
    body = pj.DeviceFunction(sr.rotating_ellipse())
    body_c = pj.DeviceFunction(sr.rotating_ellipse(), complement=True)
    f2 = lambda x, y, z, t: 0.1 - 0.1 * x + 0.2 * t
    D2 = lambda x, y, z: 2.0
    gj, hj = (lambda x, y, z=0.0: 0.2 + 0.1 * x), (lambda x, y, z=0.0: 0.5 - 0.05 * x)
    ic = pj.InterfaceConditions(pj.ScalarJump(1.0, 0.5, gj), pj.FluxJump(1.0, 2.0, hj))
    oic = po.InterfaceConditions(po.ScalarJump(1.0, 0.5, gj), po.FluxJump(1.0, 2.0, hj))
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.3) for k in HEAT_KEYS})
    obcb = po.BorderConditions({k: po.Dirichlet(0.3) for k in HEAT_KEYS})
    Ti = np.random.default_rng(11).random(4 * M)
    caps = lambda t0, t1: tuple(pj.Capacity(b, pj.SpaceTimeMesh(mesh, [t0, t1])) for b in (body, body_c))
    c1, c2 = caps(0.0, DT)
    assert np.array_equal(c1.cell_types == -1.0, c2.cell_types == -1.0)
    p1, p2 = pj.Phase(c1, pj.DiffusionOps(c1), F_SRC, D_VAR), pj.Phase(c2, pj.DiffusionOps(c2), f2, D2)
    s = pj.MovingDiffusionUnsteadyDiph(p1, p2, bcb, ic, DT, Ti, mesh, scheme)
    pj.solve_MovingDiffusionUnsteadyDiph_b(s, p1, p2, body, body_c, DT, 3.5 * DT, bcb, ic, mesh, scheme, method="bicgstab", reltol=1e-14)
    k1, k2 = _oracle_cap(c1, omesh, 0.0, DT), _oracle_cap(c2, omesh, 0.0, DT)
    q1, q2 = po.Phase(k1, po.make_diffusion_ops(k1), F_SRC, D_VAR), po.Phase(k2, po.make_diffusion_ops(k2), f2, D2)
    so = ost.MovingDiffusionUnsteadyDiph(q1, q2, obcb, oic, DT, Ti, omesh, scheme)
    assert s.unconverged == 0 and len(s.states) == 5
    t, nact, worst = 0.0, set(), 0.0
    for k in range(5):
        if k > 0:
            t += DT
            j1, j2 = (_oracle_cap(c, omesh, t, t + DT) for c in caps(t, t + DT))
            o1, o2 = po.make_diffusion_ops(j1), po.make_diffusion_ops(j2)
            so.A = ost.A_diph_unstead_diff_moving(o1, o2, j1, j2, D_VAR, D2, oic, scheme)
            so.b = ost.b_diph_unstead_diff_moving(o1, o2, j1, j2, D_VAR, D2, F_SRC, f2, oic, s.states[k - 1], DT, t, scheme)
            so.A, so.b = ost._border_diph(so.A, so.b, obcb, j1, j2, omesh, None)
        po.solve_system(so)
        A, b, idx = so.last_A_reduced, so.last_b_reduced, so.last_idx
        Ap = A.copy()
        Ap.data = Ap.data * (1.0 + 2.2e-16 * np.random.default_rng(1).standard_normal(len(Ap.data)))
        sens = rel_l2(spla.spsolve(Ap.tocsc(), b), spla.spsolve(A.tocsc(), b))
        x, xo = s.states[k], so.x
        xr = x[idx]
        berr = float((np.abs(A @ xr - b) / (abs(A) @ np.abs(xr) + np.abs(b) + 1e-300)).max())
        print(f"[spacetime-program solve {what}] state {k}: rel L2 {rel_l2(x, xo):.3e}  sens {sens:.3e}  backward {berr:.3e}")
        assert np.array_equal(np.flatnonzero(x != 0.0), np.flatnonzero(xo != 0.0)), f"active set of state {k}"
        assert rel_l2(x, xo) <= bar(sens), f"{what} state {k}: {rel_l2(x, xo):.2e} (sensitivity {sens:.1e})"
        assert berr <= 1e-9, f"{what} state {k}: backward error {berr:.2e}"
        nact.add(int(np.count_nonzero(xo)))
        worst = max(worst, sens)
    print(f"[spacetime-program solve {what}] active unknowns per slab: {sorted(nact)}")
    return worst


def test_rotating_ellipse_diphasic_matches_the_oracle(pj):
    """diphasic with the complement, 16 x 16 with an offset origin, CN: every state within 1e-10, flat.  (On this mesh the oracle's
    own solution is determined to 3e-12 or better in all five slabs.)"""
    _diphasic(pj, sr.MESH_B, "CN", "ellipse diph CN 16x16", lambda sens: TOL_T)


def test_rotating_ellipse_diphasic_with_a_sliver_cell(pj):
    """The same problem on 12 x 10, BE, whose third slab holds a space-time cut cell of 1.5e-5 of a full one.  There the ORACLE's own
    direct solution moves by 2.1e-9 under a one-ulp perturbation of its matrix: the states differ by 3.0e-9 in that slab (4e-14,
    3e-14, 4e-12, 9e-15 in the others) while the product's state solves the oracle's system with a backward error of 2e-14.  As
    test_moving_diphasic_steps_match_oracle does for the closed-form kinds, the bar is 1e-10 wherever the reference is determined
    that well and 50 sens where it is not; the backward error is held to 1e-9 in every slab.  The case must stay what it is about:
    a slab where the reference is NOT determined to 1e-10."""
    worst = _diphasic(pj, sr.MESH_A, "BE", "ellipse diph BE 12x10 (sliver)", lambda sens: max(TOL_T, 50.0 * sens))
    assert worst > TOL_T


def test_rotating_ellipse_advection_diffusion_matches_the_oracle(pj):
    from tests import moving_advdiff_oracle as oad
    from tests.test_gpu_moving_advdiff import _velocity
    n, L, x0 = sr.MESH_B
    mesh, omesh = pj.Mesh(n, L, x0), po.Mesh(n, L, x0)
    M = int(np.prod(omesh.ext))
    uo, ug = _velocity(omesh)
    body = pj.DeviceFunction(sr.rotating_ellipse())
    bc, obc = pj.Dirichlet(G_INT), po.Dirichlet(G_INT)
    bcb = pj.BorderConditions({k: pj.Dirichlet(B_VAL) for k in HEAT_KEYS})
    obcb = po.BorderConditions({k: po.Dirichlet(B_VAL) for k in HEAT_KEYS})
    Ti = np.random.default_rng(7).random(2 * M)
    cap0 = pj.Capacity(body, pj.SpaceTimeMesh(mesh, [0.0, DT]))
    ph = pj.Phase(cap0, pj.ConvectionOps(cap0, uo, ug), F_SRC, D_VAR)
    s = pj.MovingAdvDiffusionUnsteadyMono(ph, bcb, bc, DT, Ti, mesh, "BE")
    pj.solve_MovingAdvDiffusionUnsteadyMono_b(s, ph, body, DT, 0.0, 3.5 * DT, bcb, bc, mesh, "BE", uo, ug, method="bicgstab",
                                              reltol=1e-14)
    ocap = _oracle_cap(cap0, omesh, 0.0, DT)
    so = oad.MovingAdvDiffusionUnsteadyMono(po.Phase(ocap, po.make_convection_ops(ocap, uo, ug), F_SRC, D_VAR), obcb, obc, DT, Ti,
                                            omesh, "BE")
    po.solve_system(so)
    so.states.append(so.x)
    t = 0.0
    while t < 3.5 * DT:
        t += DT
        k = _oracle_cap(pj.Capacity(body, pj.SpaceTimeMesh(mesh, [t, t + DT])), omesh, t, t + DT)
        op = po.make_convection_ops(k, uo, ug)
        so.A = oad.A_mono_unstead_advdiff_moving(op, k, D_VAR, obc, "BE")
        so.b = oad.b_mono_unstead_advdiff_moving(op, k, D_VAR, F_SRC, obc, so.states[-1], DT, t, "BE")
        so.A, so.b = po.BC_border_mono(so.A, so.b, obcb, omesh, t=t)
        po.solve_system(so)
        so.states.append(so.x)
    _compare_states(s, so, "ellipse advdiff BE")


def test_program_disc_solve_matches_moving_sphere(pj):
    """the same driver with the disc as a program and as MovingSphere: states within 1e-10"""
    fn, _, n, L, x0 = sr.CASES["disc"]
    mesh = pj.Mesh(n, L, x0)
    M = int(np.prod([k + 1 for k in n]))
    bc = pj.Dirichlet(G_INT)
    bcb = pj.BorderConditions({k: pj.Dirichlet(B_VAL) for k in HEAT_KEYS})
    Ti = np.random.default_rng(7).random(2 * M)
    out = []
    for body in (pj.DeviceFunction(fn), pj.MovingSphere(sr.DISC_CEN, sr.DISC_RAD, False, dcenter=sr.DISC_DCEN, dradius=sr.DISC_DRAD)):
        cap0 = pj.Capacity(body, pj.SpaceTimeMesh(mesh, [0.0, DT]))
        ph = pj.Phase(cap0, pj.DiffusionOps(cap0), F_SRC, D_VAR)
        s = pj.MovingDiffusionUnsteadyMono(ph, bcb, bc, DT, Ti, mesh, "CN")
        pj.solve_MovingDiffusionUnsteadyMono_b(s, ph, body, DT, 0.0, 3.5 * DT, bcb, bc, mesh, "CN", method="bicgstab", reltol=1e-14)
        assert s.unconverged == 0 and len(s.states) == 5
        out.append(s.states)
    for k, (x, y) in enumerate(zip(*out)):
        assert np.array_equal(np.flatnonzero(x != 0.0), np.flatnonzero(y != 0.0))
        print(f"[spacetime-program solve disc program vs MovingSphere] state {k}: rel L2 {rel_l2(x, y):.3e}")
        assert rel_l2(x, y) <= TOL_T, (k, rel_l2(x, y))


# ------------------------------------------------------------------------------------ refusals
def _last_error():
    from penguin.jl_amd import _lib as L
    buf = C.create_string_buffer(4096)
    L.lib().pg_last_error(buf, 4096)
    return buf.value.decode("utf-8", "replace")


def test_the_entry_refuses_each_with_its_own_message(pj):
    from penguin.jl_amd import _lib as L
    from penguin.jl_amd.devfn import pg_program
    lib = L.lib()
    mesh = pj.Mesh((12, 10), (4.0, 4.0), (0.1, 0.05))
    df = pj.DeviceFunction(sr.moving_disc)
    phi, d = df.moving_body_program(2), df.moving_gradient_programs(2)
    grad = (pg_program * 2)(*d[:2])
    ok = np.ascontiguousarray(np.column_stack(sr.time_rule(T0, T0 + DT, 2, 2)))

    def call(m=mesh, p=phi, g=grad, dt=d[2], t0=T0, t1=T0 + DT, nq=4, tw=ok):
        h = C.c_void_p()
        ref = lambda q: C.byref(q) if q is not None else None
        rc = lib.pg_capacity_create_spacetime_program(m._h, ref(p), g, ref(dt), C.c_int32(0), C.c_double(t0), C.c_double(t1),
                                                      C.c_int32(nq), L.dptr(tw) if tw is not None else None, C.byref(h))
        assert (rc == 0) == bool(h.value)
        return rc, _last_error(), h

    bad = pg_program.from_buffer_copy(phi)
    bad.op[0] = 200
    heavy, outside = ok.copy(), ok.copy()
    heavy[:, 1] *= 1.0 + 1e-9
    outside[3, 0] = T0 + DT
    w1 = pj.DeviceFunction(sr.wall_1d)
    cases = [
        (dict(m=pj.Mesh((4, 4, 4), (1.0,) * 3, (0.0,) * 3)), "1-D+t and 2-D+t"),
        (dict(p=None), "NULL level-set program"), (dict(g=None), "grad == NULL"), (dict(dt=None), "dphidt == NULL"),
        (dict(tw=None), "tau_w == NULL"),
        (dict(p=bad), "the level-set program is invalid"),
        (dict(g=(pg_program * 2)(d[0], bad)), "gradient program 1 is invalid"),
        (dict(dt=bad), "the time-derivative program is invalid"),
        (dict(m=pj.Mesh((10,), (1.0,), (0.0,)), g=(pg_program * 1)(*w1.moving_gradient_programs(1)[:1])), "reads coordinate 1"),
        (dict(nq=0), "1 .. 4096 time nodes"), (dict(nq=4097), "1 .. 4096 time nodes"),
        (dict(t1=T0), "empty time slab"),
        (dict(tw=outside), "inside (t0, t1)"),
        (dict(tw=heavy), "add up to t1 - t0"),
        (dict(g=(pg_program * 2)(d[1], d[0])), "central differences"),
        (dict(dt=pj.DeviceFunction(lambda x, y, t: -sr.moving_disc(x, y, t)).moving_gradient_programs(2)[2]),
         "the time-derivative program gives"),
    ]
    for kw, want in cases:
        rc, msg, _ = call(**kw)
        assert rc != 0 and want in msg, (want, rc, msg)
    rc, _, h = call()
    assert rc == 0
    lib.pg_capacity_destroy(h)


def test_python_side_refusals_and_what_stays(pj):
    mesh = pj.Mesh((12, 10), (4.0, 4.0), (0.1, 0.05))
    st = pj.SpaceTimeMesh(mesh, [T0, T0 + DT])
    with pytest.raises(pj.PenguinHipError, match="an arbitrary moving level set needs SpaceTimeCapacity.from_arrays"):
        pj.Capacity(sr.moving_disc, st)                                     # a plain callable: today's refusal, today's message
    with pytest.raises(pj.PenguinHipError, match=r"1-D\+t and 2-D\+t"):
        pj.Capacity(pj.DeviceFunction(lambda x, y, z, t: x + y + z - t),
                    pj.SpaceTimeMesh(pj.Mesh((4, 4, 4), (1.0,) * 3, (0.0,) * 3), [0.0, 0.1]))
    with pytest.raises(pj.PenguinHipError, match="cannot trace the moving body"):
        pj.Capacity(pj.DeviceFunction(lambda x, y: x + y), st)
    a = pj.Capacity(pj.DeviceFunction(sr.moving_disc), st, complement=True)
    b = pj.Capacity(pj.DeviceFunction(sr.moving_disc, complement=True), st)
    assert a.body.complement and np.array_equal(a.V, b.V) and np.array_equal(a.cell_types, b.cell_types)
    full = pj.Capacity(pj.DeviceFunction(sr.moving_disc), st)
    cell = (4.0 / 12) * (4.0 / 10)
    assert np.max(np.abs((full.Vn + a.Vn)[full.cell_types != 0.0] - cell)) <= 1e-12 * cell      # the two phases fill the cell
    with pytest.raises(pj.PenguinHipError, match="DeviceFunction bodies"):
        pj.Capacity(pj.MovingSphere(sr.DISC_CEN, sr.DISC_RAD), st, complement=True)


def test_a_moving_body_behind_a_communicator_is_refused():
    """the one-rank refusal behind a 1-rank communicator, in a fresh child process (the library is initialised once per process)"""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    env = {**os.environ, "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    r = subprocess.run([sys.executable, str(root / "scripts" / "spacetime_program_rank_refusal.py")], cwd=root, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "single rank only" in r.stdout
