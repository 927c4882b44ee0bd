"""GPU tests of moving marker polygons: Capacity(MovingFront, SpaceTimeMesh(...)) and Capacity((front_n, front_np1), STmesh) through
pg_capacity_create_spacetime_polygon.

* every case of tests/moving_polygon_cases.py against the exact rational arbiter, held to the bars the HOST build set on the CPU
  (10 times its worst plus the order term; the GPU never sets a bar), cell types identical;
* the cheap pass against the all-nodes rule on every cell; two builds bitwise equal; Vn of a slab bitwise Vn_1 of the next; the
  pair of fronts equal to the MovingFront of the same markers;
* the analytic sums no arbiter shares, and the fine circle against MovingSphere through the product;
* the C entry's refusals with a good call after them, the communicator refusal in a fresh child process, the single-front refusal;
* the moving drivers fed to the oracle's literal algebra on the product's capacities, 1 + 4 slabs, 1e-10 (a slab where the
  oracle's own direct solve moves by more than 2e-12 under a one-ulp perturbation of its matrix is held to 50 times that);
* a translating 4096-marker circle against MovingSphere through the driver."""
import ctypes as C
from fractions import Fraction as Fr

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from oracle import penguin_oracle as po
from oracle import spacetime as ost
from tests import moving_polygon_cases as mc
from tests import spacetime_polygon_reference as spr
from tests.common import rel_l2
from tests.spacetime_program_reference import Layer
from tests.test_gpu_moving import _oracle_cap
from tests.test_moving_polygon_host import _exact_areas

pytestmark = pytest.mark.gpu
TOL_T, SENS_OK = 1e-10, 2e-12
T0, DT = mc.T0, mc.DT


def _product(pj, name, t0=T0, t1=T0 + DT):
    fn, n, L, x0, comp, pr = mc.CASES[name]
    mesh = pj.Mesh(n, L, x0)
    mf = pj.MovingFront(fn, complement=comp)
    return pj.Capacity(mf, pj.SpaceTimeMesh(mesh, [t0, t1]), time_panels=pr[0], time_order=pr[1]), mf


@pytest.fixture(scope="module")
def caps(pj):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _product(pj, name)[0]
        return cache[name]
    return get


# ------------------------------------------------------------------------------------ against the arbiter
@pytest.mark.parametrize("name", list(mc.CASES))
def test_capacities_match_the_arbiter_within_the_host_bars(pj, caps, name):
    _, n, L, x0, comp, _ = mc.CASES[name]
    cap, ref = caps(name), mc.reference(name)
    assert isinstance(cap, pj.SpaceTimeCapacity) and isinstance(cap.body, pj.MovingFront) and cap.body.complement == comp
    M = int(np.prod([k + 1 for k in n]))
    assert np.array_equal(cap.cell_types, ref.cell_types)
    assert set(cap.cell_types) == {0.0, 1.0, -1.0}
    assert np.array_equal(np.flatnonzero(cap.Γ > 0), np.flatnonzero(ref.G > 0))
    mc.check(name, Layer(cap, 2, M), what="gpu ")
    assert len(cap.A_st) == 3 and all(len(a) == 2 * M for a in cap.A_st)
    _, listed = cap.spacetime_kernel_ms
    assert int(np.count_nonzero(cap.cell_types == -1.0)) <= listed < n[0] * n[1]      # the cheap pass finished cells and lost no cut cell


@pytest.mark.parametrize("name", ["heptagon_nq3", "crystal_16", "leaving", "aligned_rect_16", "complement_heptagon"])
def test_cheap_pass_agrees_with_the_all_nodes_rule_on_every_cell(caps, name):
    """the all-nodes rule is the arbiter's: a cell is FULL / EMPTY only if it is so at every node and both faces, taken on EVERY
    cell; the product finishes the cells with an empty swept list early.  Types, and the plain values of the finished cells"""
    _, n, L, x0, _, _ = mc.CASES[name]
    cap, ref = caps(name), mc.reference(name)
    assert np.array_equal(cap.cell_types, ref.cell_types)
    hfull, dt = (L[0] / n[0]) * (L[1] / n[1]), (T0 + DT) - T0
    full, empty = cap.cell_types == 1.0, cap.cell_types == 0.0
    assert np.all(cap.V[full] == hfull * dt) and np.all(cap.Vn[full] == hfull) and np.all(cap.Vn_1[full] == hfull)
    assert np.all(cap.V[empty] == 0.0) and np.all(cap.Vn[empty] == 0.0) and np.all(cap.Vn_1[empty] == 0.0)


def test_two_builds_consecutive_slabs_and_the_pair_of_fronts_are_bitwise_equal(pj):
    name = "heptagon_nq64"
    fn, n, L, x0, _, pr = mc.CASES[name]
    t1 = T0 + DT
    a, mf = _product(pj, name, T0, t1)
    b, _ = _product(pj, name, t1, t1 + DT)
    assert np.array_equal(a.Vn, b.Vn_1) and np.count_nonzero((a.Vn > 0) & (a.Vn < a.Vn.max())) > 10
    c, _ = _product(pj, name, T0, t1)
    pair = pj.Capacity((mf.at(T0), mf.at(t1)), pj.SpaceTimeMesh(pj.Mesh(n, L, x0), [T0, t1]), time_panels=pr[0], time_order=pr[1])
    assert isinstance(pair.body, pj.MovingFront)
    for other in (c, pair):
        for f in ("V", "Γ", "cell_types", "Vn_1", "Vn", "C_ω_st", "C_γ_st"):
            assert np.array_equal(getattr(a, f), getattr(other, f)), f
        for f in ("A", "B", "W"):
            assert all(np.array_equal(p, q) for p, q in zip(getattr(a, f), getattr(other, f))), f
    comp = pj.Capacity((mf.at(T0), mf.at(t1)), pj.SpaceTimeMesh(pj.Mesh(n, L, x0), [T0, t1]), time_panels=pr[0], time_order=pr[1],
                       complement=True)
    assert comp.body.complement and np.array_equal(comp.cell_types == -1.0, a.cell_types == -1.0)
    cell = (L[0] / n[0]) * (L[1] / n[1])
    real = np.zeros((n[1] + 1, n[0] + 1), dtype=bool)
    real[:n[1], :n[0]] = True
    assert np.max(np.abs((a.Vn + comp.Vn)[real.ravel()] - cell)) <= 8 * 2.0 ** -52 * cell      # the two phases fill every cell


# ------------------------------------------------------------------------------------ analytic sums
@pytest.mark.parametrize("name", ["heptagon_nq3", "heptagon_nq80", "fine_2000_8", "crystal_16", "triangle", "aligned_rect_16"])
def test_sums_of_volumes_are_the_closed_forms(caps, name):
    """tests/test_moving_polygon_host.py::test_sums_of_volumes_are_the_closed_forms, on the GPU's capacities"""
    got = caps(name)
    A0, A1, A01 = _exact_areas(*mc.ends(name))
    ncut = int(np.count_nonzero(got.cell_types == -1))
    for what, arr, want in (("Vn_1", got.Vn_1, A0), ("Vn", got.Vn, A1), ("V", got.V, Fr(DT) * (A0 + A1 + A01) / 3)):
        d, tol = abs(mc.lsum(arr) - np.longdouble(float(want))), mc.sum_tol(arr, ncut, float(want))
        print(f"[moving-polygon gpu {name}] sum {what} off by {float(d):.3g} (bound {float(tol):.3g})")
        assert d <= tol, (name, what, float(d), float(tol))


@pytest.mark.parametrize("name, c", [("fine_2000_8", (1.7, 0.9)), ("aligned_rect_16", (7.5, 0.0))])
def test_translation_sum_of_gamma_is_the_closed_form(caps, name, c):
    got = caps(name)
    p0, _ = spr.normalise(*mc.ends(name))
    e = (np.roll(p0, -1, axis=0) - p0).astype(np.longdouble)
    ln = np.sqrt(e[:, 0] ** 2 + e[:, 1] ** 2)
    vn = (c[0] * e[:, 1] - c[1] * e[:, 0]) / ln
    want = np.longdouble(DT) * np.sum(ln * np.sqrt(1 + vn * vn))
    ncut = int(np.count_nonzero(got.cell_types == -1))
    d, tol = abs(mc.lsum(got.Γ) - want), mc.sum_tol(got.Γ, ncut + 8 + len(p0), want)
    print(f"[moving-polygon gpu {name}] sum Gamma off by {float(d):.3g} (bound {float(tol):.3g})")
    assert d <= tol


def test_fine_circle_is_the_moving_sphere_within_the_sagitta(pj, caps):
    """2000 markers against MovingSphere through the product, the same time rule: per cell within the lens bound of
    tests/test_moving_polygon_host.py::test_fine_circle_is_the_moving_ball_within_the_sagitta"""
    name = "fine_2000_8"
    _, n, L, x0, _, pr = mc.CASES[name]
    got = caps(name)
    ball = pj.MovingSphere(lambda t: (2.01 + 1.7 * (t - T0), 2.01 + 0.9 * (t - T0)), lambda t: 1.0, dcenter=lambda t: (1.7, 0.9),
                           dradius=lambda t: 0.0)
    ref = pj.Capacity(ball, pj.SpaceTimeMesh(pj.Mesh(n, L, x0), [T0, T0 + DT]), time_panels=pr[0], time_order=pr[1])
    u, h = mc.unit(x0, L, n)
    sag = np.pi ** 2 / (2 * 2000.0 ** 2)
    bound = (got.Γ + ref.Γ) * sag + mc.bars(name)["V"] * u * h * h * DT
    d = np.abs(got.V - ref.V)
    print(f"[moving-polygon gpu {name}] worst |V - V_sphere| / bound = {float(np.max(d / np.maximum(bound, 1e-300))):.3g}, "
          f"worst |dV| = {float(np.max(d)):.3g}")
    assert np.all(d <= bound) and np.max(d) > 0.0
    assert np.array_equal(got.cell_types, ref.cell_types)


# ------------------------------------------------------------------------------------ refusals
def _last_error():
    from penguin.jl_amd import _lib as L
    buf = C.create_string_buffer(4096)
    L.lib().pg_last_error(buf, 4096)
    return buf.value.decode("utf-8", "replace")


def test_the_entry_refuses_each_with_its_own_message(pj):
    from penguin.jl_amd import _lib as L
    lib = L.lib()
    mesh = pj.Mesh((12, 10), (4.0, 4.0), (-0.3, 0.2))
    tri0, tri1 = np.array([(1.0, 1), (3, 1), (2, 3)]), np.array([(1.1, 1), (3.1, 1), (2.1, 3)])
    ok = np.ascontiguousarray(np.column_stack(spr.time_rule(T0, T0 + DT, 2, 2)))

    def call(m=mesh, a=tri0, b=tri1, t0=T0, t1=T0 + DT, nq=4, tw=ok, out=True):
        h = C.c_void_p()
        flat = lambda p: np.ascontiguousarray(np.asarray(p, dtype=float).reshape(-1)) if p is not None else None
        a, b = flat(a), flat(b)
        M = len(a if a is not None else b) // 2
        rc = lib.pg_capacity_create_spacetime_polygon(m._h if m is not None else None, L.dptr(a) if a is not None else None,
                                                      L.dptr(b) if b is not None else None, C.c_int64(M), C.c_int32(0), C.c_double(t0),
                                                      C.c_double(t1), C.c_int32(nq), L.dptr(tw) if tw is not None else None,
                                                      C.byref(h) if out else None)
        assert (rc == 0) == bool(h.value)
        return rc, _last_error(), h

    heavy, outside = ok.copy(), ok.copy()
    heavy[:, 1] *= 1.0 + 1e-9
    outside[3, 0] = T0 + DT
    cases = [
        (dict(m=None), "NULL mesh"), (dict(out=False), "NULL output pointer"),
        (dict(a=None), "xy0 == NULL"), (dict(b=None), "xy1 == NULL"), (dict(tw=None), "tau_w == NULL"),
        (dict(a=tri0[:2], b=tri1[:2]), "at least 3 markers (got 2)"),
        (dict(a=[(1, 1), (3, np.nan), (2, 3)]), "marker 1 has a non-finite coordinate at t0"),
        (dict(b=[(1, 1), (3, 1), (np.inf, 3)]), "marker 2 has a non-finite coordinate at t1"),
        (dict(m=pj.Mesh((10,), (1.0,), (0.0,))), "2-D body, the mesh is 1-D"),
        (dict(m=pj.Mesh((4, 4, 4), (1.0,) * 3, (0.0,) * 3)), "2-D body, the mesh is 3-D"),
        (dict(nq=0), "1 .. 4096 time nodes"), (dict(nq=4097), "1 .. 4096 time nodes"),
        (dict(t1=T0), "empty time slab"),
        (dict(tw=outside), "inside (t0, t1)"),
        (dict(tw=heavy), "add up to t1 - t0"),
        (dict(a=[(1, 1), (3, 1), (3, 1), (2, 3)], b=[(1, 1), (3, 1), (3, 2), (2, 3)]), "at t0: zero-length edge: markers 1 and 2 coincide"),
        (dict(b=[(1, 1), (2, 2), (3, 3)]), "at t1: the polygon has zero signed area"),
        (dict(a=[(0, 0), (2, 0), (2, 1), (1, 1.5), (0, 2)], b=[(0, 0), (2, 0), (2, 1), (1, -1), (0, 2)]),
         "at t1: the polygon intersects itself: edges 0 and 2"),
        (dict(a=[(0, 0), (2, 0), (2, 2), (0, 2)], b=[(2, 2), (0, 2), (0, 0), (2, 0)]), "at mid time: zero-length edge"),
        (dict(b=[(1, 1), (3, 1), (2.2, -1.5)]), "orientation of the polygon differs between t0 and t1"),
    ]
    for kw, want in cases:
        rc, msg, _ = call(**kw)
        assert rc != 0 and want in msg, (want, rc, msg)
    rc, _, h = call()                                              # a good call after them still works
    assert rc == 0
    lib.pg_capacity_destroy(h)


def test_python_side_refusals_and_what_stays(pj):
    mesh = pj.Mesh((8, 8), (4.0, 4.0), (0.0, 0.0))
    st = pj.SpaceTimeMesh(mesh, [0.0, 0.1])
    a = pj.create_circle_b(pj.FrontTracker(), 2.0, 2.0, 1.0, 16)
    with pytest.raises(pj.PenguinHipError, match="SpaceTimeMesh"):
        pj.Capacity(a, st)                                                    # a single front has no motion: still refused
    with pytest.raises(pj.PenguinHipError, match="at t1: the polygon has zero signed area"):
        pj.Capacity(pj.MovingFront(lambda t: a.polygon() * np.array([1.0, 1.0 - 10.0 * t])), st)
    good = pj.Capacity(pj.MovingFront.rigid(a, shift=lambda t: (t, 0.0)), st)     # and a good one after the refusal
    assert abs(good.Vn.sum() - float(mc.shoelace(a.polygon()))) <= 1e-13


def test_a_moving_front_behind_a_communicator_is_refused():
    """the one-rank refusal behind a 1-rank communicator, in a fresh child process (the library is initialised once per process)"""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    env = {**os.environ, "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    r = subprocess.run([sys.executable, str(root / "scripts" / "moving_polygon_rank_refusal.py")], cwd=root, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "single rank only" in r.stdout


# ------------------------------------------------------------------------------------ solves
HEAT_KEYS = ("left", "right", "top", "bottom")
F_SRC = lambda x, y, z, t: 0.3 + 0.2 * x + 0.5 * t
D_VAR = lambda x, y, z: 1.0 + 0.1 * x
G_INT = lambda x, y, z=0.0: 1.0 + 0.2 * x + 0.3 * y
B_VAL = lambda *a: 0.2 + 0.1 * a[-1]


def _sensitivity(so):
    """how far the ORACLE's own direct solution moves when its matrix entries move by one rounding error
    (tests/test_gpu_moving.py:136-155)"""
    A, b = so.last_A_reduced, so.last_b_reduced
    Ap = A.copy()
    Ap.data = Ap.data * (1.0 + 2.2e-16 * np.random.default_rng(1).standard_normal(len(Ap.data)))
    return rel_l2(spla.spsolve(Ap.tocsc(), b), spla.spsolve(A.tocsc(), b))


def _hold(what, k, x, xo, sens):
    bar = TOL_T if sens <= SENS_OK else max(TOL_T, 50.0 * sens)
    print(f"[moving-polygon solve {what}] state {k}: rel L2 {rel_l2(x, xo):.3e}  sens {sens:.3e}  bar {bar:.1e}")
    assert np.array_equal(np.flatnonzero(x != 0.0), np.flatnonzero(xo != 0.0)), f"{what}: active set of state {k}"
    assert rel_l2(x, xo) <= bar, f"{what} state {k}: {rel_l2(x, xo):.2e} (sensitivity {sens:.1e})"


def _no_sliver(cap, n, L, what):
    frac = mc.smallest_cut_fraction(cap, n, L)
    assert frac >= mc.SLIVER, (what, frac)


def _mono(pj, name, scheme, advdiff):
    """the oracle's literal blocks and direct solves on the capacities the product computed, every slab from the product's
    previous state, 1 + 4 slabs"""
    fn, n, L, x0 = mc.SOLVES[name]
    mesh, omesh = pj.Mesh(n, L, x0), po.Mesh(n, L, x0)
    M = int(np.prod(omesh.ext))
    body = pj.MovingFront(fn)
    bc, obc = pj.Dirichlet(G_INT), po.Dirichlet(G_INT)
    bcb = pj.BorderConditions({k: pj.Dirichlet(B_VAL) for k in HEAT_KEYS})
    obcb = po.BorderConditions({k: po.Dirichlet(B_VAL) for k in HEAT_KEYS})
    Ti = np.random.default_rng(7).random(2 * M)
    cap_of = lambda t0, t1: pj.Capacity(body, pj.SpaceTimeMesh(mesh, [t0, t1]))
    cap0 = cap_of(0.0, DT)
    if advdiff:
        from tests import moving_advdiff_oracle as oad
        from tests.test_gpu_moving_advdiff import _velocity
        uo, ug = _velocity(omesh)
        ph = pj.Phase(cap0, pj.ConvectionOps(cap0, uo, ug), F_SRC, D_VAR)
        s = pj.MovingAdvDiffusionUnsteadyMono(ph, bcb, bc, DT, Ti, mesh, scheme)
        pj.solve_MovingAdvDiffusionUnsteadyMono_b(s, ph, body, DT, 0.0, 3.5 * DT, bcb, bc, mesh, scheme, uo, ug, method="bicgstab",
                                                  reltol=1e-14)
        ops = lambda k: po.make_convection_ops(k, uo, ug)
        mkA, mkb = oad.A_mono_unstead_advdiff_moving, oad.b_mono_unstead_advdiff_moving
        first = oad.MovingAdvDiffusionUnsteadyMono
    else:
        ph = pj.Phase(cap0, pj.DiffusionOps(cap0), F_SRC, D_VAR)
        s = pj.MovingDiffusionUnsteadyMono(ph, bcb, bc, DT, Ti, mesh, scheme)
        pj.solve_MovingDiffusionUnsteadyMono_b(s, ph, body, DT, 0.0, 3.5 * DT, bcb, bc, mesh, scheme, method="bicgstab", reltol=1e-14)
        ops = po.make_diffusion_ops
        mkA, mkb = ost.A_mono_unstead_diff_moving, ost.b_mono_unstead_diff_moving
        first = ost.MovingDiffusionUnsteadyMono
    assert s.unconverged == 0 and len(s.states) == 5
    what = f"{name} {'advdiff' if advdiff else 'mono'} {scheme}"
    ocap = _oracle_cap(cap0, omesh, 0.0, DT)
    _no_sliver(cap0, n, L, what)
    so = first(po.Phase(ocap, ops(ocap), F_SRC, D_VAR), obcb, obc, DT, Ti, omesh, scheme)
    t = 0.0
    for k in range(5):
        if k > 0:
            t += DT
            cap = cap_of(t, t + DT)
            _no_sliver(cap, n, L, what)
            j = _oracle_cap(cap, omesh, t, t + DT)
            op = ops(j)
            so.A = mkA(op, j, D_VAR, obc, scheme)
            so.b = mkb(op, j, D_VAR, F_SRC, obc, s.states[k - 1], DT, t, scheme)
            so.A, so.b = po.BC_border_mono(so.A, so.b, obcb, omesh, t=t)
        po.solve_system(so)
        _hold(what, k, s.states[k], so.x, _sensitivity(so))


@pytest.mark.parametrize("scheme", ["BE", "CN"])
def test_turning_heptagon_mono_matches_the_oracle(pj, scheme):
    _mono(pj, "mono_12x10", scheme, advdiff=False)


def test_turning_star_advection_diffusion_matches_the_oracle(pj):
    _mono(pj, "advdiff_16", "BE", advdiff=True)


def test_turning_star_diphasic_with_the_complement_matches_the_oracle(pj):
    name, scheme = "diph_16", "CN"
    fn, n, L, x0 = mc.SOLVES[name]
    mesh, omesh = pj.Mesh(n, L, x0), po.Mesh(n, L, x0)
    M = int(np.prod(omesh.ext))
    body, body_c = pj.MovingFront(fn), pj.MovingFront(fn, complement=True)
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
    assert s.unconverged == 0 and len(s.states) == 5
    what = f"{name} diph {scheme}"
    for c in (c1, c2):
        _no_sliver(c, n, L, what)
    k1, k2 = _oracle_cap(c1, omesh, 0.0, DT), _oracle_cap(c2, omesh, 0.0, DT)
    q1, q2 = po.Phase(k1, po.make_diffusion_ops(k1), F_SRC, D_VAR), po.Phase(k2, po.make_diffusion_ops(k2), f2, D2)
    so = ost.MovingDiffusionUnsteadyDiph(q1, q2, obcb, oic, DT, Ti, omesh, scheme)
    t = 0.0
    for k in range(5):
        if k > 0:
            t += DT
            cs = caps(t, t + DT)
            for c in cs:
                _no_sliver(c, n, L, what)
            j1, j2 = (_oracle_cap(c, omesh, t, t + DT) for c in cs)
            o1, o2 = po.make_diffusion_ops(j1), po.make_diffusion_ops(j2)
            so.A = ost.A_diph_unstead_diff_moving(o1, o2, j1, j2, D_VAR, D2, oic, scheme)
            so.b = ost.b_diph_unstead_diff_moving(o1, o2, j1, j2, D_VAR, D2, F_SRC, f2, oic, s.states[k - 1], DT, t, scheme)
            so.A, so.b = ost._border_diph(so.A, so.b, obcb, j1, j2, omesh, None)
        po.solve_system(so)
        _hold(what, k, s.states[k], so.x, _sensitivity(so))


def test_translating_circle_of_4096_markers_against_moving_sphere_through_the_driver(pj):
    """The same driver with a 4096-marker circle and with MovingSphere, 1 + 4 slabs on 16^2.  The capacities differ by the lenses
    between chords and arcs, of height sag = r pi^2 / (2 M^2) = 2.9e-7: a cut cell's entries move by at most
    delta = sag max(Gamma_cell / V_cell) relatively.  The bar of the states is 50 times how far the ORACLE's own direct solution of
    the first slab's system (on the MovingSphere capacities) moves when its matrix entries move by delta relatively, the probe of
    tests/test_gpu_moving.py with delta in place of one ulp."""
    n, L, x0 = mc.SQ16
    mesh, omesh = pj.Mesh(n, L, x0), po.Mesh(n, L, x0)
    M = int(np.prod(omesh.ext))
    cen, vel = (1.83, 2.07), (0.9, -0.5)
    base = pj.create_circle_b(pj.FrontTracker(), cen[0], cen[1], 1.0, 4096)
    bodies = (pj.MovingFront.rigid(base, shift=lambda t: (vel[0] * t, vel[1] * t)),
              pj.MovingSphere(lambda t: (cen[0] + vel[0] * t, cen[1] + vel[1] * t), lambda t: 1.0, dcenter=lambda t: vel, dradius=lambda t: 0.0))
    bc = pj.Dirichlet(G_INT)
    bcb = pj.BorderConditions({k: pj.Dirichlet(B_VAL) for k in HEAT_KEYS})
    Ti = np.random.default_rng(7).random(2 * M)
    out, cap0s = [], []
    for body in bodies:
        cap0 = pj.Capacity(body, pj.SpaceTimeMesh(mesh, [0.0, DT]))
        ph = pj.Phase(cap0, pj.DiffusionOps(cap0), F_SRC, D_VAR)
        s = pj.MovingDiffusionUnsteadyMono(ph, bcb, bc, DT, Ti, mesh, "BE")
        pj.solve_MovingDiffusionUnsteadyMono_b(s, ph, body, DT, 0.0, 3.5 * DT, bcb, bc, mesh, "BE", method="bicgstab", reltol=1e-14)
        assert s.unconverged == 0 and len(s.states) == 5
        out.append(s.states)
        cap0s.append(cap0)
    poly, ball = cap0s
    assert np.array_equal(poly.cell_types, ball.cell_types)
    cut = ball.cell_types == -1.0
    sag = np.pi ** 2 / (2 * 4096.0 ** 2)
    delta = sag * float(np.max(ball.Γ[cut] / ball.V[cut]))
    ocap = _oracle_cap(ball, omesh, 0.0, DT)
    obc, obcb = po.Dirichlet(G_INT), po.BorderConditions({k: po.Dirichlet(B_VAL) for k in HEAT_KEYS})
    so = ost.MovingDiffusionUnsteadyMono(po.Phase(ocap, po.make_diffusion_ops(ocap), F_SRC, D_VAR), obcb, obc, DT, Ti, omesh, "BE")
    po.solve_system(so)
    A, b = so.last_A_reduced, so.last_b_reduced
    Ap = A.copy()
    Ap.data = Ap.data * (1.0 + delta * np.random.default_rng(1).standard_normal(len(Ap.data)))
    sens = rel_l2(spla.spsolve(Ap.tocsc(), b), spla.spsolve(A.tocsc(), b))
    worst = max(rel_l2(x, y) for x, y in zip(*out))
    print(f"[moving-polygon solve circle 4096 vs MovingSphere] worst rel L2 {worst:.3e}  delta {delta:.3e}  sens(delta) {sens:.3e}  "
          f"bar {50.0 * sens:.3e}")
    for k, (x, y) in enumerate(zip(*out)):
        assert np.array_equal(np.flatnonzero(x != 0.0), np.flatnonzero(y != 0.0))
        assert rel_l2(x, y) <= 50.0 * sens, (k, rel_l2(x, y), sens)
    assert worst > 0.0
