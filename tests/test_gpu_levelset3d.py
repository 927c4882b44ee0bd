"""Capacity(DeviceFunction(lambda x, y, z: ...), mesh3d, quadrature="height") on the GPU: traced 3-D level sets evaluated inside
the capacity kernels (pg_capacity_create_program3, penguin/jl_amd/csrc/pg_geom_program3.h).  Against the 30-digit torus fixture,
against the product's own closed-form kinds, the phases and two builds bit for bit, the sums of the torus, end to end against
the oracle's direct solves, a Poisson order study, and every refusal.

Bars and classes: tests/levelset3d_cases.py (regular entries: 10 times the host build's worst against the same arbiter, never
set from the GPU; irregular entries: the recorded worst, capped).  Every figure is printed before it is held to its bar."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from oracle import penguin_oracle as po
from tests import levelset3d_cases as lc
from tests.common import oracle_capacity_from_product, rel_l2

pytestmark = pytest.mark.gpu

TOL_T = 1e-10
KEYS = ("left", "right", "top", "bottom")


def _cube(n):
    return ((n, n, n), (4.0, 4.0, 4.0), (0.0, 0.0, 0.0))


@functools.lru_cache(maxsize=None)
def _fixture():
    return lc.load_fixture()


def _cap(pj, fn, mesh, **kw):
    return pj.Capacity(pj.DeviceFunction(fn), pj.Mesh(*mesh), quadrature="height", **kw)


@functools.lru_cache(maxsize=None)
def _cube_mesh(pj, n):
    return pj.Mesh(*_cube(n))


@functools.lru_cache(maxsize=None)
def _torus_cap(pj, n, comp=False):
    """built once and shared, unchanged, by the tests that need it; the two phases sit on ONE mesh object (a diphasic solver asks that)"""
    return pj.Capacity(pj.DeviceFunction(lc.torus()), _cube_mesh(pj, n), quadrature="height", complement=comp)


# ------------------------------------------------------------------------------------ 1. the fixture
@pytest.mark.parametrize("name", ["torus", "torus_complement"])
def test_capacities_match_the_torus_fixture(pj, name):
    f = _fixture()[name]
    cap = _torus_cap(pj, 12, f.complement)
    assert np.array_equal(cap.cell_types, f.cell_types)
    lc.check(name, cap, f, (f.n, f.L, f.x0), lc.Shape("torus", lc.TORUS_C), what="gpu ", keep=f.keep)


# ------------------------------------------------------------------------------------ 2. the closed-form kinds of the product
@pytest.mark.parametrize("comp", [False, True])
def test_oblique_plane_against_the_product_plane(pj, comp):
    cap = _cap(pj, lc.plane(), lc.PLANE_MESH, complement=comp)
    ref = pj.Capacity(pj.Plane(lc.PLANE_N, lc.PLANE_OFF, complement=comp), pj.Mesh(*lc.PLANE_MESH))
    assert np.array_equal(cap.cell_types, ref.cell_types)
    lc.check("plane", cap, ref, lc.PLANE_MESH, what=f"gpu comp={comp} ")


def test_plane_on_a_node_plane_against_the_product_halfspace(pj):
    cap = _cap(pj, lambda x, y, z: x - 1.75, _cube(8))
    ref = pj.Capacity(pj.HalfSpace(0, 1.75), pj.Mesh(*_cube(8)))
    assert np.array_equal(cap.cell_types, ref.cell_types)
    assert not np.any(cap.cell_types == -1)                    # touching is EMPTY
    lc.check("plane", cap, ref, _cube(8), what="gpu node plane ")


@pytest.mark.parametrize("n", [8, 12, 16])
def test_ball_against_the_product_sphere(pj, n):
    cap = _cap(pj, lc.ball(), _cube(n))
    ref = pj.Capacity(pj.Sphere(lc.BALL_C, lc.BALL_R), pj.Mesh(*_cube(n)))
    assert np.array_equal(cap.cell_types, ref.cell_types)
    lc.check("ball", cap, ref, _cube(n), lc.Shape("sphere", lc.BALL_C, (lc.BALL_R,) * 3), what=f"gpu n={n} ")


@pytest.mark.parametrize("n", [8, 12, 16])
def test_ellipsoid_against_the_product_ellipsoid(pj, n):
    cap = _cap(pj, lc.ellipsoid(), _cube(n))
    ref = pj.Capacity(pj.Ellipsoid(lc.ELL_C, lc.ELL_A), pj.Mesh(*_cube(n)))
    assert np.array_equal(cap.cell_types, ref.cell_types)
    lc.check("ellipsoid", cap, ref, _cube(n), lc.Shape("sphere", lc.ELL_C, lc.ELL_A), what=f"gpu n={n} ")


# ------------------------------------------------------------------------------------ 3. bit for bit
FIELDS = ("V", "Γ", "cell_types", "C_ω", "C_γ")


def _same_bits(a, b):
    for k in FIELDS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for k in ("A", "B", "W"):
        for d in range(3):
            assert np.array_equal(getattr(a, k)[d], getattr(b, k)[d]), (k, d)


def test_complement_keyword_equals_complement_body(pj):
    a = _torus_cap(pj, 12, True)
    b = pj.Capacity(pj.DeviceFunction(lc.torus(), complement=True), pj.Mesh(*_cube(12)), quadrature="height")
    _same_bits(a, b)
    assert a.body.complement


def test_two_builds_are_bitwise_equal(pj):
    _same_bits(_cap(pj, lc.rotated_ellipsoid(), _cube(12)), _cap(pj, lc.rotated_ellipsoid(), _cube(12)))


def test_sums_of_the_torus(pj):
    """sum V and sum Gamma at 16^3 against 2 pi^2 R r^2 and 4 pi^2 R r, within the summed per-cell bars of the torus case (every
    cut cell at its regular bar, in units of u, times the cell or face it is normalised by)"""
    cap = _torus_cap(pj, 16)
    n, L, x0 = _cube(16)
    u, h = lc.unit(x0, L, n)
    ncut = int(np.sum(cap.cell_types == -1))
    R, r = lc.TORUS_R, lc.TORUS_r
    dV, dG = abs(np.sum(cap.V) - 2.0 * math.pi ** 2 * R * r * r), abs(np.sum(cap.Γ) - 4.0 * math.pi ** 2 * R * r)
    barV, barG = ncut * lc.BARS["torus"]["V"] * u * h ** 3, ncut * lc.BARS["torus"]["G"] * u * h ** 2
    print(f"[levelset3d sums] {ncut} cut cells  dV {dV:.3g}/{barV:.3g}  dGamma {dG:.3g}/{barG:.3g}")
    assert dV <= barV and dG <= barG


# ------------------------------------------------------------------------------------ 4. end to end on the torus, 12^3
def _check_system(s, so):
    A, b, idx = s.system(0)
    Ar, br, oidx = po.remove_zero_rows_cols(so.A, so.b)
    assert np.array_equal(idx, oidx)
    A = A[:, : len(idx)]
    assert abs(A - Ar).max() <= 1e-12 * abs(Ar).max()
    assert np.max(np.abs(b - br)) <= 1e-12 * max(np.max(np.abs(br)), 1e-300)


def _mono(pj, steady=False):
    cap = _torus_cap(pj, 12)
    ocap = oracle_capacity_from_product(cap, po.Mesh(*_cube(12)))
    f = (lambda x, y, z: 0.0) if steady else (lambda x, y, z, t: 0.0)
    D = lambda x, y, z: 1.0
    return pj.Phase(cap, pj.DiffusionOps(cap), f, D), po.Phase(ocap, po.make_diffusion_ops(ocap), f, D)


@pytest.mark.parametrize("bc_kind", ["dirichlet", "robin"])
def test_mono_unsteady_be_then_cn(pj, bc_kind):
    bci, obci = (pj.Dirichlet(1.0), po.Dirichlet(1.0)) if bc_kind == "dirichlet" else (pj.Robin(1.0, 0.5, 2.0), po.Robin(1.0, 0.5, 2.0))
    ph, oph = _mono(pj)
    M = 13 ** 3
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS})
    obcb = po.BorderConditions({k: po.Dirichlet(0.0) for k in KEYS})
    dt = 0.25 * (4.0 / 12) ** 2
    u0 = np.concatenate([np.zeros(M), np.ones(M)])
    s = pj.DiffusionUnsteadyMono(ph, bcb, bci, dt, u0, "BE")
    so = po.DiffusionUnsteadyMono(oph, obcb, obci, dt, u0, "BE")
    _check_system(s, so)
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 4 * dt, bcb, bci, "CN", reltol=1e-13)
    po.solve_DiffusionUnsteadyMono(so, oph, dt, 4 * dt, obcb, obci, "CN", method="\\")
    assert len(s.states) == len(so.states) >= 4
    worst = max(rel_l2(a, b) for a, b in zip(s.states, so.states))
    print(f"[levelset3d solve {bc_kind}] worst state difference {worst:.2e}")
    assert worst <= TOL_T
    assert float(np.max(np.abs(so.x[:M]))) > 1e-3


def test_mono_steady(pj):
    ph, oph = _mono(pj, steady=True)
    s = pj.DiffusionSteadyMono(ph, pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS}), pj.Dirichlet(1.0))
    so = po.DiffusionSteadyMono(oph, po.BorderConditions({k: po.Dirichlet(0.0) for k in KEYS}), po.Dirichlet(1.0))
    _check_system(s, so)
    pj.solve_DiffusionSteadyMono_b(s, reltol=1e-13)
    po.solve_DiffusionSteadyMono(so, method="\\")
    assert s.ch[-1]["converged"]
    assert rel_l2(s.x, so.x) <= TOL_T


def test_diphasic_with_the_complement_as_second_phase(pj):
    M = 13 ** 3
    omesh = po.Mesh(*_cube(12))
    cap1, cap2 = _torus_cap(pj, 12), _torus_cap(pj, 12, True)
    oc1, oc2 = oracle_capacity_from_product(cap1, omesh), oracle_capacity_from_product(cap2, omesh)
    f = lambda x, y, z, t: 0.0
    D1 = lambda x, y, z: 1.0
    D2 = lambda x, y, z: 2.0
    p1, p2 = pj.Phase(cap1, pj.DiffusionOps(cap1), f, D1), pj.Phase(cap2, pj.DiffusionOps(cap2), f, D2)
    q1, q2 = po.Phase(oc1, po.make_diffusion_ops(oc1), f, D1), po.Phase(oc2, po.make_diffusion_ops(oc2), f, D2)
    ic = pj.InterfaceConditions(pj.ScalarJump(1.0, 0.5, 0.0), pj.FluxJump(1.0, 1.0, 0.0))
    oic = po.InterfaceConditions(po.ScalarJump(1.0, 0.5, 0.0), po.FluxJump(1.0, 1.0, 0.0))
    bcb, obcb = pj.BorderConditions({}), po.BorderConditions({})
    u0 = np.concatenate([np.ones(M), np.ones(M), np.zeros(M), np.zeros(M)])
    dt = 0.5 * (4.0 / 12) ** 2
    s = pj.DiffusionUnsteadyDiph(p1, p2, bcb, ic, dt, u0, "BE")
    so = po.DiffusionUnsteadyDiph(q1, q2, obcb, oic, dt, u0, "BE")
    _check_system(s, so)
    pj.solve_DiffusionUnsteadyDiph_b(s, p1, p2, dt, 4 * dt, bcb, ic, "BE", reltol=1e-13)
    po.solve_DiffusionUnsteadyDiph(so, q1, q2, dt, 4 * dt, obcb, oic, "BE", method="\\")
    assert len(s.states) == len(so.states)
    worst = max(rel_l2(a, b) for a, b in zip(s.states, so.states))
    print(f"[levelset3d diphasic] worst state difference {worst:.2e}")
    assert worst <= TOL_T


# ------------------------------------------------------------------------------------ 5. convergence
def test_poisson_in_a_rotated_ellipsoid_converges(pj):
    """-lap u = 2 (1 / a^2 + 1 / b^2 + 1 / c^2) inside the ellipsoid turned about z and then about x, u = 0 on it: u = 1 - q, q the
    body's quadratic form.  Volume-weighted L2 error of the bulk unknowns at the cell centroids on 8^3, 16^3, 32^3; both observed
    orders must exceed 1.0, the reference's own bar for its convergence suites.  Measured on an MI355X: DESIGN.md section 27
    (the figures are printed by this test)."""
    phi = lc.rotated_ellipsoid()
    src = 2.0 * sum(1.0 / a ** 2 for a in phi.axes)
    errs = {}
    for n in (8, 16, 32):
        M = (n + 1) ** 3
        cap = _cap(pj, phi, _cube(n))
        ph = pj.Phase(cap, pj.DiffusionOps(cap), lambda x, y, z: src, lambda x, y, z: 1.0)
        s = pj.DiffusionSteadyMono(ph, pj.BorderConditions({}), pj.Dirichlet(0.0))
        pj.solve_DiffusionSteadyMono_b(s, reltol=1e-13)
        V, Cw = cap.V, cap.C_ω
        inside = V > 0.0
        exact = -phi(Cw[:, 0], Cw[:, 1], Cw[:, 2])
        errs[n] = math.sqrt(np.sum(V[inside] * (s.x[:M][inside] - exact[inside]) ** 2) / np.sum(V[inside]))
    orders = [math.log(errs[p] / errs[q]) / math.log(2.0) for p, q in ((8, 16), (16, 32))]
    print(f"[levelset3d poisson] errors {errs} orders {orders}")
    assert errs[8] < 0.2                         # (u is O(1): the sign convention of the source is right)
    assert min(orders) > 1.0


# ------------------------------------------------------------------------------------ 6. refusals
def test_python_refusals_each_with_its_own_message(pj):
    df = pj.DeviceFunction(lc.ball())
    mesh3 = pj.Mesh(*_cube(4))
    with pytest.raises(pj.PenguinHipError, match=r'3-D.*quadrature="height"'):
        pj.Capacity(df, mesh3)                                                   # without the keyword: today's refusal, extended
    with pytest.raises(pj.PenguinHipError, match="this mesh is 2-D"):
        pj.Capacity(pj.DeviceFunction(lambda x, y: x + y - 1.0), pj.Mesh((4, 4), (1.0, 1.0), (0.0, 0.0)), quadrature="height")
    with pytest.raises(pj.PenguinHipError, match="this mesh is 1-D"):
        pj.Capacity(pj.DeviceFunction(lambda x: x - 0.3), pj.Mesh((4,), (1.0,), (0.0,)), quadrature="height")
    with pytest.raises(pj.PenguinHipError, match="is for DeviceFunction bodies"):
        pj.Capacity(pj.Sphere((2.0, 2.0, 2.0), 1.0), mesh3, quadrature="height")
    with pytest.raises(pj.PenguinHipError, match="is for DeviceFunction bodies"):
        pj.Capacity(lambda x, y, z: x + y + z - 1.0, mesh3, quadrature="height")
    with pytest.raises(pj.PenguinHipError, match="only rule to choose"):
        pj.Capacity(df, mesh3, quadrature="simpson")
    with pytest.raises(pj.PenguinHipError, match="SpaceTimeMesh"):
        pj.Capacity(pj.DeviceFunction(lambda x, y, t: x + y - t), pj.SpaceTimeMesh(pj.Mesh((4, 4), (1.0, 1.0), (0.0, 0.0)), [0.0, 0.1]),
                    quadrature="height")
    with pytest.raises(pj.PenguinHipError, match="cannot trace"):
        pj.Capacity(pj.DeviceFunction(lambda x, y, z, t: x + y + z - t), mesh3, quadrature="height")


def _last_error():
    from penguin.jl_amd import _lib as L
    buf = C.create_string_buffer(4096)
    L.lib().pg_last_error(buf, 4096)
    return buf.value.decode("utf-8", "replace")


def test_the_entry_refuses_each_with_its_own_message(pj):
    """pg_capacity_create_program3 itself: every refusal comes back as an error with no capacity, a good call after them still
    works, and pg_capacity_create_program keeps refusing a 3-D mesh and says where to go"""
    from penguin.jl_amd import _lib as L
    from penguin.jl_amd.devfn import pg_program
    lib = L.lib()
    mesh = pj.Mesh(*_cube(8))
    df = pj.DeviceFunction(lc.ball())
    phi, grad = df.body_program(3), (pg_program * 3)(*df.gradient_programs(3))

    def call(m, p, g, entry=None):
        h = C.c_void_p()
        rc = (entry or lib.pg_capacity_create_program3)(m._h, C.byref(p) if p is not None else None, g, C.c_int32(0), C.byref(h))
        assert (rc == 0) == bool(h.value)
        return rc, _last_error(), h

    bad = pg_program.from_buffer_copy(phi)
    bad.op[0] = 200
    cases = [
        (mesh, None, grad, "NULL level-set program"),
        (mesh, phi, None, "grad == NULL"),
        (mesh, bad, grad, "level-set program is invalid"),
        (mesh, phi, (pg_program * 3)(grad[0], bad, grad[2]), "gradient program 1 is invalid"),
        (mesh, pj.DeviceFunction(lambda x, y, z, t: x + y + z - t).program_for(3), grad, "reads t"),
        (pj.Mesh((8, 8), (4.0, 4.0), (0.0, 0.0)), phi, grad, "must be 3-D"),
        (mesh, phi, (pg_program * 3)(grad[2], grad[1], grad[0]), "central differences"),
    ]
    for m, p, g, want in cases:
        rc, msg, _ = call(m, p, g)
        assert rc != 0 and want in msg and "pg_capacity_create_program3 refused" in msg, (want, rc, msg)
    rc, msg, _ = call(mesh, phi, grad, lib.pg_capacity_create_program)
    assert rc != 0 and "3-D" in msg and "pg_capacity_create_program3" in msg, msg
    rc, _, h = call(mesh, phi, grad)
    assert rc == 0
    lib.pg_capacity_destroy(h)
