"""Oblique half spaces (pj.Plane, PG_BODY_PLANE) through the HIP path against the CPU oracle.

The oracle side is oracle.penguin_oracle.make_capacity, unmodified, on the duck-typed body of tests/plane_oracle.py
(Sutherland-Hodgman / convex-hull geometry: nothing in common with the kernels' section integrals).  Bars: the project's bars
for its other exact body (tests/test_gpu_parity.py, half-space capacities) and the north star's 1e-10 on the states."""
import functools
import math

import numpy as np
import pytest
from scipy.special import erfc

from oracle import penguin_oracle as po
from penguin.jl_amd import _lib as L
from tests.common import oracle_capacity_from_product, rel_l2
from tests.plane_oracle import ObliqueHalfSpace

pytestmark = pytest.mark.gpu

TOL_T = 1e-10
KEYS = ("left", "right", "top", "bottom")

CASES = [
    (1, 37, 1.3, -0.2, (-2.0,), -0.62),
    (2, 24, 2.0, 0.1, (0.6, 0.8), 1.37),
    (2, 24, 2.0, 0.1, (-0.28, 0.96), 0.9),
    (2, 16, 1.0, 0.0, (1e-9, 1.0), 0.53),
    (3, 8, 1.0, 0.0, (2.0 / 7.0, 3.0 / 7.0, 6.0 / 7.0), 0.7857),
    (3, 8, 1.0, 0.0, (-0.6, 0.0, 0.8), 0.13),
    (3, 10, 2.0, 0.1, (0.36, 0.48, 0.8), 1.804),
]
CASE_2D = CASES[1]
CASE_3D = CASES[4]


@functools.lru_cache(maxsize=None)
def _oracle_cap(case, comp):
    """computed once per case and phase, shared by the tests below, never modified"""
    N, n, Lx, x0, normal, offset = case
    return po.make_capacity(ObliqueHalfSpace(normal, offset, comp), po.Mesh((n,) * N, (Lx,) * N, (x0,) * N))


def _meshes(pj, case):
    N, n, Lx, x0, _, _ = case
    return pj.Mesh((n,) * N, (Lx,) * N, (x0,) * N), po.Mesh((n,) * N, (Lx,) * N, (x0,) * N)


def _check_system(s, so):
    """Reduced system of the constructor: same active index set (bit-exact), same matrix, same rhs."""
    A, b, idx = s.system(0)
    Ar, br, oidx = po.remove_zero_rows_cols(so.A, so.b)
    assert np.array_equal(idx, oidx)
    A = A[:, : len(idx)]
    assert abs(A - Ar).max() <= 1e-12 * abs(Ar).max()
    assert np.max(np.abs(b - br)) <= 1e-12 * max(np.max(np.abs(br)), 1e-300)
    return idx


# ------------------------------------------------------------------------------------ 1. capacities
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}d-n{c[1]}-{c[4]}")
def test_plane_capacities_match_oracle(pj, case):
    N, n, Lx, x0, normal, offset = case
    mesh, _ = _meshes(pj, case)
    h = Lx / n
    full, face, span = h ** N, max(h ** (N - 1), 1.0), abs(x0) + Lx
    first = None
    for comp in (False, True):
        cap = pj.Capacity(pj.Plane(normal, offset, complement=comp), mesh)
        ocap = _oracle_cap(case, comp)
        assert np.array_equal(cap.cell_types, ocap.cell_types)                                  # bit-exact classification
        assert np.array_equal(np.flatnonzero(cap.Γ > 0), np.flatnonzero(ocap.G > 0))
        assert np.array_equal(np.flatnonzero(cap.cell_types == -1), np.flatnonzero(cap.Γ > 0))  # Γ > 0 <=> CUT
        assert np.count_nonzero(cap.cell_types == -1) >= (1 if N == 1 else n)
        print(f"[plane caps] N={N} n={n} comp={comp}: dV {np.max(np.abs(cap.V - ocap.V)) / full:.2e} full, "
              f"dΓ {np.max(np.abs(cap.Γ - ocap.G)):.2e}")
        assert np.max(np.abs(cap.V - ocap.V)) <= 1e-12 * full
        assert np.max(np.abs(cap.Γ - ocap.G)) <= 1e-12 * face
        for d in range(N):
            assert np.max(np.abs(cap.A[d] - ocap.A[d])) <= 1e-12 * face
            assert np.max(np.abs(cap.B[d] - ocap.B[d])) <= 1e-12 * face
            assert np.max(np.abs(cap.W[d] - ocap.W[d])) <= 1e-12 * full
        big = ocap.V > 1e-3 * full
        assert np.max(np.abs(cap.C_ω[big] - ocap.C_w[big])) <= 1e-12 * span
        cutbig = big & (ocap.G > 0)
        assert np.max(np.abs(cap.C_γ[cutbig] - ocap.C_g[cutbig])) <= 1e-12 * span
        if not comp:
            first = cap.V.copy()
        else:
            assert np.sum(first) + np.sum(cap.V) == pytest.approx(Lx ** N, rel=1e-13)           # the phases tile the box


# ------------------------------------------------------------------------------------ 2. solve path, same capacities
def _mono_problem(pj, case, comp=False, own_geometry=False, steady=False):
    N, n, Lx, x0, normal, offset = case
    mesh, omesh = _meshes(pj, case)
    cap = pj.Capacity(pj.Plane(normal, offset, complement=comp), mesh)
    ocap = _oracle_cap(case, comp) if own_geometry else oracle_capacity_from_product(cap, omesh)
    f = (lambda x, y, z=0.0: 0.0) if steady else (lambda x, y, z, t: 0.0)      # a steady source has no time argument
    D = lambda x, y, z=0.0: 1.0
    return cap, ocap, pj.Phase(cap, pj.DiffusionOps(cap), f, D), po.Phase(ocap, po.make_diffusion_ops(ocap), f, D)


def _run_mono(pj, case, bci, obci, steps=4, own_geometry=False):
    N, n, Lx = case[0], case[1], case[2]
    M = (n + 1) ** N
    _, _, ph, oph = _mono_problem(pj, case, own_geometry=own_geometry)
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS})
    obcb = po.BorderConditions({k: po.Dirichlet(0.0) for k in KEYS})
    dt = (0.25 if N == 2 else 0.75) * (Lx / n) ** 2
    u0 = np.concatenate([np.zeros(M), np.ones(M)])
    s = pj.DiffusionUnsteadyMono(ph, bcb, bci, dt, u0, "BE")
    so = po.DiffusionUnsteadyMono(oph, obcb, obci, dt, u0, "BE")
    if own_geometry:
        _, _, idx = s.system(0)
        _, _, oidx = po.remove_zero_rows_cols(so.A, so.b)
        assert np.array_equal(idx, oidx)
    else:
        _check_system(s, so)
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, steps * dt, bcb, bci, "CN", reltol=1e-13)
    po.solve_DiffusionUnsteadyMono(so, oph, dt, steps * dt, obcb, obci, "CN", method="\\")
    assert len(s.states) == len(so.states) >= steps
    worst = max(rel_l2(a, b) for a, b in zip(s.states, so.states))
    print(f"[plane solve] N={N} n={n} own_geometry={own_geometry}: worst state difference {worst:.2e}")
    assert worst <= TOL_T
    assert float(np.max(np.abs(so.x[:M]))) > 1e-3                                               # something diffused in


@pytest.mark.parametrize("bc_kind", ["dirichlet", "robin"])
def test_mono_unsteady_be_then_cn_2d(pj, bc_kind):
    if bc_kind == "dirichlet":
        _run_mono(pj, CASE_2D, pj.Dirichlet(1.0), po.Dirichlet(1.0))
    else:
        _run_mono(pj, CASE_2D, pj.Robin(1.0, 0.5, 2.0), po.Robin(1.0, 0.5, 2.0))


def test_mono_unsteady_be_then_cn_3d(pj):
    _run_mono(pj, CASE_3D, pj.Dirichlet(1.0), po.Dirichlet(1.0))


def test_mono_steady_2d(pj):
    _, _, ph, oph = _mono_problem(pj, CASE_2D, steady=True)
    s = pj.DiffusionSteadyMono(ph, pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS}), pj.Dirichlet(1.0))
    so = po.DiffusionSteadyMono(oph, po.BorderConditions({k: po.Dirichlet(0.0) for k in KEYS}), po.Dirichlet(1.0))
    _check_system(s, so)
    pj.solve_DiffusionSteadyMono_b(s, reltol=1e-13)
    po.solve_DiffusionSteadyMono(so, method="\\")
    assert s.ch[-1]["converged"]
    assert rel_l2(s.x, so.x) <= TOL_T


def test_diphasic_unsteady_2d(pj):
    """Plane and its complement: an inclined two-phase interface with a Henry jump."""
    N, n, Lx, x0, normal, offset = CASE_2D
    M = (n + 1) ** N
    mesh, omesh = _meshes(pj, CASE_2D)
    cap1 = pj.Capacity(pj.Plane(normal, offset), mesh)
    cap2 = pj.Capacity(pj.Plane(normal, offset, complement=True), mesh)
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
    dt = 0.5 * (Lx / n) ** 2
    s = pj.DiffusionUnsteadyDiph(p1, p2, bcb, ic, dt, u0, "BE")
    so = po.DiffusionUnsteadyDiph(q1, q2, obcb, oic, dt, u0, "BE")
    _check_system(s, so)
    pj.solve_DiffusionUnsteadyDiph_b(s, p1, p2, dt, 5 * dt, bcb, ic, "BE", reltol=1e-13)
    po.solve_DiffusionUnsteadyDiph(so, q1, q2, dt, 5 * dt, obcb, oic, "BE", method="\\")
    assert len(s.states) == len(so.states)
    worst = max(rel_l2(a, b) for a, b in zip(s.states, so.states))
    print(f"[plane diphasic] worst state difference {worst:.2e}")
    assert worst <= TOL_T


# ------------------------------------------------------------------------------------ 3. independent geometry on both sides
@pytest.mark.parametrize("case", [CASE_2D, CASE_3D], ids=["24x24", "8x8x8"])
def test_end_to_end_independent_geometry(pj, case):
    N, n, Lx = case[0], case[1], case[2]
    full = (Lx / n) ** N
    thinnest = min(float(np.min(_oracle_cap(case, comp).V[_oracle_cap(case, comp).cell_types == -1])) for comp in (False, True)) / full
    print(f"[plane end to end] N={N} n={n}: thinnest cut cell {thinnest:.2e} of a full cell")
    assert thinnest >= 1e-4                      # the condition under which two geometries 1e-12 apart give states 1e-10 apart
    _run_mono(pj, case, pj.Dirichlet(1.0), po.Dirichlet(1.0), own_geometry=True)


# ------------------------------------------------------------------------------------ 4. order of convergence
ORACLE_ERRORS = {16: 8.69e-3, 32: 2.16e-3, 64: 5.58e-4}      # CPU oracle with exact plane geometry, same set-up


def test_second_order_on_an_inclined_wall(pj):
    """Unit square, Plane((0.6, 0.8), 0.83), BE, Δt = h²/4, Tend = 0.02, against erfc(distance / 2 sqrt(t)).  The border
    values are taken one spacing further in (x + h, y + h): mesh.centers = x0 + j h lie one spacing below the centres of
    the cells the unknowns belong to; without it the scheme itself is first order."""
    exact = lambda x, y, t: erfc((0.83 - 0.6 * np.asarray(x) - 0.8 * np.asarray(y)) / (2.0 * np.sqrt(t)))
    shifted = lambda h: (lambda x, y, t: exact(x + h, y + h, t))
    errs = {}
    for n in (16, 32, 64):
        h = 1.0 / n
        M = (n + 1) ** 2
        mesh = pj.Mesh((n, n), (1.0, 1.0), (0.0, 0.0))
        cap = pj.Capacity(pj.Plane((0.6, 0.8), 0.83), mesh)
        ph = pj.Phase(cap, pj.DiffusionOps(cap), lambda x, y, z, t: 0.0, lambda x, y, z: 1.0)
        with np.errstate(divide="ignore"):
            bcb = pj.BorderConditions({k: pj.Dirichlet(shifted(h)) for k in KEYS})
            dt = 0.25 * h * h
            u0 = np.concatenate([np.zeros(M), np.ones(M)])
            s = pj.DiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(1.0), dt, u0, "BE")
            pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 0.02, bcb, pj.Dirichlet(1.0), "BE", reltol=1e-13)
        t_final = len(s.states) * dt
        errs[n] = pj.check_convergence(lambda x, y: exact(x, y, t_final), s, cap, 2)[2]
    orders = [math.log(errs[a] / errs[b]) / math.log(2.0) for a, b in ((16, 32), (32, 64))]
    print(f"[plane convergence] errors {errs} pairwise orders {orders}")
    assert orders[0] > 1.5 and orders[1] > 1.5
    for n, ref in ORACLE_ERRORS.items():
        assert abs(errs[n] - ref) <= 0.01 * ref, (n, errs[n], ref)


# ------------------------------------------------------------------------------------ 5. ABI errors
def test_abi_refuses_bad_planes(pj):
    mesh = pj.Mesh((8, 8), (1.0, 1.0), (0.0, 0.0))
    with pytest.raises(pj.PenguinHipError, match="PG_BODY_PLANE"):
        pj.Capacity(pj.Plane((0.0, 0.0), 0.3), mesh)                                 # a zero normal
    with pytest.raises(pj.PenguinHipError, match="PG_BODY_PLANE"):
        pj.Capacity(pj.Plane((float("nan"), 1.0), 0.3), mesh)
    with pytest.raises(pj.PenguinHipError, match="PG_BODY_PLANE"):
        pj.Capacity(pj.Plane((0.6, 0.0, 0.8), 0.3), mesh)                            # a normal of the wrong dimension
    import ctypes as C
    params = np.array([0.6, 0.8])                                                   # the offset is missing
    h = C.c_void_p()
    with pytest.raises(pj.PenguinHipError, match="PG_BODY_PLANE"):
        L.check(L.lib().pg_capacity_create_levelset(mesh._h, C.c_int32(L.PG_BODY_PLANE), L.dptr(params), C.c_int32(2), C.c_int32(0),
                                                    C.byref(h)))
    # and the plane through a point
    p = pj.Plane.through((0.5, 0.25), (0.6, 0.8))
    assert p.offset == 0.6 * 0.5 + 0.8 * 0.25 and p(0.5, 0.25) == 0.0 and pj.Plane.through((0.5, 0.25), (0.6, 0.8), complement=True)(0.0, 0.0) > 0.0
