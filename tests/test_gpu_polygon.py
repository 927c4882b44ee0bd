"""Capacity(FrontTracker, mesh) on the GPU: the closed polygon of the markers measured inside the capacity kernels
(PG_BODY_POLYGON, penguin/jl_amd/csrc/pg_geom_polygon.h).  Against the exact rational arbiter tests/polygon_reference.py on every
case of tests/polygon_cases.py, the sum identities, repeatability, against Sphere, end to end against the oracle's direct solves,
Poisson convergence, and every refusal of the C entry.

Bars: tests/polygon_cases.py (10 times what the HOST build shows against the arbiter on the CPU, no floor; never from the GPU).
Every figure is printed before it is held to its bar.  Measured on an MI355X: DESIGN.md section 25."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import penguin_oracle as po
from tests import polygon_cases as pc
from tests.common import oracle_capacity_from_product, rel_l2
from tests.levelset_cases import unit

pytestmark = pytest.mark.gpu

TOL_T = 1e-10
KEYS = ("left", "right", "top", "bottom")


def _cap(pj, name):
    make, n, L, x0, comp = pc.CASES[name]
    return pj.Capacity(make(), pj.Mesh(n, L, x0), complement=comp)


def _arrays(cap):
    return (cap.V, cap.Γ, cap.C_ω, cap.C_γ, cap.cell_types, *cap.A, *cap.B, *cap.W)


# ------------------------------------------------------------------------------------ 1. against the arbiter
@pytest.mark.parametrize("name", pc.ARBITRATED)
def test_capacities_match_the_arbiter(pj, name):
    cap, ref = _cap(pj, name), pc.reference(name)
    assert np.array_equal(cap.cell_types, ref.cell_types)
    assert np.array_equal(np.flatnonzero(cap.Γ > 0), np.flatnonzero(ref.G > 0))
    pc.check(name, cap, ref, what="gpu ")


def test_complement_tiles_every_cell_and_face(pj):
    a, b = _cap(pj, "circle_16"), _cap(pj, "complement_16")
    h = 0.25
    assert np.array_equal(a.cell_types == -1, b.cell_types == -1)
    real = np.zeros((17, 17), dtype=bool)
    real[:16, :16] = True
    real = real.ravel()
    assert np.array_equal((a.cell_types + b.cell_types)[real & (a.cell_types != -1)], np.ones(np.count_nonzero(real & (a.cell_types != -1))))
    dv = np.max(np.abs(a.V + b.V - h * h)[real])
    print(f"[polygon gpu complement] V + V_c - h^2: {dv:.3g}")
    assert dv <= 4 * 2.0 ** -52 * h * h
    for d in range(2):
        face = np.ones((17, 17), dtype=bool)                      # [j, i]: A_d exists on the padding face of d itself only
        face[(16, slice(None)) if d == 0 else (slice(None), 16)] = False
        da = np.max(np.abs(a.A[d] + b.A[d] - h)[face.ravel()])
        print(f"[polygon gpu complement] A_{d} + A_c_{d} - h: {da:.3g}")
        assert da <= 4 * 2.0 ** -52 * h


@pytest.mark.parametrize("name", pc.SQUARES)
def test_squares_on_node_and_centre_lines(pj, name):
    cap, ref = _cap(pj, name), pc.reference(name)
    assert np.array_equal(cap.cell_types, ref.cell_types)
    assert np.array_equal(cap.V, ref.V)
    assert float(np.sum(cap.Γ)) == 8.0
    for a in _arrays(cap):
        assert np.all(np.isfinite(a))
    if name == "node_square_16":
        assert np.count_nonzero(cap.cell_types == -1) == 0 and np.count_nonzero(cap.Γ > 0) == 31


@pytest.mark.parametrize("name", list(pc.CASES))
def test_sum_identities(pj, name):
    pc.check_identities(name, _cap(pj, name), what="gpu ")


def test_two_builds_agree_bit_for_bit(pj):
    a, b = _cap(pj, "crystal_24"), _cap(pj, "crystal_24")
    for x, y in zip(_arrays(a), _arrays(b)):
        assert np.array_equal(x, y)


def test_each_kernel_and_the_binning_report_their_time(pj):
    cap = _cap(pj, "circle_16")
    ms = cap.kernel_ms_parts
    assert all(ms[k] > 0.0 for k in ("classify", "cut_cells", "sections", "stagger", "stagger_cut"))
    both = cap.polygon_ms_parts
    assert both["binning"] > 0.0 and all(both[k] == ms[k] for k in ms)


def test_a_polygon_beside_or_around_the_mesh(pj):
    """no edge reaches a cell: nothing is listed, no cut kernel is launched, the types come from the parity alone"""
    mesh = pj.Mesh((12, 9), (3.0, 2.0), (0.1, -0.2))
    away = pj.Capacity(pc.circle(10.0, 10.0, 1.0, 32), mesh)
    assert np.all(away.cell_types == 0.0) and np.all(away.V == 0.0) and np.all(away.Γ == 0.0)
    assert away.kernel_ms_parts["cut_cells"] == 0.0 and away.kernel_ms_parts["stagger_cut"] == 0.0
    around = pj.Capacity(pc.circle(1.5, 1.0, 10.0, 32), mesh)
    real = np.zeros((10, 13), dtype=bool)
    real[:9, :12] = True
    assert np.all(around.cell_types[real.ravel()] == 1.0) and np.all(around.V[real.ravel()] == (3.0 / 12) * (2.0 / 9))
    outside = pj.Capacity(pc.circle(1.5, 1.0, 10.0, 32), mesh, complement=True)
    assert np.all(outside.cell_types == 0.0)


# ------------------------------------------------------------------------------------ 2. against Sphere
def test_fine_circle_against_sphere(pj):
    """an inscribed polygon of M markers lies within the sagitta r (1 - cos(pi / M)) <= r pi^2 / (2 M^2) of its circle: per cell
    the volumes differ by at most (the arc length in the cell) times that, plus the rounding bar of circle_16's V"""
    M, r = 4096, 1.0
    mesh = pj.Mesh((16, 16), (4.0, 4.0), (0.0, 0.0))
    cap = pj.Capacity(pc.circle(2.01, 2.01, r, M), mesh)
    ref = pj.Capacity(pj.Sphere((2.01, 2.01), r), mesh)
    u, h = unit((0.0, 0.0), (4.0, 4.0), (16, 16))
    bound = ref.Γ * r * math.pi ** 2 / (2.0 * M * M) + pc.BARS["circle_16"]["V"] * u * h * h
    excess = np.max(np.abs(cap.V - ref.V) - bound)
    print(f"[polygon gpu sphere] worst |dV| {np.max(np.abs(cap.V - ref.V)):.3g}, worst excess over the bound {excess:.3g}")
    assert excess <= 0.0
    assert abs(np.sum(cap.Γ) - 2.0 * math.pi * r) <= 2.0 * math.pi * r * math.pi ** 2 / (6.0 * M * M) + 1e-13


# ------------------------------------------------------------------------------------ 3. end to end on circle_16's polygon, 24^2
N24 = ((24, 24), (4.0, 4.0), (0.0, 0.0))


def _front():
    return pc.circle(2.01, 2.01, 1.0, 40)


def _check_system(s, so):
    A, b, idx = s.system(0)
    Ar, br, oidx = po.remove_zero_rows_cols(so.A, so.b)
    assert np.array_equal(idx, oidx)
    A = A[:, : len(idx)]
    assert abs(A - Ar).max() <= 1e-12 * abs(Ar).max()
    assert np.max(np.abs(b - br)) <= 1e-12 * max(np.max(np.abs(br)), 1e-300)


def _mono(pj, steady=False):
    mesh, omesh = pj.Mesh(*N24), po.Mesh(*N24)
    cap = pj.Capacity(_front(), mesh)
    ocap = oracle_capacity_from_product(cap, omesh)
    f = (lambda x, y, z=0.0: 0.0) if steady else (lambda x, y, z, t: 0.0)
    D = lambda x, y, z=0.0: 1.0
    return pj.Phase(cap, pj.DiffusionOps(cap), f, D), po.Phase(ocap, po.make_diffusion_ops(ocap), f, D)


@pytest.mark.parametrize("bc_kind", ["dirichlet", "robin"])
def test_mono_unsteady_be_then_cn(pj, bc_kind):
    bci, obci = (pj.Dirichlet(1.0), po.Dirichlet(1.0)) if bc_kind == "dirichlet" else (pj.Robin(1.0, 0.5, 2.0), po.Robin(1.0, 0.5, 2.0))
    ph, oph = _mono(pj)
    M = 25 * 25
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS})
    obcb = po.BorderConditions({k: po.Dirichlet(0.0) for k in KEYS})
    dt = 0.25 * (4.0 / 24) ** 2
    u0 = np.concatenate([np.zeros(M), np.ones(M)])
    s = pj.DiffusionUnsteadyMono(ph, bcb, bci, dt, u0, "BE")
    so = po.DiffusionUnsteadyMono(oph, obcb, obci, dt, u0, "BE")
    _check_system(s, so)
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 4 * dt, bcb, bci, "CN", reltol=1e-13)
    po.solve_DiffusionUnsteadyMono(so, oph, dt, 4 * dt, obcb, obci, "CN", method="\\")
    assert len(s.states) == len(so.states) >= 4
    worst = max(rel_l2(a, b) for a, b in zip(s.states, so.states))
    print(f"[polygon solve {bc_kind}] worst state difference {worst:.2e}")
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
    M = 25 * 25
    mesh, omesh = pj.Mesh(*N24), po.Mesh(*N24)
    cap1 = pj.Capacity(_front(), mesh)
    cap2 = pj.Capacity(_front(), mesh, complement=True)
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
    dt = 0.5 * (4.0 / 24) ** 2
    s = pj.DiffusionUnsteadyDiph(p1, p2, bcb, ic, dt, u0, "BE")
    so = po.DiffusionUnsteadyDiph(q1, q2, obcb, oic, dt, u0, "BE")
    _check_system(s, so)
    pj.solve_DiffusionUnsteadyDiph_b(s, p1, p2, dt, 4 * dt, bcb, ic, "BE", reltol=1e-13)
    po.solve_DiffusionUnsteadyDiph(so, q1, q2, dt, 4 * dt, obcb, oic, "BE", method="\\")
    assert len(s.states) == len(so.states)
    worst = max(rel_l2(a, b) for a, b in zip(s.states, so.states))
    print(f"[polygon diphasic] worst state difference {worst:.2e}")
    assert worst <= TOL_T


# ------------------------------------------------------------------------------------ 4. convergence
def test_poisson_in_a_disc_of_markers_converges(pj):
    """-lap u = 4 / R^2 in the disc of radius R = 1 about (2.01, 2.01), u = 0 on it: u = 1 - r^2 / R^2.  The disc is the polygon
    of M = 8 n markers on n^2 cells, n = 16, 32, 64.  Volume-weighted L2 error of the bulk unknowns at the cell centroids; the
    order between successive meshes must exceed 1.0, the bar of DESIGN.md section 23.  Measured on an MI355X: DESIGN.md section 25
    (the figures are printed by this test)."""
    R, c = 1.0, (2.01, 2.01)
    errs = {}
    for n in (16, 32, 64):
        M = (n + 1) ** 2
        cap = pj.Capacity(pc.circle(c[0], c[1], R, 8 * n), pj.Mesh((n, n), (4.0, 4.0), (0.0, 0.0)))
        ph = pj.Phase(cap, pj.DiffusionOps(cap), lambda x, y, z=0.0: 4.0 / R ** 2, lambda x, y, z=0.0: 1.0)
        s = pj.DiffusionSteadyMono(ph, pj.BorderConditions({}), pj.Dirichlet(0.0))
        pj.solve_DiffusionSteadyMono_b(s, reltol=1e-13)
        V, Cw = cap.V, cap.C_ω
        inside = V > 0.0
        exact = 1.0 - ((Cw[:, 0] - c[0]) ** 2 + (Cw[:, 1] - c[1]) ** 2) / R ** 2
        errs[n] = math.sqrt(np.sum(V[inside] * (s.x[:M][inside] - exact[inside]) ** 2) / np.sum(V[inside]))
    orders = [math.log(errs[p] / errs[q]) / math.log(2.0) for p, q in ((16, 32), (32, 64))]
    print(f"[polygon poisson] errors {errs} orders {orders}")
    assert errs[16] < 0.1
    assert orders[0] > 1.0 and orders[1] > 1.0


# ------------------------------------------------------------------------------------ 5. refusals
def _last_error():
    from penguin.jl_amd import _lib as L
    buf = C.create_string_buffer(4096)
    L.lib().pg_last_error(buf, 4096)
    return buf.value.decode("utf-8", "replace")


def test_the_entry_refuses_each_with_its_own_message(pj):
    """pg_capacity_create_polygon itself (polygon_body_check is tested message by message in tests/test_polygon_host.py): every
    refusal comes back as an error with no capacity, and a good call after them still works."""
    from penguin.jl_amd import _lib as L
    lib = L.lib()
    mesh = pj.Mesh((16, 16), (4.0, 4.0), (0.0, 0.0))

    def call(m, pts):
        h = C.c_void_p(12345)
        xy = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1)) if pts is not None else None
        rc = lib.pg_capacity_create_polygon(m._h, L.dptr(xy) if xy is not None else None, C.c_int64(len(pts) if pts is not None else 4),
                                            C.c_int32(0), C.byref(h))
        assert (rc == 0) == bool(h.value)
        return rc, _last_error(), h

    good = [(1.0, 1.0), (3.0, 1.2), (2.0, 3.0)]
    cases = [
        (pj.Mesh((8,), (4.0,), (0.0,)), good, "2-D body, the mesh is 1-D"),
        (pj.Mesh((4, 4, 4), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), good, "2-D body, the mesh is 3-D"),
        (mesh, None, "NULL marker array"),
        (mesh, good[:2], "at least 3 markers (got 2)"),
        (mesh, good[:2] + good[:1], "at least 3 markers (got 2)"),
        (mesh, [(1.0, 1.0), (3.0, float("nan")), (2.0, 3.0)], "marker 1 has a non-finite coordinate"),
        (mesh, [(1.0, 1.0), (3.0, 1.0), (3.0, 1.0), (2.0, 3.0)], "zero-length edge: markers 1 and 2 coincide"),
        (mesh, [(1.0, 1.0), (2.0, 2.0), (3.0, 3.0)], "zero signed area"),
        (mesh, [(0.0, 0.0), (2.0, 0.0), (2.0, 1.0), (1.0, -1.0), (0.0, 2.0)], "intersects itself: edges 0 and 2"),
    ]
    for m, pts, want in cases:
        rc, msg, _ = call(m, pts)
        assert rc != 0 and want in msg, (want, rc, msg)
    for pts in (good, good[::-1], good + good[:1]):            # either orientation, with or without the closing duplicate
        rc, _, h = call(mesh, pts)
        assert rc == 0
        lib.pg_capacity_destroy(h)


def test_a_front_behind_a_communicator_is_refused():
    """The one-rank refusal (`nranks == 1 && !comm`) through its communicator half: a 1-rank RCCL communicator on one GPU, in a
    fresh child process (the library is initialised once per process), as tests/test_gpu_levelset.py does for program bodies."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    env = {**os.environ, "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    r = subprocess.run([sys.executable, str(root / "scripts" / "polygon_rank_refusal.py")], cwd=root, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "single rank only" in r.stdout


def test_orientation_and_body(pj):
    """clockwise markers give the same capacity; cap.body is the front, callable as its signed distance"""
    make, n, L, x0, _ = pc.CASES["circle_16"]
    f = make()
    mesh = pj.Mesh(n, L, x0)
    a = pj.Capacity(f, mesh)
    b = pj.Capacity(pj.FrontTracker([f.markers[0]] + f.markers[:0:-1]), mesh)
    for x, y in zip(_arrays(a), _arrays(b)):
        assert np.array_equal(x, y)
    assert a.body is f and a.body(2.01, 2.01) < 0.0 < a.body(0.0, 0.0)
    nc = pj.Capacity(f, mesh, compute_centroids=False)
    assert np.array_equal(nc.V, a.V) and nc.C_γ.shape == (0, 2)
