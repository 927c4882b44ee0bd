"""Capacity(DeviceFunction(...), mesh) on the GPU: traced level sets evaluated inside the capacity kernels (PG_BODY_PROGRAM,
penguin/jl_amd/csrc/pg_geom_program.h).  Against the 30-digit fixture tests/golden/levelset_cells.json, against the closed-form
kinds through the product itself, the edges of the work lists, and end to end against the oracle's direct solves.

Bars: tests/levelset_cases.py (c * 2^-52 (|x0| + L) / h per quantity, c from the host build on the CPU, never from the GPU).
Every figure is printed before it is held to its bar.

Poisson orders measured on an MI355X (test_poisson_in_a_rotated_ellipse_converges): see the test's docstring."""
import functools
import math

import numpy as np
import pytest

from oracle import penguin_oracle as po
from tests import levelset_cases as lc
from tests.common import oracle_capacity_from_product, rel_l2

pytestmark = pytest.mark.gpu

TOL_T = 1e-10
KEYS = ("left", "right", "top", "bottom")
SQ = ((0.0, 0.0), (4.0, 4.0))


@functools.lru_cache(maxsize=None)
def _fixture():
    return lc.load_fixture()


def _body(pj, name):
    make, comp = lc.FIXTURE_BODIES[name]
    return pj.DeviceFunction(make(), complement=comp)


# ------------------------------------------------------------------------------------ 1. against the fixture
@pytest.mark.parametrize("name", list(lc.FIXTURE_BODIES))
def test_capacities_match_the_fixture(pj, name):
    f = _fixture()[name]
    cap = pj.Capacity(_body(pj, name), pj.Mesh(f.n, f.L, f.x0))
    assert np.array_equal(cap.cell_types, f.cell_types)
    assert np.array_equal(np.flatnonzero(cap.Γ > 0), np.flatnonzero(f.G > 0))
    lc.check(name, cap, f, f.x0, f.L, f.n, what="gpu ")
    if name == "discs_24":
        lc.check("discs_24_smooth", lc.Masked(cap, f, (f.n[0] + 1, f.n[1] + 1)), f, f.x0, f.L, f.n, what="gpu ")
        lc.check_kink(cap, f, f.L, f.n, what="gpu ")


def test_phases_tile_the_box(pj):
    f = _fixture()["ellipse_16"]
    mesh = pj.Mesh(f.n, f.L, f.x0)
    v1 = pj.Capacity(_body(pj, "ellipse_16"), mesh).V
    v2 = pj.Capacity(_body(pj, "ellipse_complement_16"), mesh).V
    assert np.sum(v1) + np.sum(v2) == pytest.approx(16.0, rel=1e-13)


# ------------------------------------------------------------------------------------ 2. against the closed-form kinds
def _same(pj, bars, prog, tagged, n, L=(4.0, 4.0), x0=(0.0, 0.0)):
    mesh = pj.Mesh(n, L, x0)
    cap, ref = pj.Capacity(pj.DeviceFunction(prog), mesh), pj.Capacity(tagged, mesh)
    assert np.array_equal(cap.cell_types, ref.cell_types)
    assert np.count_nonzero(cap.cell_types == -1) >= 1
    lc.check(bars, cap, ref, x0, L, n, what=f"gpu n={n} ")


@pytest.mark.parametrize("n", [16, 24])
def test_circle_against_sphere(pj, n):
    _same(pj, "circle", lc.circle(), pj.Sphere((2.01, 2.01), 1.0), (n, n))


@pytest.mark.parametrize("n", [16, 24])
def test_ellipse_at_angle_zero_against_ellipse(pj, n):
    _same(pj, "ellipse0", lc.ellipse_sqrt(2.01, 1.97, 1.3, 0.6), pj.Ellipse((2.01, 1.97), (1.3, 0.6)), (n, n))


@pytest.mark.parametrize("n", [16, 24])
def test_plane_against_plane(pj, n):
    _same(pj, "plane", lc.plane(0.6, -0.8, 0.31), pj.Plane((0.6, -0.8), 0.31), (n, n))


def test_plane_on_a_node_line(pj):
    """x = 1.375 is the node line i = 5 of Mesh((16, 16), (4, 4)) (nodes at (j + 1/2) / 4): phi is exactly 0 on it.  The cells on
    the left are FULL (phi <= 0 is fluid), those on the right only touch the interface and are EMPTY: no cut cell."""
    mesh = pj.Mesh((16, 16), (4.0, 4.0), (0.0, 0.0))
    for comp in (False, True):
        cap = pj.Capacity(pj.DeviceFunction(lc.plane(1.0, 0.0, 1.375), complement=comp), mesh)
        ref = pj.Capacity(pj.Plane((1.0, 0.0), 1.375, complement=comp), mesh)
        assert np.array_equal(cap.cell_types, ref.cell_types)
        assert np.count_nonzero(cap.cell_types == -1) == 0
        lc.check("plane", cap, ref, (0.0, 0.0), (4.0, 4.0), (16, 16), what=f"gpu node line comp={comp} ")


def test_half_line_in_1d_against_halfspace(pj):
    mesh = pj.Mesh((10,), (1.0,), (0.0,))
    cap, ref = pj.Capacity(pj.DeviceFunction(lambda x: x - 0.37), mesh), pj.Capacity(pj.HalfSpace(0, 0.37), mesh)
    assert np.array_equal(cap.cell_types, ref.cell_types)
    assert np.count_nonzero(cap.cell_types == -1) == 1
    lc.check("halfspace1d", cap, ref, (0.0,), (1.0,), (10,), what="gpu ")


# ------------------------------------------------------------------------------------ 3. work-list edges
def test_negative_everywhere_is_all_full_and_launches_no_cut_kernel(pj):
    mesh = pj.Mesh((12, 9), (3.0, 2.0), (0.1, -0.2))
    cap = pj.Capacity(pj.DeviceFunction(lambda x, y: -1.0 - x * x), mesh)
    real = np.zeros((10, 13), dtype=bool)
    real[:9, :12] = True
    assert np.all(cap.cell_types[real.ravel()] == 1.0) and np.all(cap.cell_types[~real.ravel()] == 0.0)
    assert np.all(cap.Γ == 0.0)
    h2 = (3.0 / 12) * (2.0 / 9)
    assert np.all(cap.V[real.ravel()] == h2)
    assert np.all(cap.W[0][real.ravel()].reshape(9, 12)[:, 1:] == h2)
    ms = cap.kernel_ms_parts                     # each kernel between its own events; 0.0: never launched
    assert ms["cut_cells"] == 0.0 and ms["stagger_cut"] == 0.0
    assert ms["classify"] > 0.0 and ms["sections"] > 0.0 and ms["stagger"] > 0.0
    cut = pj.Capacity(_body(pj, "ellipse_16"), pj.Mesh((16, 16), (4.0, 4.0), (0.0, 0.0))).kernel_ms_parts
    assert cut["cut_cells"] > 0.0 and cut["stagger_cut"] > 0.0


def test_positive_everywhere_is_all_empty(pj):
    cap = pj.Capacity(pj.DeviceFunction(lambda x, y: 1.0 + y * y), pj.Mesh((12, 9), (3.0, 2.0), (0.1, -0.2)))
    assert np.all(cap.cell_types == 0.0) and np.all(cap.V == 0.0) and np.all(cap.Γ == 0.0)
    assert all(np.all(cap.A[d] == 0.0) and np.all(cap.B[d] == 0.0) and np.all(cap.W[d] == 0.0) for d in range(2))


def test_cut_count_that_is_no_multiple_of_the_lane_group(pj):
    f = _fixture()["ellipse_17x13"]
    assert np.count_nonzero(f.cell_types == -1) % 16 != 0        # 34 cut cells: the last block of k_cut_cells is ragged
    cap = pj.Capacity(_body(pj, "ellipse_17x13"), pj.Mesh(f.n, f.L, f.x0))
    assert np.count_nonzero(cap.cell_types == -1) == np.count_nonzero(f.cell_types == -1)


def test_under_resolved_disc_is_finite_and_bounded(pj):
    h = 4.0 / 16
    cap = pj.Capacity(pj.DeviceFunction(lc.circle(2.03, 2.01, 0.6 * h)), pj.Mesh((16, 16), (4.0, 4.0), (0.0, 0.0)))
    for a in (cap.V, cap.Γ, cap.C_ω, cap.C_γ, *cap.A, *cap.B, *cap.W):
        assert np.all(np.isfinite(a))
    assert np.all(cap.V >= 0.0) and np.all(cap.V <= h * h) and np.all(cap.Γ >= 0.0)
    assert all(np.all(cap.A[d] >= 0.0) and np.all(cap.A[d] <= h) and np.all(cap.B[d] >= 0.0) and np.all(cap.B[d] <= h)
               for d in range(2))
    assert 0.0 < np.sum(cap.V) < 4.0 * h * h


def test_two_builds_agree_bit_for_bit(pj):
    f = _fixture()["discs_24"]
    mesh = pj.Mesh(f.n, f.L, f.x0)
    a, b = pj.Capacity(_body(pj, "discs_24"), mesh), pj.Capacity(_body(pj, "discs_24"), mesh)
    for x, y in ((a.V, b.V), (a.Γ, b.Γ), (a.C_ω, b.C_ω), (a.C_γ, b.C_γ), (a.cell_types, b.cell_types),
                 *zip(a.A, b.A), *zip(a.B, b.B), *zip(a.W, b.W)):
        assert np.array_equal(x, y)


def test_a_plain_callable_is_still_refused(pj):
    mesh = pj.Mesh((8, 8), (1.0, 1.0), (0.0, 0.0))
    with pytest.raises(pj.PenguinHipError, match="DeviceFunction"):
        pj.Capacity(lambda x, y: x + y - 1.0, mesh)
    with pytest.raises(pj.PenguinHipError, match="3-D"):
        pj.Capacity(pj.DeviceFunction(lambda x, y, z: x + y + z - 1.0), pj.Mesh((4, 4, 4), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)))


def _last_error():
    import ctypes as C
    from penguin.jl_amd import _lib as L
    buf = C.create_string_buffer(4096)
    L.lib().pg_last_error(buf, 4096)
    return buf.value.decode("utf-8", "replace")


def test_the_entry_refuses_each_with_its_own_message(pj):
    """pg_capacity_create_program itself (the host-side check is tested message by message in tests/test_levelset_host.py): every
    refusal comes back as an error with no capacity, and a good call after them still works."""
    import ctypes as C
    from penguin.jl_amd import _lib as L
    from penguin.jl_amd.devfn import pg_program
    lib = L.lib()
    mesh = pj.Mesh((16, 16), (4.0, 4.0), (0.0, 0.0))
    df = pj.DeviceFunction(lc.circle())
    phi, grad = df.body_program(2), (pg_program * 2)(*df.gradient_programs(2))

    def call(m, p, g):
        h = C.c_void_p()
        rc = lib.pg_capacity_create_program(m._h, C.byref(p) if p is not None else None, g, C.c_int32(0), C.byref(h))
        assert (rc == 0) == bool(h.value)
        return rc, _last_error(), h

    bad = pg_program.from_buffer_copy(phi)
    bad.op[0] = 200
    cases = [
        (mesh, None, grad, "NULL argument"),
        (mesh, phi, None, "grad == NULL"),
        (mesh, bad, grad, "level-set program is invalid"),
        (mesh, phi, (pg_program * 2)(grad[0], bad), "gradient program 1 is invalid"),
        (mesh, pj.DeviceFunction(lambda x, y, z, t: x + y - t).program_for(3), grad, "reads t"),
        (mesh, pj.DeviceFunction(lambda x, y, z: x + y + z - 1.0).body_program(3), grad, "reads coordinate 2"),
        (pj.Mesh((4, 4, 4), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), phi, grad, "3-D"),
        (mesh, phi, (pg_program * 2)(grad[1], grad[0]), "central differences"),
    ]
    for m, p, g, want in cases:
        rc, msg, _ = call(m, p, g)
        assert rc != 0 and want in msg, (want, rc, msg)
    rc, _, h = call(mesh, phi, grad)
    assert rc == 0
    lib.pg_capacity_destroy(h)


def test_a_body_behind_a_communicator_is_refused():
    """The one-rank refusal (`nranks == 1 && !comm`) through its communicator half: a 1-rank RCCL communicator on one GPU, in a
    fresh child process (the library is initialised once per process), as tests/test_gpu_device_function.py does for programs
    in solvers.  The child checks the message of the C entry and of Capacity(DeviceFunction) itself."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    env = {**os.environ, "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    r = subprocess.run([sys.executable, str(root / "scripts" / "levelset_rank_refusal.py")], cwd=root, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "single rank only" in r.stdout


def test_complement_keyword_and_body_only_flag(pj):
    mesh = pj.Mesh((16, 16), (4.0, 4.0), (0.0, 0.0))
    a = pj.Capacity(pj.DeviceFunction(lc.rotated_ellipse()), mesh, complement=True)
    b = pj.Capacity(pj.DeviceFunction(lc.rotated_ellipse(), complement=True), mesh)
    assert np.array_equal(a.V, b.V) and np.array_equal(a.cell_types, b.cell_types) and a.body.complement
    assert a.body(2.01, 1.97) == 1.0                                  # -phi at the centre
    with pytest.raises(pj.PenguinHipError, match="DeviceFunction bodies"):
        pj.Capacity(pj.Sphere((2.0, 2.0), 1.0), mesh, complement=True)
    with pytest.raises(pj.PenguinHipError, match="BODY"):
        pj.DeviceFunction(lambda x, y, z, t: x + t, complement=True).program


# ------------------------------------------------------------------------------------ 4. end to end on the rotated ellipse, 24^2
N24 = ((24, 24), (4.0, 4.0), (0.0, 0.0))


def _check_system(s, so):
    A, b, idx = s.system(0)
    Ar, br, oidx = po.remove_zero_rows_cols(so.A, so.b)
    assert np.array_equal(idx, oidx)
    A = A[:, : len(idx)]
    assert abs(A - Ar).max() <= 1e-12 * abs(Ar).max()
    assert np.max(np.abs(b - br)) <= 1e-12 * max(np.max(np.abs(br)), 1e-300)


def _mono(pj, steady=False):
    mesh, omesh = pj.Mesh(*N24), po.Mesh(*N24)
    cap = pj.Capacity(pj.DeviceFunction(lc.rotated_ellipse()), mesh)
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
    print(f"[levelset solve {bc_kind}] worst state difference {worst:.2e}")
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
    cap1 = pj.Capacity(pj.DeviceFunction(lc.rotated_ellipse()), mesh)
    cap2 = pj.Capacity(pj.DeviceFunction(lc.rotated_ellipse(), complement=True), mesh)
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
    print(f"[levelset diphasic] worst state difference {worst:.2e}")
    assert worst <= TOL_T


# ------------------------------------------------------------------------------------ 5. convergence
def test_poisson_in_a_rotated_ellipse_converges(pj):
    """-lap u = 2 (1 / a^2 + 1 / b^2) inside the ellipse turned by 0.5 rad, u = 0 on it: u = 1 - q(x, y), q the body's quadratic
    form.  Volume-weighted L2 error of the bulk unknowns at the cell centroids on 16^2, 32^2, 64^2; the order between
    successive meshes must exceed 1.0, the reference's own bar for its convergence suites (orders.all > 1.0).
    Measured on an MI355X: see DESIGN.md section 23 (the figures are printed by this test)."""
    a, b = 1.3, 0.6
    phi = lc.rotated_ellipse()
    src = 2.0 * (1.0 / a ** 2 + 1.0 / b ** 2)
    errs = {}
    for n in (16, 32, 64):
        M = (n + 1) ** 2
        cap = pj.Capacity(pj.DeviceFunction(phi), pj.Mesh((n, n), (4.0, 4.0), (0.0, 0.0)))
        ph = pj.Phase(cap, pj.DiffusionOps(cap), lambda x, y, z=0.0: src, lambda x, y, z=0.0: 1.0)
        s = pj.DiffusionSteadyMono(ph, pj.BorderConditions({}), pj.Dirichlet(0.0))
        pj.solve_DiffusionSteadyMono_b(s, reltol=1e-13)
        V, C = cap.V, cap.C_ω
        inside = V > 0.0
        exact = -phi(C[:, 0], C[:, 1])
        errs[n] = math.sqrt(np.sum(V[inside] * (s.x[:M][inside] - exact[inside]) ** 2) / np.sum(V[inside]))
    orders = [math.log(errs[p] / errs[q]) / math.log(2.0) for p, q in ((16, 32), (32, 64))]
    print(f"[levelset poisson] errors {errs} orders {orders}")
    assert errs[16] < 0.1                        # (u is O(1): the sign convention of the source is right)
    assert orders[0] > 1.0 and orders[1] > 1.0
