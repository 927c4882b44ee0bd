"""Edge rows of the marching units (pg_spmv.hip "edge rows"): the irregular rows at the ends of the marched ranges are computed
by the units from per-row values.  y must stay bitwise what the CSR kernels give, for the run matrix and for the matrix the
warm loop iterates on, in every launch mode; the image must show the rows (rows_edge > 0) and fewer rows in the packed
irregular chunks than the CSR has rows with values of their own."""
import ctypes as C
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _solver(pj, case):
    if case == "sphere80_be":
        # the same sphere on twice the cells: chords of up to 40 cells, runs of the default length -- the image that ships
        mesh = pj.Mesh((80, 72, 64), (4.0, 4.0, 4.0))
        cap = pj.Capacity(pj.Sphere((2.01, 2.01, 2.01), 1.0), mesh)
        bcb = pj.BorderConditions({k: pj.Dirichlet(1.0) for k in ("left", "right", "top", "bottom")})
        dt, scheme = 5e-4, "BE"
    elif case in ("sphere_be", "sphere_cn"):
        mesh = pj.Mesh((40, 36, 32), (4.0, 4.0, 4.0))
        cap = pj.Capacity(pj.Sphere((2.01, 2.01, 2.01), 1.0), mesh)
        bcb = pj.BorderConditions({k: pj.Dirichlet(1.0) for k in ("left", "right", "top", "bottom")})
        dt, scheme = 2e-3, ("BE" if case == "sphere_be" else "CN")
    elif case == "offcentre":
        # the off-centre ball of test_gpu_parity's mono3d_march_offcentre on half the cells per direction
        mesh = pj.Mesh((48, 40, 36), (2.0, 1.7, 1.5), (0.1, -0.2, 0.05))
        cap = pj.Capacity(pj.Sphere((0.5, 0.3, 0.4), 0.9), mesh)
        bcb = pj.BorderConditions({"left": pj.Dirichlet(0.0), "top": pj.Dirichlet(2.0), "backward": pj.Dirichlet(1.0)})
        dt, scheme = 4e-4, "BE"
    elif case == "disc2d":
        mesh = pj.Mesh((96, 80), (4.0, 4.0))
        cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.6), mesh)
        bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in ("left", "right", "top", "bottom")})
        dt, scheme = 1e-3, "CN"
    else:
        assert case == "two_balls"
        mesh = pj.Mesh((96, 32, 32), (6.0, 2.0, 2.0))
        cap = pj.Capacity(pj.MultiSphere([(1.5, 1.0, 1.0), (4.4, 1.02, 0.97)], 0.9), mesh)
        bcb = pj.BorderConditions({k: pj.Dirichlet(1.0) for k in ("left", "right", "top", "bottom")})
        dt, scheme = 1e-3, "CN"
    ph = pj.Phase(cap, pj.DiffusionOps(cap), 0.0, 1.0)
    s = pj.DiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(1.0), dt, None, scheme)
    return s, ph, bcb, dt, scheme


_CACHE = {}


def _stepped(pj, case):
    """The solver after its initial solve and one step of the time loop (run matrix and loop matrix exist), once per case."""
    if case not in _CACHE:
        s, ph, bcb, dt, scheme = _solver(pj, case)
        pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 0.5 * dt, bcb, pj.Dirichlet(1.0), scheme, reltol=1e-12)   # first solve + one step
        _CACHE[case] = s
    return _CACHE[case]


def _info(s, which):
    from penguin.jl_amd import _lib as L
    info = L.pg_system_info()
    L.check(L.lib().pg_solver_system_info(s._h, C.c_int32(which), C.byref(info)))
    return info


def _rows_outside_uniform_runs(s, which):
    """Rows of the preconditioned CSR that are in no run of at least PG_SPMV_MINRUN (24) consecutive rows with one stencil --
    same entry count, same col - row offsets, bitwise the same values: the rows whose values a kernel has to read row by row,
    whatever the format."""
    from penguin.jl_amd import _lib as L
    n, nnz = _info(s, which).n_own, _info(s, which).nnz
    rp, col, val = np.zeros(n + 1, np.int64), np.zeros(nnz, np.int64), np.zeros(nnz)
    L.check(L.lib().pg_solver_get_system_csr(s._h, C.c_int32(which), rp.ctypes.data_as(C.POINTER(C.c_int64)),
                                             col.ctypes.data_as(C.POINTER(C.c_int64)), val.ctypes.data_as(C.POINTER(C.c_double)),
                                             None, None))
    minrun = int(os.environ.get("PG_SPMV_MINRUN", "24"))
    bits = val.view(np.int64)
    outside, start = 0, 0
    for r in range(1, n + 1):
        same = False
        if r < n:
            a, b, p = rp[r], rp[r + 1], rp[r - 1]
            same = b - a == a - p and np.array_equal(col[a:b] - 1, col[p:a]) and np.array_equal(bits[a:b], bits[p:a])
        if not same:
            if r - start < minrun:
                outside += r - start
            start = r
    return outside


def check_products(pj, case):
    """y of the slice kernel == y of the chunked CSR kernel, run matrix (which = 3) and loop matrix (7); the image has edge rows."""
    from penguin.jl_amd import _lib as L
    s = _stepped(pj, case)
    for which in (3, 7):
        info = _info(s, which)
        print(case, which, "rows", info.rows_matrix, "units", info.spmv_units, "marched", info.rows_marched, "edge", info.rows_edge,
              "irregular", info.rows_irregular, "pattern", info.rows_pattern)
        assert info.spmv_units > 0 and info.rows_edge > 0, (case, which, info.spmv_units, info.rows_edge)
        assert info.rows_uniform + info.rows_pattern + info.rows_irregular == info.rows_matrix
        d, m = C.c_double(), C.c_double()
        L.check(L.lib().pg_debug_spmv_compare(s._h, C.c_int32(which), C.c_int32(70), C.c_int32(38), C.byref(d), C.byref(m)))
        assert m.value > 0.0
        assert d.value == 0.0, (case, which, d.value, m.value)
    # fewer rows in the packed irregular chunks than the CSR of the same system has rows outside its uniform runs
    own = _rows_outside_uniform_runs(s, 3)
    info = _info(s, 3)
    print(case, "rows outside uniform runs", own, "rows_irregular", info.rows_irregular)
    assert info.rows_irregular < own, (case, info.rows_irregular, own)


def check_mode(pj, case, mode):
    """One launch mode of the slice kernel against the chunked CSR kernel on the same vectors: y exactly, the dot sums to 1e-13
    relative (their partial sums are formed in another order).  For mode 8 the reference is the CSR kernel's product s followed
    by the slice kernel's own epilogue expression (mode_out, with its fused multiply-adds spelled out): s is what is checked
    independently, the epilogue's rounding is shared."""
    from penguin.jl_amd import _lib as L
    s = _stepped(pj, case)
    for which in (3, 7):
        d, m, rel = C.c_double(), C.c_double(), C.c_double()
        L.check(L.lib().pg_debug_spmv_mode_compare(s._h, C.c_int32(which), C.c_int32(mode), C.byref(d), C.byref(m), C.byref(rel)))
        print(case, "which", which, "mode", mode, "max |dy|", d.value, "max |y|", m.value, "dot rel", rel.value)
        assert m.value > 0.0
        assert d.value == 0.0, (case, which, mode, d.value)
        assert rel.value <= 1e-13, (case, which, mode, rel.value)


# The chords of the sphere on 40 x 36 x 32 cells are 20 cells long at most: no run of identical rows reaches the 24 rows the
# image builder asks of a run by default (PG_SPMV_MINRUN, read once per process), so there would be no unit to carry an edge
# row.  These cases run in a child process with runs from 8 rows on -- ONE child per case, all its checks, result kept.
_SHORT_CHORDS = {"sphere_be": "8", "sphere_cn": "8"}
_CHILD = {}


def _child(case):
    if case not in _CHILD:
        root = pathlib.Path(__file__).resolve().parents[1]
        code = ("import sys; sys.path.insert(0, '.'); import penguin.jl_amd as pj; pj.init(0); import tests.test_gpu_spmv_edge_rows as t\n"
                f"t.check_products(pj, {case!r})\n"
                f"for m in (1, 3, 8):\n    t.check_mode(pj, {case!r}, m)\n")
        _CHILD[case] = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=300,
                                      env={**os.environ, "PG_SPMV_MINRUN": _SHORT_CHORDS[case]})
    r = _CHILD[case]
    print(r.stdout[-3000:])
    assert r.returncode == 0, (case, r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.parametrize("case", ["sphere_be", "sphere_cn", "sphere80_be", "offcentre", "disc2d", "two_balls"])
def test_edge_rows_bitwise_equal_csr_kernels(pj, case):
    if case in _SHORT_CHORDS:
        _child(case)
    else:
        check_products(pj, case)


@pytest.mark.parametrize("mode", [1, 3, 8])
@pytest.mark.parametrize("case", ["sphere_be", "sphere_cn", "sphere80_be", "disc2d"])
def test_edge_rows_launch_modes_equal_csr_reference(pj, case, mode):
    """Modes 1, 3 (fused dots) and 8 (Horner step) on the sphere (BE and CN; and on twice the cells in process) and on the 2-D disc."""
    if case in _SHORT_CHORDS:
        _child(case)   # (the child of the case has run every mode)
    else:
        check_mode(pj, case, mode)
