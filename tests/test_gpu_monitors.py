"""Monitors and the thinned state history of the device time loop: per-step observables Σ w_i x_i / Σ w_i x_i² evaluated on the
device after every solve (pj.Monitor, VolumeIntegral, InterfaceFlux, Probe; pg_solver_set_monitors) and save_every=k.

Reference and bound wherever a series value is checked against a state: for the full-length state x of that row and the
weights w as given to the library,  ref = Σ w_i x_i  (or Σ w_i x_i²) formed in np.longdouble,  S = Σ |w_i x_i|  (or Σ |w_i| x_i²),
and  |value − ref| <= 1.01·(nnz + 3)·2⁻⁵³·S  with nnz the number of non-zero weights: the first-order bound for floating-point
summation of nnz terms in any order plus at most three roundings per term (scaling by ds, square, weight).  Not a measured
number.

State forms: every solve leaves the state as the scaled z (x_valid is false after pg_solver_initial_solve and after every
pg_solver_step: do_initial and all three branches of do_step end that way), so the kernel reads z and ds on row 0 (the
constructor's matrix) and on rows >= 1 (the run matrix, after k_rescale_state when the scheme changed).  No path leaves x valid
after a step; the x form of the kernel is what pg_debug_monitor_ms runs after a state download
(test_the_x_form_of_the_kernel_agrees_with_the_z_form)."""
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

U = 2.0 ** -53


def _ref_bound(w, x, kind):
    wl, xl = np.asarray(w, dtype=np.longdouble), np.asarray(x, dtype=np.longdouble)
    terms = wl * xl if kind == "sum" else wl * xl * xl
    nnz = int(np.count_nonzero(w))
    return terms.sum(), 1.01 * (nnz + 3) * U * np.abs(terms).sum(), nnz


def _check_series(s, mons, W, rows=None, states=None, label=""):
    """Every monitor on every row (or the given rows against the given states) against the bound of the module docstring."""
    rows = range(len(s.monitor_series)) if rows is None else rows
    states = s.states if states is None else states
    worst = 0.0
    for q, x in zip(rows, states):
        for k, m in enumerate(mons):
            ref, bound, nnz = _ref_bound(W[k], x, m.kind)
            err = abs(np.longdouble(s.monitor_series[q, k]) - ref)
            print(f"{label} row {q} monitor {k} ({m.name}, {m.kind}, nnz {nnz}): value {s.monitor_series[q, k]:.17g} "
                  f"|err| {float(err):.3e} bound {float(bound):.3e}")
            assert err <= bound, (label, q, k, float(err), float(bound))
            if bound > 0:
                worst = max(worst, float(err / bound))
    return worst


def _info(s):
    K, rows = C.c_int32(-1), C.c_int64(-1)
    sparse, stored = (C.c_int32 * 8)(), (C.c_int64 * 8)()
    L.check(L.lib().pg_solver_monitor_info(s._h, C.byref(K), C.byref(rows), sparse, stored))
    return K.value, rows.value, list(sparse)[: max(K.value, 0)], list(stored)[: max(K.value, 0)]


def _last_error():
    buf = C.create_string_buffer(4096)
    L.lib().pg_last_error(buf, 4096)
    return buf.value.decode("utf-8", "replace")


# constant data: the oracle calls every source with a time argument, so the source has one, and the product is told that no
# closure depends on it (CONST) -- the calls then take the branches constant data take
F2 = lambda x, y, z, t=0.0: 1.0 + 0.3 * x
CONST = dict(time_independent=True)
D2 = lambda x, y, z: 1.0 + 0.3 * x + 0.1 * y
G2 = lambda x, y, z: np.cos(x)


def _disc24(pj, scheme0, f=F2, g=G2, bv=0.25):
    """2-D 24² disc, Dirichlet interface: the compact loop (γ rows and border rows left out of the iteration)."""
    n = 24
    M = (n + 1) ** 2
    u0 = np.concatenate([0.2 * np.ones(M), np.ones(M)])
    dt = 0.4 * (4.0 / n) ** 2
    pair = _mono_pair(pj, 2, n, 4.0, (2.01, 2.01), 1.7, pj.Dirichlet(g), po.Dirichlet(g), {k: pj.Dirichlet(bv) for k in HEAT_BORDERS},
                      {k: po.Dirichlet(bv) for k in HEAT_BORDERS}, dt, u0, scheme0, f=f, D=D2)
    return pair, dt, M


def _active(s):
    """Full-vector index of every row of the system, in row order (ω rows, then γ rows)."""
    _, _, idx = s.system(0)
    return np.asarray(idx, dtype=np.int64)


def _unit(nunk, i):
    w = np.zeros(nunk)
    w[i] = 1.0
    return w


# ---------------------------------------------------------------------------------------------------- 1. indexing
def test_indexing_eight_unit_weight_monitors(pj):
    ((s, ph, bcb, bci), _), dt, M = _disc24(pj, "BE")
    mesh = ph.capacity.mesh
    idx = _active(s)
    om, ga = idx[idx < M], idx[idx >= M]
    assert len(om) > 4 and len(ga) > 2
    eliminated = int(np.setdiff1d(np.arange(2 * M), idx)[0])
    picks = [int(om[0]), int(om[-1]), int(ga[0]), int(ga[-1]), int(om[len(om) // 2]), int(om[len(om) // 3]), eliminated]
    # Probe for the unknowns named by a cell, raw unit vectors for the rest: the same weights either way
    mons = [pj.Probe(mesh, i % M, kind="omega" if i < M else "gamma") for i in picks[:4]]
    mons += [pj.Monitor(_unit(2 * M, i), name=f"unit_{i}") for i in picks[4:]]
    sq = int(om[len(om) // 2])
    mons.append(pj.Monitor(_unit(2 * M, sq), kind="sumsq", name="square"))
    picks.append(sq)
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 6 * dt, bcb, bci, "CN", reltol=1e-13, monitors=mons, **CONST)
    assert s.time_data is None and len(s.states) == 7
    assert s.monitor_series.shape == (7, 8) and len(s.monitor_times) == 7 and len(s.monitor_names) == 8
    K, rows, sparse, stored = _info(s)
    assert (K, rows) == (8, 7)
    assert sparse == [1] * 8, sparse
    assert stored == [1, 1, 1, 1, 1, 1, 0, 1], stored          # (the eliminated unknown is no row: dropped)
    for q, x in enumerate(s.states):
        for k, i in enumerate(picks):
            want = x[i] * x[i] if k == 7 else x[i]
            err = abs(s.monitor_series[q, k] - want)
            print(f"row {q} unknown {i}: series {s.monitor_series[q, k]:.17g} state {want:.17g} |diff| {err:.3e}")
            assert err <= 2 * U * abs(want), (q, k, err)
        assert s.monitor_series[q, 6] == 0.0
    assert np.max(np.abs(s.states[-1])) > 0.1                   # (a solution, not zeros)
    t = 0.0
    for q in range(7):                                          # the solver's clock: fp64 t += Δt
        assert s.monitor_times[q] == t
        t += dt


# ---------------------------------------------------------------------------------------------------- 2. dense against sparse
def _dense_sparse_monitors(pj, nunk, idx, rng):
    a = rng.uniform(-1.0, 1.0, nunk)
    b = np.zeros(nunk)
    keep = idx[np.linspace(0, len(idx) - 1, 5).astype(int)]
    b[keep] = a[keep]
    return [pj.Monitor(a, name="A"), pj.Monitor(a, kind="sumsq", name="A2"), pj.Monitor(b, name="B"), pj.Monitor(b, kind="sumsq", name="B2")]


def test_dense_against_sparse(pj):
    ((s, ph, bcb, bci), _), dt, M = _disc24(pj, "BE")
    idx = _active(s)
    mons = _dense_sparse_monitors(pj, 2 * M, idx, np.random.default_rng(11))
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 6 * dt, bcb, bci, "CN", reltol=1e-13, monitors=mons, **CONST)
    K, rows, sparse, stored = _info(s)
    assert (K, rows) == (4, 7)
    assert sparse == [0, 0, 1, 1], sparse
    assert stored == [len(idx), len(idx), 5, 5], stored
    W = [m._w for m in mons]
    worst = _check_series(s, mons, W, label="24^2 dense/sparse")
    print("worst |err| / bound:", worst)


# sizes with an odd number of rows, one and two blocks (512 rows per block): the pair loads' odd last row, the partials of
# several blocks summed when the series is read
@pytest.mark.parametrize("N,n,c,r", [(2, 19, (2.01, 2.01), 1.5), (3, 9, (2.01, 2.01, 2.3), 1.3)])      # n_own = 323, 643
def test_odd_row_counts_and_more_than_one_block(pj, N, n, c, r):
    M = (n + 1) ** N
    u0 = np.concatenate([0.2 * np.ones(M), np.ones(M)])
    dt = 0.4 * (4.0 / n) ** 2
    (s, ph, bcb, bci), _ = _mono_pair(pj, N, n, 4.0, c, r, pj.Dirichlet(G2), po.Dirichlet(G2), {k: pj.Dirichlet(0.25) for k in HEAT_BORDERS},
                                      {k: po.Dirichlet(0.25) for k in HEAT_BORDERS}, dt, u0, "CN", f=F2)
    idx = _active(s)
    assert len(idx) % 2 == 1, f"n_own = {len(idx)}: choose a size with an odd number of rows"
    assert (len(idx) > 512) == (N == 3)
    rng = np.random.default_rng(5)
    mons = _dense_sparse_monitors(pj, 2 * M, idx, rng)
    last = np.zeros(2 * M)
    last[idx[-1]] = 1.0                                        # dense company makes no difference to a sparse monitor
    mons.append(pj.Monitor(last, name="last_row"))
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 3 * dt, bcb, bci, "CN", reltol=1e-13, monitors=mons, **CONST)
    assert _info(s)[2] == [0, 0, 1, 1, 1]
    _check_series(s, mons, [m._w for m in mons], label=f"{N}-D n_own {len(idx)}")
    for q, x in enumerate(s.states):
        assert s.monitor_series[q, 4] == x[idx[-1]]


def _eval_now(s, K):
    vals, xf = np.zeros(K), C.c_int32(-1)
    L.check(L.lib().pg_debug_monitor_eval(s._h, L.dptr(vals), C.byref(xf)))
    return vals, xf.value


def test_the_x_form_of_the_kernel_agrees_with_the_z_form(pj):
    """pg_debug_monitor_eval evaluates the monitors once on the current state without touching the series.  After the run the
    state is z: the values are the last series row, bit for bit.  After a state download x is valid and the kernel reads x alone
    (ds == nullptr): x = fl(ds·z) is the product the z form rounds, summed in the same order -- the same bits again -- and the
    values meet the module's bound against the downloaded state.  pg_debug_monitor_ms then reports the x form's bytes, 8 n less."""
    ((s, ph, bcb, bci), _), dt, M = _disc24(pj, "CN")
    idx = _active(s)
    mons = _dense_sparse_monitors(pj, 2 * M, idx, np.random.default_rng(3))
    opts = api._krylov_opts("bicgstab", {"reltol": 1e-13})
    info = L.pg_step_info()
    api._install_monitors(s, mons)
    L.check(L.lib().pg_solver_initial_solve(s._h, C.byref(opts), C.byref(info)))
    for _ in range(2):
        L.check(L.lib().pg_solver_step(s._h, C.c_int32(1), C.byref(opts), C.byref(info)))
    api._fetch_monitors(s)
    before = s.monitor_series.copy()
    assert before.shape == (3, 4)
    z_vals, z_form = _eval_now(s, 4)
    assert z_form == 0 and np.array_equal(z_vals, before[-1])
    x = s._fetch_state()                                       # (materialises x)
    x_vals, x_form = _eval_now(s, 4)
    assert x_form == 1
    for k, m in enumerate(mons):
        ref, bound, _ = _ref_bound(m._w, x, m.kind)
        print(f"x form monitor {k}: {x_vals[k]:.17g} z form {z_vals[k]:.17g} |err| {float(abs(x_vals[k] - ref)):.3e} bound {float(bound):.3e}")
        assert abs(np.longdouble(x_vals[k]) - ref) <= bound
    assert np.array_equal(x_vals, z_vals)
    ms, nbytes = C.c_double(-1.0), C.c_int64(-1)
    L.check(L.lib().pg_debug_monitor_ms(s._h, C.c_int32(3), C.byref(ms), C.byref(nbytes)))
    n = len(idx)
    assert ms.value > 0.0
    G = max(1, -(-n // 512))
    # two dense monitors' weights, the state once as x alone, two 5-entry lists at 268 bytes an entry, G x K partials written
    assert nbytes.value == 2 * 8 * n + 8 * n + 2 * 5 * 268 + G * 4 * 8, nbytes.value
    api._fetch_monitors(s)
    assert np.array_equal(s.monitor_series, before)


def test_series_longer_than_the_first_reservation(pj):
    """The series buffer starts at 64 rows: 70 steps of the per-step branch grow it once by doubling (the copy), 70 steps of
    pg_solver_run reserve the whole loop before the first step.  Both give the same 71 rows, bit for bit."""
    out = []
    for save_states in (True, False):
        ((s, ph, bcb, bci), _), dt, M = _disc24(pj, "BE")
        mons = [pj.VolumeIntegral(ph.capacity), pj.Monitor(_unit(2 * M, int(_active(s)[3])), kind="sumsq")]
        pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 69.5 * dt, bcb, bci, "BE", reltol=1e-13, monitors=mons, save_states=save_states, **CONST)
        assert s.monitor_series.shape == (71, 2) and _info(s)[1] == 71
        out.append(s)
    _check_series(out[0], mons, api._monitor_weights(mons, 2 * M), rows=[0, 63, 64, 65, 70],
                  states=[out[0].states[q] for q in (0, 63, 64, 65, 70)], label="71 rows")
    assert np.array_equal(out[0].monitor_series, out[1].monitor_series)


# ---------------------------------------------------------------------------------------------------- 4. other systems
def _ld_matvec(A, x):
    """A x in np.longdouble (A scipy sparse, x longdouble)."""
    A = A.tocoo()
    y = np.zeros(A.shape[0], dtype=np.longdouble)
    np.add.at(y, A.row, A.data.astype(np.longdouble) * x[A.col])
    return y


def _oracle_flux(oph, x, off_w, off_g):
    """Σ D·(Hᵀ Wꜝ (G Tω + H Tγ)) with the oracle's operators, in longdouble, and the oracle-built weights (Gᵀ Wꜝ H d, Hᵀ Wꜝ H d)."""
    op, cap = oph.operator, oph.capacity
    M = int(np.prod(op.size))
    d = po.build_I_D(op, oph.Diffusion_coeff, cap).astype(np.longdouble)
    xl = np.asarray(x, dtype=np.longdouble)
    Tw, Tg = xl[off_w:off_w + M], xl[off_g:off_g + M]
    winv = op.Winv.diagonal().astype(np.longdouble)
    flux = _ld_matvec(op.H.T, winv * (_ld_matvec(op.G, Tw) + _ld_matvec(op.H, Tg)))
    q = winv * _ld_matvec(op.H, d)
    w = np.zeros(len(x), dtype=np.longdouble)
    w[off_w:off_w + M] = _ld_matvec(op.G.T, q)
    w[off_g:off_g + M] = _ld_matvec(op.H.T, q)
    return (d * flux).sum(), w


def _standard_monitors(pj, ph, mesh, probe_cell, phase=0):
    return [pj.VolumeIntegral(ph.capacity, phase=phase), pj.VolumeIntegral(ph.capacity, phase=phase, square=True),
            pj.InterfaceFlux(ph, phase=phase), pj.Probe(mesh, probe_cell, phase=phase)]


def _check_flux_against_oracle(s, k, oph, off_w, off_g, label):
    for q, x in enumerate(s.states):
        ref, w = _oracle_flux(oph, x, off_w, off_g)
        S = np.abs(w * np.asarray(x, dtype=np.longdouble)).sum()
        nnz = int(np.count_nonzero(w))
        bound = 1.01 * (nnz + 3) * U * S
        err = abs(np.longdouble(s.monitor_series[q, k]) - ref)
        print(f"{label} row {q}: InterfaceFlux {s.monitor_series[q, k]:.17g} oracle operators {float(ref):.17g} |err| {float(err):.3e} "
              f"bound {float(bound):.3e} (nnz {nnz})")
        assert err <= bound, (label, q, float(err), float(bound))


def _mono_case(pj, name):
    if name == "robin16":
        n, N, c, r = 16, 2, (2.01, 2.01), 1.0
        bi, boi = pj.Robin(1.0, 0.5, 2.0), po.Robin(1.0, 0.5, 2.0)
    else:                                                       # "sphere12"
        n, N, c, r = 12, 3, (2.01, 2.01, 2.01), 1.3
        bi, boi = pj.Dirichlet(G2), po.Dirichlet(G2)
    M = (n + 1) ** N
    u0 = np.concatenate([0.2 * np.ones(M), np.ones(M)])
    dt = 0.4 * (4.0 / n) ** 2
    pair = _mono_pair(pj, N, n, 4.0, c, r, bi, boi, {k: pj.Dirichlet(0.25) for k in HEAT_BORDERS},
                      {k: po.Dirichlet(0.25) for k in HEAT_BORDERS}, dt, u0, "BE", f=F2, D=D2)
    return pair, dt, M, N


def _run_mono_case(pj, name):
    ((s, ph, bcb, bci), (so, oph, obcb, obci)), dt, M, N = _mono_case(pj, name)
    mesh = ph.capacity.mesh
    idx = _active(s)
    cell = int(idx[idx < M][len(idx) // 4])
    mons = _standard_monitors(pj, ph, mesh, cell)
    W = api._monitor_weights(mons, 2 * M)
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 4 * dt, bcb, bci, "CN", reltol=1e-13, monitors=mons, **CONST)
    return s, oph, mons, W, M


@pytest.mark.parametrize("name", ["robin16", "sphere12"])
def test_plain_warm_path_and_3d(pj, name):
    s, oph, mons, W, M = _run_mono_case(pj, name)
    assert s.monitor_series.shape == (5, 4) and len(s.states) == 5
    assert s.monitor_names == ["mean_0", "mean_sq_0", "interface_flux_0", mons[3].name]
    _check_series(s, mons, W, label=name)
    _check_flux_against_oracle(s, 2, oph, 0, M, name)


def _diph16(pj, conv=False):
    n = 16
    Lx, c, r = 8.0, (4.0, 4.0), 2.0
    M = (n + 1) ** 2
    mesh, omesh = pj.Mesh((n, n), (Lx, Lx), (0.0, 0.0)), po.Mesh((n, n), (Lx, Lx), (0.0, 0.0))
    cap1, cap2 = pj.Capacity(pj.Sphere(c, r), mesh), pj.Capacity(pj.Sphere(c, r, complement=True), mesh)
    oc1, oc2 = oracle_capacity_from_product(cap1, omesh), oracle_capacity_from_product(cap2, omesh)
    f1, f2 = (lambda x, y, z: 1.0 + 0.1 * x), (lambda x, y, z: 0.5 + 0.1 * y)
    D1, D2_ = (lambda x, y, z: 1.0), (lambda x, y, z: 2.0 + 0.1 * x)
    p1, p2 = pj.Phase(cap1, pj.DiffusionOps(cap1), f1, D1), pj.Phase(cap2, pj.DiffusionOps(cap2), f2, D2_)
    q1, q2 = po.Phase(oc1, po.make_diffusion_ops(oc1), f1, D1), po.Phase(oc2, po.make_diffusion_ops(oc2), f2, D2_)
    ic = pj.InterfaceConditions(pj.ScalarJump(1.0, 0.5, 0.0), pj.FluxJump(1.0, 1.0, 0.0))
    bcb = pj.BorderConditions({})
    u0 = np.concatenate([np.ones(M), np.ones(M), np.zeros(M), np.zeros(M)])
    dt = 0.5 * (Lx / n) ** 2
    s = pj.DiffusionUnsteadyDiph(p1, p2, bcb, ic, dt, u0, "BE")
    return s, (p1, p2), (q1, q2), bcb, ic, dt, M, mesh


def test_diphasic_both_phases(pj):
    s, (p1, p2), (q1, q2), bcb, ic, dt, M, mesh = _diph16(pj)
    idx = _active(s)
    c0 = int(idx[idx < M][5])
    c1 = int(idx[(idx >= 2 * M) & (idx < 3 * M)][7]) - 2 * M
    mons = _standard_monitors(pj, p1, mesh, c0, phase=0) + _standard_monitors(pj, p2, mesh, c1, phase=1)
    assert len(mons) == 8
    W = api._monitor_weights(mons, 4 * M)
    assert W.shape == (8, 4 * M)
    assert not W[0:4, 2 * M:].any() and not W[4:8, :2 * M].any()      # each phase's monitors on its own blocks
    pj.solve_DiffusionUnsteadyDiph_b(s, p1, p2, dt, 4 * dt, bcb, ic, "CN", reltol=1e-13, monitors=mons)
    assert s.monitor_series.shape == (5, 8) and len(s.states) == 5
    _check_series(s, mons, W, label="diph16")
    _check_flux_against_oracle(s, 2, q1, 0, M, "diph16 phase 0")
    _check_flux_against_oracle(s, 6, q2, 2 * M, 3 * M, "diph16 phase 1")


def test_advection_diffusion(pj):
    n, N = 16, 2
    M = (n + 1) ** 2
    mesh, omesh = pj.Mesh((n, n), (4.0, 4.0)), po.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0), mesh)
    ocap = oracle_capacity_from_product(cap, omesh)
    u, ug = _velocity_fields(cap, N, M)
    op, oop = pj.ConvectionOps(cap, u, ug), po.make_convection_ops(ocap, u, ug)
    f, D = (lambda x, y, z=0.0: 1.0 + 0.2 * x), (lambda x, y, z=0.0: 0.5 + 0.1 * y)
    ph, oph = pj.Phase(cap, op, f, D), po.Phase(ocap, oop, f, D)
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in HEAT_BORDERS})
    dt = 0.25 * (4.0 / n) ** 2
    u0 = np.concatenate([np.zeros(M), np.ones(M)])
    s = pj.AdvectionDiffusionUnsteadyMono(ph, bcb, pj.Robin(1.0, 0.5, 1.0), dt, u0, "BE")
    idx = _active(s)
    mons = _standard_monitors(pj, ph, mesh, int(idx[idx < M][9]))
    W = api._monitor_weights(mons, 2 * M)
    pj.solve_AdvectionDiffusionUnsteadyMono_b(s, ph, dt, 4 * dt, bcb, pj.Robin(1.0, 0.5, 1.0), "BE", reltol=1e-13, monitors=mons)
    assert s.monitor_series.shape == (5, 4) and len(s.states) == 5
    _check_series(s, mons, W, label="advdiff16")
    _check_flux_against_oracle(s, 2, oph, 0, M, "advdiff16")


def test_darcy_unsteady(pj):
    n = 16
    M = (n + 1) ** 2
    mesh, omesh = pj.Mesh((n, n), (2.0, 2.0)), po.Mesh((n, n), (2.0, 2.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((0.5, 0.5), 0.5), mesh)
    ocap = oracle_capacity_from_product(cap, omesh)
    f, D = (lambda x, y, z=0.0: 0.0), (lambda x, y, z=0.0: 1.0)
    ph, oph = pj.Phase(cap, pj.DiffusionOps(cap), f, D), po.Phase(ocap, po.make_diffusion_ops(ocap), f, D)
    bcb = pj.BorderConditions({"left": pj.Dirichlet(10.0), "right": pj.Dirichlet(20.0)})
    dt = 0.1 * (2.0 / n) ** 2
    s = pj.DarcyFlowUnsteady(ph, bcb, pj.Neumann(0.0), dt, np.linspace(10.0, 20.0, 2 * M), "BE")      # (a pressure with a gradient: a flux)
    idx = _active(s)
    mons = _standard_monitors(pj, ph, mesh, int(idx[idx < M][11]))
    W = api._monitor_weights(mons, 2 * M)
    pj.solve_DarcyFlowUnsteady_b(s, ph, dt, 4 * dt, bcb, pj.Neumann(0.0), "BE", reltol=1e-13, monitors=mons)
    assert s.monitor_series.shape == (5, 4) and len(s.states) == 5
    _check_series(s, mons, W, label="darcy16")
    _check_flux_against_oracle(s, 2, oph, 0, M, "darcy16")


def test_volume_mean_of_a_uniform_state_is_one(pj):
    """Initial state 1, interface value 1, border values 1, no source: the solution stays 1, and the mean is 1 within nnz·2⁻⁵³ --
    the weights V_i / ΣV sum to 1 within that (ΣV carries at most nnz − 1 roundings, each quotient one).  The distance of the
    solved state from 1 is printed and held to 16·2⁻⁵³ of its own: a state that drifts does not pass by way of the mean."""
    n = 16
    M = (n + 1) ** 2
    dt = 0.4 * (4.0 / n) ** 2
    one = lambda x, y, z: 1.0
    (s, ph, bcb, bci), _ = _mono_pair(pj, 2, n, 4.0, (2.01, 2.01), 1.2, pj.Dirichlet(1.0), po.Dirichlet(1.0),
                                      {k: pj.Dirichlet(1.0) for k in HEAT_BORDERS}, {k: po.Dirichlet(1.0) for k in HEAT_BORDERS}, dt,
                                      np.ones(2 * M), "BE", f=lambda x, y, z, t=0.0: 0.0, D=one)
    mon = pj.VolumeIntegral(ph.capacity)
    w = mon._weights(2 * M)
    nnz = int(np.count_nonzero(w))
    assert nnz > 50 and not w[M:].any()
    assert abs(np.asarray(w, dtype=np.longdouble).sum() - 1) <= nnz * U
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 3 * dt, bcb, bci, "BE", reltol=1e-14, monitors=[mon], **CONST)
    for q, x in enumerate(s.states):
        dev = float(np.max(np.abs(x[w != 0.0] - 1.0)))
        err = abs(s.monitor_series[q, 0] - 1.0)
        print(f"row {q}: mean {s.monitor_series[q, 0]:.17g} |mean - 1| {err:.3e} nnz*u {nnz * U:.3e} max|x - 1| {dev:.3e}")
        assert err <= nnz * U
        assert dev <= 16 * U


# ---------------------------------------------------------------------------------------------------- 5. device loop, thinned history
def _loop_monitors(pj, ph, s, M):
    idx = _active(s)
    return _standard_monitors(pj, ph, ph.capacity.mesh, int(idx[idx < M][len(idx) // 4]))


def _num_states(s):
    n = C.c_int64(-1)
    L.check(L.lib().pg_solver_num_states(s._h, C.byref(n)))
    return n.value


def test_device_loop_with_a_thinned_history(pj):
    ((s, ph, bcb, bci), (so, oph, obcb, obci)), dt, M = _disc24(pj, "CN")
    mons = _loop_monitors(pj, ph, s, M)
    W = api._monitor_weights(mons, 2 * M)
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 9 * dt, bcb, bci, "CN", reltol=1e-13, monitors=mons, save_every=3, save_states=False, **CONST)
    assert s.last_run is not None and s.last_run.steps == 9      # (pg_solver_run took the steps)
    assert s.state_steps == [0, 3, 6, 9]
    assert len(s.states) == 4 and len(s.monitor_series) == 10
    assert _num_states(s) == 0
    _check_series(s, mons, W, rows=[0, 3, 6, 9], states=s.states, label="24^2 CN device loop")
    po.solve_DiffusionUnsteadyMono(so, oph, dt, 9 * dt, obcb, obci, "CN", method="\\")
    assert len(so.states) == 10
    errs = [rel_l2(x, so.states[q]) for q, x in zip(s.state_steps, s.states)]
    print("kept states against the oracle's direct solves:", errs)
    assert max(errs) <= TOL_T
    assert np.array_equal(s.x, s.states[-1])
    t = 0.0
    for q in range(10):
        assert s.monitor_times[q] == t
        t += dt
    # save_states=True takes the run branch too
    ((s2, ph2, bcb2, bci2), _), dt, M = _disc24(pj, "CN")
    pj.solve_DiffusionUnsteadyMono_b(s2, ph2, dt, 9 * dt, bcb2, bci2, "CN", reltol=1e-13, save_every=3, **CONST)
    assert s2.last_run is not None and s2.last_run.steps == 9 and s2.state_steps == [0, 3, 6, 9] and len(s2.states) == 4
    assert all(np.array_equal(a, b) for a, b in zip(s.states, s2.states))
    assert _info(s2)[:2] == (0, 0) and s2.monitor_series.shape == (0, 0)


def test_thinned_history_with_separable_data_and_with_a_plain_closure(pj):
    f = pj.TimeSeparable([(1.0, lambda t: 1.0), (lambda x, *_: x, lambda t: math.sin(40.0 * t))])
    ((s, ph, bcb, bci), (so, oph, obcb, obci)), dt, M = _disc24(pj, "CN", f=f)
    mons = _loop_monitors(pj, ph, s, M)
    W = api._monitor_weights(mons, 2 * M)
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 9 * dt, bcb, bci, "CN", reltol=1e-13, monitors=mons, save_every=3, save_states=False)
    assert s.time_data == "device" and s.last_run.steps == 9
    assert s.state_steps == [0, 3, 6, 9] and len(s.states) == 4 and len(s.monitor_series) == 10 and _num_states(s) == 0
    _check_series(s, mons, W, rows=[0, 3, 6, 9], states=s.states, label="separable data")
    po.solve_DiffusionUnsteadyMono(so, oph, dt, 9 * dt, obcb, obci, "CN", method="\\")
    assert max(rel_l2(x, so.states[q]) for q, x in zip(s.state_steps, s.states)) <= TOL_T
    # the same data as a plain closure: the host-driven loop, every step a pg_solver_step, the same series
    fl = lambda x, y, z, t: f(x, y, z, t)
    ((sh, phh, bcbh, bcih), _), dt, M = _disc24(pj, "CN", f=fl)
    monsh = _loop_monitors(pj, phh, sh, M)
    pj.solve_DiffusionUnsteadyMono_b(sh, phh, dt, 9 * dt, bcbh, bcih, "CN", reltol=1e-13, monitors=monsh, save_every=3, save_states=False)
    assert sh.time_data == "host"
    assert len(sh.monitor_series) == len(s.monitor_series) == 10
    assert sh.state_steps == [0, 3, 6, 9] and len(sh.states) == 4
    _check_series(sh, monsh, W, rows=[0, 3, 6, 9], states=sh.states, label="plain closure")
    scale = np.max(np.abs(s.monitor_series), axis=0)
    assert np.all(np.max(np.abs(sh.monitor_series - s.monitor_series), axis=0) <= 1e-9 * scale)


# ---------------------------------------------------------------------------------------------------- 6. reproducibility
def test_series_is_bitwise_reproducible(pj):
    a = _run_mono_case(pj, "sphere12")[0].monitor_series
    b = _run_mono_case(pj, "sphere12")[0].monitor_series
    assert a.shape == (5, 4) and np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------- 7. refusals, 8. default path
def test_refusals_through_the_raw_abi(pj):
    lib = L.lib()
    ((s, ph, bcb, bci), _), dt, M = _disc24(pj, "BE")
    opts = api._krylov_opts("bicgstab", {"reltol": 1e-12})
    info = L.pg_step_info()
    W = np.ones((9, 2 * M))
    kinds = lambda *k: (C.c_int32 * len(k))(*k)
    setm = lambda sol, K, kd, ln: lib.pg_solver_set_monitors(sol._h, C.c_int32(K), kd, L.dptr(W), C.c_int64(ln))
    assert setm(s, 9, kinds(*[0] * 9), 2 * M) != 0 and "more than 8 monitors" in _last_error()
    assert setm(s, 1, kinds(7), 2 * M) != 0 and "unknown kind 7" in _last_error()
    assert setm(s, 1, kinds(0), 2 * M + 1) != 0 and "len must be" in _last_error()
    assert setm(s, 1, kinds(0), 2 * M - 1) != 0
    assert setm(s, 0, kinds(0), 2 * M) != 0
    assert lib.pg_solver_set_monitors(s._h, C.c_int32(1), None, L.dptr(W), C.c_int64(2 * M)) != 0
    assert lib.pg_solver_set_monitors(s._h, C.c_int32(1), kinds(0), None, C.c_int64(2 * M)) != 0
    assert lib.pg_solver_set_monitors(None, C.c_int32(1), kinds(0), L.dptr(W), C.c_int64(2 * M)) != 0
    assert _info(s) == (0, 0, [], [])
    # the solver is still usable, and a good call goes through
    assert setm(s, 2, kinds(0, 1), 2 * M) == 0
    L.check(lib.pg_solver_initial_solve(s._h, C.byref(opts), C.byref(info)))
    L.check(lib.pg_solver_step(s._h, C.c_int32(1), C.byref(opts), C.byref(info)))
    assert _info(s)[:2] == (2, 2)
    vals, times = np.zeros((2, 2)), np.zeros(2)
    get = lambda r0, nr: lib.pg_solver_get_monitor_series(s._h, C.c_int64(r0), C.c_int64(nr), L.dptr(vals), L.dptr(times))
    assert get(0, 3) != 0 and "the series has 2" in _last_error()
    assert get(2, 1) != 0 and get(-1, 1) != 0 and get(0, -1) != 0
    assert lib.pg_solver_get_monitor_series(s._h, C.c_int64(0), C.c_int64(2), None, None) != 0
    assert get(0, 2) == 0
    x = s._fetch_state()
    ref, bound, _ = _ref_bound(W[0], x, "sum")
    assert abs(vals[1, 0] - ref) <= bound and times[1] == dt
    assert lib.pg_solver_get_monitor_series(s._h, C.c_int64(1), C.c_int64(1), L.dptr(vals), None) == 0      # times may be NULL
    assert abs(vals[0, 0] - ref) <= bound
    # installing again clears the series; clearing removes the monitors, and a later step records nothing
    assert setm(s, 1, kinds(1), 2 * M) == 0
    assert _info(s)[:2] == (1, 0)
    L.check(lib.pg_solver_step(s._h, C.c_int32(1), C.byref(opts), C.byref(info)))
    assert _info(s)[:2] == (1, 1)
    L.check(lib.pg_solver_clear_monitors(s._h))
    assert _info(s) == (0, 0, [], [])
    L.check(lib.pg_solver_step(s._h, C.c_int32(1), C.byref(opts), C.byref(info)))
    assert _info(s) == (0, 0, [], [])
    assert get(0, 0) != 0 and "no monitors" in _last_error()
    # a steady solver
    mesh = pj.Mesh((16, 16), (4.0, 4.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.2), mesh)
    one = lambda x, y, z: 1.0
    st = pj.DiffusionSteadyMono(pj.Phase(cap, pj.DiffusionOps(cap), one, one), pj.BorderConditions({k: pj.Dirichlet(0.0) for k in HEAT_BORDERS}),
                                pj.Dirichlet(0.0))
    Ws = np.ones((1, 2 * 17 * 17))
    assert lib.pg_solver_set_monitors(st._h, C.c_int32(1), kinds(0), L.dptr(Ws), C.c_int64(Ws.shape[1])) != 0
    assert "steady solver" in _last_error()
    pj.solve_DiffusionSteadyMono_b(st, reltol=1e-12)             # (still usable)
    # a moving solver
    cen, rad = (lambda t: (2.01 + 0.8 * t, 1.97 - 0.5 * t)), (lambda t: 1.0 + 0.4 * t)
    body = pj.MovingSphere(cen, rad, False, dcenter=lambda t: (0.8, -0.5), dradius=lambda t: 0.4)
    cap0 = pj.Capacity(body, pj.SpaceTimeMesh(mesh, [0.0, 0.05]))
    phm = pj.Phase(cap0, pj.DiffusionOps(cap0), lambda x, y, z, t=0.0: 0.0, one)
    bcbm = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in HEAT_BORDERS})
    sm = pj.MovingDiffusionUnsteadyMono(phm, bcbm, pj.Dirichlet(1.0), 0.05, np.ones(2 * 17 * 17), mesh, "BE")
    assert lib.pg_solver_set_monitors(sm._h, C.c_int32(1), kinds(0), L.dptr(Ws), C.c_int64(Ws.shape[1])) != 0
    assert "moving-body" in _last_error()
    L.check(lib.pg_solver_initial_solve(sm._h, C.byref(opts), C.byref(info)))       # (still usable)


def test_refused_on_stefan_and_stream_function_vorticity_solvers(pj):
    from tests.test_gpu_liquid import _hip_cap

    lib = L.lib()
    kinds = (C.c_int32 * 1)(0)
    # a Stefan diphasic slab
    nx = 32
    mesh = pj.Mesh((nx,), (1.0,), (0.0,))
    M, dt, t0 = nx + 1, 0.005, 0.01
    c1 = _hip_cap(pj, mesh, 0.4513, 0.4702, t0, t0 + dt, False)
    c2 = _hip_cap(pj, mesh, 0.4513, 0.4702, t0, t0 + dt, False, True)
    one, src = (lambda x, y, z: 1.0), (lambda x, y, z, t: 0.3)
    p1, p2 = pj.Phase(c1, pj.DiffusionOps(c1), src, one), pj.Phase(c2, pj.DiffusionOps(c2), src, one)
    ic = pj.InterfaceConditions(pj.ScalarJump(1.0, 1.0, 0.0), pj.FluxJump(1.0, 1.0, 2.0))
    bcb = pj.BorderConditions({"bottom": pj.Dirichlet(1.0), "top": pj.Dirichlet(-0.5)})
    ss = pj.MovingLiquidDiffusionUnsteadyDiph(p1, p2, bcb, ic, dt, np.ones(4 * M), mesh, "BE")
    W = np.ones((1, 4 * M))
    assert lib.pg_solver_set_monitors(ss._h, C.c_int32(1), kinds, L.dptr(W), C.c_int64(4 * M)) != 0
    assert "Stefan" in _last_error()
    assert _info(ss) == (0, 0, [], [])
    # the two solvers of a stream function - vorticity step: the steady Poisson solver, and the vorticity solver that is built
    # for one solve and replaced by the next step
    mesh2 = pj.Mesh((10, 10), (1.0, 1.0), (0.0, 0.0))
    cap = pj.Capacity(pj.HalfSpace(0, 10.0), mesh2)
    zb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in ("left", "right", "bottom", "top")})
    sv = pj.StreamVorticity(cap, 0.02, 1e-2, bc_stream=pj.Dirichlet(0.0), bc_vorticity=pj.Dirichlet(0.0), bc_stream_border=zb,
                            bc_vorticity_border=zb, ω0=np.zeros(2 * 121))
    pj.step_StreamVorticity_b(sv, method="gmres")
    W2 = np.ones((1, 2 * 121))
    psi, om = sv.psi_solver, sv.omega_solver
    assert om is not None
    assert lib.pg_solver_set_monitors(psi._h, C.c_int32(1), kinds, L.dptr(W2), C.c_int64(2 * 121)) != 0
    assert "steady solver" in _last_error()
    assert lib.pg_solver_set_monitors(om._h, C.c_int32(1), kinds, L.dptr(W2), C.c_int64(2 * 121)) != 0
    assert "stream-function - vorticity" in _last_error()
    pj.step_StreamVorticity_b(sv, method="gmres")               # (still usable)
    assert len(sv.states) == 3


def test_default_path_reports_no_monitors(pj):
    ((s, ph, bcb, bci), _), dt, M = _disc24(pj, "BE")
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 3 * dt, bcb, bci, "CN", reltol=1e-13, save_states=False, **CONST)
    assert _info(s) == (0, 0, [], [])
    assert s.monitor_series.shape == (0, 0) and s.monitor_names == [] and s.state_steps is None and _num_states(s) == 0
    # ... and with one installed, a row per solve
    ((s, ph, bcb, bci), _), dt, M = _disc24(pj, "BE")
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 2 * dt, bcb, bci, "BE", reltol=1e-13, monitors=[pj.VolumeIntegral(ph.capacity)], **CONST)
    assert _info(s)[:2] == (1, 3)
