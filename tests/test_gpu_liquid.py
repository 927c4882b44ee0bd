"""GPU parity of the 1-D liquid-motion (Stefan) solvers (penguin/jl_amd/liquid.py) against the literal restatement in
tests/liquid_oracle.py, which is fed with the space-time capacities the HIP path computed for each interface position:
the Stefan terms of a solved slab (pg_solver_stefan_terms), the Stefan diphasic blocks (pg_solver_create_moving_stefan_diph),
the full Newton / time loops, two learning-rate strategies, the one- and two-phase Neumann solutions, and the state traffic
of a run."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import penguin_oracle as po
from oracle import spacetime as ost
from tests import liquid_oracle as lo
from tests.common import rel_l2

pytestmark = pytest.mark.gpu


def _oracle_cap(cap, omesh, t0, t1) -> po.Capacity:
    """The 2-D (x, t) oracle capacity holding the fields the HIP path computed (as tests/test_gpu_moving.py does)."""
    z = np.zeros_like(cap.V)
    two = lambda a: np.concatenate([a, z])
    A = tuple(two(a) for a in cap.A) + (np.concatenate([cap.Vn_1, cap.Vn]),)
    B = tuple(two(b) for b in cap.B) + (two(z),)
    W = tuple(two(w) for w in cap.W) + (two(z),)
    zz = np.zeros((len(z), 2))
    return po.Capacity(A, B, two(cap.V), W, np.vstack([cap.C_ω_st, zz]), np.vstack([cap.C_γ_st, zz]), two(cap.Γ),
                       two(cap.cell_types), ost.SpaceTimeMesh(omesh, [t0, t1]), None)


def _hip_cap(pj, mesh, xf0, xf1, t0, t1, static, complement=False):
    from penguin.jl_amd import liquid

    dt = t1 - t0
    body = liquid._static(xf0, complement) if static else liquid._front(xf0, xf1, t0, t1, dt, complement)
    return pj.Capacity(body, pj.SpaceTimeMesh(mesh, [t0, t1]))


def _cap_fn(pj, mesh, omesh, diph=False):
    def fn(xf0, xf1, t0, t1, static):
        c = _oracle_cap(_hip_cap(pj, mesh, xf0, xf1, t0, t1, static), omesh, t0, t1)
        if not diph:
            return c
        return c, _oracle_cap(_hip_cap(pj, mesh, xf0, xf1, t0, t1, static, True), omesh, t0, t1)
    return fn


def _close(a, b, tol, scale=0.0):
    return abs(a - b) <= tol * max(abs(b), scale)


# ------------------------------------------------------------------------------------------------------------ (a) terms
@pytest.mark.parametrize("scheme", ["BE", "CN"])
@pytest.mark.parametrize("diph", [False, True])
def test_stefan_terms_match_the_restatement(pj, scheme, diph):
    """Hₙ₊₁, Hₙ, Σq and max|q| of a solved slab whose interface crosses the cell face x = 0.2875 during the slab, variable D."""
    from penguin.jl_amd import liquid

    nx, L = 40, 1.0
    mesh, omesh = pj.Mesh((nx,), (L,), (0.0,)), po.Mesh((nx,), (L,), (0.0,))
    M, dt, t0 = nx + 1, 0.004, 0.02
    xf0, xf1 = 0.2812, 0.2971
    D1, D2 = (lambda x, y, z: 1.0 + 0.3 * x), (lambda x, y, z: 0.7)
    f = lambda x, y, z, t: 0.2 + x * t
    c1 = _hip_cap(pj, mesh, xf0, xf1, t0, t0 + dt, False)
    assert np.count_nonzero(c1.Vn_1) != np.count_nonzero(c1.Vn)          # a cell changes phase in the slab
    bcb = pj.BorderConditions({"bottom": pj.Dirichlet(1.0), "top": pj.Dirichlet(0.0)})
    T0 = np.random.default_rng(3).random((4 if diph else 2) * M)
    p1 = pj.Phase(c1, pj.DiffusionOps(c1), f, D1)
    if diph:
        c2 = _hip_cap(pj, mesh, xf0, xf1, t0, t0 + dt, False, True)
        p2 = pj.Phase(c2, pj.DiffusionOps(c2), f, D2)
        ic = pj.InterfaceConditions(pj.ScalarJump(1.0, 1.0, 0.0), pj.FluxJump(1.0, 1.0, 1.0))
        s = pj.MovingLiquidDiffusionUnsteadyDiph(p1, p2, bcb, ic, dt, T0, mesh, scheme)
    else:
        s = pj.MovingLiquidDiffusionUnsteadyMono(p1, bcb, pj.Dirichlet(0.25), dt, T0, mesh, scheme)
    from penguin.jl_amd.moving import _solve_current
    _solve_current(s, pj.api._krylov_opts("bicgstab", {"reltol": 1e-14}), "slab", True, False)
    a, b = liquid.stefan_terms(s), liquid.stefan_terms(s)
    assert np.array_equal(a, b) and a.tobytes() == b.tobytes()           # bitwise reproducible
    x = s.states[-1]
    phases = [(c1, D1, x[:2 * M])] + ([(c2, D2, x[2 * M:])] if diph else [])
    for q, (cap, D, Ti) in enumerate(phases):
        oc = _oracle_cap(cap, omesh, t0, t0 + dt)
        ref = lo.stefan_terms(po.make_diffusion_ops(oc), oc, D, Ti)
        qs = ref[3] * M
        assert _close(a[q, 0], ref[0], 1e-12) and _close(a[q, 1], ref[1], 1e-12), (q, a[q], ref)
        assert _close(a[q, 2], ref[2], 1e-12, qs) and _close(a[q, 3], ref[3], 1e-12), (q, a[q], ref)
        assert a[q, 3] > 0.0


# --------------------------------------------------------------------------------------------------- (b) Stefan diph slab
@pytest.mark.parametrize("scheme,Tm,a1,a2", [("BE", 0.3, 1.0, 2.0), ("CN", 0.3, 1.5, 0.5), ("CN", 0.0, 1.0, 1.0)])
def test_stefan_diph_slab_matches_the_restatement(pj, scheme, Tm, a1, a2):
    """A_/b_diph_unstead_diff_moving_stef + BC_border_diph! of one slab: matrix, right-hand side and state.  Tm ≠ 0 with
    α₁ ≠ α₂ pins b₂ = b₄ = gᵧ and row block 4 = [0 0 0 Iα₂]; the CN cases start from Tγ ≠ 0 (the γ term of b₁ / b₃ has no Ψ)."""
    nx, L = 32, 1.0
    mesh, omesh = pj.Mesh((nx,), (L,), (0.0,)), po.Mesh((nx,), (L,), (0.0,))
    M, dt, t0 = nx + 1, 0.005, 0.01
    xf0, xf1 = 0.4513, 0.4702
    D1, D2 = (lambda x, y, z: 1.0 + 0.2 * x), (lambda x, y, z: 2.0)
    f1, f2 = (lambda x, y, z, t: 0.3 + x + t), (lambda x, y, z, t: -0.1 + 0.5 * t)
    c1 = _hip_cap(pj, mesh, xf0, xf1, t0, t0 + dt, False)
    c2 = _hip_cap(pj, mesh, xf0, xf1, t0, t0 + dt, False, True)
    p1, p2 = pj.Phase(c1, pj.DiffusionOps(c1), f1, D1), pj.Phase(c2, pj.DiffusionOps(c2), f2, D2)
    ic = pj.InterfaceConditions(pj.ScalarJump(a1, a2, Tm), pj.FluxJump(1.0, 1.0, 2.0))
    oic = po.InterfaceConditions(po.ScalarJump(a1, a2, Tm), po.FluxJump(1.0, 1.0, 2.0))
    bcb = pj.BorderConditions({"bottom": pj.Dirichlet(1.0), "top": pj.Dirichlet(-0.5)})
    obcb = po.BorderConditions({"bottom": po.Dirichlet(1.0), "top": po.Dirichlet(-0.5)})
    T0 = 0.5 + np.random.default_rng(5).random(4 * M)
    s = pj.MovingLiquidDiffusionUnsteadyDiph(p1, p2, bcb, ic, dt, T0, mesh, scheme)
    oc1, oc2 = _oracle_cap(c1, omesh, t0, t0 + dt), _oracle_cap(c2, omesh, t0, t0 + dt)
    q1, q2 = po.Phase(oc1, po.make_diffusion_ops(oc1), f1, D1), po.Phase(oc2, po.make_diffusion_ops(oc2), f2, D2)
    Ao, bo = lo.stefan_diph_system(q1, q2, obcb, oic, T0, dt, 0.0, omesh, scheme)
    A, b, idx = s.system(0)
    Aor = Ao.tocsr()[idx][:, idx]
    scale = abs(Aor).max()
    assert abs(A[:, : len(idx)] - Aor).max() <= 1e-13 * scale
    assert np.max(np.abs(b - bo[idx])) <= 1e-13 * max(np.max(np.abs(bo)), 1.0)
    g_rows = idx[(idx >= M) & (idx < 2 * M)]
    assert np.all(bo[g_rows] == Tm) and np.all(bo[g_rows + 2 * M] == Tm)         # b₂ = b₄ = gᵧ
    from penguin.jl_amd.moving import _solve_current
    _solve_current(s, pj.api._krylov_opts("bicgstab", {"reltol": 1e-14}), "slab", True, False)
    so = po.Solver("Unsteady", "Diphasic", "Diffusion")
    so.A, so.b = Ao, bo
    po.solve_system(so)
    x = s.states[-1]
    assert rel_l2(x, so.x) <= 1e-10, rel_l2(x, so.x)
    live = np.flatnonzero(so.x[3 * M:] != 0.0)
    assert np.allclose(a2 * x[3 * M + live], Tm, rtol=0, atol=1e-12)             # α₂ Tγ₂ = g


# ---------------------------------------------------------------------------------------------------------- (c) loops
def _mono_problem(pj, nx=40, scheme="BE"):
    """examples/1D/LiquidMoving/stefan.jl: lx = 1, xf = 0.05, Δt = 0.5 h², T = 1 at the bottom, 0 at the top and on the front."""
    L = 1.0
    mesh, omesh = pj.Mesh((nx,), (L,), (0.0,)), po.Mesh((nx,), (L,), (0.0,))
    xf, dt = 0.05 * L, 0.5 * (L / nx) ** 2
    cap = _hip_cap(pj, mesh, xf, xf, 0.0, dt, True)
    f, K = (lambda x, y, z, t: 0.0), (lambda x, y, z: 1.0)
    ph = pj.Phase(cap, pj.DiffusionOps(cap), f, K)
    bcb = pj.BorderConditions({"top": pj.Dirichlet(0.0), "bottom": pj.Dirichlet(1.0)})
    obcb = po.BorderConditions({"top": po.Dirichlet(0.0), "bottom": po.Dirichlet(1.0)})
    ic = pj.InterfaceConditions(None, pj.FluxJump(1.0, 1.0, 1.0))
    oic = po.InterfaceConditions(None, po.FluxJump(1.0, 1.0, 1.0))
    oc = _oracle_cap(cap, omesh, 0.0, dt)
    oph = po.Phase(oc, po.make_diffusion_ops(oc), f, K)
    return mesh, omesh, xf, dt, ph, oph, bcb, obcb, ic, oic


def _run_mono(pj, scheme, adaptive, Newton_params, Tend, strategy="fixed", options=None, save_states=True, nx=40):
    mesh, omesh, xf, dt, ph, oph, bcb, obcb, ic, oic = _mono_problem(pj, nx, scheme)
    M = nx + 1
    T0 = np.zeros(2 * M)
    s = pj.MovingLiquidDiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(0.0), dt, T0, mesh, scheme)
    out = pj.solve_MovingLiquidDiffusionUnsteadyMono_b(
        s, ph, xf, dt, 0.0, Tend, bcb, pj.Dirichlet(0.0), ic, mesh, scheme, Newton_params=Newton_params,
        adaptive_timestep=adaptive, method="bicgstab", reltol=1e-14, learning_rate_strategy=strategy,
        learning_rate_options=options, save_states=save_states)
    ref = lo.solve_mono(oph, obcb, po.Dirichlet(0.0), oic, omesh, scheme, xf, dt, 0.0, Tend, T0, _cap_fn(pj, mesh, omesh),
                        Newton_params=Newton_params, adaptive_timestep=adaptive, learning_rate_strategy=strategy,
                        learning_rate_options=options)
    return out, ref


def _compare_loops(out_states, res, xf_log, ref_states, ref_res, ref_xf, bar=1e-9):
    assert sorted(res) == sorted(ref_res)
    assert [len(res[k]) for k in sorted(res)] == [len(ref_res[k]) for k in sorted(ref_res)]     # iterations per step
    assert len(xf_log) == len(ref_xf)
    assert all(abs(a - b) <= 1e-11 for a, b in zip(xf_log, ref_xf)), (xf_log, ref_xf)
    assert len(out_states) == len(ref_states)
    for k, (x, xo) in enumerate(zip(out_states, ref_states)):
        assert rel_l2(x, xo) <= bar, (k, rel_l2(x, xo))


@pytest.mark.parametrize("scheme,adaptive", [("BE", False), ("CN", False), ("BE", True), ("CN", True)])
def test_mono_loop_matches_the_restatement(pj, scheme, adaptive):
    """solve_MovingLiquidDiffusionUnsteadyMono! on the examples/1D/LiquidMoving/stefan.jl shape: xf_log, timestep_history,
    per-step iteration counts and states against the restatement (Newton tolerance 1e-9)."""
    (s, res, xf_log, hist), (ref_states, ref_res, ref_xf, ref_hist) = _run_mono(pj, scheme, adaptive, (20, 1e-9, 1e-9, 1.0),
                                                                                 0.0015 if adaptive else 0.002)
    _compare_loops(s.states, res, xf_log, ref_states, ref_res, ref_xf)
    assert len(hist) == len(ref_hist)
    for (t, d), (to, do) in zip(hist, ref_hist):
        assert abs(t - to) <= 1e-14 and abs(d - do) <= 1e-12 * do, (hist, ref_hist)
    if adaptive:
        assert len({round(d, 14) for _, d in hist}) > 1           # the step did change
    assert xf_log[-1] > 0.05 and max(len(v) for v in res.values()) > 1


def test_mono_loop_fixed_iterations(pj):
    """tol = 0: every step runs max_iter = 3 iterations and pushes new_xf at the last one (the mono loops' break)."""
    (s, res, xf_log, _), (ref_states, ref_res, ref_xf, _) = _run_mono(pj, "BE", False, (3, 0.0, 0.0, 1.0), 0.001)
    assert all(len(v) == 3 for v in res.values()) and len(xf_log) == len(res)
    _compare_loops(s.states, res, xf_log, ref_states, ref_res, ref_xf)


def _run_diph(pj, scheme, Newton_params, Tend, save_states=True, nx=32):
    """examples/1D/LiquidMoving/stefan_2ph.jl shape: liquid x < xf at T = 1 on the bottom border, solid at T = -0.5 on the top."""
    L = 1.0
    mesh, omesh = pj.Mesh((nx,), (L,), (0.0,)), po.Mesh((nx,), (L,), (0.0,))
    M = nx + 1
    xf, dt = 0.5, 0.5 * (L / nx) ** 2
    f, K1, K2 = (lambda x, y, z, t: 0.0), (lambda x, y, z: 1.0), (lambda x, y, z: 0.5)
    c1, c2 = _hip_cap(pj, mesh, xf, xf, 0.0, dt, True), _hip_cap(pj, mesh, xf, xf, 0.0, dt, True, True)
    p1, p2 = pj.Phase(c1, pj.DiffusionOps(c1), f, K1), pj.Phase(c2, pj.DiffusionOps(c2), f, K2)
    bcb = pj.BorderConditions({"bottom": pj.Dirichlet(1.0), "top": pj.Dirichlet(-0.5)})
    obcb = po.BorderConditions({"bottom": po.Dirichlet(1.0), "top": po.Dirichlet(-0.5)})
    ic = pj.InterfaceConditions(pj.ScalarJump(1.0, 1.0, 0.0), pj.FluxJump(1.0, 1.0, 1.0))
    oic = po.InterfaceConditions(po.ScalarJump(1.0, 1.0, 0.0), po.FluxJump(1.0, 1.0, 1.0))
    T0 = np.zeros(4 * M)
    s = pj.MovingLiquidDiffusionUnsteadyDiph(p1, p2, bcb, ic, dt, T0, mesh, scheme)
    out = pj.solve_MovingLiquidDiffusionUnsteadyDiph_b(s, p1, p2, xf, dt, 0.0, Tend, bcb, ic, mesh, scheme,
                                                       Newton_params=Newton_params, method="bicgstab", reltol=1e-14,
                                                       save_states=save_states)
    oc1, oc2 = _oracle_cap(c1, omesh, 0.0, dt), _oracle_cap(c2, omesh, 0.0, dt)
    q1, q2 = po.Phase(oc1, po.make_diffusion_ops(oc1), f, K1), po.Phase(oc2, po.make_diffusion_ops(oc2), f, K2)
    ref = lo.solve_diph(q1, q2, obcb, oic, omesh, scheme, xf, dt, 0.0, Tend, T0, _cap_fn(pj, mesh, omesh, True),
                        Newton_params=Newton_params)
    return out, ref


@pytest.mark.parametrize("scheme", ["BE", "CN"])
def test_diph_loop_matches_the_restatement(pj, scheme):
    (s, res, xf_log), (ref_states, ref_res, ref_xf) = _run_diph(pj, scheme, (20, 1e-9, 1e-9, 1.0), 0.003)
    _compare_loops(s.states, res, xf_log, ref_states, ref_res, ref_xf)
    assert xf_log[-1] != 0.5


def test_diph_loop_fixed_iterations(pj):
    """tol = 0: the diph loops never break at max_iter; they leave through the while test with nothing pushed."""
    (s, res, xf_log), (ref_states, ref_res, ref_xf) = _run_diph(pj, "BE", (3, 0.0, 0.0, 1.0), 0.001)
    assert all(len(v) == 3 for v in res.values()) and xf_log == [] and ref_xf == []
    _compare_loops(s.states, res, xf_log, ref_states, ref_res, ref_xf)


# ------------------------------------------------------------------------------------------------------- (d) strategies
@pytest.mark.parametrize("strategy,options", [("secant", {"min_lr": 0.1, "max_lr": 5.0}), ("nadam", {"beta1": 0.5})])
def test_learning_rate_strategies_on_the_gpu(pj, strategy, options):
    (s, res, xf_log, _), (ref_states, ref_res, ref_xf, _) = _run_mono(pj, "BE", False, (30, 1e-9, 1e-9, 1.0), 0.0012,
                                                                      strategy=strategy, options=options)
    _compare_loops(s.states, res, xf_log, ref_states, ref_res, ref_xf)


# --------------------------------------------------------------------------------------------------------- (e) analytic
def _find_lambda(rhs):
    lo_, hi = 1e-6, 5.0
    for _ in range(200):
        mid = 0.5 * (lo_ + hi)
        if rhs(mid) > 0:
            hi = mid
        else:
            lo_ = mid
    return 0.5 * (lo_ + hi)


LAM = _find_lambda(lambda l: l * math.exp(l * l) * math.erf(l) - 1.0 / math.sqrt(math.pi))   # Ste = 1 (both benchmarks)
# measured on the MI355X: (final-position errors, L2 errors) per nx; a run must stay within 5 % of them
#   1ph, nx = 20 / 40 / 80 / 160:  position 0.2596, 0.2233, 0.1000, 0.0721;  L2 0.3557, 0.2463, 0.1317, 0.0933
#   2ph, nx = 64 / 128:             position 0.0486, 0.0338;                  L2 0.0981, 0.0674
STEFAN_1PH_BARS = ([0.2596347448910947, 0.22332028072994914, 0.09999914946458893, 0.07213123838963309],
                   [0.35569122633395994, 0.24625233442161487, 0.13169153608738746, 0.09326316920145333])
STEFAN_2PH_BARS = ([0.04859744436543434, 0.033805140245571935], [0.09811763356348696, 0.06743389608637136])


def _l2(x, mesh, xf, exact):
    """√(h Σ (T - T_exact)²) over the liquid cells of the final interface position (the benchmarks' bulk-field norm)."""
    import penguin.jl_amd as pj

    M = len(mesh.nodes[0])
    cap = pj.Capacity(pj.HalfSpace(0, xf), mesh)
    sel = (cap.V > 0) & (x[:M] != 0.0)
    ex = np.array([exact(c) for c in cap.C_ω[:, 0]])
    h = float(mesh.nodes[0][1] - mesh.nodes[0][0])
    return float(np.sqrt(h * np.sum((x[:M][sel] - ex[sel]) ** 2)))


def _stefan_1ph(pj, nx, t_end, x0=0.0):
    """benchmark/Stefan_1d_1ph.jl:126-190: T₀ = 1, k = 1, Ste = 1, lx = 10 x(0.1), Tstart = 0.01, Δt = 0.5 (lx/nx)²,
    the constructor on SpaceTimeMesh(mesh, [Δt, 2Δt]), FluxJump(k, 0, ρL), Newton (20, 1e-12, 1e-12, 1), BE, fixed Δt."""
    pos = lambda t: 2 * LAM * math.sqrt(t)
    Texact = lambda x, t: (1.0 - 1.0 / math.erf(LAM) * math.erf(x / (2 * math.sqrt(t)))) if x < pos(t) else 0.0
    lx, t0 = 10.0 * pos(0.1), 0.01
    mesh = pj.Mesh((nx,), (lx,), (x0,))
    dt = 0.5 * (lx / nx) ** 2
    xi = pos(t0)
    cap = _hip_cap(pj, mesh, xi, xi, dt, 2 * dt, True)
    f, K = (lambda x, y, z, t: 0.0), (lambda x, y, z: 1.0)
    ph = pj.Phase(cap, pj.DiffusionOps(cap), f, K)
    bcb = pj.BorderConditions({"bottom": pj.Dirichlet(1.0), "top": pj.Dirichlet(0.0)})
    ic = pj.InterfaceConditions(None, pj.FluxJump(1.0, 0.0, 1.0))
    u = np.array([Texact(x, t0) if x < xi else 0.0 for x in mesh.nodes[0]])
    s = pj.MovingLiquidDiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(0.0), dt, np.concatenate([u, u]), mesh, "BE")
    s, res, xf_log, _ = pj.solve_MovingLiquidDiffusionUnsteadyMono_b(
        s, ph, xi, dt, t0, t_end, bcb, pj.Dirichlet(0.0), ic, mesh, "BE", Newton_params=(20, 1e-12, 1e-12, 1.0),
        adaptive_timestep=False, method="bicgstab", reltol=1e-14, save_states=False)
    return abs(xf_log[-1] - pos(t_end)), _l2(s.x, mesh, xf_log[-1], lambda x: Texact(x, t_end))


def test_stefan_one_phase_neumann_solution(pj):
    """The one-phase benchmark to its own Tend = 0.1 (about 15 s), with the domain from x0 = 0: the final-position error and the
    L2 error of the bulk field fall with nx = 20 / 40 / 80 / 160.  (The benchmark's x0 = 0.1 leaves the whole liquid of the
    start, [0.1, 0.124], inside the Dirichlet border cell below nx = 160: the front does not move there, at any Tend.)"""
    errs = [_stefan_1ph(pj, nx, 0.1) for nx in (20, 40, 80, 160)]
    pos_err, l2 = [e[0] for e in errs], [e[1] for e in errs]
    print("1ph position errors", pos_err, "L2", l2)
    assert all(b < a for a, b in zip(pos_err, pos_err[1:])), pos_err
    assert all(b < a for a, b in zip(l2, l2[1:])), l2
    if STEFAN_1PH_BARS:
        assert all(e <= 1.05 * b for e, b in zip(pos_err + l2, STEFAN_1PH_BARS[0] + STEFAN_1PH_BARS[1])), (pos_err, l2)


def _stefan_2ph(pj, nx, t_span, alpha=1.0):
    """benchmark/Stefan_1d_2ph.jl:155-235, 915-963: uL = 1, uS = 0, αL = αS = 1, SteL = 1, SteS = 0, lx = 2, x0 = 0,
    xint_init = 0.05 lx, Tstart from it, Δt = 0.5 (lx/nx)², ScalarJump(1, 1, 0), FluxJump(kL, kS, ρL), Newton
    (100, 1e-8, 1e-8, 1), BE; Tend = Tstart + t_span (the benchmark: + 0.1)."""
    pos = lambda t: 2 * LAM * math.sqrt(t)
    uL = lambda x, t: (1.0 - math.erf(x / (2 * math.sqrt(t))) / math.erf(LAM)) if x < pos(t) else 0.0
    lx = 2.0
    xi = 0.05 * lx
    t0 = (xi / (2 * LAM)) ** 2
    mesh = pj.Mesh((nx,), (lx,), (0.0,))
    dt = 0.5 * (lx / nx) ** 2
    c1, c2 = _hip_cap(pj, mesh, xi, xi, 0.0, dt, True), _hip_cap(pj, mesh, xi, xi, 0.0, dt, True, True)
    f, K = (lambda x, y, z, t: 0.0), (lambda x, y, z: 1.0)
    p1, p2 = pj.Phase(c1, pj.DiffusionOps(c1), f, K), pj.Phase(c2, pj.DiffusionOps(c2), f, K)
    bcb = pj.BorderConditions({"bottom": pj.Dirichlet(1.0), "top": pj.Dirichlet(0.0)})
    ic = pj.InterfaceConditions(pj.ScalarJump(1.0, 1.0, 0.0), pj.FluxJump(1.0, 1.0, 1.0))
    M = nx + 1
    u = np.array([uL(x, t0) if x < xi else 0.0 for x in mesh.nodes[0]])
    T0 = np.concatenate([u, u, np.zeros(M), np.zeros(M)])
    s = pj.MovingLiquidDiffusionUnsteadyDiph(p1, p2, bcb, ic, dt, T0, mesh, "BE")
    t_end = t0 + t_span
    s, res, xf_log = pj.solve_MovingLiquidDiffusionUnsteadyDiph_b(s, p1, p2, xi, dt, t0, t_end, bcb, ic, mesh, "BE",
                                                                  Newton_params=(100, 1e-8, 1e-8, alpha), method="bicgstab",
                                                                  reltol=1e-14, save_states=False)
    return abs(xf_log[-1] - pos(t_end)), _l2(s.x, mesh, xf_log[-1], lambda x: uL(x, t_end))


def test_stefan_two_phase_neumann_solution(pj):
    """The two-phase benchmark with Tend = Tstart + 0.02 (the benchmark: + 0.1) at nx = 64 / 128: the final-position and L2
    errors fall.  At nx = 32 the front starts on a 10 % sliver of a cell and the fixed point on xf diverges (position error
    3.5e3 after 0.02, also with α = 0.5), so that size is left out."""
    errs = [_stefan_2ph(pj, nx, 0.02) for nx in (64, 128)]
    pos_err, l2 = [e[0] for e in errs], [e[1] for e in errs]
    print("2ph position errors", pos_err, "L2", l2)
    assert all(b < a for a, b in zip(pos_err, pos_err[1:])), pos_err
    assert all(b < a for a, b in zip(l2, l2[1:])), l2
    if STEFAN_2PH_BARS:
        assert all(e <= 1.05 * b for e, b in zip(pos_err + l2, STEFAN_2PH_BARS[0] + STEFAN_2PH_BARS[1])), (pos_err, l2)


# ----------------------------------------------------------------------------------------------- (f) state round trips
@pytest.mark.parametrize("diph", [False, True])
def test_one_state_download_per_time_step(pj, diph, monkeypatch):
    counts = []
    real = pj.Solver._fetch_state

    def counting(self, index=-1):
        counts[-1] += 1
        return real(self, index)

    monkeypatch.setattr(pj.Solver, "_fetch_state", counting)
    outs = []
    for keep in (True, False):
        counts.append(0)
        if diph:
            (s, res, xf_log), _ = _run_diph(pj, "BE", (20, 1e-9, 1e-9, 1.0), 0.002, save_states=keep)
        else:
            (s, res, xf_log, _), _ = _run_mono(pj, "BE", False, (20, 1e-9, 1e-9, 1.0), 0.002, save_states=keep)
        assert counts[-1] == (len(res) if keep else 1), (keep, counts[-1], len(res))
        outs.append((s.states[-1], xf_log))
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]
