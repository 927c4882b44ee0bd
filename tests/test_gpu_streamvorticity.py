"""StreamVorticity on the GPU (penguin/jl_amd/streamvorticity.py, csrc/pg_streamvort.hip) against the oracle composition of the
reference's step (tests/streamvorticity_oracle.py), on capacities computed by the product (isolates the solver path).

Shapes
  A  12², all fluid, ν = 0.01, Δt = 5e-3, ω0 = sin(πx) sin(πy), zero Dirichlet everywhere
  B  24², fluid inside the disc r = 0.2 at (0.5, 0.5), ν = 5e-3, Δt = 5e-3, ω0 = exp(-r²/0.04), zero Dirichlet, 3 steps
  C  32², flow past the cylinder r = 0.15 at (0.5, 0.47) (off the grid lines): ψ = y on the four borders (a uniform stream),
     ψ = 0.47 on the body, ω = 0 on borders and body, ω0 = 20 exp(-((x-0.25)² + (y-0.6)²)/0.01), ν = 1e-3, Δt = 1e-2, 4 steps

Bars
  stage by stage (every stage against the oracle fed with the product's own previous stage): ψ and ω ≤ 1e-10 relative L2
  (the project's parity bar); u, v as `grad` in test_gpu_parity.py (rtol 1e-12, atol 1e-12 max|.|); the ω system as
  _check_system there (same index set, 1e-12 of the largest entry).
  chained run against the oracle's own chained run: ≤ 1e-8.  Perturbing every oracle solve by relative 1e-12 white noise
  (the Krylov stopping tolerance) moves the final fields by about 1e-10 (the gradient amplifies by 1/h and Wꜝ); 1e-8 leaves
  two decades.  A wrong term shows far above it: with the velocity zeroed the oracle's final ω differs by 0.12 ... 0.46, and
  the test asserts that difference is ≥ 1e-2 on the inputs it uses.
"""
import numpy as np
import pytest

from oracle import penguin_oracle as po
from tests.common import oracle_capacity_from_product, rel_l2
from tests.streamvorticity_oracle import OracleStreamVorticity

pytestmark = pytest.mark.gpu

KEYS = ("left", "right", "bottom", "top")
TOL = 1e-10           # parity bar, relative L2
TOL_CHAIN = 1e-8      # chained run (see the module docstring)
RELTOL = 1e-13        # Krylov tolerance of the product's solves, as the other parity tests


def _stream(x, y, t=0.0):
    return y


def _build(pj, name, source=None, osource=None, nu=None):
    """-> (product solver, oracle twin, steps)"""
    zb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS})
    ozb = po.BorderConditions({k: po.Dirichlet(0.0) for k in KEYS})
    if name == "A":
        n, body, nu0, dt, steps = 12, pj.HalfSpace(0, 10.0), 0.01, 5e-3, 2
    elif name == "B":
        n, body, nu0, dt, steps = 24, pj.Sphere((0.5, 0.5), 0.2), 5e-3, 5e-3, 3
    else:
        n, body, nu0, dt, steps = 32, pj.Sphere((0.5, 0.47), 0.15, complement=True), 1e-3, 1e-2, 4
    mesh, omesh = pj.Mesh((n, n), (1.0, 1.0), (0.0, 0.0)), po.Mesh((n, n), (1.0, 1.0), (0.0, 0.0))
    cap = pj.Capacity(body, mesh)
    ocap = oracle_capacity_from_product(cap, omesh)
    M = (n + 1) ** 2
    x, y = cap.C_ω[:, 0], cap.C_ω[:, 1]
    if name == "A":
        w = np.sin(np.pi * x) * np.sin(np.pi * y)
    elif name == "B":
        w = np.exp(-((x - 0.5) ** 2 + (y - 0.5) ** 2) / 0.04)
    else:
        w = 20.0 * np.exp(-((x - 0.25) ** 2 + (y - 0.6) ** 2) / 0.01)
    w0 = np.concatenate([w, np.zeros(M)])
    kw = dict(bc_stream_border=zb, bc_vorticity_border=zb, ω0=w0)
    okw = dict(bc_stream_border=ozb, bc_vorticity_border=ozb, omega0=w0)
    if name == "C":
        kw.update(bc_stream=pj.Dirichlet(0.47), bc_stream_border=pj.BorderConditions({k: pj.Dirichlet(_stream) for k in KEYS}))
        okw.update(bc_stream=po.Dirichlet(0.47), bc_stream_border=po.BorderConditions({k: po.Dirichlet(_stream) for k in KEYS}))
    if source is not None:
        kw["source"] = source
        okw["source"] = osource
    s = pj.StreamVorticity(cap, nu0 if nu is None else nu, dt, **kw)
    so = OracleStreamVorticity(ocap, nu0, dt, **okw)
    return s, so, steps


def _check_system(s, so):
    """as test_gpu_parity._check_system: same active index set (bit-exact), same matrix, same right-hand side"""
    A, b, idx = s.system(0)
    Ar, br, oidx = po.remove_zero_rows_cols(so.A, so.b)
    assert np.array_equal(idx, oidx)
    A = A[:, : len(idx)]
    assert abs(A - Ar).max() <= 1e-12 * abs(Ar).max()
    assert np.max(np.abs(b - br)) <= 1e-12 * max(np.max(np.abs(br)), 1e-300)
    return idx


# ------------------------------------------------------------------------------------ the reference's three testsets
def test_reference_testset_uniform(pj):
    """test/solver/stream_vorticity_test.jl:8-52 on shape A; the residual from the ψ solver's exported system."""
    s, _, _ = _build(pj, "A")
    M = 13 * 13
    Cw = s.capacity.C_ω
    s.ω = np.concatenate([np.sin(np.pi * Cw[:, 0]) * np.sin(np.pi * Cw[:, 1]), np.zeros(M)])      # :34-35
    pj.solve_StreamVorticity_b(s, method="gmres")                                                  # :37
    A, b, idx = s.psi_solver.system(0)
    residual = np.linalg.norm(A[:, : len(idx)] @ s.ψ[idx] - b) / max(np.linalg.norm(b), 1.0)
    print("Poisson residual", residual)
    assert residual <= 1e-8                                                                        # :43
    assert np.max(np.abs(b)) > 0
    u, v = s.velocity
    assert len(u) == M and len(v) == M                                                             # :46-47
    assert s.last_convection is s.last_convection and isinstance(s.last_convection, pj.ConvectionOps)   # :49-51
    assert s.Aψ.shape == (2 * M, 2 * M)


def test_reference_testset_step(pj):
    """:54-92 -- 10², ω0 = 0."""
    mesh = pj.Mesh((10, 10), (1.0, 1.0), (0.0, 0.0))
    cap = pj.Capacity(pj.HalfSpace(0, 10.0), mesh)
    zb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS})
    dt = 1e-2
    s = pj.StreamVorticity(cap, 0.02, dt, bc_stream=pj.Dirichlet(0.0), bc_vorticity=pj.Dirichlet(0.0), bc_stream_border=zb,
                           bc_vorticity_border=zb, ω0=np.zeros(2 * 121))
    pj.step_StreamVorticity_b(s, method="gmres")
    assert abs(s.time - dt) <= 1e-12 and len(s.states) == 2 and np.linalg.norm(s.ω) <= 1e-12       # :82-84
    pj.run_StreamVorticity_b(s, 2, method="gmres")
    assert abs(s.time - 3 * dt) <= 1e-12 and len(s.states) == 4                                    # :87-88
    times = [st.time for st in s.states]
    assert times == sorted(times)                                                                  # :91


def test_reference_testset_cut_cell(pj):
    """:94-134 on shape B."""
    s, _, _ = _build(pj, "B")
    assert s.last_convection is None
    pj.solve_StreamVorticity_b(s, method="gmres")
    u, v = s.velocity
    assert np.max(np.abs(u)) > 0 and np.max(np.abs(v)) > 0                                         # :128-129
    pj.step_StreamVorticity_b(s, method="gmres")
    assert isinstance(s.last_convection, pj.ConvectionOps)                                         # :132
    assert np.all(np.isfinite(s.ω))                                                                # :133


# ------------------------------------------------------------------------------------ stage by stage
@pytest.mark.parametrize("name,scheme", [("B", "BE"), ("B", "CN"), ("C", "BE"), ("C", "CN")])
def test_every_stage_matches_the_oracle_fed_with_the_products_previous_stage(pj, name, scheme):
    """Measured on an MI355X: ψ <= 2.2e-12, ω <= 1.4e-13 on every stage.  Shape B's FIRST vorticity system is close to singular
    (condition number 3.3e16, 4.5e5 once equilibrated): the bulk row of the solid cell (16, 16) (V = 0) is reached only by the
    convection stencil of its two cut neighbours, and as B's data are mirror symmetric about the diagonal through that cell the
    two entries cancel to a diagonal of -4.5e-20 next to off-diagonals of +-1.5e-6 -- a constraint between the neighbours, its
    unknown their multiplier.  BiCGStab stopped at 1e-13 alone leaves 5.2e-9 (BE) / 9.2e-7 (CN) there (the oracle's own BiCGStab
    restatement: 4e-8); with the step of iterative refinement that follows the vorticity solve: 3.5e-15 / 1.4e-14."""
    s, so, steps = _build(pj, name)
    M = s._M
    missed = []                     # (every step is measured before the verdict)
    for k in range(steps):
        t, w_n = s.time, s.ω.copy()
        pj.step_StreamVorticity_b(s, scheme, reltol=RELTOL)
        psi, (u, v), w_np1 = s.ψ, s.velocity, s.ω
        e_psi = rel_l2(psi, so.poisson(w_n, t))
        g = po.grad(so.op, psi)
        ou, ov = g[M:], -g[:M]
        print(f"{name}-{scheme} step {k}: psi {e_psi:.2e}  max|u| {np.abs(u).max():.3f} max|v| {np.abs(v).max():.3f}")
        if e_psi > TOL:
            missed.append((k, "psi", e_psi))
        assert np.allclose(u, ou, rtol=1e-12, atol=1e-12 * np.abs(ou).max())
        assert np.allclose(v, ov, rtol=1e-12, atol=1e-12 * np.abs(ov).max())
        osys = so.omega_system(u, v, w_n, t, scheme)
        _check_system(s.omega_solver, osys)
        po.solve_system(osys, method="\\")
        e_w = rel_l2(w_np1, osys.x)
        print(f"{name}-{scheme} step {k}: omega {e_w:.2e}")
        if e_w > TOL:
            missed.append((k, "omega", e_w))
    assert not missed, f"stages above {TOL:.0e}: {missed}"
    assert np.abs(s.velocity[0]).max() > 0 and np.abs(s.velocity[1]).max() > 0


# ------------------------------------------------------------------------------------ chained run
@pytest.mark.parametrize("name,scheme", [("B", "BE"), ("B", "CN"), ("C", "BE"), ("C", "CN")])
def test_chained_run_matches_the_oracles_chained_run(pj, name, scheme):
    """Measured on an MI355X (ψ, ω, u, v): B-BE 1.2e-14, 2.2e-13, 1.6e-14, 2.0e-14; B-CN 1.6e-14, 1.7e-12, 3.2e-14, 3.3e-14;
    C-BE 1.6e-12, 7.7e-12, 5.4e-12, 2.2e-11; C-CN 1.9e-12, 1.4e-11, 5.0e-12, 2.8e-11."""
    s, so, steps = _build(pj, name)
    _, sz, _ = _build(pj, name)
    sz.zero_velocity = True
    pj.run_StreamVorticity_b(s, steps, scheme, reltol=RELTOL)
    so.run(steps, scheme)
    sz.run(steps, scheme)
    blind = rel_l2(sz.omega, so.omega)
    errs = dict(psi=rel_l2(s.ψ, so.psi), omega=rel_l2(s.ω, so.omega), u=rel_l2(s.velocity[0], so.velocity[0]),
                v=rel_l2(s.velocity[1], so.velocity[1]))
    print(f"{name}-{scheme}: {errs}; the oracle without convection differs by {blind:.3f}")
    assert blind >= 1e-2          # the inputs make convection visible
    assert len(s.states) == len(so.states) == steps + 1
    for key, e in errs.items():
        assert e <= TOL_CHAIN, (key, e)


# ------------------------------------------------------------------------------------ behaviour
def test_states_time_and_the_lag_of_psi(pj):
    s, so, steps = _build(pj, "B")
    pj.run_StreamVorticity_b(s, steps, reltol=RELTOL)
    st = s.states
    assert len(st) == steps + 1 and st[0].time == 0.0 and np.array_equal(st[0].ω, so.omega) and not st[0].ψ.any()
    t = 0.0
    for k in range(1, steps + 1):
        t += s.Δt
        assert st[k].time == t
        assert rel_l2(st[k].ψ, so.poisson(st[k - 1].ω, st[k - 1].time)) <= TOL      # ψ of state k: solved from ω of state k-1
    assert s.time == t and np.array_equal(st[-1].ω, s.ω) and np.array_equal(st[-1].ψ, s.ψ)


def test_run_until_stops_by_the_reference_rule(pj):
    s, _, _ = _build(pj, "B")
    dt = s.Δt
    pj.run_until_StreamVorticity_b(s, 3 * dt)
    assert len(s.states) == 4 and abs(s.time - 3 * dt) <= 1e-12
    pj.run_until_StreamVorticity_b(s, s.time + 1e-13)          # time < t_end - 1e-12 is false: no step
    assert len(s.states) == 4
    pj.run_until_StreamVorticity_b(s, s.time + 1e-9)           # ... true: one step
    assert len(s.states) == 5


def test_step_after_assigning_omega_uses_it(pj):
    s, so, _ = _build(pj, "B")
    pj.step_StreamVorticity_b(s, reltol=RELTOL)
    Cw = s.capacity.C_ω
    w = np.concatenate([np.cos(3 * Cw[:, 0]) * np.exp(-((Cw[:, 1] - 0.45) ** 2) / 0.02), np.zeros(s._M)])
    s.ω = w
    assert np.array_equal(s.ω, w)
    t = s.time
    pj.step_StreamVorticity_b(s, "CN", reltol=RELTOL)
    psi, u, v, w1 = so.step_from(w, t, "CN")
    assert rel_l2(s.ψ, psi) <= TOL and rel_l2(s.ω, w1) <= TOL_CHAIN


def test_time_dependent_and_constant_source_give_the_same_states(pj):
    """the host-driven loop (a source with a time parameter) and the loop inside the library (the same source without one)"""
    f_t = lambda x, y, z, t: 3.0 * np.sin(2 * np.pi * x) * np.cos(np.pi * y)
    f_c = lambda x, y, z: 3.0 * np.sin(2 * np.pi * x) * np.cos(np.pi * y)
    f_o = lambda x, y, z, t: 3.0 * np.sin(2 * np.pi * x) * np.cos(np.pi * y)
    a, so, steps = _build(pj, "B", source=f_t, osource=f_o)
    b, _, _ = _build(pj, "B", source=f_c, osource=f_o)
    assert a._dynamic and not b._dynamic
    pj.run_StreamVorticity_b(a, steps, "CN", reltol=RELTOL)
    pj.run_StreamVorticity_b(b, steps, "CN", reltol=RELTOL)
    assert b.last_run is not None and b.last_run.steps == steps and a.last_run is None
    assert len(a.states) == len(b.states) == steps + 1
    for x, y in zip(a.states, b.states):
        assert x.time == y.time and rel_l2(x.ψ, y.ψ) <= 1e-12 and rel_l2(x.ω, y.ω) <= 1e-12
    so.run(steps, "CN")
    plain, _, _ = _build(pj, "B")
    pj.run_StreamVorticity_b(plain, steps, "CN", reltol=RELTOL)
    assert rel_l2(b.ω, so.omega) <= TOL_CHAIN and rel_l2(plain.ω, so.omega) >= 1e-3       # the source is in the answer


def test_viscosity_as_a_function(pj):
    a, _, steps = _build(pj, "B")
    b, _, _ = _build(pj, "B", nu=lambda x, y, z: 5e-3 + 0.0 * x)
    pj.run_StreamVorticity_b(a, steps, "CN", reltol=RELTOL)
    pj.run_StreamVorticity_b(b, steps, "CN", reltol=RELTOL)
    assert rel_l2(b.ω, a.ω) <= 1e-12 and rel_l2(b.ψ, a.ψ) <= 1e-12


def test_refusals_carry_a_message(pj):
    for N in (1, 3):
        mesh = pj.Mesh((6,) * N, (1.0,) * N)
        cap = pj.Capacity(pj.Sphere((0.5,) * N, 0.3), mesh)
        with pytest.raises(pj.PenguinHipError, match="two-dimensional"):
            pj.StreamVorticity(cap, 0.01, 1e-3)
    s, _, _ = _build(pj, "B")
    with pytest.raises(ValueError, match="Unknown scheme."):
        pj.step_StreamVorticity_b(s, "RK4")
    with pytest.raises(ValueError, match="Unknown scheme."):
        pj.run_StreamVorticity_b(s, 2, "euler")
    other = pj.Capacity(pj.Sphere((0.5, 0.5), 0.3), s.capacity.mesh)
    with pytest.raises(pj.PenguinHipError, match="different capacity"):
        pj.StreamVorticity(s.capacity, 0.01, 1e-3, operator=pj.DiffusionOps(other))
    assert len(s.states) == 1 and s.time == 0.0


def test_save_every(pj):
    a, _, _ = _build(pj, "B")
    b, _, _ = _build(pj, "B")
    pj.run_StreamVorticity_b(a, 4, reltol=RELTOL)
    pj.run_StreamVorticity_b(b, 4, save_every=2, reltol=RELTOL)
    assert len(a.states) == 5 and len(b.states) == 3
    assert [st.time for st in b.states] == [a.states[k].time for k in (0, 2, 4)]
    for st, k in zip(b.states, (0, 2, 4)):
        assert rel_l2(st.ω, a.states[k].ω) <= 1e-12 if k else np.array_equal(st.ω, a.states[k].ω)
    c, _, _ = _build(pj, "B")
    pj.run_StreamVorticity_b(c, 4, save_every=0, reltol=RELTOL)
    assert len(c.states) == 1 and rel_l2(c.ω, a.ω) <= 1e-12


# ------------------------------------------------------------------------------------ device residency
@pytest.mark.parametrize("scheme", ["BE", "CN"])
def test_a_run_in_the_library_equals_single_steps(pj, scheme):
    """pg_streamvort_run (states handed from solver to solver on the device) against three pg_streamvort_step calls"""
    a, _, _ = _build(pj, "C")
    b, _, _ = _build(pj, "C")
    pj.run_StreamVorticity_b(a, 3, scheme, reltol=RELTOL)
    for _ in range(3):
        pj.step_StreamVorticity_b(b, scheme, reltol=RELTOL)
    assert a.time == b.time
    assert rel_l2(a.ω, b.ω) <= 1e-12 and rel_l2(a.ψ, b.ψ) <= 1e-12
    for p, q in zip(a.velocity, b.velocity):
        assert rel_l2(p, q) <= 1e-12
    r = a.last_run
    assert r.steps == 3 and r.unconverged == 0 and r.psi_products > 0 and r.omega_products > 0
    assert r.total_ms > 0 and abs(r.psi_ms + r.velocity_ms + r.build_ms + r.omega_ms - r.total_ms) <= 0.05 * r.total_ms + 1.0
