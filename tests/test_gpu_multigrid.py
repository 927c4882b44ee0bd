"""The aggregation multigrid preconditioner (precond="mg", csrc/pg_multigrid.hip) against its numpy restatement
(tests/mg_reference.py) and against the oracle's direct solve.

Shapes are the smallest at which the kernels can go wrong: odd and even padded extents (n = 32 / 33, 40 / 41), non-square and
non-cubic grids (48 x 40, 21 x 20 x 19), N = 1, 2, 3, a system small enough to be ONE level (the dense inverse alone), and
96 x 96, whose four levels (8908, 2262, 584 and 152 rows) put two levels above the fused one-workgroup tail and two --
the last a handful of rows per kind -- inside it.

Bars
  hierarchy     aggregate maps exactly; level matrices within 1e-12 x (sum of the absolute values of the fine terms an entry
                was added up from): an entry is a sum of at most 2^N * 2 (2N + 1) products, so 1e-12 leaves two decades.
  application   max(10 δ, 1e-13 ||z||inf) with δ = the difference between the restatement in float64 and in long double on the
                same input -- measured against the reference only.
  solves        the suite's TOL_T = 1e-10 relative L2 against the oracle's direct solve fed with the product's capacities.
  stream        the bars of tests/test_gpu_streamvorticity.py: 1e-10 per stage, 1e-8 chained.

The refusal on a virtual-rank run is raised by pg_debug_run_virtual_ranks itself, before a rank thread exists (a virtual rank
that fails ends the process: it must not leave the others in a barrier), with the text of the one-rank condition.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import penguin_oracle as po
from tests import mg_reference as mg
from tests.common import oracle_capacity_from_product, rel_l2

pytestmark = pytest.mark.gpu

TOL_T = 1e-10
KEYS2 = ("left", "right", "bottom", "top")
ONE = lambda x, y=0.0, z=0.0: 1.0


# ------------------------------------------------------------------------------------ the systems
def _spec(name):
    """-> (cells, lengths, body factory, border keys)"""
    out = lambda pj: pj.Sphere((2.01, 2.01), 0.5, complement=True)
    table = {
        "out33": ((33, 33), (4.0, 4.0), out, KEYS2),
        "out32": ((32, 32), (4.0, 4.0), out, KEYS2),
        "out48x40": ((48, 40), (4.0, 4.0), out, KEYS2),
        "out96": ((96, 96), (4.0, 4.0), out, KEYS2),
        "out128": ((128, 128), (4.0, 4.0), out, KEYS2),
        "in40": ((40, 40), (4.0, 4.0), lambda pj: pj.Sphere((2.01, 2.01), 1.0), ()),
        "sph20": ((20, 20, 20), (4.0, 4.0, 4.0), lambda pj: pj.Sphere((2.01, 2.01, 2.01), 1.0), ()),
        "sph21x20x19": ((21, 20, 19), (4.0, 4.0, 4.0), lambda pj: pj.Sphere((2.01, 2.01, 2.01), 1.0), ()),
        "half40": ((40,), (1.0,), lambda pj: pj.HalfSpace(0, 0.613), ("bottom",)),
        "half41": ((41,), (1.0,), lambda pj: pj.HalfSpace(0, 0.613), ("bottom",)),
    }
    return table[name]


PARITY = ["out33", "out32", "out48x40", "out96", "in40", "sph20", "sph21x20x19", "half40", "half41"]
_BUILT = {}


def _build(pj, name, f=ONE, D=ONE, bc_i=None, borders=None, oborders=None, ctor="DiffusionSteadyMono", cache=True):
    """-> dict(s: product solver, so: oracle solver (solved directly), ext)"""
    if cache and name in _BUILT:
        return _BUILT[name]
    n, Ls, body, keys = _spec(name)
    N = len(n)
    mesh, omesh = pj.Mesh(n, Ls), po.Mesh(n, Ls, (0.0,) * N)
    cap = pj.Capacity(body(pj), mesh)
    ocap = oracle_capacity_from_product(cap, omesh)
    ph, oph = pj.Phase(cap, pj.DiffusionOps(cap), f, D), po.Phase(ocap, po.make_diffusion_ops(ocap), f, D)
    bcb = pj.BorderConditions(borders if borders is not None else {k: pj.Dirichlet(0.0) for k in keys})
    obcb = po.BorderConditions(oborders if oborders is not None else {k: po.Dirichlet(0.0) for k in keys})
    bi, obi = bc_i if bc_i is not None else (pj.Dirichlet(0.0), po.Dirichlet(0.0))
    s = getattr(pj, ctor)(ph, bcb, bi)
    so = getattr(po, ctor)(oph, obcb, obi)
    po.solve_system(so, method="\\")
    out = {"s": s, "so": so, "ext": tuple(k + 1 for k in n), "make": lambda: getattr(pj, ctor)(ph, bcb, bi), "keep": (cap, ph, bcb)}
    if cache:
        _BUILT[name] = out
    return out


def _reference_hierarchy(sy):
    if "H" not in sy:
        A, bhat, idx = sy["s"].system(2)
        ds = sy["s"].row_scaling(0)
        sy["Ahat"], sy["bhat"], sy["idx"], sy["ds"] = sp.csr_matrix(A[:, : len(idx)]), bhat, idx, ds
        sy["H"] = mg.build_hierarchy(sy["Ahat"], ds, idx, sy["ext"])
    return sy["H"]


# ------------------------------------------------------------------------------------ 1. hierarchy parity
@pytest.mark.parametrize("name", PARITY)
def test_hierarchy_equals_the_restatement(pj, name):
    from penguin.jl_amd import _lib as L

    sy = _build(pj, name)
    H = _reference_hierarchy(sy)
    h = sy["s"]._h
    level0 = L.debug_mg_level_csr(h, 0)                                     # (builds the hierarchy)
    info = sy["s"].mg_info()
    print(name, "rows", info["rows"], "nnz", info["nnz"], "tail from", info["tail_level"], f"set-up {info['setup_ms']:.2f} ms")
    assert info["levels"] == len(H.levels)
    assert info["rows"] == H.rows
    assert info["rows"][-1] <= mg.COARSEST_ROWS and all(r > mg.COARSEST_ROWS for r in info["rows"][:-1])
    assert 0 <= info["tail_level"] <= info["levels"] - 1
    worst = 0.0
    for l, lv in enumerate(H.levels):
        if l + 1 < len(H.levels):
            agg = L.debug_mg_aggregates(h, l)
            assert np.array_equal(agg, lv.agg), (name, l)
        rp, col, val = level0 if l == 0 else L.debug_mg_level_csr(h, l)
        A = sp.csr_matrix((val, col, rp), shape=lv.A.shape)
        if l == 0:
            assert abs(A - lv.A).nnz == 0 or abs(A - lv.A).max() == 0.0
            continue
        diff = abs(A - lv.A).tocoo()
        bound = lv.absA.tocsr()
        ratio = diff.data / np.maximum(np.asarray(bound[diff.row, diff.col]).ravel(), 1e-300)
        worst = max(worst, ratio.max() if ratio.size else 0.0)
        assert A.nnz == lv.A.nnz == info["nnz"][l], (name, l, A.nnz, lv.A.nnz, info["nnz"][l])
    print(name, f"largest entry difference / sum of |fine terms|: {worst:.2e}")
    assert worst <= 1e-12


def test_the_deep_case_has_levels_above_and_inside_the_tail(pj):
    sy = _build(pj, "out96")
    _reference_hierarchy(sy)
    from penguin.jl_amd import _lib as L
    L.debug_mg_apply(sy["s"]._h, np.zeros(len(sy["idx"])))
    info = sy["s"].mg_info()
    assert info["tail_level"] >= 1, info                     # at least one level above the fused tail ...
    assert info["tail_level"] <= info["levels"] - 2, info    # ... and one inside it besides the exact last level
    assert info["rows"][-1] <= 200


# ------------------------------------------------------------------------------------ 2. one application
@pytest.mark.parametrize("name", ["out96", "out33", "out48x40", "sph21x20x19", "half41", "in40"])
def test_one_application_within_the_rounding_of_the_restatement(pj, name):
    from penguin.jl_amd import _lib as L

    sy = _build(pj, name)
    H = _reference_hierarchy(sy)
    n = len(sy["idx"])
    M = int(np.prod(sy["ext"]))
    rng = np.random.default_rng(20240607)
    unit = np.zeros(n)
    unit[np.flatnonzero(sy["idx"] >= M)[0]] = 1.0            # an interface unknown: a row of a cut cell
    v64, vld = mg.VCycle(H, np.float64), mg.VCycle(H, np.longdouble)
    for what, r in (("random", rng.standard_normal(n)), ("unit at a cut cell", unit), ("b", sy["bhat"].copy())):
        z = L.debug_mg_apply(sy["s"]._h, r)
        z2 = L.debug_mg_apply(sy["s"]._h, r)
        assert np.array_equal(z, z2), "an application is not bitwise reproducible"
        zld = vld(r)
        delta = float(np.max(np.abs(v64(r).astype(np.longdouble) - zld)))
        err = float(np.max(np.abs(z.astype(np.longdouble) - zld)))
        bar = max(10.0 * delta, 1e-13 * float(np.max(np.abs(zld))))
        print(f"{name} {what}: |z - z_ld| {err:.2e}, delta {delta:.2e}, bar {bar:.2e}, |z| {float(np.max(np.abs(zld))):.2e}")
        assert err <= bar, (name, what, err, bar)


# ------------------------------------------------------------------------------------ 3. solve parity
def _solve_both(pj, sy, solve="solve_DiffusionSteadyMono_b"):
    s = sy["s"]
    getattr(pj, solve)(s, precond="mg", reltol=1e-13)
    assert s.ch[-1]["converged"]
    e_mg = rel_l2(s.x, sy["so"].x)
    p = sy["make"]()
    getattr(pj, solve)(p, precond=-1, reltol=1e-13)
    assert p.ch[-1]["converged"]
    e_plain = rel_l2(p.x, sy["so"].x)
    return e_mg, e_plain, s.ch[-1]["iters"], p.ch[-1]["iters"]


@pytest.mark.parametrize("name", PARITY)
def test_solution_equals_the_direct_solve(pj, name):
    sy = _build(pj, name)
    e_mg, e_plain, it_mg, it_plain = _solve_both(pj, sy)
    print(f"{name}: multigrid {it_mg} iterations, {e_mg:.2e}; plain {it_plain} iterations, {e_plain:.2e}")
    assert e_mg <= TOL_T and e_plain <= TOL_T


def _variants(pj):
    Dvar = lambda x, y, z=0.0: 1.0 + 0.8 * np.sin(3 * x) * np.cos(2 * y)
    fvar = lambda x, y, z=0.0: 1.0 + x * np.sin(2 * y)
    g = lambda x, y, z=0.0: 0.3 + 0.1 * x - 0.2 * y
    return {
        "variable D": dict(name="out48x40", D=Dvar),
        "source f(x, y)": dict(name="out48x40", f=fvar),
        "interface value as a function": dict(name="out48x40", bc_i=(pj.Dirichlet(g), po.Dirichlet(g))),
        "periodic pair": dict(name="out32",
                              borders={"left": pj.Periodic(), "right": pj.Periodic(), "top": pj.Dirichlet(1.0), "bottom": pj.Dirichlet(0.0)},
                              oborders={"left": po.Periodic(), "right": po.Periodic(), "top": po.Dirichlet(1.0), "bottom": po.Dirichlet(0.0)}),
        "DarcyFlow": dict(name="out32", ctor="DarcyFlow",
                          borders={"left": pj.Dirichlet(10.0), "right": pj.Dirichlet(20.0)},
                          oborders={"left": po.Dirichlet(10.0), "right": po.Dirichlet(20.0)}),
    }


@pytest.mark.parametrize("what", ["variable D", "source f(x, y)", "interface value as a function", "periodic pair", "DarcyFlow"])
def test_variants_equal_the_direct_solve(pj, what):
    kw = _variants(pj)[what]
    sy = _build(pj, cache=False, **kw)
    e_mg, e_plain, it_mg, it_plain = _solve_both(pj, sy, "solve_DarcyFlow_b" if what == "DarcyFlow" else "solve_DiffusionSteadyMono_b")
    print(f"{what}: multigrid {it_mg} iterations, {e_mg:.2e}; plain {it_plain} iterations, {e_plain:.2e}")
    assert e_mg <= TOL_T and e_plain <= TOL_T


def test_all_fluid_box_equals_the_direct_solve(pj):
    n = 24
    mesh, omesh = pj.Mesh((n, n), (1.0, 1.0)), po.Mesh((n, n), (1.0, 1.0), (0.0, 0.0))
    cap = pj.Capacity(pj.HalfSpace(0, 10.0), mesh)            # the interface lies beyond the domain
    ocap = oracle_capacity_from_product(cap, omesh)
    f = lambda x, y, z=0.0: np.sin(np.pi * x) * np.sin(np.pi * y)
    ph, oph = pj.Phase(cap, pj.DiffusionOps(cap), f, ONE), po.Phase(ocap, po.make_diffusion_ops(ocap), f, ONE)
    s = pj.DiffusionSteadyMono(ph, pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS2}), pj.Dirichlet(0.0))
    so = po.DiffusionSteadyMono(oph, po.BorderConditions({k: po.Dirichlet(0.0) for k in KEYS2}), po.Dirichlet(0.0))
    po.solve_system(so, method="\\")
    pj.solve_DiffusionSteadyMono_b(s, precond="mg", reltol=1e-13)
    p = pj.DiffusionSteadyMono(ph, pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS2}), pj.Dirichlet(0.0))
    pj.solve_DiffusionSteadyMono_b(p, precond=-1, reltol=1e-13)
    print("all fluid 24^2:", s.ch[-1]["iters"], "iterations,", s.mg_info()["rows"], "; plain", p.ch[-1]["iters"])
    assert s.ch[-1]["converged"] and rel_l2(s.x, so.x) <= TOL_T
    assert p.ch[-1]["converged"] and rel_l2(p.x, so.x) <= TOL_T


# ------------------------------------------------------------------------------------ 4. it is a preconditioner
def test_iterations_fall_to_a_quarter_and_do_not_grow_with_the_mesh(pj):
    """What fails loudest when the 1 / s weights, the over-correction or a transfer is wrong while the solve still converges."""
    iters = {}
    for name in ("out32", "out128"):
        sy = _build(pj, name)
        s = sy["make"]()
        pj.solve_DiffusionSteadyMono_b(s, precond="mg", reltol=1e-13)
        assert s.ch[-1]["converged"]
        iters[name] = s.ch[-1]["iters"]
    p = _build(pj, "out128")["make"]()
    pj.solve_DiffusionSteadyMono_b(p, precond=-1, reltol=1e-13)
    print(f"iterations: multigrid 32^2 {iters['out32']}, 128^2 {iters['out128']}; plain 128^2 {p.ch[-1]['iters']}")
    assert 4 * iters["out128"] <= p.ch[-1]["iters"]
    assert iters["out128"] <= 2 * iters["out32"]


# ------------------------------------------------------------------------------------ 5. StreamVorticity
@pytest.mark.parametrize("shape", ["B", "C"])
@pytest.mark.parametrize("scheme", ["BE", "CN"])
def test_stream_vorticity_steps_with_multigrid_on_psi(pj, shape, scheme):
    from tests.test_gpu_streamvorticity import RELTOL, TOL, TOL_CHAIN, _build as build_sv

    s, so, _ = build_sv(pj, shape)
    p, _, _ = build_sv(pj, shape)
    M = s._M
    psi_mg = psi_plain = 0
    for k in range(3):
        t, w_n = s.time, s.ω.copy()
        pj.step_StreamVorticity_b(s, scheme, reltol=RELTOL, precond="mg")
        pj.step_StreamVorticity_b(p, scheme, reltol=RELTOL, precond=0)
        (ip, iw), (jp, jw) = s.last_step, p.last_step
        psi_mg += ip.iters
        psi_plain += jp.iters
        # stage bars: ψ against the oracle's Poisson solve of the product's own ω, the velocity from it, ω from both
        assert rel_l2(s.ψ, so.poisson(w_n, t)) <= TOL
        g = po.grad(so.op, s.ψ)
        u, v = s.velocity
        assert np.allclose(u, g[M:], rtol=1e-12, atol=1e-12 * np.abs(g[M:]).max())
        assert np.allclose(v, -g[:M], rtol=1e-12, atol=1e-12 * np.abs(g[:M]).max())
        osys = so.omega_system(u, v, w_n, t, scheme)
        po.solve_system(osys, method="\\")
        assert rel_l2(s.ω, osys.x) <= TOL
        # The vorticity solve is not touched -- but its SYSTEM is not the plain run's: the convection operators are built from
        # a ψ that another iteration stopped at 1e-13, and BiCGStab's count is not a continuous function of its data (measured
        # on an MI355X, first step: shape B, BE 28 against 29; shape C, BE 63 against 66).  The counts of two runs on different
        # data are therefore printed, not compared (DESIGN.md section 14 records the deviation).  That the vorticity solve ran as
        # with precond = 0 is asserted where it can be: on bitwise the same input -- with ψ = 0 and with a ψ, u, v that are not
        # zero -- it takes the same iterations to the same bits (the two tests below).  And had the option reached it, the step
        # would have failed: an unsteady system refuses it (test_refused_on_an_unsteady_system).
        print(f"{shape}-{scheme} step {k}: omega iterations {iw.iters} (psi by multigrid) / {jw.iters} (plain)")
    so.run(3, scheme)
    for key, e in dict(psi=rel_l2(s.ψ, so.psi), omega=rel_l2(s.ω, so.omega), u=rel_l2(s.velocity[0], so.velocity[0]),
                       v=rel_l2(s.velocity[1], so.velocity[1])).items():
        assert e <= TOL_CHAIN, (key, e)
    for a, b in zip(s.states, so.states):
        assert rel_l2(a.ψ, b[1]) <= TOL_CHAIN and rel_l2(a.ω, b[2]) <= TOL_CHAIN
    print(f"{shape}-{scheme}: psi iterations over 3 steps: multigrid {psi_mg}, plain {psi_plain}; levels {s.psi_solver.mg_info()['rows']}")
    assert psi_mg < psi_plain


@pytest.mark.parametrize("scheme", ["BE", "CN"])
def test_vorticity_solve_is_bitwise_the_plain_one_on_the_same_input(pj, scheme):
    """ω0 = 0 and zero stream data: ψ = 0 exactly whatever solves for it, so the two vorticity solves of the first step (driven by
    a source) get bitwise the same system and start -- the one behind a multigrid ψ solve must take the same iterations to
    the same bits as the one behind precond = 0."""
    from tests.test_gpu_streamvorticity import RELTOL, _build as build_sv

    f = lambda x, y, z: 3.0 * np.sin(2 * np.pi * x) * np.cos(np.pi * y)
    out = []
    for precond in ("mg", 0):
        s, _, _ = build_sv(pj, "B", source=f, osource=lambda x, y, z, t: f(x, y, z))
        s.ω = np.zeros(2 * s._M)
        pj.step_StreamVorticity_b(s, scheme, reltol=RELTOL, precond=precond)
        assert not s.ψ.any() and s.ω.any()
        out.append((s.ω.copy(), s.last_step[1].iters))
    assert out[0][1] == out[1][1] and np.array_equal(out[0][0], out[1][0])


@pytest.mark.parametrize("shape", ["B", "C"])
@pytest.mark.parametrize("scheme", ["BE", "CN"])
def test_vorticity_solve_is_bitwise_the_plain_one_behind_the_same_nonzero_psi(pj, shape, scheme):
    """Both solvers first solve ψ the SAME way (plain, to 1e-14): bitwise the same ψ.  The step that follows starts its ψ solve
    from that ψ with the looser 1e-12: the start residual already meets it, the solve ends at its start whatever preconditions
    it (0 iterations asserted) and ψ, u, v stay what they were -- not zero.  The two vorticity solves therefore get bitwise the
    same convection operators, state and start, one behind precond="mg", one behind precond=0: same iterations, same bits."""
    from tests.test_gpu_streamvorticity import _build as build_sv

    out = []
    for precond in ("mg", 0):
        s, _, _ = build_sv(pj, shape)
        pj.solve_StreamVorticity_b(s, reltol=1e-14, precond=-1)
        psi = s.ψ.copy()
        pj.step_StreamVorticity_b(s, scheme, reltol=1e-12, precond=precond)
        ip, iw = s.last_step
        assert ip.iters == 0 and ip.converged and np.array_equal(s.ψ, psi), (precond, ip.iters)
        u, v = s.velocity
        assert psi.any() and np.abs(u).max() > 0 and np.abs(v).max() > 0
        if precond == "mg":
            assert s.psi_solver.mg_info()["levels"] >= 1          # the option did reach the ψ solve
        out.append((s.ω.copy(), iw.iters, psi))
    assert np.array_equal(out[0][2], out[1][2])
    assert out[0][1] == out[1][1] and out[0][1] > 0, (out[0][1], out[1][1])
    assert np.array_equal(out[0][0], out[1][0])


# ------------------------------------------------------------------------------------ 6. refusals
def _small(pj):
    n = 24
    mesh = pj.Mesh((n, n), (4.0, 4.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0), mesh)
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS2})
    return n, mesh, cap, bcb


@pytest.mark.parametrize("kind,word", [("robin", "Robin"), ("neumann", "Neumann")])
def test_refused_on_robin_and_neumann_interfaces(pj, kind, word):
    n, mesh, _, bcb = _small(pj)
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0, complement=True), mesh)      # fluid outside: the Dirichlet borders pin the solution
    bc = pj.Robin(1.0, 1.0, 0.5) if kind == "robin" else pj.Neumann(0.0)
    s = pj.DiffusionSteadyMono(pj.Phase(cap, pj.DiffusionOps(cap), ONE, ONE), bcb, bc)
    with pytest.raises(pj.PenguinHipError, match=word):
        pj.solve_DiffusionSteadyMono_b(s, precond="mg")
    pj.solve_DiffusionSteadyMono_b(s, precond=0)
    assert s.ch[-1]["converged"]


def test_refused_on_a_diphasic_system(pj):
    n, mesh, c1, bcb = _small(pj)
    c2 = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0, complement=True), mesh)
    ic = pj.InterfaceConditions(pj.ScalarJump(1.0, 1.0, 0.0), pj.FluxJump(1.0, 1.0, 0.0))
    s = pj.DiffusionSteadyDiph(pj.Phase(c1, pj.DiffusionOps(c1), ONE, ONE), pj.Phase(c2, pj.DiffusionOps(c2), ONE, ONE), bcb, ic)
    with pytest.raises(pj.PenguinHipError, match="diphasic"):
        pj.solve_DiffusionSteadyDiph_b(s, precond="mg")
    pj.solve_DiffusionSteadyDiph_b(s, precond=0)
    assert s.ch[-1]["converged"]


def test_refused_on_an_unsteady_system(pj):
    n, mesh, cap, bcb = _small(pj)
    M = (n + 1) ** 2
    ph = pj.Phase(cap, pj.DiffusionOps(cap), 0.0, 1.0)
    dt = 0.25 * (4.0 / n) ** 2
    s = pj.DiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(1.0), dt, np.concatenate([np.zeros(M), np.ones(M)]), "BE")
    with pytest.raises(pj.PenguinHipError, match="unsteady"):
        pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 3 * dt, bcb, pj.Dirichlet(1.0), "BE", precond="mg")
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 3 * dt, bcb, pj.Dirichlet(1.0), "BE", precond=0)
    assert s.unconverged == 0


def test_refused_on_an_advection_diffusion_system(pj):
    from tests.test_gpu_parity import _velocity_fields

    n, mesh, cap, bcb = _small(pj)
    u, ug = _velocity_fields(cap, 2, (n + 1) ** 2)
    s = pj.AdvectionDiffusionSteadyMono(pj.Phase(cap, pj.ConvectionOps(cap, u, ug), ONE, ONE), bcb, pj.Dirichlet(1.0))
    with pytest.raises(pj.PenguinHipError, match="ConvectionOps"):
        pj.solve_AdvectionDiffusionSteadyMono_b(s, precond="mg")
    pj.solve_AdvectionDiffusionSteadyMono_b(s, precond=0)
    assert s.ch[-1]["converged"]


@pytest.mark.parametrize("method,word", [("cg", "CG"), ("gmres", "GMRES")])
def test_refused_with_cg_and_gmres(pj, method, word):
    n, mesh, cap, bcb = _small(pj)
    s = pj.DiffusionSteadyMono(pj.Phase(cap, pj.DiffusionOps(cap), ONE, ONE), bcb, pj.Dirichlet(0.0))
    with pytest.raises(pj.PenguinHipError, match=word):
        pj.solve_DiffusionSteadyMono_b(s, method=method, precond="mg")
    pj.solve_DiffusionSteadyMono_b(s, precond=0)
    assert s.ch[-1]["converged"]


def test_refused_on_a_virtual_rank_run(pj):
    """2 virtual ranks on a 16^2 disc problem: refused by the entry point with the one-rank condition, before a rank starts;
    the same configuration then runs with precond = 0."""
    import ctypes as C
    from penguin.jl_amd import _lib as L

    lib = L.lib()
    nn, LL = np.array([16, 16], dtype=np.int64), np.array([4.0, 4.0])
    params = np.array([2.01, 2.01, 1.0])
    keys = np.array([L.PG_KEY[k] for k in ("left", "right", "top", "bottom")], dtype=np.int32)
    x = np.zeros(2 * 17 * 17)
    outs = [np.zeros(2, dtype=np.int64) for _ in range(4)]

    def run():
        return lib.pg_debug_run_virtual_ranks(2, 2, L.iptr(nn), L.dptr(LL), L.PG_BODY_BALL, L.dptr(params), len(params), C.c_double(1.0),
                                              C.c_double(1.0), len(keys), keys.ctypes.data_as(L.c_i32_p), C.c_double(0.04), 0, 0,
                                              C.c_int64(2), L.dptr(x), *(L.iptr(o) for o in outs))

    try:
        L.check(lib.pg_debug_set_virtual_rank_precond(L.PG_PRECOND_MG))
        with pytest.raises(pj.PenguinHipError, match="one rank"):
            L.check(run())
    finally:
        L.check(lib.pg_debug_set_virtual_rank_precond(0))
    L.check(run())
    assert outs[0].sum() > 0 and np.isfinite(x).all() and x.any()


def test_an_unknown_preconditioner_name_is_a_value_error(pj):
    n, mesh, cap, bcb = _small(pj)
    s = pj.DiffusionSteadyMono(pj.Phase(cap, pj.DiffusionOps(cap), ONE, ONE), bcb, pj.Dirichlet(0.0))
    with pytest.raises(ValueError):
        pj.solve_DiffusionSteadyMono_b(s, precond="amg")


# ------------------------------------------------------------------------------------ 7. nothing else moved
def test_other_paths_are_bitwise_unchanged_by_a_multigrid_solve_in_the_process(pj):
    n, mesh, cap, bcb = _small(pj)
    M = (n + 1) ** 2
    dt = 0.25 * (4.0 / n) ** 2

    def run(precond):
        st = pj.DiffusionSteadyMono(pj.Phase(cap, pj.DiffusionOps(cap), ONE, ONE), bcb, pj.Dirichlet(0.0))
        pj.solve_DiffusionSteadyMono_b(st, precond=precond, reltol=1e-13)
        ph = pj.Phase(cap, pj.DiffusionOps(cap), 0.0, 1.0)
        un = pj.DiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(1.0), dt, np.concatenate([np.zeros(M), np.ones(M)]), "BE")
        pj.solve_DiffusionUnsteadyMono_b(un, ph, dt, 1e30, bcb, pj.Dirichlet(1.0), "BE", max_steps=1, precond=precond, reltol=1e-13)
        return st.x.copy(), un.x.copy(), st.ch[-1]["iters"]

    before = {p: run(p) for p in (0, -1, 6)}
    other = pj.DiffusionSteadyMono(pj.Phase(cap, pj.DiffusionOps(cap), ONE, ONE), bcb, pj.Dirichlet(0.0))
    pj.solve_DiffusionSteadyMono_b(other, precond="mg", reltol=1e-13)
    assert other.ch[-1]["converged"] and other.mg_info()["levels"] >= 1
    for p, (x_st, x_un, it) in before.items():
        a_st, a_un, a_it = run(p)
        assert np.array_equal(a_st, x_st) and np.array_equal(a_un, x_un) and a_it == it, p
