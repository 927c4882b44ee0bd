"""The multigrid preconditioner of the time loop (precond="mg-step", PG_PRECOND_MG_STEP): the cell-aggregated V-cycle of
csrc/pg_multigrid.hip as right preconditioner of the device BiCGStab on the systems of DiffusionUnsteadyMono, at steps far above
h².  Against its numpy restatement (tests/mgc_reference.py), the oracle's direct solves, and the same runs under default options.

Shapes: 32^2 (fluid outside the disc, four border rows), 33^2 (odd padded extent, fluid inside the disc, no border rows), 48 x 40
and 12^3 -- the smallest at which cut cells, border rows, odd extents and the fused tail all occur.  Δt = 64 h² unless a test says
otherwise.

Bars
  hierarchy     as tests/test_gpu_mg_cell.py::test_hierarchy_equals_the_restatement: aggregate maps exactly, every level within
                1e-12 x (sum of |fine terms|) of Pᵀ A P of the library's own level above, and within 1e-12 x (sum of |level-0
                terms|) of the restatement's own level.  Both hierarchies: which = 0 (BE constructor system), 1 (CN run system).
  application   max(10 δ, 1e-13 ||z||inf), δ = restatement in float64 against long double (the bar of that file's
                test_one_application_within_the_rounding_of_the_restatement); bitwise reproducible.
  states        the suite's TOL_T = 1e-10 relative L2 against the oracle's direct solves, step by step.
  Δt = 1024 h²  max(TOL_T, 10 x the error of the default-option device run against the same oracle solves): the condition number
                of the system grows with the step, and what a solve stopped at reltol = 1e-12 can promise grows with it.
  counts        first solve: 2 x iterations <= the restatement's applications on the same Â + 4; 3 x that <= the products of the
                precond = -1 run; a warm step takes no more iterations than the zero-start solve of the same step.
  loop          states within TOL_T and monitor series within 1e-9 x their scale of the same run under default options (the
                bars of tests/test_gpu_time_separable.py and tests/test_gpu_monitors.py).
"""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import penguin_oracle as po
from tests import mgc_reference as mgc
from tests.common import oracle_capacity_from_product, rel_l2

pytestmark = pytest.mark.gpu

TOL_T = 1e-10
KEYS2 = ("left", "right", "bottom", "top")
SRC = lambda x, y, z=0.0, t=0.0: 1.0 + 0.3 * x        # (constant in time: every run passes time_independent=True)
ONE = lambda x, y, z=0.0: 1.0
SCHEMES = [("BE", "BE"), ("BE", "CN"), ("CN", "CN")]


# ------------------------------------------------------------------------------------ the systems
def _bc(mod, kind, value=None):
    if kind == "dirichlet":
        return mod.Dirichlet(1.0 if value is None else value)
    return {"robin": mod.Robin(1.0, 1.0, 1.0), "neumann": mod.Neumann(0.0)}[kind]


def _spec(name):
    """-> (cells, body factory, border keys, interface condition)"""
    out = lambda pj: pj.Sphere((2.01, 2.01), 1.0, complement=True)        # the 2-D body of tests/specest_systems.py::mono
    disc = lambda pj: pj.Sphere((2.01, 2.01), 1.0)
    ball = lambda pj: pj.Sphere((2.01, 2.01, 2.01), 1.0)                   # the sphere of tests/test_mgc_reference.py
    return {
        "dirichlet32": ((32, 32), out, KEYS2, "dirichlet"),
        "robin32": ((32, 32), out, KEYS2, "robin"),
        "robin33": ((33, 33), disc, (), "robin"),
        "neumann48x40": ((48, 40), out, KEYS2, "neumann"),
        "dirichlet12c": ((12, 12, 12), ball, (), "dirichlet"),
        "robin12c": ((12, 12, 12), ball, (), "robin"),
    }[name]


def _pair(pj, name, scheme0, ratio=64, f=SRC, g=None, oracle=True):
    """-> dict(s, ph, bcb, bci, dt, ext, M and, with oracle, so, oph, obcb, obci).  Δt = ratio h², h the first direction's."""
    n, body, keys, kind = _spec(name)
    N = len(n)
    Ls = (4.0,) * N
    mesh = pj.Mesh(n, Ls)
    cap = pj.Capacity(body(pj), mesh)
    M = int(np.prod([k + 1 for k in n]))
    u0 = np.concatenate([0.2 * np.ones(M), np.ones(M)])
    dt = ratio * (4.0 / n[0]) ** 2
    ph = pj.Phase(cap, pj.DiffusionOps(cap), f, ONE)
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in keys})
    bci = _bc(pj, kind, g)
    c = {"s": pj.DiffusionUnsteadyMono(ph, bcb, bci, dt, u0, scheme0), "ph": ph, "bcb": bcb, "bci": bci, "dt": dt,
         "ext": tuple(k + 1 for k in n), "M": M, "keep": (mesh, cap)}
    if oracle:
        omesh = po.Mesh(n, Ls, (0.0,) * N)
        ocap = oracle_capacity_from_product(cap, omesh)
        c["oph"] = po.Phase(ocap, po.make_diffusion_ops(ocap), f, ONE)
        c["obcb"] = po.BorderConditions({k: po.Dirichlet(0.0) for k in keys})
        c["obci"] = _bc(po, kind, g)
        c["so"] = po.DiffusionUnsteadyMono(c["oph"], c["obcb"], c["obci"], dt, u0, scheme0)
    return c


def _solve(pj, c, scheme, steps, **kw):
    kw.setdefault("reltol", 1e-12)
    kw.setdefault("time_independent", True)
    pj.solve_DiffusionUnsteadyMono_b(c["s"], c["ph"], c["dt"], steps * c["dt"], c["bcb"], c["bci"], scheme, **kw)
    return c["s"]


_ORACLE = {}


def _oracle_states(pj, name, scheme0, scheme, ratio, steps=6):
    """The oracle's direct solves of a case, computed once and left unchanged."""
    key = (name, scheme0, scheme, ratio, steps)
    if key not in _ORACLE:
        c = _pair(pj, name, scheme0, ratio)
        po.solve_DiffusionUnsteadyMono(c["so"], c["oph"], c["dt"], steps * c["dt"], c["obcb"], c["obci"], scheme, method="\\")
        _ORACLE[key] = [np.array(x) for x in c["so"].states]
    return _ORACLE[key]


# ------------------------------------------------------------------------------------ 1. both hierarchies
_TWO = {}


def _two_hierarchies(pj, name):
    """A BE constructor, two CN steps under the option: both hierarchies exist.  With the restatement's hierarchy of each of the
    product's two matrices, computed once."""
    if name not in _TWO:
        c = _pair(pj, name, "BE", oracle=False)
        s = _solve(pj, c, "CN", 2, precond="mg-step")
        assert s.unconverged == 0
        _restate(c)
        _TWO[name] = c
    return _TWO[name]


def _restate(c):
    """The restatement's hierarchy of each of the solver's two matrices (pg_solver_get_system_csr of the same matrix)."""
    s = c["s"]
    c["ref"] = []
    for which in (0, 1):
        A, bhat, idx = s.system(2 + which)
        ds = s.row_scaling(which)
        Ahat = sp.csr_matrix(A[:, : len(idx)])
        c["ref"].append({"Ahat": Ahat, "bhat": bhat, "idx": idx, "ds": ds, "H": mgc.build_hierarchy_cells(Ahat, ds, idx, c["ext"])})


def _worst_ratio(A, ref, bound):
    diff = abs(A - ref).tocoo()
    b = np.asarray(bound.tocsr()[diff.row, diff.col]).ravel()
    ratio = diff.data / np.maximum(b, 1e-300)
    return float(ratio.max()) if ratio.size else 0.0


@pytest.mark.parametrize("name", ["dirichlet32", "robin33", "robin12c"])
def test_both_hierarchies_equal_the_restatement(pj, name):
    _check_both_hierarchies(_two_hierarchies(pj, name), name)


def _check_both_hierarchies(c, name):
    from penguin.jl_amd import _lib as L

    s = c["s"]
    infos = s.mg_step_info()
    assert s.mg_info("mg")["levels"] == 0 and s.mg_info("mg-cell")["levels"] == 0        # slots of its own
    assert abs(c["ref"][0]["Ahat"] - c["ref"][1]["Ahat"]).max() > 1e-3                   # (two different matrices)
    for which in (0, 1):
        H, info, h = c["ref"][which]["H"], infos[which], s._h
        print(name, "which", which, "rows", info["rows"], "nnz", info["nnz"], "tail from", info["tail_level"],
              f"set-up {info['setup_ms']:.2f} ms, {info['bytes']} bytes")
        assert info["levels"] == len(H.levels) >= 2
        assert info["rows"] == H.rows
        assert info["rows"][-1] <= mgc.COARSEST_ROWS and all(r > mgc.COARSEST_ROWS for r in info["rows"][:-1])
        assert 0 <= info["tail_level"] <= info["levels"] - 1
        worst = whole = 0.0
        below = None
        for l, lv in enumerate(H.levels):
            if l + 1 < len(H.levels):
                assert np.array_equal(L.debug_mg_step_aggregates(h, which, l), lv.agg), (name, which, l)
            rp, col, val = L.debug_mg_step_level_csr(h, which, l)
            A = sp.csr_matrix((val, col, rp), shape=lv.A.shape)
            if l == 0:
                assert abs(A - c["ref"][which]["Ahat"]).max() == 0.0                    # level 0 IS the loop's matrix
            else:
                f = H.levels[l - 1]
                ref, bound = mgc.galerkin(below, f.w if f.w is not None else np.ones(below.shape[0]), f.agg, lv.A.shape[0])
                assert A.nnz == ref.nnz == lv.A.nnz == info["nnz"][l], (name, which, l, A.nnz, ref.nnz, lv.A.nnz, info["nnz"][l])
                worst = max(worst, _worst_ratio(A, ref, bound))
                whole = max(whole, _worst_ratio(A, lv.A, lv.fine0))
                assert np.all(A.diagonal() > 0.0)
            below = A
        print(name, "which", which, f"largest entry difference / sum of |fine terms|: {worst:.2e}; against the restatement's own "
                                    f"levels / sum of |level-0 terms|: {whole:.2e}")
        assert worst <= 1e-12
        assert whole <= 1e-12
    assert s.mg_step_info() == infos                                                     # (the diagnostics rebuilt nothing)


# ------------------------------------------------------------------------------------ 2. one application
@pytest.mark.parametrize("name", ["dirichlet32", "robin33", "robin12c"])
def test_one_application_within_the_rounding_of_the_restatement(pj, name):
    from penguin.jl_amd import _lib as L

    c = _two_hierarchies(pj, name)
    rng = np.random.default_rng(20240607)
    for which in (0, 1):
        ref = c["ref"][which]
        n = len(ref["idx"])
        unit = np.zeros(n)
        unit[np.flatnonzero(ref["idx"] >= c["M"])[0]] = 1.0                              # an interface unknown: a row of a cut cell
        v64, vld = mgc.VCycle(ref["H"], np.float64), mgc.VCycle(ref["H"], np.longdouble)
        for what, r in (("random", rng.standard_normal(n)), ("unit at a cut cell", unit), ("b", ref["bhat"].copy())):
            z = L.debug_mg_step_apply(c["s"]._h, which, r)
            assert np.array_equal(z, L.debug_mg_step_apply(c["s"]._h, which, r)), "an application is not bitwise reproducible"
            zld = vld(r)
            delta = float(np.max(np.abs(v64(r).astype(np.longdouble) - zld)))
            err = float(np.max(np.abs(z.astype(np.longdouble) - zld)))
            bar = max(10.0 * delta, 1e-13 * float(np.max(np.abs(zld))))
            print(f"{name} which {which} {what}: |z - z_ld| {err:.2e}, delta {delta:.2e}, bar {bar:.2e}")
            assert err <= bar, (name, which, what, err, bar)


# ------------------------------------------------------------------------------------ 3. states
@pytest.mark.parametrize("scheme0,scheme", SCHEMES)
@pytest.mark.parametrize("name", ["dirichlet32", "robin33", "neumann48x40", "dirichlet12c", "robin12c"])
def test_six_steps_equal_the_direct_solves(pj, name, scheme0, scheme):
    ref = _oracle_states(pj, name, scheme0, scheme, 64)
    c = _pair(pj, name, scheme0, oracle=False)
    s = _solve(pj, c, scheme, 6, precond="mg-step", log=True)
    assert s.unconverged == 0 and len(s.states) == len(ref) == 7
    errs = [rel_l2(a, b) for a, b in zip(s.states, ref)]
    print(name, scheme0, scheme, "iterations per solve", [h["iters"] for h in s.ch], "rel L2 per state", [f"{e:.1e}" for e in errs])
    assert max(errs) <= TOL_T
    infos = s.mg_step_info()
    assert infos[0]["levels"] >= 2 and (infos[1]["levels"] >= 2) == (scheme0 != scheme)


def test_the_very_large_step(pj):
    """12^3 Dirichlet, BE, Δt = 1024 h²."""
    name, ratio = "dirichlet12c", 1024
    ref = _oracle_states(pj, name, "BE", "BE", ratio)
    errs = {}
    for precond in (0, "mg-step"):
        c = _pair(pj, name, "BE", ratio, oracle=False)
        s = _solve(pj, c, "BE", 6, precond=precond)
        assert s.unconverged == 0
        errs[precond] = max(rel_l2(a, b) for a, b in zip(s.states, ref))
    bar = max(TOL_T, 10.0 * errs[0])
    print(f"dt = 1024 h^2: default options {errs[0]:.2e}, mg-step {errs['mg-step']:.2e}, bar {bar:.2e}")
    assert errs["mg-step"] <= bar


# ------------------------------------------------------------------------------------ 4. it is a preconditioner
def test_first_solve_follows_the_restatement_and_takes_a_third_of_the_plain_products(pj):
    c = _two_hierarchies(pj, "dirichlet32")
    ref = c["ref"][0]
    _, napp, _ = mgc.bicgstab_right(ref["Ahat"], ref["bhat"], mgc.VCycle(ref["H"]), reltol=1e-12)
    counts = {}
    for precond in ("mg-step", -1):
        s = _solve(pj, _pair(pj, "dirichlet32", "BE", oracle=False), "BE", 0, precond=precond, log=True)
        assert s.ch[0]["isconverged"] and len(s.ch) == 1
        counts[precond] = 2 * s.ch[0]["iters"]
    print(f"dirichlet32 BE, first solve: GPU <= {counts['mg-step']} applications, restatement {napp}, plain loop {counts[-1]} products")
    assert counts["mg-step"] <= napp + 4
    assert 3 * counts["mg-step"] <= counts[-1]


@pytest.mark.parametrize("name,scheme0,scheme", [("dirichlet32", "BE", "BE"), ("dirichlet32", "BE", "CN"), ("robin33", "CN", "CN")])
def test_a_warm_step_takes_no_more_than_the_zero_start_solve(pj, name, scheme0, scheme):
    """The same six steps from the previous state and from zero (warm_start=False): the same matrix, the same right-hand side to
    the tolerance of the solves."""
    iters = {}
    for warm in (True, False):
        s = _solve(pj, _pair(pj, name, scheme0, oracle=False), scheme, 6, precond="mg-step", log=True, warm_start=warm)
        assert s.unconverged == 0
        iters[warm] = [h["iters"] for h in s.ch]
    print(name, scheme0, scheme, "warm", iters[True], "from zero", iters[False])
    assert iters[True][0] == iters[False][0]                                             # (the first solve starts from zero either way)
    assert all(w <= z for w, z in zip(iters[True][1:], iters[False][1:]))


# ------------------------------------------------------------------------------------ 5. through the loop
def _loop_case(pj, precond):
    f = pj.TimeSeparable([(1.0, lambda t: 1.0), (lambda x, *_: x, lambda t: math.sin(40.0 * t))])
    g = pj.TimeSeparable([(lambda x, *_: np.cos(x), lambda t: 1.0 + 0.1 * t)])
    c = _pair(pj, "dirichlet32", "BE", f=f, g=g, oracle=False)
    s = c["s"]
    _, _, idx = s.system(0)
    cell = int(idx[idx < c["M"]][len(idx) // 4])
    mons = [pj.VolumeIntegral(c["ph"].capacity), pj.Probe(c["ph"].capacity.mesh, cell)]
    _solve(pj, c, "CN", 6, precond=precond, monitors=mons, save_every=2, save_states=False, time_independent=False)
    return s


def test_run_with_separable_data_monitors_and_a_thinned_history(pj):
    a, b = _loop_case(pj, "mg-step"), _loop_case(pj, 0)
    for s in (a, b):
        assert s.time_data == "device" and s.last_run is not None and s.last_run.steps == 6 and s.unconverged == 0
        assert s.state_steps == [0, 2, 4, 6] and len(s.states) == 4 and s.monitor_series.shape == (7, 2)
    assert a.last_run.poly_degree == 0 and a.last_run.poly_xspace == 0
    assert all(i["levels"] >= 2 for i in a.mg_step_info()) and all(i["levels"] == 0 for i in b.mg_step_info())
    errs = [rel_l2(x, y) for x, y in zip(a.states, b.states)]
    scale = np.max(np.abs(b.monitor_series), axis=0)
    dev = np.max(np.abs(a.monitor_series - b.monitor_series), axis=0)
    print("kept states against the default-option run:", errs, "series:", dev / scale,
          f"products mg-step {a.last_run.products}, default {b.last_run.products}")
    assert max(errs) <= TOL_T
    assert np.all(dev <= 1e-9 * scale)
    assert np.array_equal(a.monitor_times, b.monitor_times)


def test_darcy_flow_unsteady(pj):
    """DarcyFlowUnsteady past an impermeable disc, left = 10, right = 20: three steps against the direct solves."""
    n = 32
    M = (n + 1) ** 2
    mesh, omesh = pj.Mesh((n, n), (4.0, 4.0)), po.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0, complement=True), mesh)
    ocap = oracle_capacity_from_product(cap, omesh)
    zero = lambda x, y, z=0.0, t=0.0: 0.0
    ph, oph = pj.Phase(cap, pj.DiffusionOps(cap), zero, ONE), po.Phase(ocap, po.make_diffusion_ops(ocap), zero, ONE)
    bcb = pj.BorderConditions({"left": pj.Dirichlet(10.0), "right": pj.Dirichlet(20.0)})
    obcb = po.BorderConditions({"left": po.Dirichlet(10.0), "right": po.Dirichlet(20.0)})
    dt = 64 * (4.0 / n) ** 2
    p0 = np.linspace(10.0, 20.0, 2 * M)
    s = pj.DarcyFlowUnsteady(ph, bcb, pj.Neumann(0.0), dt, p0, "BE")
    pj.solve_DarcyFlowUnsteady_b(s, ph, dt, 3 * dt, bcb, pj.Neumann(0.0), "BE", reltol=1e-12, precond="mg-step", time_independent=True)
    so = po.DiffusionUnsteadyMono(oph, obcb, po.Neumann(0.0), dt, p0, "BE")
    po.solve_DiffusionUnsteadyMono(so, oph, dt, 3 * dt, obcb, po.Neumann(0.0), "BE", method="\\")
    assert s.unconverged == 0 and len(s.states) == len(so.states) == 4
    errs = [rel_l2(a, b) for a, b in zip(s.states, so.states)]
    print("DarcyFlowUnsteady:", errs)
    assert max(errs) <= TOL_T
    assert s.mg_step_info()[0]["levels"] >= 2


# ------------------------------------------------------------------------------------ 6. reproducibility and isolation
def test_two_identical_runs_are_bitwise_equal(pj):
    runs = [_solve(pj, _pair(pj, "robin33", "BE", oracle=False), "CN", 4, precond="mg-step", log=True) for _ in range(2)]
    assert [h["iters"] for h in runs[0].ch] == [h["iters"] for h in runs[1].ch]
    assert all(np.array_equal(a, b) for a, b in zip(runs[0].states, runs[1].states))


def test_a_default_run_is_bitwise_the_same_before_and_after_an_mg_step_run_on_another_solver(pj):
    before = _solve(pj, _pair(pj, "dirichlet32", "BE", oracle=False), "CN", 4, log=True)
    other = _solve(pj, _pair(pj, "dirichlet32", "BE", oracle=False), "CN", 4, precond="mg-step")
    after = _solve(pj, _pair(pj, "dirichlet32", "BE", oracle=False), "CN", 4, log=True)
    assert other.unconverged == 0
    assert [h["iters"] for h in before.ch] == [h["iters"] for h in after.ch]
    assert all(np.array_equal(a, b) for a, b in zip(before.states, after.states))
    assert all(i["levels"] == 0 for i in after.mg_step_info())


def test_one_solver_default_steps_then_the_option_then_default_again(pj):
    """The option on a solver that has stepped without it, and default options after it: every state stays at the direct solve."""
    ref = _oracle_states(pj, "dirichlet32", "BE", "CN", 64)
    c = _pair(pj, "dirichlet32", "BE", oracle=False)
    s = c["s"]
    _solve(pj, c, "CN", 2)
    import ctypes as C

    from penguin.jl_amd import _lib as L
    from penguin.jl_amd import api

    info = L.pg_step_info()
    for q, precond in enumerate(("mg-step", "mg-step", 0, "mg-step"), start=3):
        opts = api._krylov_opts("bicgstab", {"precond": precond, "reltol": 1e-12})
        L.check(L.lib().pg_solver_step(s._h, C.c_int32(L.PG_SCHEME["CN"]), C.byref(opts), C.byref(info)))
        assert info.converged
        assert rel_l2(s._fetch_state(), ref[q]) <= TOL_T, (q, precond)


# ------------------------------------------------------------------------------------ 7. refusals
def _small(pj):
    n = 24
    mesh = pj.Mesh((n, n), (4.0, 4.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0), mesh)
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS2})
    return n, mesh, cap, bcb


def _small_unsteady(pj):
    n, mesh, cap, bcb = _small(pj)
    M = (n + 1) ** 2
    ph = pj.Phase(cap, pj.DiffusionOps(cap), 0.0, 1.0)
    dt = 0.25 * (4.0 / n) ** 2
    s = pj.DiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(1.0), dt, np.concatenate([np.zeros(M), np.ones(M)]), "BE")
    return s, ph, bcb, dt


def test_refused_on_a_steady_solver(pj):
    n, mesh, cap, bcb = _small(pj)
    s = pj.DiffusionSteadyMono(pj.Phase(cap, pj.DiffusionOps(cap), ONE, ONE), bcb, pj.Dirichlet(0.0))
    with pytest.raises(pj.PenguinHipError, match="PG_PRECOND_MG_STEP.*steady.*PG_PRECOND_MG and PG_PRECOND_MG_CELL"):
        pj.solve_DiffusionSteadyMono_b(s, precond="mg-step")
    pj.solve_DiffusionSteadyMono_b(s, precond=0)
    assert s.ch[-1]["converged"]


def test_refused_on_a_convection_system(pj):
    from tests.test_gpu_parity import _velocity_fields

    n, mesh, cap, bcb = _small(pj)
    M = (n + 1) ** 2
    u, ug = _velocity_fields(cap, 2, M)
    ph = pj.Phase(cap, pj.ConvectionOps(cap, u, ug), ONE, ONE)
    dt = 0.25 * (4.0 / n) ** 2
    u0 = np.concatenate([np.zeros(M), np.ones(M)])
    s = pj.AdvectionDiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(1.0), dt, u0, "BE")
    with pytest.raises(pj.PenguinHipError, match="PG_PRECOND_MG_STEP.*ConvectionOps"):
        pj.solve_AdvectionDiffusionUnsteadyMono_b(s, ph, dt, 2 * dt, bcb, pj.Dirichlet(1.0), "BE", precond="mg-step")
    pj.solve_AdvectionDiffusionUnsteadyMono_b(s, ph, dt, 2 * dt, bcb, pj.Dirichlet(1.0), "BE", precond=0)
    assert s.unconverged == 0


def test_refused_on_a_moving_solver(pj):
    n = 16
    mesh = pj.Mesh((n, n), (4.0, 4.0))
    body = pj.MovingSphere(lambda t: (2.01, 2.01), lambda t: 0.8 + 0.5 * t, complement=True)
    dt = 0.5 * (4.0 / n) ** 2
    cap = pj.Capacity(body, pj.SpaceTimeMesh(mesh, [0.0, dt]))
    ph = pj.Phase(cap, pj.DiffusionOps(cap), lambda x, y=0.0, z=0.0, t=0.0: 0.0, ONE)
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS2})
    u0 = np.concatenate([np.zeros((n + 1) ** 2), np.ones((n + 1) ** 2)])
    args = (ph, body, dt, 0.0, 2 * dt, bcb, pj.Dirichlet(1.0), mesh, "BE")
    s = pj.MovingDiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(1.0), dt, u0, mesh, "BE")
    with pytest.raises(pj.PenguinHipError, match="PG_PRECOND_MG_STEP.*moving-body"):
        pj.solve_MovingDiffusionUnsteadyMono_b(s, *args, method="bicgstab", precond="mg-step")
    s = pj.MovingDiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(1.0), dt, u0, mesh, "BE")
    pj.solve_MovingDiffusionUnsteadyMono_b(s, *args, method="bicgstab", precond=0)
    assert s.unconverged == 0


def test_refused_on_a_stream_vorticity_solver(pj):
    from tests.test_gpu_streamvorticity import RELTOL, _build as build_sv

    s, _, _ = build_sv(pj, "B")
    with pytest.raises(pj.PenguinHipError, match="PG_PRECOND_MG_STEP.*StreamVorticity"):
        pj.step_StreamVorticity_b(s, "BE", reltol=RELTOL, precond="mg-step")
    pj.step_StreamVorticity_b(s, "BE", reltol=RELTOL, precond=0)
    ip, iw = s.last_step
    assert ip.converged and iw.converged


@pytest.mark.parametrize("method,kw,word", [("cg", {}, "CG"), ("gmres", {}, "GMRES"), ("bicgstabl", {"l": 2}, r"BiCGStab\(l\)")])
def test_refused_with_another_krylov_method(pj, method, kw, word):
    s, ph, bcb, dt = _small_unsteady(pj)
    with pytest.raises(pj.PenguinHipError, match="PG_PRECOND_MG_STEP.*" + word):
        pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 2 * dt, bcb, pj.Dirichlet(1.0), "BE", method=method, precond="mg-step", **kw)
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 2 * dt, bcb, pj.Dirichlet(1.0), "BE", precond=0)
    assert s.unconverged == 0


def test_refused_on_a_virtual_rank_run(pj):
    """2 virtual ranks on a 16^2 disc problem: refused by the entry point with the one-rank condition, before a rank starts; the
    same configuration then runs with precond = 0."""
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
        L.check(lib.pg_debug_set_virtual_rank_precond(L.PG_PRECOND_MG_STEP))
        with pytest.raises(pj.PenguinHipError, match="PG_PRECOND_MG_STEP.*one rank"):
            L.check(run())
    finally:
        L.check(lib.pg_debug_set_virtual_rank_precond(0))
    L.check(run())
    assert outs[0].sum() > 0 and np.isfinite(x).all() and x.any()


def test_refused_on_a_steady_diphasic_solver(pj):
    n, mesh, c1, bcb = _small(pj)
    c2 = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0, complement=True), mesh)
    ic = pj.InterfaceConditions(pj.ScalarJump(1.0, 1.0, 0.0), pj.FluxJump(1.0, 1.0, 0.0))
    s = pj.DiffusionSteadyDiph(pj.Phase(c1, pj.DiffusionOps(c1), ONE, ONE), pj.Phase(c2, pj.DiffusionOps(c2), ONE, ONE), bcb, ic)
    with pytest.raises(pj.PenguinHipError, match="PG_PRECOND_MG_STEP.*steady"):
        pj.solve_DiffusionSteadyDiph_b(s, precond="mg-step")
    pj.solve_DiffusionSteadyDiph_b(s, precond=0)
    assert s.ch[-1]["converged"]


def test_a_hierarchy_that_cannot_be_built_is_a_refusal(pj):
    """Robin outside the disc, 32^2, BE, Δt = h²: the first Galerkin product has a diagonal entry that is not positive (the
    restatement refuses the same system, tests/test_mg_step_reference.py).  The solve is refused with the library's words, no
    hierarchy is kept, the refusal repeats, and the same solver then runs under default options."""
    c = _pair(pj, "robin32", "BE", ratio=1, oracle=False)
    for _ in range(2):
        with pytest.raises(pj.PenguinHipError, match="coarse diagonal entry is not positive"):
            _solve(pj, c, "BE", 2, precond="mg-step")
        assert all(i["levels"] == 0 for i in c["s"].mg_step_info())
    s = _solve(pj, c, "BE", 2, precond=0)
    assert s.unconverged == 0 and len(s.states) == 3


def test_the_steady_values_keep_refusing_a_time_step(pj):
    s, ph, bcb, dt = _small_unsteady(pj)
    for name, word in (("mg", "PG_PRECOND_MG\\)"), ("mg-cell", "PG_PRECOND_MG_CELL")):
        with pytest.raises(pj.PenguinHipError, match=word + ".*unsteady"):
            pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 2 * dt, bcb, pj.Dirichlet(1.0), "BE", precond=name)


# ------------------------------------------------------------------------------------ 8. diphasic systems
# box 8 x 8, the disc r = 2 at the centre and its complement (tests/specest_systems.py::diph), 32^2, Δt = 16 h², BE -> CN.
# States at the bar of the suite's diphasic parity tests, 1e-9.
TOL_DIPH = 1e-9
DIPH = {"he1": (1.0, 1.0), "he05-d2": (0.5, 2.0)}
_DIPH = {}


def _diph(pj, kind, oracle=False):
    He, D2 = DIPH[kind]
    n, Lx, ctr, r = 32, 8.0, (4.0, 4.0), 2.0
    M = (n + 1) ** 2
    mesh = pj.Mesh((n, n), (Lx, Lx), (0.0, 0.0))
    cap1, cap2 = pj.Capacity(pj.Sphere(ctr, r), mesh), pj.Capacity(pj.Sphere(ctr, r, complement=True), mesh)
    zero = lambda x, y, z=0.0, t=0.0: 0.0
    d2 = lambda x, y, z=0.0: D2
    p1, p2 = pj.Phase(cap1, pj.DiffusionOps(cap1), zero, ONE), pj.Phase(cap2, pj.DiffusionOps(cap2), zero, d2)
    ic = pj.InterfaceConditions(pj.ScalarJump(1.0, He, 0.0), pj.FluxJump(1.0, 1.0, 0.0))
    bcb = pj.BorderConditions({})
    u0 = np.concatenate([np.ones(M), np.ones(M), np.zeros(M), np.zeros(M)])
    dt = 16 * (Lx / n) ** 2
    c = {"s": pj.DiffusionUnsteadyDiph(p1, p2, bcb, ic, dt, u0, "BE"), "args": (p1, p2, dt), "tail": (bcb, ic), "dt": dt,
         "ext": (n + 1, n + 1), "M": M, "keep": (mesh, cap1, cap2)}
    if oracle:
        omesh = po.Mesh((n, n), (Lx, Lx), (0.0, 0.0))
        oc1, oc2 = oracle_capacity_from_product(cap1, omesh), oracle_capacity_from_product(cap2, omesh)
        q1, q2 = po.Phase(oc1, po.make_diffusion_ops(oc1), zero, ONE), po.Phase(oc2, po.make_diffusion_ops(oc2), zero, d2)
        oic = po.InterfaceConditions(po.ScalarJump(1.0, He, 0.0), po.FluxJump(1.0, 1.0, 0.0))
        so = po.DiffusionUnsteadyDiph(q1, q2, po.BorderConditions({}), oic, dt, u0, "BE")
        po.solve_DiffusionUnsteadyDiph(so, q1, q2, dt, 6 * dt, po.BorderConditions({}), oic, "CN", method="\\")
        c["oracle"] = [np.array(x) for x in so.states]
    return c


def _solve_diph(pj, c, steps, **kw):
    p1, p2, dt = c["args"]
    pj.solve_DiffusionUnsteadyDiph_b(c["s"], p1, p2, dt, steps * dt, *c["tail"], "CN", reltol=1e-12, time_independent=True, **kw)
    return c["s"]


def _diph_two_hierarchies(pj, kind):
    if kind not in _DIPH:
        c = _diph(pj, kind)
        assert _solve_diph(pj, c, 2, precond="mg-step").unconverged == 0
        _restate(c)
        _DIPH[kind] = c
    return _DIPH[kind]


@pytest.mark.parametrize("kind", list(DIPH))
def test_diphasic_hierarchies_equal_the_restatement(pj, kind):
    c = _diph_two_hierarchies(pj, kind)
    idx = c["ref"][0]["idx"]
    assert len(np.unique(idx // c["M"])) == 4                                            # (four kinds of unknowns among the children)
    _check_both_hierarchies(c, "diphasic " + kind)


@pytest.mark.parametrize("kind", list(DIPH))
def test_diphasic_states_equal_the_direct_solves(pj, kind):
    c = _diph(pj, kind, oracle=True)
    s = _solve_diph(pj, c, 6, precond="mg-step")
    assert s.unconverged == 0 and len(s.states) == len(c["oracle"]) == 7
    errs = [rel_l2(a, b) for a, b in zip(s.states, c["oracle"])]
    print("diphasic", kind, "rel L2 per state", [f"{e:.1e}" for e in errs])
    assert max(errs) <= TOL_DIPH
    assert all(i["levels"] >= 2 for i in s.mg_step_info())


@pytest.mark.parametrize("kind", list(DIPH))
def test_diphasic_first_solve_follows_the_restatement(pj, kind):
    ref = _diph_two_hierarchies(pj, kind)["ref"][0]
    _, napp, _ = mgc.bicgstab_right(ref["Ahat"], ref["bhat"], mgc.VCycle(ref["H"]), reltol=1e-12)
    import ctypes as C

    from penguin.jl_amd import _lib as L
    from penguin.jl_amd import api

    counts = {}
    for precond in ("mg-step", -1):
        c = _diph(pj, kind)
        info = L.pg_step_info()
        opts = api._krylov_opts("bicgstab", {"precond": precond, "reltol": 1e-12})
        L.check(L.lib().pg_solver_initial_solve(c["s"]._h, C.byref(opts), C.byref(info)))      # (the diphasic driver keeps no log)
        assert info.converged
        counts[precond] = 2 * info.iters
    print(f"diphasic {kind}, first solve: GPU <= {counts['mg-step']} applications, restatement {napp}, plain loop {counts[-1]} products")
    assert counts["mg-step"] <= napp + 4
    assert 3 * counts["mg-step"] <= counts[-1]
