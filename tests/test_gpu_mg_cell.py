"""The cell-aggregated multigrid preconditioner (precond="mg-cell", PG_PRECOND_MG_CELL, csrc/pg_multigrid.hip) against its numpy
restatement (tests/mgc_reference.py) and against the oracle's direct solve, on Robin, Neumann and Dirichlet interfaces.

The product's Â (cell blocks folded in), ds and idx come from s.system(2) / row_scaling, as in tests/test_gpu_multigrid.py; the
restatement builds its hierarchy from them.

Shapes are the smallest at which the kernels can go wrong: odd and even padded extents (32 / 33, 40 / 41), a non-square and a
non-cubic grid (48 x 40, 21 x 20 x 19), N = 1, 2, 3, a system of ONE level (12^2: the dense inverse alone), systems whose level 0
-- with its 16-wide child table -- runs INSIDE the fused one-workgroup tail (32^2 ... 48 x 40) and one, 96^2, with two levels
above the tail and two inside it (asserted).

Bars
  hierarchy     aggregate maps exactly; level matrices within 1e-12 x (sum of the absolute values of the fine terms an entry
                was added up from): an entry is now a sum of at most 2^N * 2 * 2 (2N + 1) products, 1e-12 leaves more than a decade.
                Each level of the library is compared with Pᵀ A P formed in numpy from the library's OWN level above, so that
                both sides add up bitwise the same terms: B⁻¹ leaves 1e-15 where it removes an ω-γ coupling, a coarse entry
                made of such residues is only the rounding of its own sum (measured at 33^2, level 2: 3e-19 on the GPU against
                -3e-18 in numpy, both correct), and two independently rounded copies of it bound nothing on the level below.
                In addition the library's levels are compared with the restatement's own, within 1e-12 x the same sum carried
                down from level 0 (a check of the hierarchy as a whole).
  level 0       the product's Â against the restated cell blocks (mgc.cell_blocks) of the product's own raw matrix: 64 eps κ per
                entry of |B⁻¹| |S A S|, κ the condition number of the cell's block (reasoning in the test).
  application   max(10 δ, 1e-13 ||z||inf) with δ = the difference between the restatement in float64 and in long double on the
                same input; two applications on the same input are bitwise equal.
  solves        the suite's TOL_T = 1e-10 relative L2 against the oracle's direct solve fed with the product's capacities.  A case
                is admitted only where the restatement ALONE (numpy, on the oracle's own system of that case, reltol 1e-13)
                ends within 1e-11 of the direct solve; the value measured when this test was written stands beside each case.
                All six case families of the feature are admitted, none was dropped.
  iterations    applications of Â on the GPU <= the restatement's on the same Â + 4 (the stopping tests differ by the half-step
                check only); at 128^2 at most a quarter of the plain loop's products.  The GPU reports iterations, not
                applications: 2 x iterations, which a stop at a half step undercuts by one, is used as its count -- the bar is
                never looser than stated.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import penguin_oracle as po
from tests import mgc_reference as mgc
from tests.common import oracle_capacity_from_product, rel_l2

pytestmark = pytest.mark.gpu

TOL_T = 1e-10
KEYS2 = ("left", "right", "bottom", "top")
ONE = lambda x, y=0.0, z=0.0: 1.0
ZERO = lambda x, y=0.0, z=0.0: 0.0


# ------------------------------------------------------------------------------------ the systems
def _bc(pj, kind):
    return {"robin": (pj.Robin(1.0, 1.0, 0.5), po.Robin(1.0, 1.0, 0.5)), "neumann": (pj.Neumann(0.0), po.Neumann(0.0)),
            "dirichlet": (pj.Dirichlet(0.0), po.Dirichlet(0.0))}[kind]


def _spec(name):
    """-> (cells, lengths, body factory, border keys, interface condition)"""
    out = lambda pj: pj.Sphere((2.01, 2.01), 0.5, complement=True)
    disc = lambda pj: pj.Sphere((2.01, 2.01), 1.0)
    ball = lambda pj: pj.Sphere((2.01, 2.01, 2.01), 1.0)
    half = lambda pj: pj.HalfSpace(0, 0.613)
    table = {
        "robin-out32": ((32, 32), (4.0, 4.0), out, KEYS2, "robin"),
        "robin-out33": ((33, 33), (4.0, 4.0), out, KEYS2, "robin"),
        "robin-out48x40": ((48, 40), (4.0, 4.0), out, KEYS2, "robin"),
        "robin-out96": ((96, 96), (4.0, 4.0), out, KEYS2, "robin"),
        "robin-out128": ((128, 128), (4.0, 4.0), out, KEYS2, "robin"),
        "neumann-out32": ((32, 32), (4.0, 4.0), out, KEYS2, "neumann"),
        "dirichlet-out33": ((33, 33), (4.0, 4.0), out, KEYS2, "dirichlet"),
        "robin-in12": ((12, 12), (4.0, 4.0), disc, (), "robin"),
        "robin-in40": ((40, 40), (4.0, 4.0), disc, (), "robin"),
        "robin-sph20": ((20, 20, 20), (4.0, 4.0, 4.0), ball, (), "robin"),
        "robin-sph21x20x19": ((21, 20, 19), (4.0, 4.0, 4.0), ball, (), "robin"),
        "robin-half40": ((40,), (1.0,), half, ("bottom",), "robin"),
        "robin-half41": ((41,), (1.0,), half, ("bottom",), "robin"),
    }
    return table[name]


PARITY = ["robin-out32", "robin-out33", "robin-out48x40", "robin-out96", "neumann-out32", "robin-sph21x20x19", "robin-half40",
          "robin-half41", "robin-in12", "dirichlet-out33"]
_BUILT = {}


def _build(pj, name, cache=True, ctor="DiffusionSteadyMono", f=ONE, borders=None, oborders=None, bc=None):
    """-> dict(s: product solver, so: oracle solver (solved directly), ext, make: another product solver of the same system)"""
    if cache and name in _BUILT:
        return _BUILT[name]
    n, Ls, body, keys, kind = _spec(name)
    N = len(n)
    mesh, omesh = pj.Mesh(n, Ls), po.Mesh(n, Ls, (0.0,) * N)
    cap = pj.Capacity(body(pj), mesh)
    ocap = oracle_capacity_from_product(cap, omesh)
    ph, oph = pj.Phase(cap, pj.DiffusionOps(cap), f, ONE), po.Phase(ocap, po.make_diffusion_ops(ocap), f, ONE)
    bcb = pj.BorderConditions(borders if borders is not None else {k: pj.Dirichlet(0.0) for k in keys})
    obcb = po.BorderConditions(oborders if oborders is not None else {k: po.Dirichlet(0.0) for k in keys})
    bi, obi = _bc(pj, bc or kind)
    make = lambda: getattr(pj, ctor)(ph, bcb, bi)
    so = getattr(po, ctor)(oph, obcb, obi)
    po.solve_system(so, method="\\")
    sy = {"s": make(), "so": so, "ext": tuple(k + 1 for k in n), "make": make, "keep": (cap, ph, bcb)}
    if cache:
        _BUILT[name] = sy
    return sy


def _reference_hierarchy(sy):
    """The restatement's hierarchy of the PRODUCT's Â, computed once per system and left unchanged."""
    if "H" not in sy:
        A, bhat, idx = sy["s"].system(2)
        ds = sy["s"].row_scaling(0)
        sy["Ahat"], sy["bhat"], sy["idx"], sy["ds"] = sp.csr_matrix(A[:, : len(idx)]), bhat, idx, ds
        sy["H"] = mgc.build_hierarchy_cells(sy["Ahat"], ds, idx, sy["ext"])
    return sy["H"]


# ------------------------------------------------------------------------------------ 1. hierarchy parity
@pytest.mark.parametrize("name", PARITY)
def test_hierarchy_equals_the_restatement(pj, name):
    from penguin.jl_amd import _lib as L

    CELL = L.PG_PRECOND_MG_CELL
    sy = _build(pj, name)
    H = _reference_hierarchy(sy)
    h = sy["s"]._h
    level0 = L.debug_mg_level_csr(h, 0, CELL)                                # (builds the hierarchy)
    info = sy["s"].mg_info("mg-cell")
    print(name, "rows", info["rows"], "nnz", info["nnz"], "tail from", info["tail_level"], f"set-up {info['setup_ms']:.2f} ms")
    assert info["levels"] == len(H.levels)
    assert info["rows"] == H.rows
    assert info["rows"][-1] <= mgc.COARSEST_ROWS and all(r > mgc.COARSEST_ROWS for r in info["rows"][:-1])
    assert 0 <= info["tail_level"] <= info["levels"] - 1
    print(name, f"largest |diagonal of level 0 - 1|: {np.max(np.abs(H.levels[0].A.diagonal() - 1.0)):.2e}")   # (taken as 1 exactly)
    if name == "robin-in12":
        assert info["levels"] == 1                                           # the dense inverse alone
    if name == "robin-out96":
        assert info["tail_level"] >= 1, info                                 # at least one level above the fused tail ...
        assert info["tail_level"] <= info["levels"] - 2, info                # ... and one inside it besides the exact last level
    worst = whole = 0.0
    below = None                                                             # the library's own matrix of the level above
    for l, lv in enumerate(H.levels):
        if l + 1 < len(H.levels):
            agg = L.debug_mg_aggregates(h, l, CELL)
            assert np.array_equal(agg, lv.agg), (name, l)
        rp, col, val = level0 if l == 0 else L.debug_mg_level_csr(h, l, CELL)
        A = sp.csr_matrix((val, col, rp), shape=lv.A.shape)
        if l > 0:
            # the bar: the library's level l against Pᵀ A P of the library's OWN level l - 1 -- the inputs of the product are
            # bitwise the same on both sides -- within 1e-12 x the sum of |terms| of that product
            f = H.levels[l - 1]
            ref, bound = mgc.galerkin(below, f.w if f.w is not None else np.ones(below.shape[0]), f.agg, lv.A.shape[0])
            assert A.nnz == ref.nnz == lv.A.nnz == info["nnz"][l], (name, l, A.nnz, ref.nnz, lv.A.nnz, info["nnz"][l])
            worst = max(worst, _worst_ratio(A, ref, bound))
            # and the whole hierarchy: against the restatement's own level, within 1e-12 x the same sum carried down from level 0
            whole = max(whole, _worst_ratio(A, lv.A, lv.fine0))
            assert np.all(A.diagonal() > 0.0)
        below = A
    print(name, f"largest entry difference / sum of |fine terms|: {worst:.2e}; against the restatement's own levels / "
                f"sum of |level-0 terms|: {whole:.2e}")
    assert worst <= 1e-12
    assert whole <= 1e-12


def _worst_ratio(A, ref, bound):
    diff = abs(A - ref).tocoo()
    b = np.asarray(bound.tocsr()[diff.row, diff.col]).ravel()
    ratio = diff.data / np.maximum(b, 1e-300)
    return float(ratio.max()) if ratio.size else 0.0


def test_level_zero_is_the_restated_cell_block_product_of_the_raw_system(pj):
    """The product's Â = B⁻¹ S A S against mgc.cell_blocks applied to the product's own raw reduced matrix (which = 0).
    Bar, per entry: 64 eps κ (|B⁻¹| |S A S|)_ij, κ the condition number (max norm) of the cell's block -- a 2 x 2 inverse by
    Gauss-Jordan in float64 is good to a few eps κ, the entry is a sum of two products with it, and S carries one rounding of a
    square root and a division per factor; un-blocked rows have κ = 1.  The row scaling agrees to 4 eps."""
    from tests.test_mgc_reference import overwritten_border_cells

    eps = np.finfo(np.float64).eps
    for name in ("robin-out33", "neumann-out32", "dirichlet-out33", "robin-sph21x20x19"):
        sy = _build(pj, name)
        _reference_hierarchy(sy)
        s = sy["s"]
        n, Ls, _, keys, _ = _spec(name)
        omesh = po.Mesh(n, Ls, (0.0,) * len(n))
        A0, _, idx0 = s.system(0)
        assert np.array_equal(idx0, sy["idx"])
        M = int(np.prod(sy["ext"]))
        Ar = sp.csr_matrix(A0[:, : len(idx0)])
        Ahat, ds, Binv = mgc.cell_blocks(Ar, idx0, M, overwritten_border_cells(omesh, {k: po.Dirichlet(0.0) for k in keys}))
        assert np.allclose(ds, sy["ds"], rtol=4 * eps, atol=0.0), name
        S = sp.diags(ds)
        bound = sp.csr_matrix(abs(Binv) @ abs(sp.csr_matrix(S @ Ar @ S)))
        # κ of every row's block: |B|_max |B⁻¹|_max over the rows of the cell (B = the inverse of B⁻¹'s block, from S A S)
        As = sp.csr_matrix(S @ Ar @ S)
        Bfw = sp.csr_matrix(abs(As).multiply(abs(Binv) > 0))
        cell = idx0 % M
        order = np.argsort(cell, kind="stable")
        start = np.flatnonzero(np.r_[True, np.diff(cell[order]) != 0])
        per_cell = lambda v: np.repeat(np.maximum.reduceat(v[order], start), np.diff(np.r_[start, len(order)]))
        kappa = np.empty(len(idx0))
        kappa[order] = per_cell(np.asarray(Bfw.sum(axis=1)).ravel()) * per_cell(np.asarray(abs(Binv).sum(axis=1)).ravel())
        diff = abs(sy["Ahat"] - Ahat).tocoo()
        b = np.asarray(bound[diff.row, diff.col]).ravel() * np.maximum(kappa[diff.row], 1.0)
        ratio = diff.data / np.maximum(64 * eps * b, 1e-300)
        print(f"{name}: largest |Â - restated Â| over its bar: {ratio.max() if ratio.size else 0.0:.2e}; largest κ {kappa.max():.1e}")
        assert ratio.size == 0 or ratio.max() <= 1.0, name


def test_interface_and_bulk_unknowns_of_a_cell_share_their_coarse_unknown(pj):
    from penguin.jl_amd import _lib as L

    sy = _build(pj, "robin-out33")
    _reference_hierarchy(sy)
    agg = L.debug_mg_aggregates(sy["s"]._h, 0, L.PG_PRECOND_MG_CELL)
    M = int(np.prod(sy["ext"]))
    idx = sy["idx"]
    bulk = {int(c): a for c, a in zip(idx[idx < M], agg[idx < M])}
    cut = [(int(c - M), a) for c, a in zip(idx[idx >= M], agg[idx >= M]) if int(c - M) in bulk]
    assert len(cut) > 8 and all(bulk[c] == a for c, a in cut)


# ------------------------------------------------------------------------------------ 2. one application
@pytest.mark.parametrize("name", ["robin-out96", "robin-out33", "robin-out48x40", "robin-sph21x20x19", "robin-half41"])
def test_one_application_within_the_rounding_of_the_restatement(pj, name):
    from penguin.jl_amd import _lib as L

    sy = _build(pj, name)
    H = _reference_hierarchy(sy)
    n = len(sy["idx"])
    M = int(np.prod(sy["ext"]))
    rng = np.random.default_rng(20240607)
    unit = np.zeros(n)
    unit[np.flatnonzero(sy["idx"] >= M)[0]] = 1.0            # an interface unknown: a row of a cut cell
    v64, vld = mgc.VCycle(H, np.float64), mgc.VCycle(H, np.longdouble)
    for what, r in (("random", rng.standard_normal(n)), ("unit at a cut cell", unit), ("b", sy["bhat"].copy())):
        z = L.debug_mg_apply(sy["s"]._h, r, L.PG_PRECOND_MG_CELL)
        z2 = L.debug_mg_apply(sy["s"]._h, r, L.PG_PRECOND_MG_CELL)
        assert np.array_equal(z, z2), "an application is not bitwise reproducible"
        zld = vld(r)
        delta = float(np.max(np.abs(v64(r).astype(np.longdouble) - zld)))
        err = float(np.max(np.abs(z.astype(np.longdouble) - zld)))
        bar = max(10.0 * delta, 1e-13 * float(np.max(np.abs(zld))))
        print(f"{name} {what}: |z - z_ld| {err:.2e}, delta {delta:.2e}, bar {bar:.2e}, |z| {float(np.max(np.abs(zld))):.2e}")
        assert err <= bar, (name, what, err, bar)


# ------------------------------------------------------------------------------------ 3. solve parity
# name -> what the restatement alone reached on the oracle's system of the case (numpy, reltol 1e-13; admitted where <= 1e-11)
SOLVES = {
    "robin-out32": 5.7e-15,
    "robin-out48x40": 3.2e-14,
    "robin-in40": 7.6e-14,
    "neumann-out32": 1.9e-14,
    "robin-sph20": 1.3e-12,
}
DARCY_RESTATEMENT = 5.2e-13     # DarcyFlow, Neumann body, 32^2, left = 10, right = 20, no source


def _solve_and_compare(pj, sy, solve):
    s = sy["s"]
    getattr(pj, solve)(s, precond="mg-cell", reltol=1e-13)
    assert s.ch[-1]["converged"]
    assert s.mg_info("mg-cell")["levels"] >= 1 and s.mg_info()["levels"] == 0      # its own hierarchy, and only that one
    return rel_l2(s.x, sy["so"].x), s.ch[-1]["iters"]


@pytest.mark.parametrize("name", list(SOLVES))
def test_solution_equals_the_direct_solve(pj, name):
    sy = _build(pj, name, cache=False)
    err, it = _solve_and_compare(pj, sy, "solve_DiffusionSteadyMono_b")
    print(f"{name}: {it} iterations, rel L2 {err:.2e} (the restatement alone: {SOLVES[name]:.1e})")
    assert err <= TOL_T


def test_darcy_flow_past_an_impermeable_disc_equals_the_direct_solve(pj):
    sy = _build(pj, "neumann-out32", cache=False, ctor="DarcyFlow", f=ZERO,
                borders={"left": pj.Dirichlet(10.0), "right": pj.Dirichlet(20.0)},
                oborders={"left": po.Dirichlet(10.0), "right": po.Dirichlet(20.0)})
    err, it = _solve_and_compare(pj, sy, "solve_DarcyFlow_b")
    print(f"DarcyFlow, Neumann body, 32^2: {it} iterations, rel L2 {err:.2e} (the restatement alone: {DARCY_RESTATEMENT:.1e})")
    assert err <= TOL_T


# ------------------------------------------------------------------------------------ 4. it is a preconditioner
def test_applications_follow_the_restatement_and_fall_to_a_quarter_of_the_plain_loop(pj):
    counts = {}
    for name in ("robin-out32", "robin-out128"):
        sy = _build(pj, name)
        H = _reference_hierarchy(sy)
        _, napp, _ = mgc.bicgstab_right(sy["Ahat"], sy["bhat"], mgc.VCycle(H), reltol=1e-12)
        s = sy["make"]()
        pj.solve_DiffusionSteadyMono_b(s, precond="mg-cell", reltol=1e-12, warm_start=False)
        assert s.ch[-1]["converged"]
        counts[name] = (2 * s.ch[-1]["iters"], napp)
        print(f"{name}: GPU {s.ch[-1]['iters']} iterations (<= {counts[name][0]} applications), restatement {napp} applications")
    p = _build(pj, "robin-out128")["make"]()
    pj.solve_DiffusionSteadyMono_b(p, precond=-1, reltol=1e-12, warm_start=False)
    assert p.ch[-1]["converged"]
    plain = 2 * p.ch[-1]["iters"]
    print(f"robin-out128: plain loop {plain} products")
    for name, (gpu, ref) in counts.items():
        assert gpu <= ref + 4, (name, gpu, ref)
    assert 4 * counts["robin-out128"][0] <= plain


# ------------------------------------------------------------------------------------ 5. refusals
def _small(pj):
    n = 24
    mesh = pj.Mesh((n, n), (4.0, 4.0))
    cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0), mesh)
    bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in KEYS2})
    return n, mesh, cap, bcb


def test_refused_on_a_diphasic_system(pj):
    n, mesh, c1, bcb = _small(pj)
    c2 = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0, complement=True), mesh)
    ic = pj.InterfaceConditions(pj.ScalarJump(1.0, 1.0, 0.0), pj.FluxJump(1.0, 1.0, 0.0))
    s = pj.DiffusionSteadyDiph(pj.Phase(c1, pj.DiffusionOps(c1), ONE, ONE), pj.Phase(c2, pj.DiffusionOps(c2), ONE, ONE), bcb, ic)
    with pytest.raises(pj.PenguinHipError, match="PG_PRECOND_MG_CELL.*diphasic"):
        pj.solve_DiffusionSteadyDiph_b(s, precond="mg-cell")
    pj.solve_DiffusionSteadyDiph_b(s, precond=0)
    assert s.ch[-1]["converged"]


def test_refused_on_an_unsteady_system(pj):
    n, mesh, cap, bcb = _small(pj)
    M = (n + 1) ** 2
    ph = pj.Phase(cap, pj.DiffusionOps(cap), 0.0, 1.0)
    dt = 0.25 * (4.0 / n) ** 2
    s = pj.DiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(1.0), dt, np.concatenate([np.zeros(M), np.ones(M)]), "BE")
    with pytest.raises(pj.PenguinHipError, match="PG_PRECOND_MG_CELL.*unsteady"):
        pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 3 * dt, bcb, pj.Dirichlet(1.0), "BE", precond="mg-cell")
    pj.solve_DiffusionUnsteadyMono_b(s, ph, dt, 3 * dt, bcb, pj.Dirichlet(1.0), "BE", precond=0)
    assert s.unconverged == 0


def test_refused_on_an_advection_diffusion_system(pj):
    from tests.test_gpu_parity import _velocity_fields

    n, mesh, cap, bcb = _small(pj)
    u, ug = _velocity_fields(cap, 2, (n + 1) ** 2)
    s = pj.AdvectionDiffusionSteadyMono(pj.Phase(cap, pj.ConvectionOps(cap, u, ug), ONE, ONE), bcb, pj.Dirichlet(1.0))
    with pytest.raises(pj.PenguinHipError, match="PG_PRECOND_MG_CELL.*ConvectionOps"):
        pj.solve_AdvectionDiffusionSteadyMono_b(s, precond="mg-cell")
    pj.solve_AdvectionDiffusionSteadyMono_b(s, precond=0)
    assert s.ch[-1]["converged"]


@pytest.mark.parametrize("method,word", [("cg", "CG"), ("gmres", "GMRES")])
def test_refused_with_cg_and_gmres(pj, method, word):
    n, mesh, cap, bcb = _small(pj)
    s = pj.DiffusionSteadyMono(pj.Phase(cap, pj.DiffusionOps(cap), ONE, ONE), bcb, pj.Robin(1.0, 1.0, 0.5))
    with pytest.raises(pj.PenguinHipError, match="PG_PRECOND_MG_CELL.*" + word):
        pj.solve_DiffusionSteadyMono_b(s, method=method, precond="mg-cell")
    pj.solve_DiffusionSteadyMono_b(s, precond=0)
    assert s.ch[-1]["converged"]


def test_refused_on_a_stream_vorticity_solver(pj):
    from tests.test_gpu_streamvorticity import RELTOL, _build as build_sv

    s, _, _ = build_sv(pj, "B")
    with pytest.raises(pj.PenguinHipError, match="PG_PRECOND_MG_CELL.*StreamVorticity"):
        pj.step_StreamVorticity_b(s, "BE", reltol=RELTOL, precond="mg-cell")
    with pytest.raises(pj.PenguinHipError, match="PG_PRECOND_MG_CELL.*StreamVorticity"):
        pj.solve_StreamVorticity_b(s, reltol=RELTOL, precond="mg-cell")
    pj.step_StreamVorticity_b(s, "BE", reltol=RELTOL, precond=0)
    ip, iw = s.last_step
    assert ip.converged and iw.converged


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
        L.check(lib.pg_debug_set_virtual_rank_precond(L.PG_PRECOND_MG_CELL))
        with pytest.raises(pj.PenguinHipError, match="PG_PRECOND_MG_CELL.*one rank"):
            L.check(run())
    finally:
        L.check(lib.pg_debug_set_virtual_rank_precond(0))
    L.check(run())
    assert outs[0].sum() > 0 and np.isfinite(x).all() and x.any()


def test_amg_is_still_a_value_error(pj):
    n, mesh, cap, bcb = _small(pj)
    s = pj.DiffusionSteadyMono(pj.Phase(cap, pj.DiffusionOps(cap), ONE, ONE), bcb, pj.Dirichlet(0.0))
    with pytest.raises(ValueError):
        pj.solve_DiffusionSteadyMono_b(s, precond="amg")
    with pytest.raises(ValueError):
        s.mg_info("amg")


# ------------------------------------------------------------------------------------ 6. nothing else moved
def test_a_kind_rule_solve_is_bitwise_the_same_before_and_after_a_cell_rule_solve(pj):
    """One solver, a Dirichlet system both values serve: "mg", "mg-cell", "mg" again.  Each value has its own hierarchy; the second
    "mg" solve finds its hierarchy as the first left it (mg_info unchanged, set-up time included: it was not rebuilt)."""
    s = _build(pj, "dirichlet-out33", cache=False)["s"]
    pj.solve_DiffusionSteadyMono_b(s, precond="mg", reltol=1e-13)
    x1, it1, info1 = s.x.copy(), s.ch[-1]["iters"], s.mg_info()
    assert s.ch[-1]["converged"] and info1["levels"] >= 2 and s.mg_info("mg-cell")["levels"] == 0
    pj.solve_DiffusionSteadyMono_b(s, precond="mg-cell", reltol=1e-13)
    xc, infoc = s.x.copy(), s.mg_info("mg-cell")
    assert s.ch[-1]["converged"] and infoc["levels"] >= 2
    assert infoc["rows"][1:] != info1["rows"][1:]                  # (another hierarchy: one kind below level 0)
    assert s.mg_info() == info1
    pj.solve_DiffusionSteadyMono_b(s, precond="mg", reltol=1e-13)
    assert np.array_equal(s.x, x1) and s.ch[-1]["iters"] == it1
    assert s.mg_info() == info1 and s.mg_info("mg-cell") == infoc
    assert rel_l2(xc, x1) <= 1e-10


def test_a_plain_solve_on_a_robin_system_is_bitwise_the_same_before_and_after_a_cell_rule_solve(pj):
    s = _build(pj, "robin-out33", cache=False)["s"]
    pj.solve_DiffusionSteadyMono_b(s, precond=0, reltol=1e-13)
    x0, it0 = s.x.copy(), s.ch[-1]["iters"]
    assert s.ch[-1]["converged"]
    pj.solve_DiffusionSteadyMono_b(s, precond="mg-cell", reltol=1e-13)
    assert s.ch[-1]["converged"] and s.ch[-1]["iters"] < it0
    pj.solve_DiffusionSteadyMono_b(s, precond=0, reltol=1e-13)
    assert np.array_equal(s.x, x0) and s.ch[-1]["iters"] == it0
    with pytest.raises(pj.PenguinHipError, match="Robin"):                       # "mg" keeps its refusal on this solver
        pj.solve_DiffusionSteadyMono_b(s, precond="mg")
