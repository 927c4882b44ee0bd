"""Every SpMV launch mode, as the Krylov driver issues it, against an extended-precision product on the host.

pg_debug_spmv_apply runs ONE launch through launch_spmv on host vectors and hands back everything it wrote; the matrix comes
from pg_solver_get_system_csr (which = 2 constructor, 3 run, 7 the matrix the warm loop iterates on, in its own numbering);
tests/spmv_reference.py forms the product in extended precision and holds y, the fused dots and the folded sums against the
forward error bounds stated there (tests/test_spmv_reference.py shows on the CPU what that checker rejects).  Reached here and
by no kernel-vs-kernel comparison: launch mode 2 (CG), the (y, .) dot of modes 2 / 3 with an operand that is not x
(FinArgs::dotx: the polynomial-preconditioned BiCGStab, twice per iteration), mode 8 with base aliased to x (the chain's first
step), the scalar phase folded into the launch (ticket, agent-scope partials, reset), the return at the done flag -- and the
chunked CSR kernel itself, the reference of every other comparison.

Partial sums: every variant (70, 38 / 2, 1) writes one partial per block and slot, slot-major with stride grid, slots 0 / 1 / 4 as
pg_spmv.h states them; the entry sums them on the host in index order (slot_sums).  Slots 2 and 3 belong to another kernel
(k_bicg_s) and hold zeros when a mode-3 launch folds its five slots.

Cases: the four smallest shapes of tests/test_gpu_spmv_edge_rows.py that have marching units and edge rows at the default
PG_SPMV_MINRUN, and two 2-D systems (Robin disc, diphasic) for the P slices and G chunks."""
import zlib

import numpy as np
import pytest

from tests import spmv_reference as R
from tests.test_gpu_spmv_edge_rows import _info, _stepped

pytestmark = pytest.mark.gpu

MARCHING = ("sphere80_be", "offcentre", "disc2d", "two_balls")
WHICH = {**{c: (2, 3, 7) for c in MARCHING}, "mono2d_robin": (2, 3, 7), "diph2d": (2,)}
PAIRS = [(c, w) for c, ws in WHICH.items() for w in ws]
# mode 8 as the chain sets it (pg_krylov.hip): first step (τ_(m-1), -τ_(m-1) τ_k, τ_k), later steps (1, -τ_k, τ_k); and the
# coefficients of pg_debug_spmv_mode_compare
TAU_K, TAU_M1 = 1.37, 0.61
PCS = ((TAU_M1, -TAU_M1 * TAU_K, TAU_K), (1.0, -TAU_K, TAU_K), (0.75, -0.4375, 1.25))

_SOLVERS, _SYSTEMS, _VECTORS, _PRODUCTS = {}, {}, {}, {}


def _solver(pj, case):
    if case in MARCHING:
        return _stepped(pj, case)
    if case not in _SOLVERS:
        if case == "mono2d_robin":
            mesh = pj.Mesh((96, 64), (4.0, 4.0))
            cap = pj.Capacity(pj.Sphere((2.01, 2.01), 1.0), mesh)
            bcb = pj.BorderConditions({k: pj.Dirichlet(0.0) for k in ("left", "right", "top", "bottom")})
            ph = pj.Phase(cap, pj.DiffusionOps(cap), 0.0, 1.0)
            s = pj.DiffusionUnsteadyMono(ph, bcb, pj.Robin(1.0, 0.3, 1.0), 1e-3, None, "CN")
            pj.solve_DiffusionUnsteadyMono_b(s, ph, 1e-3, 0.5e-3, bcb, pj.Robin(1.0, 0.3, 1.0), "CN", reltol=1e-12)   # run matrix
        else:
            assert case == "diph2d"
            n, M = 64, 65 * 65
            mesh = pj.Mesh((n, n), (8.0, 8.0))
            c1, c2 = pj.Capacity(pj.Sphere((4.0, 4.0), 2.0), mesh), pj.Capacity(pj.Sphere((4.0, 4.0), 2.0, complement=True), mesh)
            ic = pj.InterfaceConditions(pj.ScalarJump(1.0, 1.0, 0.0), pj.FluxJump(1.0, 1.0, 0.0))
            s = pj.DiffusionUnsteadyDiph(pj.Phase(c1, pj.DiffusionOps(c1), 0.0, 1.0), pj.Phase(c2, pj.DiffusionOps(c2), 0.0, 1.0),
                                         pj.BorderConditions({}), ic, 1e-3, np.zeros(4 * M), "BE")
        _SOLVERS[case] = s
    return _SOLVERS[case]


def _system(pj, case, which):
    """(solver, rowptr, col, val, n, n_vec) of one matrix, downloaded once"""
    from penguin.jl_amd import _lib as L
    if (case, which) not in _SYSTEMS:
        s = _solver(pj, case)
        n, nv, nnz, grid = L.debug_spmv_sizes(s._h, which)
        rowptr, col, val = L.loop_system_csr(s._h, which)
        info = _info(s, which)
        assert n == info.rows_matrix and nnz == info.nnz and rowptr[-1] == nnz and nv >= n and grid >= 1
        assert col.min() >= 0 and col.max() < nv
        _SYSTEMS[(case, which)] = (s, rowptr, col, val, n, nv)
    return _SYSTEMS[(case, which)]


def _vectors(pj, case, which, family):
    """x (n_vec), aux, dotx, base (n): drawn independently, fixed seed per (case, which, family); and the reference product of
    x, computed once and never changed"""
    key = (case, which, family)
    if key not in _VECTORS:
        _, rowptr, col, val, n, nv = _system(pj, case, which)
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        v = {k: R.vector(family, nv if k == "x" else n, rng) for k in ("x", "aux", "dotx", "base")}
        for a in v.values():
            a.setflags(write=False)
        _VECTORS[key] = v
        _PRODUCTS[key] = R.Product(rowptr, col, val, v["x"])
    return _VECTORS[key], _PRODUCTS[key]


def _apply(s, which, variant, mode, v, dotx=False, base=False, **kw):
    from penguin.jl_amd import _lib as L
    return L.debug_spmv_apply(s._h, which, variant, mode, v["x"], aux=v["aux"] if mode in (1, 3) else None,
                              dotx=v["dotx"] if dotx else None, base=v["base"] if base else None, **kw)


def _check(prod, mode, out, v, dotx=False, base=False, pc=(0.0, 0.0, 0.0), fold=False, label=""):
    return R.check_launch(prod, mode, out["y"], out["slot_sums"] if R.DOT_SLOTS[mode] else None,
                          aux=v["aux"] if mode in (1, 3) else None, dotx=v["dotx"] if dotx else None,
                          base=v["base"] if base else None, pc=pc, folded=out["folded"] if fold else None,
                          partials=out["partials"] if fold else None, ticket=out["ticket"] if fold else None, label=label)


def _sentinel(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) == np.uint64(R.SENTINEL_BITS)


@pytest.mark.parametrize("case", list(WHICH))
def test_images_hold_what_the_cases_are_there_for(pj, case):
    """Marching units and edge rows on the four marching cases -- a change of the image builder must not quietly empty the
    tests below; irregular rows (G chunks) and rows in P slices everywhere; no unit at all in the diphasic image (the Robin
    disc has a few short ones)."""
    s = _solver(pj, case)
    for which in WHICH[case]:
        i = _info(s, which)
        print(case, which, "rows", i.rows_matrix, "units", i.spmv_units, "marched", i.rows_marched, "edge", i.rows_edge, "uniform",
              i.rows_uniform, "pattern", i.rows_pattern, "irregular", i.rows_irregular, "slices", i.spmv_slices)
        assert i.rows_uniform + i.rows_pattern + i.rows_irregular == i.rows_matrix
        assert i.rows_irregular > 0 and i.spmv_slices > 0, (case, which)
        assert i.rows_pattern > i.rows_edge, (case, which, i.rows_pattern, i.rows_edge)      # rows in P slices
        if case == "diph2d":
            assert i.spmv_units == 0, (case, i.spmv_units)                                   # the image without any unit
        if case in MARCHING:
            assert i.rows_edge > 0 and i.spmv_units > 0, (case, which, i.rows_edge, i.spmv_units)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case,which", PAIRS)
def test_launch_modes_against_the_host_product(pj, case, which, family):
    """Slice kernel (70): modes 0, 1, 2, 3 (dot operand x, and dotx) and 8 (base distinct, and aliased to x; three coefficient
    sets); chunked CSR kernel (38): modes 0 - 3; variants 2 and 1: mode 0.  Every row of y within its bound and written, the
    guard words untouched, every dot within its bound of Σ w_i y_i over the returned y."""
    s = _system(pj, case, which)[0]
    v, prod = _vectors(pj, case, which, family)
    worst = {"row": 0.0, "dot": 0.0}

    def run(variant, mode, dotx=False, base=False, pc=(0.0, 0.0, 0.0)):
        label = f"{case} which {which} {family} variant {variant} mode {mode} dotx {dotx} base {base} pc {pc}"
        out = _apply(s, which, variant, mode, v, dotx, base, pc=pc)
        r = _check(prod, mode, out, v, dotx, base, pc, label=label)
        # what the mode does not write still holds the sentinel: partial slots, the scalar block's sums, the ticket
        written = sorted(R.DOT_SLOTS[mode])
        assert [k for k in range(5) if not _sentinel(out["partials"][k]).any()] == written, label
        assert all(_sentinel(out["partials"][k]).all() for k in range(5) if k not in written), label
        assert _sentinel(out["folded"]).all() and out["ticket"] == 0, label
        for k in worst:
            worst[k] = max(worst[k], r[k])

    run(70, 0)
    run(70, 1)
    for mode in (2, 3):
        run(70, mode)
        run(70, mode, dotx=True)
    for pc in PCS:
        run(70, 8, base=True, pc=pc)
        run(70, 8, base=False, pc=pc)
    for mode in (0, 1, 2, 3):
        run(38, mode)
    run(2, 0)
    run(1, 0)
    print(f"RATIO modes {case} which {which} {family}: largest error / bound: row {worst['row']:.4f} dot {worst['dot']:.3e}")


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case,which", PAIRS)
def test_folded_scalar_phase_against_the_host_sums(pj, case, which, family):
    """fold = 1, modes 1, 2, 3 (with and without dotx): the sums the last block left in the scalar block equal the exact sum of
    the partials the launch stored, within γ_grid Σ|partial|, and meet the dots' own bound; the ticket reads 0 afterwards; a
    second launch on the same buffers (repeat = 2: the ticket was reset, the partials overwritten) gives bitwise the same y,
    partials and sums."""
    s = _system(pj, case, which)[0]
    v, prod = _vectors(pj, case, which, family)
    worst = {"row": 0.0, "dot": 0.0, "fold": 0.0}
    for mode, dotx in ((1, False), (2, False), (2, True), (3, False), (3, True)):
        label = f"{case} which {which} {family} folded mode {mode} dotx {dotx}"
        one = _apply(s, which, 70, mode, v, dotx, fold=1, repeat=1)
        r = _check(prod, mode, one, v, dotx, fold=True, label=label)
        nslots = R.FOLD_SLOTS[mode]
        assert not _sentinel(one["folded"][:nslots]).any() and _sentinel(one["folded"][nslots:]).all(), label
        if mode == 3:
            assert np.all(one["folded"][2:4] == 0.0), label
        assert one["ticket"] == 0, label
        two = _apply(s, which, 70, mode, v, dotx, fold=1, repeat=2)
        for k in ("y", "partials", "slot_sums", "folded"):
            assert np.array_equal(one[k].view(np.uint64), two[k].view(np.uint64)), (label, k)
        assert two["ticket"] == 0, label
        for k in worst:
            worst[k] = max(worst[k], r[k])
    print(f"RATIO fold {case} which {which} {family}: largest error / bound: row {worst['row']:.4f} dot {worst['dot']:.3e} "
          f"fold {worst['fold']:.4f}")


@pytest.mark.parametrize("case,which", PAIRS)
def test_launch_behind_the_done_flag_writes_nothing(pj, case, which):
    """done = 1: y, the partials and the sums still hold the sentinel and no ticket was drawn -- plain, folded and Horner
    launches, slice and CSR kernels; the next launch on the same solver with done = 0 passes the ordinary check."""
    s = _system(pj, case, which)[0]
    v, prod = _vectors(pj, case, which, "uniform")
    n = prod.n
    for variant, mode, kw in ((70, 0, {}), (70, 3, {"fold": 1}), (70, 3, {"fold": 1, "repeat": 2}), (70, 8, {"pc": PCS[0]}), (38, 2, {}),
                              (1, 1, {})):
        label = f"{case} which {which} done variant {variant} mode {mode} {kw}"
        out = _apply(s, which, variant, mode, v, dotx=(variant == 70 and mode == 3), done=1, **kw)
        R.check_untouched(out["y"], n, ticket=out["ticket"], label=label)
        assert _sentinel(out["partials"][[0, 1, 4]]).all() and _sentinel(out["folded"]).all(), label
        after = _apply(s, which, variant, mode, v, dotx=(variant == 70 and mode == 3), done=0, **kw)
        _check(prod, mode, after, v, dotx=(variant == 70 and mode == 3), pc=kw.get("pc", (0.0, 0.0, 0.0)), fold=bool(kw.get("fold")),
               label=label + " then done = 0")
