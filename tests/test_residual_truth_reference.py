"""The checker of tests/residual_truth.py on the host alone: it accepts honest double-precision BiCGStab / CG runs (the oracle's
C restatement, oracle/krylov_c) on small block-triangular systems of the library's shape -- equilibrated rows, then rows of
the identity coupled into them -- and rejects every tampering a wrong start kernel, a skipped k_renorm or a verdict one
iteration early would amount to; the two row reductions agree with dense algebra and notice a wrong compact matrix."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import residual_truth as rt
from oracle import krylov_c

RELTOLS = (1e-6, 1e-9)


def _system(nx, ny, n_g, seed, symmetric=False):
    """[[Aww, Awg], [0, I]] with Aww = the equilibrated I + 2 (5-point Laplacian) (+ a skew part), every third ω row coupled
    to one or two identity rows; odd and even sizes come from (nx, ny, n_g)"""
    rng = np.random.default_rng(seed)
    n_w = nx * ny
    T = lambda m: sp.diags([-np.ones(m - 1), 2 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])
    Aww = (sp.identity(n_w) + 2.0 * (sp.kron(sp.identity(ny), T(nx)) + sp.kron(T(ny), sp.identity(nx)))).tocsr()
    if not symmetric:
        Aww = (Aww + 0.1 * sp.kron(sp.identity(ny), sp.diags([np.ones(nx - 1), -np.ones(nx - 1)], [1, -1]))).tocsr()
    d = 1.0 / np.sqrt(Aww.diagonal())
    Aww = (sp.diags(d) @ Aww @ sp.diags(d)).tocsr()
    if symmetric:
        return Aww, rng.uniform(-1.0, 1.0, n_w), np.ones(n_w), n_w
    rows = np.arange(0, n_w, 3)
    Awg = sp.csr_matrix((rng.uniform(-0.3, -0.05, rows.size), (rows, rng.integers(0, n_g, rows.size))), shape=(n_w, n_g))
    Awg = Awg + sp.csr_matrix((rng.uniform(-0.3, -0.05, rows.size // 2), (rows[::2][: rows.size // 2], rng.integers(0, n_g, rows.size // 2))),
                              shape=(n_w, n_g))
    A = sp.bmat([[Aww, Awg], [None, sp.identity(n_g)]]).tocsr()
    A.sort_indices()
    n = n_w + n_g
    return A, rng.uniform(-1.0, 1.0, n), rng.uniform(0.5, 2.0, n), n_w


CASES = {"odd": (9, 7, 6, 1), "even": (8, 7, 6, 2)}      # n = 69 and 62; n_w = 63 and 56


def _honest(A, b, ds, reltol, m=0, g=0.9, maxiter=10000, x0=None):
    x, it, res, nmv = krylov_c.solve_poly(A, b, m, g, x0=x0, weights=ds, reltol=reltol, maxiter=maxiter)
    t = rt.truth(A, b, ds, x)
    info = {"bnorm": float(np.sqrt(np.sum((ds * b) ** 2))), "resnorm": res, "converged": int(res <= reltol * np.sqrt(np.sum((ds * b) ** 2))),
            "iters": it}
    return info, t, nmv, x


@pytest.fixture(scope="module", params=sorted(CASES))
def run(request):
    A, b, ds, n_w = _system(*CASES[request.param])
    info, t, nmv, x = _honest(A, b, ds, 1e-9)
    prev, _, _, _ = _honest(A, b, ds, 1e-9, maxiter=info["iters"] - 1)
    return {"A": A, "b": b, "ds": ds, "n_w": n_w, "info": info, "t": t, "nmv": nmv, "x": x, "prev": prev}


def _tampered(run, **change):
    info = dict(run["info"], **change)
    with pytest.raises(rt.ResidualMismatch) as e:
        rt.check_step(info, run["t"], 1e-9, 0.0, run["nmv"], label="tampered")
    return str(e.value)


def test_truth_agrees_with_a_dense_double_product():
    A, b, ds, _ = _system(*CASES["odd"])
    y = np.random.default_rng(3).uniform(-1, 1, A.shape[0])
    t = rt.truth(A, b, ds, y)
    r = b - A.toarray() @ y
    assert abs(t.res - np.linalg.norm(ds * r)) <= 1e-13 * t.sigma
    assert abs(t.bnorm - np.linalg.norm(ds * b)) <= 1e-14 * t.bnorm
    assert abs(t.sigma - (np.linalg.norm(ds * (abs(A).toarray() @ abs(y))) + t.bnorm)) <= 1e-13 * t.sigma
    assert np.max(np.abs(t.r - r)) <= 1e-14 * t.sigma


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("reltol", RELTOLS)
@pytest.mark.parametrize("m", [0, 2, 5])
def test_honest_bicgstab_runs_are_accepted_and_never_vacuous(case, reltol, m):
    """zero start and a start from a state with the identity rows snapped (the warm steps), plain and preconditioned; the
    restatement's own gap stays under C_GAP / 8 -- the c of the checker covers it with the factor it was derived with"""
    A, b, ds, n_w = _system(*CASES[case])
    x0 = np.zeros(A.shape[0])
    x0[n_w:] = b[n_w:]
    for start in (None, x0):
        info, t, nmv, _ = _honest(A, b, ds, reltol, m=m, x0=start)
        assert info["converged"] == 1 and info["iters"] >= 2
        fig = rt.check_step(info, t, reltol, 0.0, nmv, label=f"{case} m={m}")
        assert fig["delta"] <= rt.VACUITY * fig["tol"]
        assert rt.gap_ratio(info["resnorm"], t, nmv) <= rt.C_GAP / 8.0
        # a solve capped one iteration early: not converged, and the checker agrees with that verdict too
        early, te, nmve, _ = _honest(A, b, ds, reltol, m=m, x0=start, maxiter=info["iters"] - 1)
        assert early["converged"] == 0
        rt.check_step(early, te, reltol, 0.0, nmve, label=f"{case} m={m} capped")


@pytest.mark.parametrize("reltol", RELTOLS)
def test_honest_cg_run_is_accepted(reltol):
    A, b, ds, _ = _system(9, 7, 0, 4, symmetric=True)
    x, it, res = krylov_c.solve(A, b, "cg", reltol=reltol)
    t = rt.truth(A, b, ds, x)
    info = {"bnorm": float(np.linalg.norm(b)), "resnorm": res, "converged": 1}
    rt.check_step(info, t, reltol, 0.0, it, label="cg")
    assert rt.gap_ratio(res, t, it) <= rt.C_GAP / 8.0


def test_bnorm_scaled_by_1_0001_is_rejected(run):
    assert "(a)" in _tampered(run, bnorm=run["info"]["bnorm"] * 1.0001)


def test_bnorm_scaled_by_4_is_rejected(run):
    assert "(a)" in _tampered(run, bnorm=run["info"]["bnorm"] * 4.0)


def test_resnorm_of_the_previous_iterate_is_rejected(run):
    assert "(b)" in _tampered(run, resnorm=run["prev"]["resnorm"])


def test_flipped_verdict_is_rejected(run):
    assert "(c)" in _tampered(run, converged=0)
    # ... and the other way round: the previous iterate, honestly reported, called converged
    x, it, res, nmv = krylov_c.solve_poly(run["A"], run["b"], 0, 0.9, weights=run["ds"], reltol=1e-9, maxiter=run["info"]["iters"] - 1)
    with pytest.raises(rt.ResidualMismatch, match=r"\(c\)"):
        rt.check_step({"bnorm": run["info"]["bnorm"], "resnorm": res, "converged": 1}, rt.truth(run["A"], run["b"], run["ds"], x),
                      1e-9, 0.0, nmv)


def test_unweighted_norms_are_rejected(run):
    r = run["b"] - run["A"] @ run["x"]
    assert "(b)" in _tampered(run, resnorm=float(np.linalg.norm(r)))
    assert "(a)" in _tampered(run, resnorm=float(np.linalg.norm(r)), bnorm=float(np.linalg.norm(run["b"])))


def test_a_vacuous_case_is_an_error(run):
    with pytest.raises(rt.ResidualMismatch, match=r"\(d\)"):
        rt.check_step(run["info"], run["t"], 1e-14, 0.0, run["nmv"])


# ---- the row reductions ---------------------------------------------------------------------------------------------------
def _compact_solve(A, b, red):
    """solve through the reduction: eliminated rows on the spot, the compact system with the coupling block on the right"""
    n = A.shape[0]
    x = np.zeros(n)
    x[red["elist"]] = b[red["elist"]] / red["gdiag"]
    bc = b[red["rlist"]].copy()
    for q, r in enumerate(red["wg_rows"]):
        a, e = red["wg_ptr"][q], red["wg_ptr"][q + 1]
        bc[red["cmap"][r]] -= np.dot(red["wg_val"][a:e], x[red["elist"]][red["wg_col"][a:e]])
    Ac = sp.csr_matrix((red["val"], red["col"], red["rowptr"]), shape=(red["n_c"], red["n_c"]))
    x[red["rlist"]] = np.linalg.solve(Ac.toarray(), bc)
    return x


@pytest.mark.parametrize("case", sorted(CASES))
def test_reductions_are_the_full_system_restricted(case):
    A, b, ds, n_w = _system(*CASES[case])
    n = A.shape[0]
    xd = np.linalg.solve(A.toarray(), b)
    rd = rt.restrict_diag(A.indptr, A.indices, A.data, n, n)
    rg = rt.restrict_gamma(A.indptr, A.indices, A.data, n_w)
    assert rd["n_e"] == rg["n_e"] == n - n_w and rd["n_c"] == n_w
    for red in (rd, rg):
        assert np.max(np.abs(_compact_solve(A, b, red) - xd)) <= 1e-12 * np.max(np.abs(xd))
        assert red["wg_ptr"][-1] == A.nnz - red["rowptr"][-1] - red["n_e"]
    rt.same_matrix((rd["rowptr"], rd["col"], rd["val"]), rg, "gamma vs diag")
    # rows alone on their diagonal in the MIDDLE of the order: only restrict_diag takes them, the order is the full one restricted
    P = np.random.default_rng(7).permutation(n)
    Ap = A[P][:, P].tocsr()
    Ap.sort_indices()
    rp = rt.restrict_diag(Ap.indptr, Ap.indices, Ap.data, n, n)
    assert rp["n_e"] == n - n_w and np.all(np.diff(rp["rlist"]) > 0)
    assert np.array_equal(np.sort(P[rp["elist"]]), np.arange(n_w, n))
    assert np.max(np.abs(_compact_solve(Ap, b[P], rp) - xd[P])) <= 1e-12 * np.max(np.abs(xd))
    assert rt.restrict_gamma(Ap.indptr, Ap.indices, Ap.data, n_w) is None
    # a diagonal off 1 by more than the equilibration's rounding is no such row
    Aq = A.copy()
    Aq.data[Aq.indptr[n - 1]] = 1.0 + 1e-11
    assert rt.restrict_diag(Aq.indptr, Aq.indices, Aq.data, n, n)["n_e"] == n - n_w - 1
    assert rt.restrict_gamma(Aq.indptr, Aq.indices, Aq.data, n_w) is None


def _device_like(A):
    """the host's restriction and a copy of its compact matrix for a test to tamper with"""
    n = A.shape[0]
    rd = rt.restrict_diag(A.indptr, A.indices, A.data, n, n)
    return rd, [rd["rowptr"].copy(), rd["col"].copy(), rd["val"].copy()]


def test_a_coupling_entry_left_in_is_rejected():
    A, _, _, n_w = _system(*CASES["odd"])
    rd, got = _device_like(A)
    r = int(rd["wg_rows"][0])                                   # a row that loses an entry: leave it in, at the row's end
    c = int(rd["cmap"][r])
    at = int(got[0][c + 1])
    got[1] = np.insert(got[1], at, 0)
    got[2] = np.insert(got[2], at, rd["wg_val"][0])
    got[0][c + 1:] += 1
    with pytest.raises(rt.ResidualMismatch):
        rt.same_matrix(got, rd, "left in")


def test_two_entries_of_a_row_swapped_are_rejected():
    A, _, _, n_w = _system(*CASES["even"])
    rd, got = _device_like(A)
    a = int(got[0][5])
    assert got[0][6] - a >= 2
    for k in (1, 2):
        got[k][[a, a + 1]] = got[k][[a + 1, a]]                # the same matrix as an operator, another order of summation
    with pytest.raises(rt.ResidualMismatch, match="col"):
        rt.same_matrix(got, rd, "swapped")
    rt.same_matrix([rd["rowptr"], rd["col"], rd["val"]], rd, "honest")
