"""Host truth for what a solve REPORTS: pg_step_info.{converged, resnorm, bnorm} held against the residual and the norms
the state it left behind really has, and host restatements of the two row reductions of pg_reduce.hip.  Nothing here knows
the library: the inputs are the exported system (Â, b̂), the weights ds of the convergence test and the state y = x / ds.

truth(Ahat, bhat, ds, y), in np.longdouble (as tests/spmv_reference.py):
    bnorm_true = ||ds∘b̂||₂      res_true = ||ds∘(b̂ − Â y)||₂      σ = ||ds∘(|Â||y|)||₂ + ||ds∘b̂||₂

check_step(info, truth, reltol, abstol, products), u = 2⁻⁵³:
    (a) |info.bnorm − bnorm_true| <= 2 n u bnorm_true        n non-negative terms (each (ds_i b̂_i)², three roundings) summed
                                                              in any order: relative error < (n + 2) u on the sum, and the
                                                              square root halves it -- 2 n u leaves a factor of about four
    (b) |info.resnorm − res_true| <= Δ = c (products + 1) u σ the recurrence residual of a Krylov iteration drifts from the
                                                              true one by one product's rounding, u |Â||y|, per product
    (c) converged == 1  =>  res_true <= tol + Δ;   converged == 0  =>  res_true > tol − Δ;   tol = max(reltol bnorm_true, abstol)
    (d) Δ <= 1e-3 tol: a case where the slack of (b) and (c) could hide a wrong verdict is ill-chosen -- raised as an error

The constant c of (b) is not taken from the library.  It is 8 x the largest gap ratio
    |recurrence residual − true residual| / ((products + 1) u σ)
of the oracle's double-precision restatement of the same iteration (oracle/krylov_c.solve_poly with weights = ds, and
krylov_c.solve(.., "cg") for the CG case) on the same exported system from the same start -- the factor 8 pays for the
device's other order of summation and its fused dots -- and at least 1.  scripts/residual_truth_child.py measures the ratio
on every solve it checks (`gap_ratio` of its JSON line).  Largest ratio per case over all its solves (first solve and warm
steps, every child setting of tests/test_gpu_residual_truth.py), reltol 1e-6 and 1e-9:

    case           plain      degree 2   degree 4   degree 5   cg
    ball3d         2.1e-03    1.2e-03    2.2e-03    2.4e-03    -
    ball3d_odd     7.4e-04    7.4e-04    2.5e-03    1.8e-03    -
    disc2d_robin   6.1e-03    -          -          -          -
    diph2d         5.4e-02    -          -          -          -
    cg2d           -          -          -          -          4.6e-03

    largest ratio 5.4e-02, 8 x that = 0.43  ->  c = C_GAP = 1 (the floor).  Condition (d) on the restatement's own figures:
    delta / tol <= 5.4e-05 at reltol 1e-6 and 1e-9 on every case (the child fails where it exceeds 1e-3).

Row reductions (one rank).  A row is eliminated iff it has one entry, on its diagonal, with |val − 1| <= 1e-12; the compact
order is the full order restricted; entries keep their order within a row.
    restrict_diag(rowptr, col, val, n, n_vec)   build_diag_elim:  every such row of the system
    restrict_gamma(rowptr, col, val, n_w)       build_gamma_elim: rows [n_w, n) must ALL be such rows (else no reduction:
                                                None), rows [0, n_w) stay with the columns < n_w
Each returns a dict: rowptr / col / val of the compact matrix, the coupling block (wg_rows: full row numbers of the rows
that lose entries, wg_ptr, wg_col: index of the eliminated unknown among the eliminated ones, wg_val), and the maps
(cmap: full -> compact index, or -1 - e for eliminated entry e; rlist, elist; n_c, n_e).
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -53
C_GAP = 1.0
VACUITY = 1e-3                   # condition (d)
ELIM_TOL = 1e-12                 # |a_jj - 1| of a row alone on its diagonal (pg_reduce.hip)
LD = np.longdouble


class ResidualMismatch(AssertionError):
    pass


class Truth:
    """bnorm, res, sigma (doubles, rounded from longdouble), n, and r = b̂ − Â y (double) for whoever wants to look"""

    def __init__(self, bnorm, res, sigma, n, r):
        self.bnorm, self.res, self.sigma, self.n, self.r = float(bnorm), float(res), float(sigma), int(n), r

    def delta(self, products, c=None):
        return (C_GAP if c is None else c) * (products + 1) * U * self.sigma

    def tol(self, reltol, abstol=0.0):
        return max(reltol * self.bnorm, abstol)


def _csr(A):
    """(rowptr, col, val) of a scipy CSR matrix or of a triple"""
    if isinstance(A, tuple):
        rowptr, col, val = A
    else:
        A = A.tocsr()
        rowptr, col, val = A.indptr, A.indices, A.data
    return np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(val, dtype=np.float64)


def _rowsums(rowptr, terms):
    out = np.zeros(rowptr.size - 1, dtype=LD)
    rows = np.nonzero(np.diff(rowptr) > 0)[0]
    if rows.size:
        out[rows] = np.add.reduceat(terms, rowptr[rows])
    return out


def truth(Ahat, bhat, ds, y) -> Truth:
    rowptr, col, val = _csr(Ahat)
    n = rowptr.size - 1
    b, w, yy = (np.asarray(v, dtype=np.float64) for v in (bhat, ds, y))
    assert b.size == n and w.size == n and yy.size >= n and (col.size == 0 or col.max() < yy.size)
    p = val.astype(LD) * yy[col].astype(LD)
    Ay, absAy = _rowsums(rowptr, p), _rowsums(rowptr, np.abs(p))
    wl, bl = w.astype(LD), b.astype(LD)
    r = bl - Ay
    norm = lambda v: np.sqrt(np.sum((wl * v) ** 2))
    bnorm = norm(bl)
    return Truth(bnorm, norm(r), norm(absAy) + bnorm, n, r.astype(np.float64))


def gap_ratio(recurrence_resnorm, t: Truth, products) -> float:
    """the restatement's own gap in units of (products + 1) u σ: what c is derived from"""
    return abs(float(recurrence_resnorm) - t.res) / ((products + 1) * U * t.sigma)


def _field(info, name):
    return info[name] if isinstance(info, dict) else getattr(info, name)


def check_step(info, t: Truth, reltol, abstol, products, c=None, label=""):
    """Raises ResidualMismatch naming the check that failed; returns the figures (for the JSON line of the child)."""
    bnorm, resnorm, conv = float(_field(info, "bnorm")), float(_field(info, "resnorm")), int(_field(info, "converged"))
    delta, tol = t.delta(products, c), t.tol(reltol, abstol)
    fig = {"bnorm": bnorm, "bnorm_true": t.bnorm, "resnorm": resnorm, "res_true": t.res, "delta": delta, "tol": tol,
           "converged": conv, "products": int(products)}
    if not delta <= VACUITY * tol:
        raise ResidualMismatch(f"{label}: (d) vacuous case: delta {delta:.3e} > 1e-3 tol = {VACUITY * tol:.3e}")
    if not (np.isfinite(bnorm) and np.isfinite(resnorm)):
        raise ResidualMismatch(f"{label}: (a) non-finite figures: bnorm {bnorm!r} resnorm {resnorm!r}")
    if not abs(bnorm - t.bnorm) <= 2.0 * t.n * U * t.bnorm:
        raise ResidualMismatch(f"{label}: (a) bnorm {bnorm!r} but ||ds b|| = {t.bnorm!r}: off by {abs(bnorm - t.bnorm):.3e}, "
                               f"bound {2.0 * t.n * U * t.bnorm:.3e}")
    if not abs(resnorm - t.res) <= delta:
        raise ResidualMismatch(f"{label}: (b) resnorm {resnorm!r} but the state's residual is {t.res!r}: off by "
                               f"{abs(resnorm - t.res):.3e}, delta {delta:.3e}")
    if conv not in (0, 1):
        raise ResidualMismatch(f"{label}: (c) converged = {conv}")
    if conv == 1 and not t.res <= tol + delta:
        raise ResidualMismatch(f"{label}: (c) converged = 1 but the residual {t.res:.6e} is above tol {tol:.6e} + delta {delta:.3e}")
    if conv == 0 and not t.res > tol - delta:
        raise ResidualMismatch(f"{label}: (c) converged = 0 but the residual {t.res:.6e} is below tol {tol:.6e} - delta {delta:.3e}")
    return fig


# ---- the row reductions of pg_reduce.hip ----------------------------------------------------------------------------------
def alone_on_diagonal(rowptr, col, val, n):
    rowptr, col, val = _csr((rowptr, col, val))
    one = np.diff(rowptr[: n + 1]) == 1
    first = np.minimum(rowptr[:n], max(col.size - 1, 0))
    if col.size == 0:
        return np.zeros(n, dtype=bool)
    return one & (col[first] == np.arange(n)) & (np.abs(val[first] - 1.0) <= ELIM_TOL)


def _split(rowptr, col, val, rows, cmap):
    """rows `rows` of the matrix: entries whose column stays (renumbered) / entries of the coupling block, in row order"""
    rp, cc, vv = [0], [], []
    wg_rows, wg_ptr, wg_col, wg_val = [], [0], [], []
    for r in rows:
        a, b = int(rowptr[r]), int(rowptr[r + 1])
        j = cmap[col[a:b]]
        keep = j >= 0
        cc.append(j[keep]); vv.append(val[a:b][keep])
        rp.append(rp[-1] + int(keep.sum()))
        if not keep.all():
            wg_rows.append(int(r))
            wg_col.append(-1 - j[~keep]); wg_val.append(val[a:b][~keep])
            wg_ptr.append(wg_ptr[-1] + int((~keep).sum()))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
    return {"rowptr": np.asarray(rp, dtype=np.int64), "col": cat(cc, np.int64), "val": cat(vv, np.float64),
            "wg_rows": np.asarray(wg_rows, dtype=np.int64), "wg_ptr": np.asarray(wg_ptr, dtype=np.int64),
            "wg_col": cat(wg_col, np.int64), "wg_val": cat(wg_val, np.float64)}


def restrict_diag(rowptr, col, val, n, n_vec=None):
    """build_diag_elim on one rank: ghosts (columns >= n, if any) remain, behind the remaining owned rows, in their order"""
    rowptr, col, val = _csr((rowptr, col, val))
    n_vec = n if n_vec is None else n_vec
    e = np.zeros(n_vec, dtype=bool)
    e[:n] = alone_on_diagonal(rowptr, col, val, n)
    cmap = np.empty(n_vec, dtype=np.int64)
    cmap[~e] = np.arange(int((~e).sum()))
    cmap[e] = -1 - np.arange(int(e.sum()))
    rlist, elist = np.nonzero(~e[:n])[0], np.nonzero(e[:n])[0]
    out = _split(rowptr, col, val, rlist, cmap)
    out.update(cmap=cmap, rlist=rlist, elist=elist, n_c=int(rlist.size), n_e=int(elist.size), gdiag=val[rowptr[elist]])
    return out


def restrict_gamma(rowptr, col, val, n_w):
    """build_gamma_elim on one rank: None where it refuses (a row of [n_w, n) that is not alone on its diagonal, a ghost
    reference, n_w = 0 or n_w = n)"""
    rowptr, col, val = _csr((rowptr, col, val))
    n = rowptr.size - 1
    if n_w <= 0 or n_w >= n or (col.size and col.max() >= n):
        return None
    if not alone_on_diagonal(rowptr, col, val, n)[n_w:].all():
        return None
    cmap = np.concatenate([np.arange(n_w), -1 - np.arange(n - n_w)]).astype(np.int64)
    rlist, elist = np.arange(n_w), np.arange(n_w, n)
    out = _split(rowptr, col, val, rlist, cmap)
    out.update(cmap=cmap, rlist=rlist, elist=elist, n_c=int(n_w), n_e=int(n - n_w), gdiag=val[rowptr[elist]])
    return out


def same_matrix(got, want, label=""):
    """(rowptr, col, val) `got` equals the compact matrix `want` entry for entry, values bitwise"""
    for name, g in zip(("rowptr", "col", "val"), got):
        w = want[name]
        g = np.ascontiguousarray(g, dtype=w.dtype)
        if g.shape != w.shape:
            raise ResidualMismatch(f"{label}: {name} has {g.size} entries, the host's restriction {w.size}")
        same = (g.view(np.uint64) == w.view(np.uint64)) if name == "val" else (g.astype(np.int64) == w)
        if not same.all():
            k = int(np.nonzero(~same)[0][0])
            raise ResidualMismatch(f"{label}: {name}[{k}] = {g[k]!r}, the host's restriction has {w[k]!r} ({int((~same).sum())} differ)")
