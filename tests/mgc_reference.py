"""Restatement (numpy / scipy) of the cell-aggregated multigrid preconditioner (precond="mg-cell", PG_PRECOND_MG_CELL) of
penguin/jl_amd/csrc/pg_multigrid.hip, as DESIGN.md "Cell-aggregated multigrid" defines it, and of the cell-block left
preconditioner of csrc/pg_precond.hip whose product Â = B⁻¹ S A S is its level 0.  Test infrastructure:
tests/test_mgc_reference.py runs it on the oracle's systems, tests/test_gpu_mg_cell.py compares the library with it.

Everything not named here is tests/mg_reference.py unchanged (Galerkin products, ω = 0.7, 2 + 2 sweeps, the over-correction
1.8, the dense inverse of the first level with <= 200 rows): Level, Hierarchy, VCycle, bicgstab_right, dense_inverse and
equilibrate are that module's.

  level 0        Â = B⁻¹ S A S, the matrix the Krylov loop iterates on; its diagonal is 1 on blocked and un-blocked rows alike
  aggregates     0 -> 1: an unknown of ANY kind in padded cell (i, j, k3) -> coarse cell (i >> 1, j >> 1, k3 >> 1): ω and γ of a
                 2 x 2 (x 2) block of cells share one coarse unknown; coarse unknowns numbered by coarse cell, dimension 0
                 fastest.  The levels >= 1 have one kind and repeat the rule on the coarse coordinates
  prolongation   level 0 -> 1: 1 / ds_i at fine unknown i, for ω and γ alike (constant in the unknowns of A: the near-null
                 vector of [G H]); 0 / 1 between coarser levels
"""
from __future__ import annotations

from typing import Iterable, Optional, Sequence

import numpy as np
import scipy.sparse as sp

from tests import mg_reference as mg
from tests.mg_reference import Hierarchy, Level, VCycle, bicgstab_right, dense_inverse, equilibrate  # noqa: F401  (re-exported)

COARSEST_ROWS = mg.COARSEST_ROWS


def cell_blocks(Ar: sp.spmatrix, idx: np.ndarray, M: int, border_cells: Optional[Iterable[int]] = None):
    """(Â, ds, B⁻¹) of a reduced matrix, following csrc/pg_precond.hip.

    Ar: the reduced matrix; idx: index of every row in the full kind-major padded vector (kind * M + linear cell); M: padded
    cells; border_cells: linear cells whose bulk row was overwritten by a border condition.

      S    ds_i = |a_ii|^-1/2 (1 where the diagonal is zero, or zero but for rounding: |a_ii| <= 1e-13 max_j |a_ij|)
      B    per-cell diagonal blocks of S A S over the unknowns that live in one cell:
             cells with >= 2 active unknowns are blocked;
             a cell whose bulk row was overwritten by a border condition is not blocked;
             a singular block (a pivot of the Gauss-Jordan elimination with partial pivoting <= 1e-300) is not blocked.
    """
    Ar = sp.csr_matrix(Ar, dtype=np.float64)
    n = Ar.shape[0]
    idx = np.asarray(idx, dtype=np.int64)
    d = Ar.diagonal()
    rowmax = np.asarray(abs(Ar).max(axis=1).todense()).ravel()
    a = np.abs(d)
    ok = (a > 1e-13 * rowmax) & (a < 1e300)
    ds = np.where(ok, 1.0 / np.sqrt(np.where(ok, a, 1.0)), 1.0)
    S = sp.diags(ds)
    As = sp.csr_matrix(S @ Ar @ S)
    cell = idx % M
    order = np.argsort(cell, kind="stable")                # rows of one cell side by side, kinds ascending
    start = np.flatnonzero(np.r_[True, np.diff(cell[order]) != 0, True])
    skip = set(int(c) for c in border_cells) if border_cells is not None else set()
    bi, bj, bv = [], [], []
    blocked = np.zeros(n, dtype=bool)
    for s, e in zip(start[:-1], start[1:]):
        if e - s < 2 or int(cell[order[s]]) in skip:
            continue
        rows = order[s:e]
        m = As[rows][:, rows].toarray()
        inv = _small_inverse(m)
        if inv is None:
            continue
        blocked[rows] = True
        for p, r in enumerate(rows):
            for q, c in enumerate(rows):
                bi.append(r); bj.append(c); bv.append(inv[p, q])
    free = np.flatnonzero(~blocked)
    Binv = sp.csr_matrix((np.r_[bv, np.ones(free.size)], (np.r_[bi, free].astype(np.int64), np.r_[bj, free].astype(np.int64))),
                         shape=(n, n))
    Ahat = sp.csr_matrix(Binv @ As)
    Ahat.sort_indices()
    return Ahat, ds, Binv


def _small_inverse(m: np.ndarray):
    """Gauss-Jordan with partial pivoting on a small block; None where a pivot is <= 1e-300 (the cell stays un-blocked)."""
    n = m.shape[0]
    m = m.astype(np.float64).copy()
    inv = np.eye(n)
    for c in range(n):
        piv = c + int(np.argmax(np.abs(m[c:, c])))
        if not np.abs(m[piv, c]) > 1e-300:
            return None
        if piv != c:
            m[[c, piv]] = m[[piv, c]]
            inv[[c, piv]] = inv[[piv, c]]
        f = 1.0 / m[c, c]
        m[c] *= f
        inv[c] *= f
        for r in range(n):
            if r != c and m[r, c] != 0.0:
                g = m[r, c]
                m[r] -= g * m[c]
                inv[r] -= g * inv[c]
    return inv


def _on_pattern(X: sp.csr_matrix, pat: sp.coo_matrix) -> sp.csr_matrix:
    """X on the stored positions of pat (explicit zeros where X has none), column indices sorted."""
    vals = np.asarray(X[pat.row, pat.col]).ravel() if pat.nnz else np.zeros(0)
    out = sp.csr_matrix((vals, (pat.row, pat.col)), shape=pat.shape)
    out.sort_indices()
    return out


def galerkin(A: sp.csr_matrix, w: np.ndarray, agg: np.ndarray, nc: int, absolute: Optional[sp.spmatrix] = None):
    """(Pᵀ A P, |P|ᵀ |A| |P|) with P = diag(w) Z, Z the 0 / 1 aggregate map: one Galerkin product and the sum of the absolute
    values of the terms each of its entries was added up from (`absolute`: a matrix to put in the place of |A|).  The pattern is
    structural -- every coarse pair a stored entry of A maps to, also where the terms cancel to an exact zero (scipy's products
    drop those) -- as the library's Galerkin kernel builds it."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    P = sp.csr_matrix((w, (np.arange(n), agg)), shape=(n, nc))
    Z = sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, nc))
    ones = sp.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
    pat = sp.coo_matrix(Z.T @ ones @ Z)
    Ac = _on_pattern(sp.csr_matrix(P.T @ A @ P), pat)
    absA = _on_pattern(sp.csr_matrix(abs(P).T @ (abs(A) if absolute is None else absolute) @ abs(P)), pat)
    return Ac, absA


def build_hierarchy_cells(Ahat: sp.spmatrix, ds: np.ndarray, idx: np.ndarray, ext: Sequence[int]) -> Hierarchy:
    """Ahat: Â = B⁻¹ S A S; ds: the row scaling S; idx: index of every row in the full kind-major padded vector; ext: the padded
    extents n_d + 1.  Every level >= 1 carries absA = |P|ᵀ |A_l| |P|, the sum of the |fine terms| each entry was added up from (as
    mg_reference.build_hierarchy has it), and fine0, the same sum carried down from level 0."""
    Ahat = sp.csr_matrix(Ahat, dtype=np.float64)
    Ahat.sort_indices()
    n = Ahat.shape[0]
    ds = np.asarray(ds, dtype=np.float64)
    if np.any(~(Ahat.diagonal() > 0.0)) or np.any(~(ds > 0.0)):
        raise ValueError("multigrid restatement refused: a row of the system has no positive diagonal entry")
    ext = tuple(int(e) for e in ext) + (1,) * (3 - len(ext))
    M0 = ext[0] * ext[1] * ext[2]
    H = Hierarchy()
    H.levels.append(Level(A=Ahat, dinv=np.ones(n), ext=ext, key=np.asarray(idx, dtype=np.int64) % M0, w=1.0 / ds))   # kind-free keys
    while H.levels[-1].A.shape[0] > COARSEST_ROWS:
        f = H.levels[-1]
        cext = tuple((e + 1) >> 1 for e in f.ext)
        cell = f.key
        i, j, k = cell % f.ext[0], (cell // f.ext[0]) % f.ext[1], cell // (f.ext[0] * f.ext[1])
        ckey = (i >> 1) + (j >> 1) * cext[0] + (k >> 1) * cext[0] * cext[1]
        keys, agg = np.unique(ckey, return_inverse=True)
        nc = keys.size
        if f.w is None:
            f.w = np.ones(f.A.shape[0])
        f.agg = agg.astype(np.int64)
        Ac, absA = galerkin(f.A, f.w, f.agg, nc)
        # besides the bound of this product, the same sum carried down from level 0 (see test_gpu_mg_cell.py: a whole-hierarchy check)
        _, fine0 = galerkin(f.A, f.w, f.agg, nc, absolute=getattr(f, "fine0", None))
        d = Ac.diagonal()
        if np.any(~(d > 0.0)):
            raise ValueError(f"multigrid restatement: a coarse diagonal entry is not positive (level {len(H.levels)})")
        H.levels.append(Level(A=Ac, dinv=1.0 / d, ext=cext, key=keys.astype(np.int64), absA=absA))
        H.levels[-1].fine0 = fine0
    H.inv = dense_inverse(H.levels[-1].A.toarray())
    return H
