"""Restatement (numpy / scipy) of the aggregation multigrid preconditioner of penguin/jl_amd/csrc/pg_multigrid.hip, as
DESIGN.md "Multigrid" defines it.  Test infrastructure: tests/test_mg_reference.py runs it on the oracle's systems,
tests/test_gpu_multigrid.py compares the library's hierarchy and applications with it.

  level 0        Â = S A S (unit diagonal), S = diag(ds)
  aggregates     unknown of kind k in padded cell (i, j, k3) -> (k, i >> 1, j >> 1, k3 >> 1); coarse unknowns numbered kind-major,
                 then by coarse cell index with dimension 0 fastest; coarser levels repeat the rule on the coarse coordinates
  prolongation   level 0 -> 1: 1 / ds_i at fine unknown i (piecewise constant in the unknowns of A); 0 / 1 between coarser levels
  operators      Galerkin, A_(l+1) = P_lᵀ A_l P_l
  smoother       damped Jacobi, ω = 0.7: two pre-sweeps (the first from zero), two post-sweeps
  correction     scaled by 1.8
  coarsest       the first level with <= 200 rows, solved with its dense inverse (Gauss-Jordan, partial pivoting, long double)

A hierarchy is built in float64; an application runs in float64 or, on request, in np.longdouble (the same matrices, every
vector operation and the coarsest inverse carried in the wider type): their difference is the rounding of one float64
application, the yardstick the GPU test measures the library's application with.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import scipy.sparse as sp

OMEGA = 0.7
OVER = 1.8
COARSEST_ROWS = 200


@dataclass
class Level:
    A: sp.csr_matrix                 # level 0: Â; l >= 1: the Galerkin product (not equilibrated)
    dinv: np.ndarray                 # 1 / diagonal (level 0: ones -- the unit diagonal is taken as exact)
    ext: tuple                       # padded cell grid of the level (3 extents, dimension 0 fastest)
    key: np.ndarray                  # kind * cells + linear cell of every row
    agg: Optional[np.ndarray] = None  # row of the next level (all but the last level)
    w: Optional[np.ndarray] = None    # prolongation weights (level 0: 1 / ds; ones below)
    absA: Optional[sp.csr_matrix] = None   # l >= 1: Σ |fine terms| each entry was added up from (the GPU test's rounding bar)


@dataclass
class Hierarchy:
    levels: List[Level] = field(default_factory=list)
    inv: Optional[np.ndarray] = None  # np.longdouble inverse of the last level

    @property
    def rows(self):
        return [lv.A.shape[0] for lv in self.levels]

    @property
    def nnz(self):
        return [lv.A.nnz for lv in self.levels]


def dense_inverse(a: np.ndarray) -> np.ndarray:
    """Inverse by Gauss-Jordan elimination with partial pivoting in np.longdouble."""
    n = a.shape[0]
    m = np.zeros((n, 2 * n), dtype=np.longdouble)
    m[:, :n] = a
    m[np.arange(n), n + np.arange(n)] = 1.0
    for c in range(n):
        p = c + int(np.argmax(np.abs(m[c:, c])))
        if not np.abs(m[p, c]) > 0:
            raise ValueError("multigrid restatement: the coarsest system is singular")
        if p != c:
            m[[c, p]] = m[[p, c]]
        m[c] = m[c] / m[c, c]
        f = m[:, c].copy()
        f[c] = 0.0
        m -= np.outer(f, m[c])
    return m[:, n:]


def build_hierarchy(Ahat: sp.spmatrix, ds: np.ndarray, idx: np.ndarray, ext: Sequence[int]) -> Hierarchy:
    """Ahat: the equilibrated reduced matrix; ds: its row scaling S; idx: index of every row in the full kind-major padded vector
    (kind * prod(ext) + linear cell); ext: the padded extents n_d + 1."""
    Ahat = sp.csr_matrix(Ahat, dtype=np.float64)
    Ahat.sort_indices()
    n = Ahat.shape[0]
    ds = np.asarray(ds, dtype=np.float64)
    if np.any(~(Ahat.diagonal() > 0.0)) or np.any(~(ds > 0.0)):
        raise ValueError("multigrid restatement refused: a row of the system has no positive diagonal entry")
    ext = tuple(int(e) for e in ext) + (1,) * (3 - len(ext))
    H = Hierarchy()
    H.levels.append(Level(A=Ahat, dinv=np.ones(n), ext=ext, key=np.asarray(idx, dtype=np.int64), w=1.0 / ds))
    while H.levels[-1].A.shape[0] > COARSEST_ROWS:
        f = H.levels[-1]
        M = f.ext[0] * f.ext[1] * f.ext[2]
        cext = tuple((e + 1) >> 1 for e in f.ext)
        Mc = cext[0] * cext[1] * cext[2]
        kind, cell = f.key // M, f.key % M
        i, j, k = cell % f.ext[0], (cell // f.ext[0]) % f.ext[1], cell // (f.ext[0] * f.ext[1])
        ckey = kind * Mc + (i >> 1) + (j >> 1) * cext[0] + (k >> 1) * cext[0] * cext[1]
        keys, agg = np.unique(ckey, return_inverse=True)
        nc = keys.size
        if f.w is None:
            f.w = np.ones(f.A.shape[0])
        f.agg = agg.astype(np.int64)
        P = sp.csr_matrix((f.w, (np.arange(f.A.shape[0]), f.agg)), shape=(f.A.shape[0], nc))
        Ac = sp.csr_matrix(P.T @ f.A @ P)
        Ac.sum_duplicates()
        Ac.sort_indices()
        absA = sp.csr_matrix(abs(P).T @ abs(f.A) @ abs(P))
        absA.sort_indices()
        d = Ac.diagonal()
        if np.any(~(d > 0.0)):
            raise ValueError("multigrid restatement: a coarse diagonal entry is not positive")
        H.levels.append(Level(A=Ac, dinv=1.0 / d, ext=cext, key=keys.astype(np.int64), absA=absA))
    H.inv = dense_inverse(H.levels[-1].A.toarray())
    return H


class _Csr:
    """y = A x in any dtype (scipy's kernels stop at float64)."""

    def __init__(self, A: sp.csr_matrix, dtype):
        self.n = A.shape[0]
        self.rows = np.repeat(np.arange(self.n), np.diff(A.indptr))
        self.col = A.indices
        self.val = A.data.astype(dtype)
        self.A = A
        self.dtype = dtype

    def __matmul__(self, x):
        if self.dtype == np.float64:
            return self.A @ x
        y = np.zeros(self.n, dtype=self.dtype)
        np.add.at(y, self.rows, self.val * x[self.col])
        return y


class VCycle:
    """z = M⁻¹ r in `dtype` (np.float64 or np.longdouble)."""

    def __init__(self, H: Hierarchy, dtype=np.float64):
        self.H, self.dtype = H, dtype
        self.mats = [_Csr(lv.A, dtype) for lv in H.levels]
        self.dinv = [lv.dinv.astype(dtype) for lv in H.levels]
        self.w = [None if lv.w is None else lv.w.astype(dtype) for lv in H.levels]
        self.inv = H.inv.astype(dtype)
        self.applications = 0

    def _restrict(self, l, v):
        lv = self.H.levels[l]
        nc = self.H.levels[l + 1].A.shape[0]
        out = np.zeros(nc, dtype=self.dtype)
        np.add.at(out, lv.agg, self.w[l] * v)
        return out

    def _cycle(self, l, r):
        if l == len(self.H.levels) - 1:
            return self.inv @ r
        A, dinv = self.mats[l], self.dinv[l]
        om, over = self.dtype(OMEGA), self.dtype(OVER)
        x = om * dinv * r
        x = x + om * dinv * (r - A @ x)
        e = self._cycle(l + 1, self._restrict(l, r - A @ x))
        x = x + over * (self.w[l] * e[self.H.levels[l].agg])
        x = x + om * dinv * (r - A @ x)
        x = x + om * dinv * (r - A @ x)
        return x

    def __call__(self, r):
        self.applications += 1
        return self._cycle(0, np.asarray(r, dtype=self.dtype))


def bicgstab_right(A: sp.csr_matrix, b: np.ndarray, M=None, reltol: float = 1e-12, maxiter: int = 20000):
    """BiCGStab on A M⁻¹ (M = None: the plain iteration) from zero, stopped at ||r|| <= reltol ||b|| -- also after the first
    half of an iteration.  Returns (x, applications of A, ||r||)."""
    n = A.shape[0]
    x = np.zeros(n)
    r = b.astype(np.float64).copy()
    rhat = r.copy()
    p = r.copy()
    rho = rhat @ r
    tol = reltol * np.linalg.norm(b)
    napp = 0
    prec = (lambda v: np.asarray(M(v), dtype=np.float64)) if M is not None else (lambda v: v)
    res = np.linalg.norm(r)
    for _ in range(maxiter):
        if res <= tol:
            break
        ph = prec(p)
        v = A @ ph
        napp += 1
        alpha = rho / (rhat @ v)
        s = r - alpha * v
        x = x + alpha * ph
        res = np.linalg.norm(s)
        if res <= tol:
            r = s
            break
        sh = prec(s)
        t = A @ sh
        napp += 1
        om = (t @ s) / (t @ t)
        x = x + om * sh
        r = s - om * t
        res = np.linalg.norm(r)
        rho_new = rhat @ r
        beta = (rho_new / rho) * (alpha / om)
        rho = rho_new
        p = r + beta * (p - om * v)
    return x, napp, res


def equilibrate(Ar: sp.spmatrix):
    """(Â, ds) of a reduced matrix: ds = |a_ii|^-1/2 (1 where a_ii = 0), Â = S A S.  A non-positive diagonal is kept (Â gets
    its sign there) so that build_hierarchy can refuse it."""
    Ar = sp.csr_matrix(Ar)
    d = Ar.diagonal()
    ds = np.where(d != 0.0, 1.0 / np.sqrt(np.abs(np.where(d != 0.0, d, 1.0))), 1.0)
    S = sp.diags(ds)
    return sp.csr_matrix(S @ Ar @ S), ds
