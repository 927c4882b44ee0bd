"""Restatement (numpy) of the spectral estimate behind precond="poly-est" (PG_PRECOND_POLY_EST, csrc/pg_specest.hip), as
DESIGN.md section 16 defines it.  Test infrastructure: tests/test_specest_reference.py runs it on the oracle's systems,
tests/test_gpu_specest.py compares the library with it.

  start      v0[i] = cos(1 + (12.9898 * 0.7548776662) * i), normalised
  Arnoldi    m = 30 steps on Â, classical Gram-Schmidt applied twice: h1 = Vᵀw, w -= V h1, h2 = Vᵀw, w -= V h2, h = h1 + h2,
             h[j+1, j] = ||w||; a happy breakdown (h[j+1, j] <= 1e-14) ends the recursion with the Ritz values reached
  Ritz       eigenvalues θ of H[:k, :k];  g_ritz = max |θ - 1|  (complex modulus)
  rule       g_used = g_ritz + margin;  admitted when g_used < 0.95
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

STEPS = 30
BREAKDOWN = 1e-14
BOUND = 0.95
START_FREQ = 12.9898 * 0.7548776662


def start_vector(n: int, dtype=np.float64) -> np.ndarray:
    """the argument is formed in float64 whatever `dtype` is (the library has no other format); only the sums differ"""
    arg = 1.0 + START_FREQ * np.arange(n, dtype=np.float64)
    v = np.cos(arg).astype(dtype)
    return v / np.sqrt(v @ v)


def _matvec(A: sp.csr_matrix, x: np.ndarray, dtype) -> np.ndarray:
    if dtype == np.float64:
        return A @ x
    y = np.zeros(A.shape[0], dtype=dtype)      # scipy has no long double: one row at a time
    indptr, indices, data = A.indptr, A.indices, A.data.astype(dtype)
    prod = data * x[indices]
    np.add.at(y, np.repeat(np.arange(A.shape[0]), np.diff(indptr)), prod)
    return y


def arnoldi(A: sp.spmatrix, m: int = STEPS, dtype=np.float64):
    """(H, k): the (m+1) x m Hessenberg matrix (columns >= k are zero) and the steps taken"""
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    n = A.shape[0]
    m = min(m, n)
    V = np.zeros((m + 1, n), dtype=dtype)
    H = np.zeros((m + 1, m), dtype=dtype)
    V[0] = start_vector(n, dtype)
    k = 0
    for j in range(m):
        w = _matvec(A, V[j], dtype)
        h1 = V[: j + 1] @ w
        w = w - h1 @ V[: j + 1]
        h2 = V[: j + 1] @ w
        w = w - h2 @ V[: j + 1]
        H[: j + 1, j] = h1 + h2
        hn = np.sqrt(w @ w)
        H[j + 1, j] = hn
        k = j + 1
        if hn <= BREAKDOWN:
            break
        V[j + 1] = w / hn
    return H, k


def ritz_values(H: np.ndarray, k: int) -> np.ndarray:
    return np.linalg.eigvals(np.asarray(H[:k, :k], dtype=np.float64))


def estimate(A: sp.spmatrix, margin: float, m: int = STEPS, dtype=np.float64) -> dict:
    H, k = arnoldi(A, m, dtype)
    th = ritz_values(H, k)
    g_ritz = float(np.max(np.abs(th - 1.0)))
    g_used = g_ritz + margin
    return {"H": np.asarray(H, dtype=np.float64), "steps": k, "ritz": th, "g_ritz": g_ritz, "g_used": g_used, "margin": margin,
            "admitted": bool(g_used < BOUND), "re_min": float(th.real.min()), "re_max": float(th.real.max()),
            "im_max": float(np.abs(th.imag).max())}


def gershgorin_radius(A: sp.spmatrix) -> float:
    """the largest Gershgorin radius of I - Â, centre included: max_i (|1 - a_ii| + Σ_{j != i} |a_ij|)"""
    A = sp.csr_matrix(A)
    d = A.diagonal()
    off = np.asarray(abs(A).sum(axis=1)).ravel() - np.abs(d)
    return float(np.max(np.abs(1.0 - d) + off))


class Chebyshev:
    """q(Â) with 1 - λ q(λ) the scaled Chebyshev polynomial of degree m on [1 - g, 1 + g]: the Horner chain of pg_krylov.hip
    (roots taken from both ends in turn).  Counts the products with Â."""

    def __init__(self, A: sp.csr_matrix, g: float, m: int):
        lam = 1.0 + g * np.cos(np.pi * (2.0 * np.arange(m) + 1.0) / (2.0 * m))
        lo, hi, tau = 0, m - 1, []
        for k in range(m):
            if k & 1:
                tau.append(1.0 / lam[hi]); hi -= 1
            else:
                tau.append(1.0 / lam[lo]); lo += 1
        self.A, self.tau, self.products = A, tau, 0

    def __call__(self, v: np.ndarray) -> np.ndarray:
        tau = self.tau
        u = tau[-1] * v
        for k in range(len(tau) - 2, -1, -1):
            u = tau[k] * v + u - tau[k] * (self.A @ u)
            self.products += 1
        return u
