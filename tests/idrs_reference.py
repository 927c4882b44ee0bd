"""numpy restatement of the IDR(s) iteration of penguin/jl_amd/csrc/pg_idrs.hip (IDR(s) with biorthogonalisation: van Gijzen &
Sonneveld, ACM TOMS 38 (2011), Alg. 1), the definition the GPU tests compare with -- as tests/bicgstabl_reference.py is for
BiCGStab(l).  The device performs the same operations in the same order.

    start        r = b - A x0 (x0 absent: r = b, x = 0);  G = U = 0 (s vectors each);  M = I_s;  omega = 1;  f = P^T r
    cycle, k = 0 .. s-1
                 c = solution of the lower-triangular  M[k:, k:] c = f[k:]
                 U[k] = omega (r - sum_{i>=k} c_i G[i]) + sum_{i>=k} c_i U[i]
                 G[k] = A U[k]
                 h_i = (p_i, G[k]), i = 0 .. s-1, and (G[k], G[k]) -- one pass over G[k]
                 alpha = solution of  M[:k, :k] alpha = h[:k];  G[k] -= sum_{i<k} alpha_i G[i];  U[k] -= sum_{i<k} alpha_i U[i]
                 M[i, k] = h_i - sum_{j<k} M[i, j] alpha_j  (i >= k) -- from scalars: (p_i, G[j]) = M[i, j] is known
                 beta = f_k / M[k, k];  f_i -= beta M[i, k] (i > k);  r -= beta G[k];  x += beta U[k];  iters += 1;  stopping test
    then         t = A r;  omega = (t, r) / (t, t), enlarged by kappa / rho when rho = |(t, r)| / (|t| |r|) < kappa = 0.7
                 x += omega r;  r -= omega t;  iters += 1;  stopping test;  f = P^T r
    shadow       p_k[i] = shadow(i, k): a pure integer function of the row number and k (never stored on the device), the
                 splitmix64 finaliser of i + (k + 1) 0x9E3779B97F4A7C15 mapped to (z >> 11) 2^-52 - 1 in [-1, 1): exact in fp64.
                 P is not orthogonalised (as in IterativeSolvers).
    breakdown    M[k, k] not finite or |M[k, k]| <= PIV_TOL |p_k| |G[k]| (G[k] as the product left it: the scale of the rounding
                 of h_k), a c that is not finite, (t, t) = 0, (t, r) = 0, or a residual that is not finite: RESTART -- G = U = 0,
                 M = I, omega = 1 and r := the true residual b - A x (one product).  At most MAX_RESTARTS, then unconverged.
    stopping     (r, r)_W <= max(reltol^2 (b, b)_W, abstol^2), W = weights^2.  When the recurrence residual meets it the TRUE
                 residual is formed (one product) and decides: met -> converged with the true norm reported; not met -> the
                 iteration continues from it as after a restart, at most MAX_CONTINUES times, then unconverged.  A true
                 residual formed by a restart that meets the test ends the solve converged as well.
    not finite   a true residual that is not finite ends the solve unconverged with x = 0: never NaN
    counting     iters = updates of x, one product each -- the unit maxiter caps: no update starts at iters >= maxiter
                 (maxiter <= 0: 200000);  products = iters + restarts + confirmations (+ 1 when started from an x0)
"""
import math

import numpy as np

MAX_S = 8
MAX_CONTINUES = 3
MAX_RESTARTS = 16
PIV_TOL = 1e-15      # ~ 9 eps: below it M[k, k] has no correct digit left (the rounding of its own dot product)
KAPPA = 0.7
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def shadow(i, k):
    """p_k[i] for an array (or scalar) of row numbers i: bit-identical to pghost::idr_shadow."""
    with np.errstate(over="ignore"):
        z = np.asarray(i, dtype=np.uint64) + np.uint64(k + 1) * _GOLDEN
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -52 - 1.0


def lower_solve(M, lo, hi, rhs):
    """out[lo:hi] of the forward substitution M[lo:hi, lo:hi] out = rhs[lo:hi] (zero elsewhere), and whether every entry
    is finite -- pghost::idr_lower_solve."""
    s = M.shape[0]
    out = np.zeros(s)
    ok = True
    with np.errstate(all="ignore"):
        for i in range(lo, hi):
            v = rhs[i]
            for j in range(lo, i):
                v -= M[i, j] * out[j]
            out[i] = v / M[i, i]
            if not math.isfinite(out[i]):
                ok = False
    if not ok:
        out[:] = 0.0
    return out, ok


def idrs_ref(A, b, s=8, reltol=1e-12, abstol=0.0, maxiter=0, weights=None, x0=None, long_sums=False):
    """x, info.  info: iters, products, confirmations, restarts, continues, converged, resnorm (weighted; the TRUE one after a
    confirmation), bnorm, singular, breakdowns (what asked for each restart: "c", "pivot", "beta", "residual", "t", "omega").
    long_sums: every dot product and every row sum of a product with A accumulates in np.longdouble (the yardstick of the GPU tests: what the order of summation is worth)."""
    if s <= 0:
        s = 8
    if s > MAX_S:
        raise ValueError("IDR(s): s > 8 is refused")
    if maxiter <= 0:
        maxiter = 200000
    A = A.tocsr()
    b = np.asarray(b, dtype=np.float64)
    n = len(b)
    w2 = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64) ** 2
    acc = np.longdouble if long_sums else np.float64

    def dot(u, v):
        return float(np.sum(u.astype(acc) * v.astype(acc)))

    def wdot(u):
        return float(np.sum(w2.astype(acc) * u.astype(acc) * u.astype(acc)))

    if long_sums:
        data, idx, ptr = A.data.astype(acc), A.indices, A.indptr
        nonempty = np.flatnonzero(np.diff(ptr) > 0)

        def mul(v):
            out = np.zeros(n)
            if len(nonempty):
                out[nonempty] = np.add.reduceat(data * v.astype(acc)[idx], ptr[nonempty]).astype(np.float64)
            return out
    else:
        def mul(v):
            return A @ v

    P = np.array([shadow(np.arange(n), k) for k in range(s)])
    pp = [dot(P[k], P[k]) for k in range(s)]
    info = dict(iters=0, products=0, confirmations=0, restarts=0, continues=0, converged=False, singular=False, breakdowns=[])
    if x0 is None:
        x = np.zeros(n)
        r = b.copy()
    else:
        x = np.array(x0, dtype=np.float64)
        r = b - mul(x)
        info["products"] = 1
    bbw = wdot(b)
    tol2 = max(reltol * reltol * bbw, abstol * abstol)
    info["bnorm"] = math.sqrt(bbw) if math.isfinite(bbw) else math.inf
    rrw = wdot(r)
    G = np.zeros((s, n))
    U = np.zeros((s, n))
    M = np.eye(s)
    state = dict(omega=1.0, f=np.array([dot(P[k], r) for k in range(s)]))

    def finish(flag):
        info["products"] += info["iters"] + info["restarts"] + info["confirmations"]
        info["resnorm"] = math.sqrt(rrw) if math.isfinite(rrw) else math.inf
        if flag == "singular":
            info["singular"] = True
            info["resnorm"] = info["bnorm"]
            return np.zeros(n), info
        info["converged"] = flag == "converged"
        return x, info

    if not math.isfinite(rrw) or not math.isfinite(bbw):
        return finish("singular")
    if rrw <= tol2:
        return finish("converged")          # (the start residual is a true residual: nothing to confirm)

    def true_residual(kind):
        """kind "confirm" / "restart" -> None (the iteration continues from the true residual) or the flag the solve ends with."""
        nonlocal r, rrw
        r = b - mul(x)
        rrw = wdot(r)
        info["confirmations" if kind == "confirm" else "restarts"] += 1
        if not math.isfinite(rrw):
            return "singular"
        if rrw <= tol2:
            return "converged"
        if kind == "confirm":
            if info["continues"] >= MAX_CONTINUES:
                return "gave up"
            info["continues"] += 1
        elif info["restarts"] > MAX_RESTARTS:
            return "gave up"
        G[:] = 0.0
        U[:] = 0.0
        M[:] = np.eye(s)
        state["omega"] = 1.0
        state["f"] = np.array([dot(P[k], r) for k in range(s)])
        return None

    def why(reason):
        info["breakdowns"].append(reason)
        return "restart"

    def cycle():
        """None (a full cycle ran), "confirm" / "restart" (a true residual is asked for) or "maxiter"."""
        nonlocal r, rrw, x
        f = state["f"]
        for k in range(s):
            if info["iters"] >= maxiter:
                return "maxiter"
            c, ok = lower_solve(M, k, s, f)
            if not ok:
                return why("c")
            omega = state["omega"]
            v = r.copy()
            for i in range(k, s):
                v -= c[i] * G[i]
            u = omega * v
            for i in range(k, s):
                u += c[i] * U[i]
            U[k] = u
            G[k] = mul(U[k])
            h = np.array([dot(P[i], G[k]) for i in range(s)])
            gg = dot(G[k], G[k])
            alpha, ok = lower_solve(M, 0, k, h)
            for i in range(k, s):
                v_ = h[i]
                for j in range(k):
                    v_ -= M[i, j] * alpha[j]
                M[i, k] = v_
            mkk = M[k, k]
            if not ok or not math.isfinite(mkk) or not math.isfinite(gg) or abs(mkk) <= PIV_TOL * math.sqrt(pp[k] * gg):
                return why("pivot")
            beta = f[k] / mkk
            if not math.isfinite(beta):
                return why("beta")
            for i in range(k + 1, s):
                f[i] -= beta * M[i, k]
            f[k] = 0.0
            g = G[k].copy()
            u = U[k].copy()
            for i in range(k):
                g -= alpha[i] * G[i]
                u -= alpha[i] * U[i]
            G[k] = g
            U[k] = u
            r = r - beta * g
            x = x + beta * u
            rrw = wdot(r)
            info["iters"] += 1
            if not math.isfinite(rrw):
                return why("residual")
            if rrw <= tol2:
                return "confirm"
        if info["iters"] >= maxiter:
            return "maxiter"
        t = mul(r)
        tr, tt, rr = dot(t, r), dot(t, t), dot(r, r)
        if tt == 0.0 or tr == 0.0 or not math.isfinite(tt) or not math.isfinite(tr) or not math.isfinite(rr):
            return why("t")
        rho = abs(tr) / math.sqrt(tt * rr)
        if not rho > 0.0:                    # (t, r) negligible against |t| |r| (or |t|^2 |r|^2 beyond the range): no ω to take
            return why("t")
        omega = tr / tt
        if rho < KAPPA:
            omega *= KAPPA / rho
        if not math.isfinite(omega) or omega == 0.0:
            return why("omega")
        state["omega"] = omega
        x = x + omega * r
        r = r - omega * t
        rrw = wdot(r)
        state["f"] = np.array([dot(P[k], r) for k in range(s)])
        info["iters"] += 1
        if not math.isfinite(rrw):
            return why("residual")
        if rrw <= tol2:
            return "confirm"
        return None

    with np.errstate(all="ignore"):
        while True:
            ask = cycle()
            if ask == "maxiter":
                return finish("maxiter")
            if ask is not None:
                flag = true_residual(ask)
                if flag is not None:
                    return finish(flag)


# the systems shared with the BiCGStab(l) tests
from tests.bicgstabl_reference import heat_system, peclet_system  # noqa: E402,F401
