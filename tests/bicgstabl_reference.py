"""numpy restatement of the BiCGStab(l) iteration of penguin/jl_amd/csrc/pg_bicgstabl.hip (Sleijpen & Fokkema 1993), the
definition the GPU tests compare with -- as tests/mg_reference.py is for the multigrid.

One outer iteration is l BiCG sub-steps (two products each) followed by a minimal-residual step over the power basis
R[0..l] of the residual:

    sweep start       rho0 = -omega rho0;  restart pending (first sweep, breakdown, collapse, failed confirmation):
                      r~ := R[0], beta = 0, rho = (R[0], R[0])
    sub-step j        beta = alpha rho1 / rho0,  U[i] = R[i] - beta U[i]  (i <= j),  U[j+1] = A U[j],  sigma = (U[j+1], r~),
                      alpha = rho1 / sigma,  x += alpha U[0],  R[i] -= alpha U[i+1]  (i <= j),  iters += 1,
                      test on (R[0], R[0])_W,  R[j+1] = A R[j],  rho1 = (R[j+1], r~)
    breakdown         rho or sigma vanishes (or is not finite) inside a sweep: the rest of the sweep runs with alpha = beta = 0
                      -- R[0..l] stays the power basis of R[0], the minimal-residual step becomes one GMRES(l)-like step --
                      and the next sweep restarts.  At the first sub-step a vanishing rho restarts at once.
    minimal residual  G = Gram matrix of R[0..l];  the l x l system G[1:,1:] gamma = G[1:,0] by Cholesky with diagonal
                      pivoting; a pivot that is not > PIV_TOL times its diagonal entry shrinks the system to the next
                      smaller LEADING block (gamma_i = 0 beyond it), down to gamma_1 = G01 / G11;
                      x += sum gamma_i R[i-1],  R[0] -= sum gamma_i R[i],  U[0] -= sum gamma_i U[i],  omega = gamma_l
    restart rule      after the step: a breakdown in the sweep, a shrunk system, omega == 0, or
                      (r~, r)^2 < 1e-20 (r~, r~)(r, r)  -- the rule of the plain BiCGStab loop
    not finite        a residual norm that is not finite, or A R[0] = 0, ends the solve unconverged with x = 0: never NaN
    stopping          (R[0], R[0])_W <= max(reltol^2 (b, b)_W, abstol^2) -- W = weights^2, the units of x -- after a sub-step or
                      a minimal-residual step; then the TRUE residual b - A x is formed with one more product: accepted if
                      it meets the same test; otherwise the iteration continues from it (R[0] := true residual, restart),
                      at most MAX_CONTINUES times; after that the solve is reported unconverged
    counting          iters = BiCG sub-steps; products = 2 iters + confirmations; maxiter caps iters at sweep granularity
                      (no sweep starts at iters >= maxiter)
"""
import math

import numpy as np

PIV_TOL = 1e-13
MAX_CONTINUES = 3
MAX_L = 8


def small_solve(G, l):
    """gamma[0..l] (gamma[0] unused = 0) and the size k of the leading block that was solved (0: nothing safe)."""
    gamma = np.zeros(l + 1)
    for k in range(l, 0, -1):
        M = np.array(G[1:k + 1, 1:k + 1], dtype=np.float64)
        c = np.array(G[1:k + 1, 0], dtype=np.float64)
        d0 = np.diag(M).copy()
        perm = list(range(k))
        ok = True
        # right-looking Cholesky with diagonal pivoting, the right-hand side carried along (forward substitution)
        for s in range(k):
            p = s
            for q in range(s + 1, k):
                if M[q, q] > M[p, p]:
                    p = q
            if p != s:
                M[[s, p], :] = M[[p, s], :]
                M[:, [s, p]] = M[:, [p, s]]
                c[[s, p]] = c[[p, s]]
                d0[[s, p]] = d0[[p, s]]
                perm[s], perm[p] = perm[p], perm[s]
            piv = M[s, s]
            if not (piv > PIV_TOL * d0[s]) or not math.isfinite(piv):
                ok = False
                break
            root = math.sqrt(piv)
            M[s, s] = root
            c[s] = c[s] / root
            for q in range(s + 1, k):
                M[q, s] = M[q, s] / root
            for q in range(s + 1, k):
                for t in range(s + 1, q + 1):
                    M[q, t] -= M[q, s] * M[t, s]
                    M[t, q] = M[q, t]
                c[q] -= M[q, s] * c[s]
        if not ok:
            continue
        y = np.zeros(k)
        for s in range(k - 1, -1, -1):
            v = c[s]
            for q in range(s + 1, k):
                v -= M[q, s] * y[q]
            y[s] = v / M[s, s]
        if not np.all(np.isfinite(y)):
            continue
        for s in range(k):
            gamma[1 + perm[s]] = y[s]
        return gamma, k
    return gamma, 0


def bicgstabl_ref(A, b, l=2, reltol=1e-12, abstol=0.0, maxiter=100000, weights=None, confirm=True):
    """x, info.  info: iters, products, confirmations, continues, converged, resnorm (weighted; the TRUE one after a
    confirmation), bnorm, recurrence (the weighted recurrence residual that asked for the last confirmation), restarts.
    confirm=False: the recurrence residual is believed (diagnostics: what the confirmation protects from)."""
    if l <= 0:
        l = 2
    if l > MAX_L:
        raise ValueError("BiCGStab(l): l > 8 is refused")
    n = len(b)
    w2 = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64) ** 2
    x = np.zeros(n)
    R = np.zeros((l + 1, n))
    U = np.zeros((l + 1, n))
    R[0] = b
    rt = b.copy()
    bbw = float(np.sum(w2 * b * b))
    tol2 = max(reltol * reltol * bbw, abstol * abstol)
    rr = float(b @ b)
    rrw = bbw
    info = dict(iters=0, products=0, confirmations=0, continues=0, converged=False, resnorm=math.sqrt(bbw), bnorm=math.sqrt(bbw),
                recurrence=math.sqrt(bbw), restarts=0, singular=False)
    if bbw <= tol2:
        info["converged"] = True
        return x, info
    rho0, alpha, omega, rho1, rhat2 = 1.0, 0.0, 1.0, rr, rr
    restart = True
    iters = 0

    def confirmation():
        """True: the solve has ended (info filled); False: continue from the true residual."""
        nonlocal rr, rrw, restart
        info["recurrence"] = math.sqrt(rrw)
        if not confirm:
            info["converged"] = True
            info["resnorm"] = math.sqrt(rrw)
            return True
        r = b - A @ x
        info["confirmations"] += 1
        rrw_t = float(np.sum(w2 * r * r))
        info["resnorm"] = math.sqrt(rrw_t)
        if rrw_t <= tol2:
            info["converged"] = True
            return True
        if info["continues"] >= MAX_CONTINUES:
            return True
        info["continues"] += 1
        R[0] = r
        rr = float(r @ r)
        rrw = rrw_t
        restart = True
        return False

    ended = broken = False
    while not ended and iters < maxiter:
        rho0 = -omega * rho0
        force = False
        stopped = False
        for j in range(l):
            # scalar phase A
            if j == 0:
                if not restart and (rho0 == 0.0 or rho1 == 0.0 or not math.isfinite(rho0) or not math.isfinite(rho1)):
                    restart = True
                if restart:
                    rt = R[0].copy()
                    rho1 = rhat2 = rr
                    beta = 0.0
                    restart = False
                    info["restarts"] += 1
                else:
                    beta = alpha * (rho1 / rho0)
            else:
                if force or rho0 == 0.0 or rho1 == 0.0 or not math.isfinite(rho1):
                    force = True
                    beta = 0.0
                else:
                    beta = alpha * (rho1 / rho0)
            if not math.isfinite(beta):
                force, beta = True, 0.0
            rho0 = rho1
            if beta == 0.0:
                U[:j + 1] = R[:j + 1]
            else:
                U[:j + 1] = R[:j + 1] - beta * U[:j + 1]
            U[j + 1] = A @ U[j]
            sigma = float(U[j + 1] @ rt)
            # scalar phase B
            if force or sigma == 0.0 or not math.isfinite(sigma):
                force, alpha = True, 0.0
            else:
                alpha = rho0 / sigma
                if not math.isfinite(alpha):
                    force, alpha = True, 0.0
            x += alpha * U[0]
            R[:j + 1] -= alpha * U[1:j + 2]
            rrw = float(np.sum(w2 * R[0] * R[0]))
            iters += 1
            info["iters"] = iters
            if not math.isfinite(rrw):
                broken = stopped = True
                break
            if rrw <= tol2:
                if confirmation():
                    ended = True
                stopped = True
                break
            R[j + 1] = A @ R[j]
            rho1 = float(R[j + 1] @ rt)
        if broken:
            break
        if stopped:
            continue
        # minimal-residual step
        with np.errstate(all="ignore"):
            G = R @ R.T
        gamma, k = small_solve(G, l)
        if k == 0:
            broken = True                    # A R[0] = 0 (or not finite): nothing to minimise over
            break
        x += gamma[1:] @ R[:l]
        R[0] -= gamma[1:] @ R[1:]
        U[0] -= gamma[1:] @ U[1:]
        rr = float(R[0] @ R[0])
        rrw = float(np.sum(w2 * R[0] * R[0]))
        rho1 = float(R[0] @ rt)
        omega = float(gamma[l])
        info["resnorm"] = math.sqrt(rrw) if math.isfinite(rrw) else math.inf
        if not math.isfinite(rrw):
            broken = True
            break
        if rrw <= tol2:
            if confirmation():
                ended = True
            continue
        if force or k < l or omega == 0.0 or rho1 * rho1 < 1e-20 * rhat2 * rr:
            restart = True
    if broken:
        # a residual that is not finite, or A r = 0: the state is not handed back (never NaN)
        info["singular"] = True
        x = np.zeros(n)
        info["resnorm"] = info["bnorm"]
    elif not ended:
        info["resnorm"] = math.sqrt(rrw)     # maxiter: the recurrence residual, unconverged
    info["products"] = 2 * info["iters"] + info["confirmations"]
    return x, info


# ---- the systems the CPU tests and tests/golden/make_bicgstabl_products.py share ---------------------------------------------
def heat_system(n=16):
    """The oracle's cut-cell heat system of test_gmres_restatement_against_direct_solve_and_scipy (BE, disc r = 1 at (2.01, 2.01))."""
    from oracle import penguin_oracle as po
    from oracle.geometry import Ball
    mesh = po.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = po.make_capacity(Ball((2.01, 2.01), 1.0), mesh)
    M = (n + 1) ** 2
    ph = po.Phase(cap, po.make_diffusion_ops(cap), lambda x, y, z, t: 0.0, lambda x, y, z: 1.0)
    bcb = po.BorderConditions({k: po.Dirichlet(0.0) for k in ("left", "right", "top", "bottom")})
    s = po.DiffusionUnsteadyMono(ph, bcb, po.Dirichlet(1.0), 0.25 * (4.0 / n) ** 2, np.concatenate([np.zeros(M), np.ones(M)]), "BE")
    A, b, _ = po.remove_zero_rows_cols(s.A, s.b)
    return A.tocsr(), b


def peclet_system(n, kind):
    """The oracle's AdvectionDiffusionSteadyMono system inside the disc r = 1 at (2.01, 2.01) of the 4 x 4 box, f = D = 1,
    Dirichlet(1) interface, rows divided by their diagonal.  kind "rotation": rigid rotation of amplitude 100 about the centre;
    "uniform": the flow (100, 30).  Cell Peclet number |u| h = 12.5 at n = 32."""
    import scipy.sparse as sp
    from oracle import penguin_oracle as po
    from oracle.geometry import Ball
    mesh = po.Mesh((n, n), (4.0, 4.0), (0.0, 0.0))
    cap = po.make_capacity(Ball((2.01, 2.01), 1.0), mesh)
    M = (n + 1) ** 2
    x, y = cap.C_w[:, 0], cap.C_w[:, 1]
    u = [-100.0 * (y - 2.01), 100.0 * (x - 2.01)] if kind == "rotation" else [np.full(M, 100.0), np.full(M, 30.0)]
    op = po.make_convection_ops(cap, [np.ascontiguousarray(a) for a in u], np.zeros(2 * M))
    one = lambda x, y, z=0.0: 1.0
    bcb = po.BorderConditions({k: po.Dirichlet(0.0) for k in ("left", "right", "top", "bottom")})
    s = po.AdvectionDiffusionSteadyMono(po.Phase(cap, op, one, one), bcb, po.Dirichlet(1.0))
    A, b, _ = po.remove_zero_rows_cols(s.A, s.b)
    d = A.diagonal()
    return (sp.diags(1.0 / d) @ A).tocsr(), b / d
