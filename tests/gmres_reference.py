"""numpy restatement of the restarted GMRES of penguin/jl_amd/csrc/pg_gmres.hip, the definition the GPU tests compare with -- as
tests/bicgstabl_reference.py is for BiCGStab(l) and tests/idrs_reference.py for IDR(s).  It restates what gmres_solve does, not what
IterativeSolvers does (that is po.gmres_ref: modified Gram-Schmidt); the device performs the same operations in the same order.

    sizes        m = min(restart or 20, 200, n);  maxiter <= 0: 100000
    start        x = 0, r = b;  rr = (r, r), rrw = (r, r)_W, W = weights^2;  tol2 = max(reltol^2 rr, abstol^2) -- the INNER tolerance,
                 on the Givens estimate;  tolw2 = max(reltol^2 rrw, abstol^2) -- the acceptance;  both compared on squares
    begin        (pghost::gm_begin) verdict on the true residual: rrw <= tolw2 or rr = 0 -> converged.  Otherwise g = (|r|, 0, ..),
                 v_0 = r (1 / |r|), and -- not at the start -- the inner tolerance is lowered to 0.25 rr tolw2 / rrw when that is smaller
    step j       w = A v_j;  h1_i = (v_i, w), i <= j, all against the same w;  w -= sum h1_i v_i;  h2_i = (v_i, w);  w -= sum h2_i v_i;
                 nn = (w, w)  -- classical Gram-Schmidt applied twice
    hess         (pghost::gm_hess) H[:j+1, j] = h1 + h2, H[j+1, j] = hn = sqrt(max(nn, 0)); the rotations 0 .. j-1; d = hypot(H[j, j], hn);
                 iters += 1;  d = 0 -> SINGULAR: the cycle keeps its J = j columns and the solve ends unconverged.  Otherwise the new
                 rotation, g[j+1] = -sn g[j];  g[j+1]^2 <= tol2 or hn = 0 (the Krylov space is EXHAUSTED) ends the CYCLE -- never the
                 solve;  v_{j+1} = w (1 / hn)
    cycle end    y = the back substitution on H[:J, :J] (pghost::gm_solve_y);  x += sum y_k v_k;  r = b - A x;  begin
    counting     iters = Arnoldi steps, the unit maxiter caps: a cycle runs min(m, maxiter - iters) steps and the solve ends at
                 iters >= maxiter
    not finite   rr or rrw at a begin, or an entry of h1 + h2 or nn at a step, that is NaN or Inf ends the solve unconverged with
                 x = 0: never NaN
"""
import math

import numpy as np

MAX_RESTART = 200
DONE_NO, DONE_CONVERGED, DONE_STOPPED, DONE_CYCLE = 0, 1, 2, 3   # the values of the device's done flag


class GmScalars:
    """The scalar block of one solve: what pghost::gm_begin / gm_hess / gm_solve_y keep in `gm` and `sc`."""

    def __init__(self, m, reltol, abstol):
        self.m = m
        self.H = np.zeros((m + 1, m))
        self.cs, self.sn, self.g, self.y = np.zeros(m), np.zeros(m), np.zeros(m + 1), np.zeros(m)
        self.J = 0
        self.invn = 0.0
        self.reltol2, self.abstol2 = reltol * reltol, abstol * abstol
        self.tol2 = self.tolw2 = self.bb = self.rr0 = self.rrw = 0.0
        self.done = DONE_NO
        self.iters = 0
        self.notfinite = False
        self.exhausted = False
        self.just_lowered = False

    def begin(self, rr, rrw, first):
        if first:
            self.bb, self.rr0, self.iters = rrw, rr, 0
            t2 = self.reltol2 * rr
            self.tol2 = t2 if t2 > self.abstol2 else self.abstol2
            tw = self.reltol2 * rrw
            self.tolw2 = tw if tw > self.abstol2 else self.abstol2
        self.rrw = rrw
        self.just_lowered = False
        finite = math.isfinite(rr) and math.isfinite(rrw)
        beta = math.sqrt(rr) if finite and rr > 0.0 else 0.0
        self.g[:] = 0.0
        self.g[0] = beta
        self.J = 0
        self.invn = 1.0 / beta if beta > 0.0 else 0.0
        if not finite:
            self.done, self.notfinite = DONE_STOPPED, True
            return
        if self.done == DONE_STOPPED:
            return
        ok = rrw <= self.tolw2 or beta == 0.0
        self.done = DONE_CONVERGED if ok else DONE_NO
        if not ok and not first and rrw > 0.0:
            aim = 0.25 * rr * (self.tolw2 / rrw)
            if aim < self.tol2:
                self.tol2 = aim
                self.just_lowered = True

    def hess(self, j, h1, h2, nn):
        if self.done != DONE_NO:
            return
        H, cs, sn, g = self.H, self.cs, self.sn, self.g
        finite = math.isfinite(nn)
        for i in range(j + 1):
            H[i, j] = h1[i] + h2[i]
            finite = finite and math.isfinite(H[i, j])
        hn = math.sqrt(nn) if nn > 0.0 else 0.0
        H[j + 1, j] = hn
        self.iters += 1
        if not finite:
            self.J, self.done, self.notfinite = j, DONE_STOPPED, True
            return
        for i in range(j):
            a, b = H[i, j], H[i + 1, j]
            H[i, j] = cs[i] * a + sn[i] * b
            H[i + 1, j] = -sn[i] * a + cs[i] * b
        a = H[j, j]
        d = math.hypot(a, hn)
        self.J = j + 1
        if d == 0.0:
            self.J, self.done = j, DONE_STOPPED
            return
        c, s = a / d, hn / d
        cs[j], sn[j] = c, s
        H[j, j], H[j + 1, j] = d, 0.0
        gj = g[j]
        g[j] = c * gj
        g[j + 1] = -s * gj
        rr = g[j + 1] * g[j + 1]
        self.invn = 1.0 / hn if hn > 0.0 else 0.0
        if hn == 0.0:
            self.exhausted = True
        if rr <= self.tol2 or hn == 0.0:
            self.done = DONE_CYCLE

    def solve_y(self):
        H, g, y = self.H, self.g, self.y
        for i in range(self.J - 1, -1, -1):
            s = g[i]
            for k in range(i + 1, self.J):
                s -= H[i, k] * y[k]
            y[i] = s / H[i, i]


def gmres_dev_ref(A, b, restart=0, reltol=1e-12, abstol=0.0, maxiter=0, weights=None, long_sums=False, trace=None):
    """x, info.  info: iters, cycles, lowered (cycles that started with a lowered inner tolerance), converged, singular, exhausted,
    notfinite, resnorm (weighted, of the true residual at the last restart), bnorm.
    long_sums: every dot product and every row sum of a product with A accumulates in np.longdouble (the yardstick of the GPU
    tests: what the order of summation is worth).
    trace: a list that receives the scalar inputs of every kernel in order -- ("begin", rr, rrw, first), ("hess", j, h1, h2, nn),
    ("solve",) -- what tests/gmres_host.cpp replays."""
    A = A.tocsr()
    b = np.asarray(b, dtype=np.float64)
    n = len(b)
    m = min(restart if restart > 0 else 20, MAX_RESTART)
    if n > 0:
        m = min(m, n)
    if maxiter <= 0:
        maxiter = 100000
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

    sc = GmScalars(m, reltol, abstol)
    x = np.zeros(n)
    V = np.zeros((m + 1, n))
    note = trace.append if trace is not None else (lambda item: None)

    def begin(first):
        r = b.copy() if first else b - mul(x)
        rr, rrw = dot(r, r), wdot(r)
        note(("begin", rr, rrw, first))
        sc.begin(rr, rrw, first)
        V[0] = r * sc.invn if sc.done == DONE_NO else r

    cycles = lowered = 0
    with np.errstate(all="ignore"):
        begin(True)
        while True:
            steps = max(0, min(m, maxiter - sc.iters))
            low = sc.just_lowered
            for j in range(steps):
                if sc.done != DONE_NO:
                    break
                if j == 0:
                    cycles += 1
                    lowered += low
                w = mul(V[j])
                h1 = np.array([dot(V[i], w) for i in range(j + 1)])
                for i in range(j + 1):
                    w = w - h1[i] * V[i]
                h2 = np.array([dot(V[i], w) for i in range(j + 1)])
                for i in range(j + 1):
                    w = w - h2[i] * V[i]
                nn = dot(w, w)
                note(("hess", j, h1, h2, nn))
                sc.hess(j, h1, h2, nn)
                V[j + 1] = w * sc.invn if sc.done == DONE_NO else w
            note(("solve",))
            sc.solve_y()
            for k in range(sc.J):
                x = x + sc.y[k] * V[k]
            begin(False)
            if sc.done in (DONE_CONVERGED, DONE_STOPPED) or sc.iters >= maxiter or steps == 0:
                break
    bnorm = math.sqrt(sc.bb) if math.isfinite(sc.bb) else math.inf
    info = dict(iters=sc.iters, cycles=cycles, lowered=lowered, converged=sc.done == DONE_CONVERGED,
                singular=sc.done == DONE_STOPPED and not sc.notfinite, exhausted=sc.exhausted, notfinite=sc.notfinite,
                resnorm=math.sqrt(sc.rrw) if math.isfinite(sc.rrw) else math.inf, bnorm=bnorm)
    if sc.notfinite:
        x = np.zeros(n)              # the state is not handed back
        info["resnorm"] = bnorm
    return x, info


# ---- the systems of the CPU tests ---------------------------------------------------------------------------------------------
from tests.bicgstabl_reference import heat_system, peclet_system  # noqa: E402,F401


def symmetric_scaling(A, b):
    """S A S, S b and S = |a_ii|^-1/2: the oracle's stand-in for the device's Â (without its B⁻¹)."""
    import scipy.sparse as sp
    S = 1.0 / np.sqrt(np.abs(A.diagonal()))
    return (sp.diags(S) @ A @ sp.diags(S)).tocsr(), S * b, S


def small_box_system(box=0.04, n=16):
    """Heat BE on a box of `box` x `box`, n^2 cells, disc r = box / 4 at 0.5025 box, dt = 0.25 h^2, interface Dirichlet(1),
    borders Dirichlet(0), T = 0 inside: the rows differ by 1 / h in scale, so the un-weighted Givens estimate meets reltol while the
    residual in the units of x does not -- the case that reaches the tolerance-lowering branch.  -> S A S, S b, S."""
    from oracle import penguin_oracle as po
    from oracle.geometry import Ball
    mesh = po.Mesh((n, n), (box, box), (0.0, 0.0))
    cap = po.make_capacity(Ball((0.5025 * box, 0.5025 * box), 0.25 * box), mesh)
    M = (n + 1) ** 2
    ph = po.Phase(cap, po.make_diffusion_ops(cap), lambda x, y, z, t: 0.0, lambda x, y, z: 1.0)
    bcb = po.BorderConditions({k: po.Dirichlet(0.0) for k in ("left", "right", "top", "bottom")})
    s = po.DiffusionUnsteadyMono(ph, bcb, po.Dirichlet(1.0), 0.25 * (box / n) ** 2, np.concatenate([np.zeros(M), np.ones(M)]), "BE")
    A, b, _ = po.remove_zero_rows_cols(s.A, s.b)
    return symmetric_scaling(A.tocsr(), b)
