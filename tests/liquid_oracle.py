"""Literal CPU restatement of the reference's 1-D liquid-motion (Stefan) solvers, src/liquidmotionsolver/diffusion.jl:
the learning-rate state (:3-136), adapt_timestep (src/solver.jl:611-662), the Stefan terms of a solved slab (:240-255,
height_tracking.jl:23-31), A_/b_diph_unstead_diff_moving_stef (:445-651) and both solve loops (:173-442, :675-946).

Test infrastructure only: built on oracle/spacetime.py (the moving blocks) and oracle/penguin_oracle.py (direct solves).
The loops take a `capacity_fn(xf0, xf1, t0, t1, static)` that returns the oracle capacity (mono) or the pair (diph) of the
body x - (xf0 (t1 - t)/Δt + xf1 (t - t0)/Δt) on [t0, t1] (static: the body x - xf0 of a step's start); the GPU tests pass the capacities
the HIP path computed for that xf, so that the algebra and the loop logic are compared on identical geometry."""
from __future__ import annotations

import math
from typing import Callable, Optional

import numpy as np
import scipy.sparse as sp

from oracle import penguin_oracle as po
from oracle import spacetime as ost


# ------------------------------------------------------------------------------------------------- learning rate :3-136
class LRState:
    def __init__(self, strategy, base_lr, eps=1e-8, beta1=0.9, beta2=0.999, decay=0.0, min_lr=0.0, max_lr=math.inf):
        s = str(strategy).lower()
        s = {"constant": "fixed", "none": "fixed", "bb": "barzilai_borwein", "barzilaiborwein": "barzilai_borwein",
             "barzilai-borwein": "barzilai_borwein", "rms_prop": "rmsprop"}.get(s, s)
        self.strategy, self.base_lr, self.eps, self.beta1, self.beta2, self.decay = s, base_lr, eps, beta1, beta2, decay
        self.grad_accum = self.mean_grad_sq = self.m = self.v = 0.0
        self.t = 0
        self.prev_xf = self.prev_grad = None
        self.min_lr, self.max_lr = min_lr, max(max_lr, min_lr)
        self.last_lr = base_lr


def jclamp(x, lo, hi):
    """Base.clamp: ifelse(x > hi, hi, ifelse(x < lo, lo, x))."""
    if x > hi:
        return hi
    if x < lo:
        return lo
    return x


def jsign(x):
    return x if x == 0 or x != x else (1.0 if x > 0 else -1.0)


def lr_step(st: LRState, current_xf: float, grad: float) -> float:
    """apply_learning_rate_step! (:43-122)."""
    st.t += 1
    base_lr = st.base_lr / (1 + st.decay * (st.t - 1)) if st.decay > 0 else st.base_lr
    lr, direction, custom = base_lr, grad, None
    if st.strategy == "adagrad":
        st.grad_accum += grad * grad
        lr = base_lr / (math.sqrt(st.grad_accum) + st.eps)
    elif st.strategy == "rmsprop":
        st.mean_grad_sq = st.beta2 * st.mean_grad_sq + (1 - st.beta2) * grad * grad
        lr = base_lr / (math.sqrt(st.mean_grad_sq) + st.eps)
    elif st.strategy == "nadam":
        st.m = st.beta1 * st.m + (1 - st.beta1) * grad
        st.v = st.beta2 * st.v + (1 - st.beta2) * grad * grad
        bc1 = max(1 - st.beta1 ** st.t, st.eps)
        bc2 = max(1 - st.beta2 ** st.t, st.eps)
        m_hat, v_hat = st.m / bc1, st.v / bc2
        lr = base_lr / (math.sqrt(v_hat) + st.eps)
        direction = st.beta1 * m_hat + (1 - st.beta1) * grad / bc1
    elif st.strategy == "barzilai_borwein":
        if st.prev_xf is not None and st.prev_grad is not None:
            dx, dg = current_xf - st.prev_xf, grad - st.prev_grad
            denom = dg * dg if abs(dg) > st.eps else 0.0
            if denom > 0:
                lr = abs(dx * dg) / denom
    elif st.strategy == "secant":
        if st.prev_xf is not None and st.prev_grad is not None:
            dx, dg = current_xf - st.prev_xf, grad - st.prev_grad
            if abs(dg) > st.eps:
                prop = -grad * (dx / dg)
                if grad == 0.0:
                    custom, lr = prop, st.base_lr
                else:
                    max_step, min_step = st.max_lr * abs(grad), st.min_lr * abs(grad)
                    if math.isfinite(max_step):
                        prop = jclamp(prop, -max_step, max_step)
                    if min_step > 0:
                        if abs(prop) < min_step:
                            prop = jsign(prop) * min_step
                    custom = prop
                    lr = abs(prop) / max(abs(grad), st.eps)
    if custom is None:
        lr = jclamp(lr, st.min_lr, st.max_lr)
        step = lr * direction
    else:
        step = custom
    if not math.isfinite(step):
        step = 0.0
    st.prev_xf, st.prev_grad, st.last_lr = current_xf, grad, lr
    return step


# ------------------------------------------------------------------------------------------ adapt_timestep solver.jl:611-662
def adapt_timestep(velocity_field, nodes, cfl_target, dt, dt_min, dt_max, growth_factor=1.1, shrink_factor=0.8,
                   safety_factor=0.9):
    v_max = max(abs(v) for v in np.atleast_1d(velocity_field))
    if v_max < 1e-10:
        return min(dt * growth_factor, dt_max), 0.0
    dh = min(min(np.diff(np.asarray(n))) for n in nodes)
    opt = safety_factor * cfl_target * dh / v_max
    if opt > dt:
        new = min(opt, dt * shrink_factor)
    else:
        new = max(opt, dt * growth_factor)
    new = jclamp(new, dt_min, dt_max)
    return new, v_max * new / dh


# ------------------------------------------------------------------------------------------------- Stefan terms :240-255
def stefan_terms(op: po.DiffusionOps, cap: po.Capacity, D, Ti: np.ndarray):
    """(Hₙ₊₁, Hₙ, Σq, max|q|) of one phase, Ti = its [Tω; Tγ] (2M); q = Id Hᵀ Wꜝ G Tω + Id Hᵀ Wꜝ H Tγ."""
    Vn_1, Vn = ost._time_faces(op, cap)
    Wi, G, H = ost._half(op.Winv), ost._half(op.G), ost._half(op.H)
    Id = ost._half(sp.diags(po.build_I_D(op, D, cap)))
    M = len(Ti) // 2
    To, Tg = Ti[:M], Ti[M:]
    HT = H.T.tocsr()
    q = Id @ (HT @ (Wi @ (G @ To))) + Id @ (HT @ (Wi @ (H @ Tg)))
    return float(np.sum(Vn_1)), float(np.sum(Vn)), float(np.sum(q)), float(np.max(np.abs(q)))


# ------------------------------------------------------------------------------------ Stefan diphasic blocks :445-651
def A_diph_unstead_diff_moving_stef(op1, op2, cap1, cap2, D1, D2, ic: po.InterfaceConditions, scheme: str) -> sp.csr_matrix:
    jump = ic.scalar
    Vn1_1, Vn1 = ost._time_faces(op1, cap1)
    Vn2_1, Vn2 = ost._time_faces(op2, cap2)
    psip = ost.psip_cn if scheme == "CN" else ost.psip_be
    Psi1 = sp.diags(np.array([psip(a, b) for a, b in zip(Vn1, Vn1_1)]))
    Psi2 = sp.diags(np.array([psip(a, b) for a, b in zip(Vn2, Vn2_1)]))
    n = len(Vn1)
    Ia1, Ia2 = jump.alpha1 * sp.identity(n), jump.alpha2 * sp.identity(n)
    W1, G1, H1 = ost._half(op1.Winv), ost._half(op1.G), ost._half(op1.H)
    W2, G2, H2 = ost._half(op2.Winv), ost._half(op2.G), ost._half(op2.H)
    Id1, Id2 = ost._half(sp.diags(po.build_I_D(op1, D1, cap1))), ost._half(sp.diags(po.build_I_D(op2, D2, cap2)))
    G1T, G2T = G1.T.tocsr(), G2.T.tocsr()
    block1 = sp.diags(Vn1_1) + Id1 @ G1T @ W1 @ G1 @ Psi1                                     # :519-522
    block2 = -(sp.diags(Vn1_1) - sp.diags(Vn1)) + Id1 @ G1T @ W1 @ H1 @ Psi1
    block3 = sp.diags(Vn2_1) + Id2 @ G2T @ W2 @ G2 @ Psi2
    block4 = -(sp.diags(Vn2_1) - sp.diags(Vn2)) + Id2 @ G2T @ W2 @ H2 @ Psi2
    Z = sp.csr_matrix((n, n))
    return sp.bmat([[block1, block2, Z, Z], [Z, Ia1, Z, -Ia2], [Z, Z, block3, block4], [Z, Z, Z, Ia2]], format="csr")   # :534-542


def b_diph_unstead_diff_moving_stef(op1, op2, cap1, cap2, D1, D2, f1, f2, ic: po.InterfaceConditions, Ti, dt, t,
                                    scheme: str) -> np.ndarray:
    f1n, f1n1 = po.build_source(op1, f1, t, cap1), po.build_source(op1, f1, t + dt, cap1)
    f2n, f2n1 = po.build_source(op2, f2, t, cap2), po.build_source(op2, f2, t + dt, cap2)
    gg = po.build_g_g(op1, ic.scalar, cap1)
    Vn1_1, Vn1 = ost._time_faces(op1, cap1)
    Vn2_1, Vn2 = ost._time_faces(op2, cap2)
    psim = ost.psim_cn if scheme == "CN" else ost.psim_be
    Psi1 = sp.diags(np.array([psim(a, b) for a, b in zip(Vn1, Vn1_1)]))
    Psi2 = sp.diags(np.array([psim(a, b) for a, b in zip(Vn2, Vn2_1)]))
    q = len(Ti) // 4
    To1, Tg1, To2, Tg2 = Ti[:q], Ti[q:2 * q], Ti[2 * q:3 * q], Ti[3 * q:]
    f1n, f1n1, f2n, f2n1, gg = ost._half(f1n), ost._half(f1n1), ost._half(f2n), ost._half(f2n1), ost._half(gg)
    Id1, Id2 = ost._half(sp.diags(po.build_I_D(op1, D1, cap1))), ost._half(sp.diags(po.build_I_D(op2, D2, cap2)))
    W1, G1, H1, V1 = ost._half(op1.Winv), ost._half(op1.G), ost._half(op1.H), ost._half(op1.V)
    W2, G2, H2, V2 = ost._half(op2.Winv), ost._half(op2.G), ost._half(op2.H), ost._half(op2.V)
    G1T, G2T = G1.T.tocsr(), G2.T.tocsr()
    if scheme == "CN":                                                                         # :637-638
        b1 = (sp.diags(Vn1) - Id1 @ G1T @ W1 @ G1 @ Psi1) @ To1 - 0.5 * (Id1 @ G1T @ W1 @ H1 @ Tg1) + 0.5 * (V1 @ (f1n + f1n1))
        b3 = (sp.diags(Vn2) - Id2 @ G2T @ W2 @ G2 @ Psi2) @ To2 - 0.5 * (Id2 @ G2T @ W2 @ H2 @ Tg2) + 0.5 * (V2 @ (f2n + f2n1))
    else:                                                                                      # :640-641
        b1 = Vn1 * To1 + V1 @ f1n1
        b3 = Vn2 * To2 + V2 @ f2n1
    return np.concatenate([b1, gg, b3, gg])                                                    # :646-650


def stefan_diph_system(ph1: po.Phase, ph2: po.Phase, bc_b, ic, Ti, dt, t, mesh, scheme):
    """A, b of one Stefan diphasic slab with BC_border_diph!(A, b, bc_b, mesh)."""
    A = A_diph_unstead_diff_moving_stef(ph1.operator, ph2.operator, ph1.capacity, ph2.capacity, ph1.Diffusion_coeff,
                                        ph2.Diffusion_coeff, ic, scheme)
    b = b_diph_unstead_diff_moving_stef(ph1.operator, ph2.operator, ph1.capacity, ph2.capacity, ph1.Diffusion_coeff,
                                        ph2.Diffusion_coeff, ph1.source, ph2.source, ic, Ti, dt, t, scheme)
    return ost._border_diph(A, b, bc_b, ph1.capacity, ph2.capacity, mesh, None)


# ------------------------------------------------------------------------------------------------------ loops
def _phase(cap, like: po.Phase) -> po.Phase:
    return po.Phase(cap, po.make_diffusion_ops(cap), like.source, like.Diffusion_coeff)


def solve_mono(phase: po.Phase, bc_b, bc, ic, mesh: po.Mesh, scheme: str, xf: float, dt: float, Ts: float, Te: float, T0,
               capacity_fn: Callable, Newton_params=(1000, 1e-10, 1e-10, 1.0), cfl_target=0.5, dt_min=1e-4, dt_max=1.0,
               adaptive_timestep=True, learning_rate_strategy="fixed", learning_rate_options=None):
    """MovingLiquidDiffusionUnsteadyMono + solve_MovingLiquidDiffusionUnsteadyMono! -> (states, residuals, xf_log,
    timestep_history).  `phase` is the constructor's phase (its capacity: the static body at xf on [0, dt])."""
    s = ost.MovingDiffusionUnsteadyMono(phase, bc_b, bc, dt, T0, mesh, scheme)
    rho_L = ic.flux.value
    max_iter, tol, reltol, alpha = Newton_params
    opts = dict(learning_rate_options or {})
    residuals, xf_log, hist, states = {}, [], [(Ts, dt)], []
    t = Ts
    D, f = phase.Diffusion_coeff, phase.source

    def newton(ph, t, dt, xf, k, first):
        err, it = math.inf, 0
        current_xf = new_xf = xf
        lr = LRState(learning_rate_strategy, alpha, **opts)
        terms = None
        while it < max_iter and err > tol and err > reltol * abs(current_xf):
            it += 1
            po.solve_system(s)
            Ti = s.x
            terms = stefan_terms(ph.operator, ph.capacity, D, Ti)
            res = terms[0] - terms[1] - 1 / rho_L * terms[2]
            step = lr_step(lr, current_xf, res)
            new_xf = current_xf + step
            err = abs(res) if first else abs(step)
            residuals.setdefault(k, []).append(err)
            if err <= tol or err <= reltol * abs(current_xf) or it == max_iter:
                xf_log.append(new_xf)
                break
            tn1, tn = t + dt, t
            ph = _phase(capacity_fn(xf, new_xf, tn, tn1, False), phase)
            s.A = ost.A_mono_unstead_diff_moving(ph.operator, ph.capacity, D, bc, scheme)
            s.b = ost.b_mono_unstead_diff_moving(ph.operator, ph.capacity, D, f, bc, Ti, dt, t, scheme)
            s.A, s.b = po.BC_border_mono(s.A, s.b, bc_b, mesh, t=tn1)
            current_xf = new_xf
        return ph, new_xf, terms

    ph, new_xf, terms = newton(phase, t, dt, xf, 1, True)
    states.append(s.x)
    k = 2
    while t < Te:
        if adaptive_timestep:
            vel = 1 / rho_L * np.abs(_q(ph, D, s.x))
            dt, _ = adapt_timestep(vel, mesh.nodes, cfl_target, dt, dt_min, min(dt_max, Te - t))
            hist.append((t, dt))
        t += dt
        ph = _phase(capacity_fn(new_xf, new_xf, dt, 2 * dt, True), phase)
        s.A = ost.A_mono_unstead_diff_moving(ph.operator, ph.capacity, D, bc, scheme)
        s.b = ost.b_mono_unstead_diff_moving(ph.operator, ph.capacity, D, f, bc, s.x, dt, 0.0, scheme)
        s.A, s.b = po.BC_border_mono(s.A, s.b, bc_b, mesh, t=t)
        ph, new_xf, terms = newton(ph, t, dt, new_xf, k, False)
        states.append(s.x)
        k += 1
    return states, residuals, xf_log, hist


def _q(ph: po.Phase, D, Ti):
    op, cap = ph.operator, ph.capacity
    Wi, G, H = ost._half(op.Winv), ost._half(op.G), ost._half(op.H)
    Id = ost._half(sp.diags(po.build_I_D(op, D, cap)))
    M = len(Ti) // 2
    HT = H.T.tocsr()
    return Id @ (HT @ (Wi @ (G @ Ti[:M]))) + Id @ (HT @ (Wi @ (H @ Ti[M:])))


def solve_diph(phase1: po.Phase, phase2: po.Phase, bc_b, ic, mesh: po.Mesh, scheme: str, xf: float, dt: float, Ts: float,
               Te: float, T0, capacity_fn: Callable, Newton_params=(1000, 1e-10, 1e-10, 1.0), learning_rate_strategy="fixed",
               learning_rate_options=None):
    """MovingLiquidDiffusionUnsteadyDiph + solve_MovingLiquidDiffusionUnsteadyDiph! -> (states, residuals, xf_log).
    capacity_fn(xf0, xf1, t0, t1, static) -> (capacity of the body, capacity of its complement)."""
    s = po.Solver("Unsteady", "Diphasic", "Diffusion")
    s.A, s.b = stefan_diph_system(phase1, phase2, bc_b, ic, T0, dt, 0.0, mesh, scheme)
    rho_L = ic.flux.value
    max_iter, tol, reltol, alpha = Newton_params
    opts = dict(learning_rate_options or {})
    residuals, xf_log, states = {}, [], []
    t = Ts

    def newton(p1, p2, t, dt, xf, k, first):
        err, it = math.inf, 0
        current_xf = new_xf = xf
        lr = LRState(learning_rate_strategy, alpha, **opts)
        while it < max_iter and err > tol and err > reltol * abs(current_xf):
            it += 1
            po.solve_system(s)
            Ti = s.x
            M = len(Ti) // 4
            a = stefan_terms(p1.operator, p1.capacity, p1.Diffusion_coeff, Ti[:2 * M])
            b = stefan_terms(p2.operator, p2.capacity, p2.Diffusion_coeff, Ti[2 * M:])
            res = a[0] - a[1] - (1 / rho_L * a[2] + 1 / rho_L * b[2])
            step = lr_step(lr, current_xf, res)
            new_xf = current_xf + step
            err = abs(res) if first else abs(step)
            residuals.setdefault(k, []).append(err)
            if err <= tol or err <= reltol * abs(current_xf):
                xf_log.append(new_xf)
                break
            tn1, tn = t + dt, t
            c1, c2 = capacity_fn(xf, new_xf, tn, tn1, False)
            p1, p2 = _phase(c1, phase1), _phase(c2, phase2)
            s.A, s.b = stefan_diph_system(p1, p2, bc_b, ic, Ti, dt, t, mesh, scheme)
            current_xf = new_xf
        return p1, p2, new_xf

    p1, p2, new_xf = newton(phase1, phase2, t, dt, xf, 1, True)
    states.append(s.x)
    k = 2
    while t < Te:
        t += dt
        c1, c2 = capacity_fn(new_xf, new_xf, dt, 2 * dt, True)
        p1, p2 = _phase(c1, phase1), _phase(c2, phase2)
        s.A, s.b = stefan_diph_system(p1, p2, bc_b, ic, s.x, dt, 0.0, mesh, scheme)
        p1, p2, new_xf = newton(p1, p2, t, dt, new_xf, k, False)
        states.append(s.x)
        k += 1
    return states, residuals, xf_log
