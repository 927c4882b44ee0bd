"""Liquid-motion (Stefan) solvers in 1-D through the HIP path -- the reference's src/liquidmotionsolver/diffusion.jl (learning
rates :3-136, MovingLiquidDiffusionUnsteadyMono :152-171 and its loop :173-442, the Stefan diphasic blocks :445-651,
MovingLiquidDiffusionUnsteadyDiph :653-673 and its loop :675-946), height_tracking.jl:23-61 and adapt_timestep
(solver.jl:611-662), with the same names, argument order and defaults.

    STmesh   = SpaceTimeMesh(mesh, [0.0, Δt])
    body     = MovingHalfSpace(0, lambda t: xf)                # x - xf: the liquid is x < xf
    capacity = Capacity(body, STmesh)
    solver   = MovingLiquidDiffusionUnsteadyMono(Phase(capacity, DiffusionOps(capacity), f, K), bc_b, bc, Δt, u0, mesh, "BE")
    solver, residuals, xf_log, timestep_history = solve_MovingLiquidDiffusionUnsteadyMono_b(
        solver, phase, xf, Δt, Tstart, Tend, bc_b, bc, ic, mesh, "BE")

Every Newton iteration solves one space-time slab on the GPU (the moving blocks of moving.py), reads the Stefan terms of the
solved slab (pg_solver_stefan_terms: Hₙ, Hₙ₊₁, Σq and max|q|, four doubles per phase) and rebuilds the slab around the
new interface position: a MovingHalfSpace with a linear position and its exact derivative.  The state stays on the device
(`previous` hand-over); the host fetches one state per time step (save_states=True) or only the last one.  The reference's
quirks are kept as written; DESIGN.md §11 lists them.  1-D only: the reference's 2-D call feeds y into the body's time
argument, so an N ≥ 2 mesh is refused."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from . import _lib as L
from . import api
from . import moving
from ._lib import PenguinHipError


# ---------------------------------------------------------------------------------------------------------------------
# learning rate of the interface update                                                        diffusion.jl:3-136
# ---------------------------------------------------------------------------------------------------------------------
class LearningRateState:
    """mutable struct LearningRateState (:3-20)."""

    def __init__(self, strategy, base_lr, eps, beta1, beta2, decay, min_lr, max_lr):
        self.strategy, self.base_lr, self.eps, self.beta1, self.beta2, self.decay = strategy, base_lr, eps, beta1, beta2, decay
        self.grad_accum = self.mean_grad_sq = self.m = self.v = 0.0
        self.t = 0
        self.prev_xf: Optional[float] = None
        self.prev_grad: Optional[float] = None
        self.min_lr, self.max_lr, self.last_lr = min_lr, max_lr, base_lr


def normalize_lr_strategy(strategy) -> str:
    """:22-29 (symbols are strings here)."""
    normalized = str(strategy).lstrip(":").lower()
    if normalized in ("constant", "none"):
        return "fixed"
    if normalized in ("bb", "barzilaiborwein", "barzilai-borwein"):
        return "barzilai_borwein"
    if normalized in ("rms_prop",):
        return "rmsprop"
    return normalized


def init_learning_rate_state(strategy, base_lr: float, eps: float = 1e-8, beta1: float = 0.9, beta2: float = 0.999,
                             decay: float = 0.0, min_lr: float = 0.0, max_lr: float = math.inf) -> LearningRateState:
    """:31-41."""
    strat = normalize_lr_strategy(strategy)
    max_lr = max(max_lr, min_lr)
    return LearningRateState(strat, float(base_lr), float(eps), float(beta1), float(beta2), float(decay), float(min_lr),
                             float(max_lr))


def _clamp(x, lo, hi):
    """Julia's clamp(x, lo, hi): hi if x > hi, else lo if x < lo, else x (also when lo > hi)."""
    return hi if x > hi else (lo if x < lo else x)


def _sign(x: float) -> float:
    return 0.0 if x == 0 else math.copysign(1.0, x) if not math.isnan(x) else x


def apply_learning_rate_step_b(state: LearningRateState, current_xf: float, grad: float) -> float:
    """apply_learning_rate_step!(state, current_xf, grad) (:43-122): the step to add to the interface position."""
    state.t += 1
    base_lr = state.base_lr / (1 + state.decay * (state.t - 1)) if state.decay > 0 else state.base_lr
    lr = base_lr
    direction = grad
    custom_step = None
    if state.strategy == "adagrad":
        state.grad_accum += grad * grad
        lr = base_lr / (math.sqrt(state.grad_accum) + state.eps)
    elif state.strategy == "rmsprop":
        state.mean_grad_sq = state.beta2 * state.mean_grad_sq + (1 - state.beta2) * grad * grad
        lr = base_lr / (math.sqrt(state.mean_grad_sq) + state.eps)
    elif state.strategy == "nadam":
        state.m = state.beta1 * state.m + (1 - state.beta1) * grad
        state.v = state.beta2 * state.v + (1 - state.beta2) * grad * grad
        bias_correction1 = max(1 - state.beta1 ** state.t, state.eps)
        bias_correction2 = max(1 - state.beta2 ** state.t, state.eps)
        m_hat = state.m / bias_correction1
        v_hat = state.v / bias_correction2
        lr = base_lr / (math.sqrt(v_hat) + state.eps)
        direction = state.beta1 * m_hat + (1 - state.beta1) * grad / bias_correction1
    elif state.strategy == "barzilai_borwein":
        if not (state.prev_xf is None or state.prev_grad is None):
            dx = current_xf - state.prev_xf
            dg = grad - state.prev_grad
            denom = dg * dg if abs(dg) > state.eps else 0.0
            if denom > 0:
                lr = abs(dx * dg) / denom
    elif state.strategy == "secant":
        if not (state.prev_xf is None or state.prev_grad is None):
            dx = current_xf - state.prev_xf
            dg = grad - state.prev_grad
            if abs(dg) > state.eps:
                proposed_step = -grad * (dx / dg)
                if grad == 0.0:
                    custom_step = proposed_step
                    lr = state.base_lr
                else:
                    max_step = state.max_lr * abs(grad)
                    min_step = state.min_lr * abs(grad)
                    if math.isfinite(max_step):
                        proposed_step = _clamp(proposed_step, -max_step, max_step)
                    if min_step > 0 and abs(proposed_step) < min_step:
                        proposed_step = _sign(proposed_step) * min_step
                    custom_step = proposed_step
                    lr = abs(proposed_step) / max(abs(grad), state.eps)
    if custom_step is None:
        lr = _clamp(lr, state.min_lr, state.max_lr)
        step = lr * direction
    else:
        step = custom_step
    if not math.isfinite(step):
        step = 0.0
    state.prev_xf = current_xf
    state.prev_grad = grad
    state.last_lr = lr
    return step


def normalize_lr_options(options) -> dict:
    """:124-136: None, a dict or a list of (name, value) pairs."""
    if options is None:
        return {}
    if isinstance(options, dict):
        return dict(options)
    if isinstance(options, (list, tuple)):
        return dict(options)
    raise ValueError("learning_rate_options must be provided as a dict, a list of pairs, or None.")


# ---------------------------------------------------------------------------------------------------------------------
# adapt_timestep                                                                                   solver.jl:611-662
# ---------------------------------------------------------------------------------------------------------------------
def adapt_timestep(velocity_field, mesh, cfl_target: float, Δt_current: float, Δt_min: float, Δt_max: float,
                   growth_factor: float = 1.1, shrink_factor: float = 0.8, safety_factor: float = 0.9):
    """adapt_timestep(velocity_field, mesh, cfl_target, Δt_current, Δt_min, Δt_max; ...) -> (Δt_new, cfl_actual).  Literal,
    including the reference's inverted branches: a CFL-optimal step LARGER than the current one shrinks it
    (min(Δt_optimal, shrink_factor Δt)), a smaller one grows it (max(Δt_optimal, growth_factor Δt))."""
    v_max = float(np.max(np.abs(np.atleast_1d(np.asarray(velocity_field, dtype=np.float64)))))
    if v_max < 1e-10:
        return min(Δt_current * growth_factor, Δt_max), 0.0
    nodes = mesh.nodes
    if len(nodes) not in (1, 2, 3):
        raise ValueError("Unsupported mesh dimension")
    Δh_min = min(float(np.min(np.diff(np.asarray(n, dtype=np.float64)))) for n in nodes)
    Δt_optimal = safety_factor * cfl_target * Δh_min / v_max
    if Δt_optimal > Δt_current:
        Δt_new = min(Δt_optimal, Δt_current * shrink_factor)
    else:
        Δt_new = max(Δt_optimal, Δt_current * growth_factor)
    Δt_new = _clamp(Δt_new, Δt_min, Δt_max)
    return Δt_new, v_max * Δt_new / Δh_min


# ---------------------------------------------------------------------------------------------------------------------
# the Stefan terms of a solved slab                                          diffusion.jl:240-255, height_tracking.jl:23-61
# ---------------------------------------------------------------------------------------------------------------------
def stefan_terms(s: api.Solver) -> np.ndarray:
    """(nphase, 4): per phase Σ A_t(t0) = Hₙ₊₁, Σ A_t(t1) = Hₙ, Σ q, max |q| with q = Id Hᵀ Wꜝ (G Tω + H Tγ) of the solved
    slab (pg_solver_stefan_terms).  Bitwise reproducible for a given state."""
    nph = 2 if s._nunk == 4 * s._ctx["M"] else 1
    out = np.zeros(4 * nph)
    L.check(L.lib().pg_solver_stefan_terms(s._h, L.dptr(out)))
    return out.reshape(nph, 4)


def extract_height_profiles(s: api.Solver, phase: int = 0):
    """The sums of extract_height_profiles(capacity, dims) (height_tracking.jl:54-61) in 1-D: (Hₙ, Hₙ₊₁) of the solver's
    current slab, Hₙ = Σ A_t(t1), Hₙ₊₁ = Σ A_t(t0)."""
    r = stefan_terms(s)[phase]
    return float(r[1]), float(r[0])


def _require_1d(mesh: api.Mesh):
    if mesh.N != 1:
        raise PenguinHipError("the liquid-motion solvers are 1-D only (N = 1): the reference's N ≥ 2 call feeds the second "
                              "coordinate into the body's time argument (DESIGN.md §11)")


def _front(xf0: float, xf1: float, tn: float, tn1: float, Δt: float, complement: bool = False) -> moving.MovingHalfSpace:
    """body = (x, t) -> x - (xf (tn1 - t)/Δt + new_xf (t - tn)/Δt)   (:283, :397): the linear position, its exact slope."""
    return moving.MovingHalfSpace(0, lambda tt: xf0 * (tn1 - tt) / Δt + xf1 * (tt - tn) / Δt, 1.0, complement=complement,
                                  dposition=lambda tt: -xf0 / Δt + xf1 / Δt)


def _static(xf: float, complement: bool = False) -> moving.MovingHalfSpace:
    """body = (x, t) -> x - new_xf   (:341, :808)."""
    return moving.MovingHalfSpace(0, lambda tt: xf, 1.0, complement=complement, dposition=lambda tt: 0.0)


def _capacity(body, mesh, t0, t1, time_panels, time_order):
    return api.Capacity(body, moving.SpaceTimeMesh(mesh, [t0, t1]), time_panels=time_panels, time_order=time_order,
                        compute_centroids=True)


def _push_state(s: api.Solver, save_states: bool, verbose: bool):
    if save_states:
        s.x = s._fetch_state(-1)
        s.states.append(s.x)
        if verbose:
            print(f"Max value : {np.max(np.abs(s.x))}")


# ---------------------------------------------------------------------------------------------------------------------
# one phase                                                                                     diffusion.jl:152-442
# ---------------------------------------------------------------------------------------------------------------------
def MovingLiquidDiffusionUnsteadyMono(phase: api.Phase, bc_b, bc_i, Δt: float, Tᵢ: np.ndarray, mesh: api.Mesh, scheme: str,
                                      verbose: bool = False) -> api.Solver:
    """MovingLiquidDiffusionUnsteadyMono(phase, bc_b, bc_i, Δt, Tᵢ, mesh, scheme) (:152-171): the moving-mono blocks and
    BC_border_mono!(...; t=0.0) of the first slab."""
    _require_1d(mesh)
    if verbose:
        print("Solver Creation:\n- Moving problem\n- Non prescibed motion\n- Monophasic problem\n- Unsteady problem\n"
              "- Diffusion problem")
    s = api.Solver("Unsteady", "Monophasic", "Diffusion")
    Tᵢ = api._unsteady_prelude(s, 2, mesh, Tᵢ, phase=phase, bc_i=bc_i, dt=float(Δt))
    moving._create_step(s, [phase], bc_b, bc_i, float(Δt), Tᵢ, mesh, scheme, 0.0, 0.0)
    return s


def _newton_mono(s, ph, bc_b, bc, mesh, sch, opts, ρL, max_iter, tol, reltol, lr_state, t, Δt, xf, first, residuals, k,
                 xf_log, time_panels, time_order, verbose):
    """One Newton loop of solve_MovingLiquidDiffusionUnsteadyMono! (:229-311 first step, :357-421 later steps).  Returns
    (phase, new_xf, terms of the last solve)."""
    err, it = math.inf, 0
    current_xf = new_xf = xf
    terms = None
    while it < max_iter and err > tol and err > reltol * abs(current_xf):
        it += 1
        moving._solve_current(s, opts, f"Newton iteration {it} of the step at t = {t}", False, False)
        terms = stefan_terms(s)[0]
        Hn, Hn1 = terms[1], terms[0]
        interface_term = 1 / ρL * terms[2]
        res = Hn1 - Hn - interface_term
        step = apply_learning_rate_step_b(lr_state, current_xf, res)
        new_xf = current_xf + step
        err = abs(res) if first else abs(step)
        if verbose:
            print(f"Iteration {it} | xf = {new_xf} | error = {err} | res = {res} | α = {lr_state.last_lr}")
        residuals.setdefault(k, []).append(err)
        if err <= tol or err <= reltol * abs(current_xf) or it == max_iter:
            xf_log.append(new_xf)
            break
        tn1, tn = t + Δt, t
        cap = _capacity(_front(xf, new_xf, tn, tn1, Δt), mesh, tn, tn1, time_panels, time_order)
        ph = api.Phase(cap, api.DiffusionOps(cap), ph.source, ph.Diffusion_coeff)
        if it < max_iter and err > tol and err > reltol * abs(new_xf):
            moving._create_step(s, [ph], bc_b, bc, float(Δt), None, mesh, sch, t, tn1, from_previous=True)
        else:
            # the while test (reltol |new_xf|) ends the loop on a slab that is never solved: s keeps the solved state, and
            # the next step's velocity reads that state through the unsolved slab's operator (:318-330) -- a side solver
            # built from the state, whose terms read the state it was built from
            side = api.Solver("Unsteady", "Monophasic", "Diffusion")
            side._nunk, side._ctx = s._nunk, s._ctx
            moving._create_step(side, [ph], bc_b, bc, float(Δt), s._fetch_state(-1), mesh, sch, t, tn1)
            terms = stefan_terms(side)[0]
        current_xf = new_xf
    if verbose:
        conv = err <= tol or err <= reltol * abs(current_xf)
        print(f"{'Converged after' if conv else 'Reached max_iter = ' + str(max_iter) + ' after'} {it} iterations with "
              f"xf = {new_xf}, error = {err}")
    return ph, new_xf, terms


def solve_MovingLiquidDiffusionUnsteadyMono_b(s: api.Solver, phase: api.Phase, xf: float, Δt: float, Tₛ: float, Tₑ: float, bc_b,
                                              bc, ic, mesh: api.Mesh, scheme: str, Newton_params=(1000, 1e-10, 1e-10, 1.0),
                                              cfl_target: float = 0.5, Δt_min: float = 1e-4, Δt_max: float = 1.0,
                                              adaptive_timestep: bool = True, method="gmres", algorithm=None,
                                              learning_rate_strategy="fixed", learning_rate_options=None,
                                              verbose: bool = False, time_panels: int = 16, time_order: int = 4,
                                              save_states: bool = True, **kwargs):
    """solve_MovingLiquidDiffusionUnsteadyMono!(s, phase, xf, Δt, Tₛ, Tₑ, bc_b, bc, ic, mesh, scheme; Newton_params, cfl_target,
    Δt_min, Δt_max, adaptive_timestep, method, algorithm, learning_rate_strategy, learning_rate_options) (:173-442)
    -> (s, residuals, xf_log, timestep_history).  residuals: {time step (1-based): [err per iteration]}.
    `save_states=False` (not in the reference): only the last state is fetched (s.x, s.states[-1])."""
    if s is None or not s._h:
        raise PenguinHipError("Solver is not initialized. Call a solver constructor first.")
    _require_1d(mesh)
    opts = api._krylov_opts(method, kwargs)
    sch = "CN" if scheme == "CN" else "BE"
    t = float(Tₛ)
    Δt = float(Δt)
    ρL = ic.flux.value
    max_iter, tol, reltol, α = int(Newton_params[0]), Newton_params[1], Newton_params[2], Newton_params[3]
    lr_opts = normalize_lr_options(learning_rate_options)
    residuals: dict = {}
    xf_log: list = []
    timestep_history = [(t, Δt)]
    if verbose:
        print(f"Time : {t}")
    lr_state = init_learning_rate_state(learning_rate_strategy, α, **lr_opts)
    ph, new_xf, terms = _newton_mono(s, phase, bc_b, bc, mesh, sch, opts, ρL, max_iter, tol, reltol, lr_state, t, Δt,
                                     float(xf), True, residuals, 1, xf_log, time_panels, time_order, verbose)
    _push_state(s, save_states, verbose)
    k = 2
    while t < Tₑ:
        if adaptive_timestep:
            # velocity_field = 1/ρL |q| of the state just solved (:318-330): its max is that of the last Newton solve
            v_max = abs(1 / ρL * terms[3])
            time_left = Tₑ - t
            Δt_max_current = min(Δt_max, time_left)
            Δt, cfl = adapt_timestep(v_max, mesh, cfl_target, Δt, Δt_min, Δt_max_current, growth_factor=1.1,
                                     shrink_factor=0.8, safety_factor=0.9)
            timestep_history.append((t, Δt))
            if verbose:
                print(f"Adaptive timestep: Δt = {Δt:.6f}, CFL = {cfl:.3f}")
        t += Δt
        if verbose:
            print(f"Time : {t}")
        cap = _capacity(_static(new_xf), mesh, Δt, 2 * Δt, time_panels, time_order)      # SpaceTimeMesh(mesh, [Δt, 2Δt])
        ph = api.Phase(cap, api.DiffusionOps(cap), ph.source, ph.Diffusion_coeff)
        moving._create_step(s, [ph], bc_b, bc, Δt, None, mesh, sch, 0.0, t, from_previous=True)
        lr_state = init_learning_rate_state(learning_rate_strategy, α, **lr_opts)
        ph, new_xf, terms = _newton_mono(s, ph, bc_b, bc, mesh, sch, opts, ρL, max_iter, tol, reltol, lr_state, t, Δt,
                                         new_xf, False, residuals, k, xf_log, time_panels, time_order, verbose)
        _push_state(s, save_states, verbose)
        k += 1
    if not save_states:
        s.x = s._fetch_state(-1)
        s.states.append(s.x)
    return s, residuals, xf_log, timestep_history


# ---------------------------------------------------------------------------------------------------------------------
# two phases                                                                                    diffusion.jl:445-946
# ---------------------------------------------------------------------------------------------------------------------
def MovingLiquidDiffusionUnsteadyDiph(phase1: api.Phase, phase2: api.Phase, bc_b, ic, Δt: float, Tᵢ: np.ndarray, mesh: api.Mesh,
                                      scheme: str, verbose: bool = False) -> api.Solver:
    """MovingLiquidDiffusionUnsteadyDiph(phase1, phase2, bc_b, ic, Δt, Tᵢ, mesh, scheme) (:653-673): the Stefan diphasic
    blocks A_/b_diph_unstead_diff_moving_stef (pg_solver_create_moving_stefan_diph) and BC_border_diph!."""
    _require_1d(mesh)
    if verbose:
        print("Solver Creation:\n- Moving problem\n- Non prescibed motion\n- Diphasic problem\n- Unsteady problem\n"
              "- Diffusion problem")
    s = api.Solver("Unsteady", "Diphasic", "Diffusion")
    Tᵢ = api._unsteady_prelude(s, 4, mesh, Tᵢ, dt=float(Δt))
    moving._create_step(s, [phase1, phase2], bc_b, ic, float(Δt), Tᵢ, mesh, scheme, 0.0, None, stefan=True)
    return s


def _newton_diph(s, ph1, ph2, bc_b, ic, mesh, sch, opts, ρL, max_iter, tol, reltol, lr_state, t, Δt, xf, first, residuals, k,
                 xf_log, time_panels, time_order, verbose):
    """One Newton loop of solve_MovingLiquidDiffusionUnsteadyDiph! (:725-826 first step, :846-933 later steps): no break at
    max_iter, Hₙ / Hₙ₊₁ of phase 1 only, the interface term of both phases."""
    err, it = math.inf, 0
    current_xf = new_xf = xf
    while it < max_iter and err > tol and err > reltol * abs(current_xf):
        it += 1
        moving._solve_current(s, opts, f"Newton iteration {it} of the step at t = {t}", False, False)
        terms = stefan_terms(s)
        Hn, Hn1 = terms[0, 1], terms[0, 0]
        interface_term = 1 / ρL * terms[0, 2] + 1 / ρL * terms[1, 2]
        res = Hn1 - Hn - interface_term
        step = apply_learning_rate_step_b(lr_state, current_xf, res)
        new_xf = current_xf + step
        err = abs(res) if first else abs(step)
        if verbose:
            print(f"Iteration {it} | xf = {new_xf} | error = {err} | res = {res} | α = {lr_state.last_lr}")
        residuals.setdefault(k, []).append(err)
        if err <= tol or err <= reltol * abs(current_xf):
            xf_log.append(new_xf)
            break
        tn1, tn = t + Δt, t
        current_xf = new_xf
        if not (it < max_iter and err > tol and err > reltol * abs(current_xf)):
            break        # the loop ends on a rebuilt slab that is never solved and that the next step overwrites (:919-930)
        c1 = _capacity(_front(xf, new_xf, tn, tn1, Δt), mesh, tn, tn1, time_panels, time_order)
        c2 = _capacity(_front(xf, new_xf, tn, tn1, Δt, complement=True), mesh, tn, tn1, time_panels, time_order)
        ph1 = api.Phase(c1, api.DiffusionOps(c1), ph1.source, ph1.Diffusion_coeff)
        ph2 = api.Phase(c2, api.DiffusionOps(c2), ph2.source, ph2.Diffusion_coeff)
        moving._create_step(s, [ph1, ph2], bc_b, ic, float(Δt), None, mesh, sch, t, None, from_previous=True, stefan=True)
    if verbose:
        conv = err <= tol or err <= reltol * abs(current_xf)
        print(f"{'Converged after' if conv else 'Reached max_iter = ' + str(max_iter) + ' after'} {it} iterations with "
              f"xf = {new_xf}, error = {err}")
    return ph1, ph2, new_xf


def solve_MovingLiquidDiffusionUnsteadyDiph_b(s: api.Solver, phase1: api.Phase, phase2: api.Phase, xf: float, Δt: float, Tₛ: float,
                                              Tₑ: float, bc_b, ic, mesh: api.Mesh, scheme: str,
                                              Newton_params=(1000, 1e-10, 1e-10, 1.0), method="gmres", algorithm=None,
                                              learning_rate_strategy="fixed", learning_rate_options=None,
                                              verbose: bool = False, time_panels: int = 16, time_order: int = 4,
                                              save_states: bool = True, **kwargs):
    """solve_MovingLiquidDiffusionUnsteadyDiph!(s, phase1, phase2, xf, Δt, Tₛ, Tₑ, bc_b, ic, mesh, scheme; Newton_params, method,
    algorithm, learning_rate_strategy, learning_rate_options) (:675-946) -> (s, residuals, xf_log).  Fixed Δt."""
    if s is None or not s._h:
        raise PenguinHipError("Solver is not initialized. Call a solver constructor first.")
    _require_1d(mesh)
    opts = api._krylov_opts(method, kwargs)
    sch = "CN" if scheme == "CN" else "BE"
    t = float(Tₛ)
    Δt = float(Δt)
    ρL = ic.flux.value
    max_iter, tol, reltol, α = int(Newton_params[0]), Newton_params[1], Newton_params[2], Newton_params[3]
    lr_opts = normalize_lr_options(learning_rate_options)
    residuals: dict = {}
    xf_log: list = []
    if verbose:
        print(f"Time : {t}")
    lr_state = init_learning_rate_state(learning_rate_strategy, α, **lr_opts)
    ph1, ph2, new_xf = _newton_diph(s, phase1, phase2, bc_b, ic, mesh, sch, opts, ρL, max_iter, tol, reltol, lr_state, t, Δt,
                                    float(xf), True, residuals, 1, xf_log, time_panels, time_order, verbose)
    _push_state(s, save_states, verbose)
    k = 2
    while t < Tₑ:
        t += Δt
        if verbose:
            print(f"Time : {t}")
        c1 = _capacity(_static(new_xf), mesh, Δt, 2 * Δt, time_panels, time_order)       # SpaceTimeMesh(mesh, [Δt, 2Δt])
        c2 = _capacity(_static(new_xf, complement=True), mesh, Δt, 2 * Δt, time_panels, time_order)
        ph1 = api.Phase(c1, api.DiffusionOps(c1), ph1.source, ph1.Diffusion_coeff)
        ph2 = api.Phase(c2, api.DiffusionOps(c2), ph2.source, ph2.Diffusion_coeff)
        moving._create_step(s, [ph1, ph2], bc_b, ic, Δt, None, mesh, sch, 0.0, None, from_previous=True, stefan=True)
        lr_state = init_learning_rate_state(learning_rate_strategy, α, **lr_opts)
        ph1, ph2, new_xf = _newton_diph(s, ph1, ph2, bc_b, ic, mesh, sch, opts, ρL, max_iter, tol, reltol, lr_state, t, Δt,
                                        new_xf, False, residuals, k, xf_log, time_panels, time_order, verbose)
        _push_state(s, save_states, verbose)
        k += 1
    if not save_states:
        s.x = s._fetch_state(-1)
        s.states.append(s.x)
    return s, residuals, xf_log
