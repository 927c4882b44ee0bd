"""The reference's stream function - vorticity step (src/solver/streamfunction_vorticity.jl) composed from the CPU oracle:
Poisson blocks from `_blocks`, `grad`, `make_convection_ops`, `A_/b_mono_unstead_advdiff`, `BC_border_mono`, and the direct
solve of `solve_system`.  Nothing here touches the product.

Kept as the reference has them: the ψ of a state is solved from the ω of the state before; uᵧ = [u; v]; border rows are
applied without a time; the diffusion coefficient of the explicit Crank-Nicolson half is ν (the reference's call at :228
leaves the argument out -- a MethodError; D = ν is the evident intent)."""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
import scipy.sparse as sp

from oracle import penguin_oracle as po


def zero_source(x, y, z, t):
    return 0.0


class OracleStreamVorticity:
    """StreamVorticity(capacity, ν, Δt; ...) on the oracle.  `zero_velocity=True` drops the convection (a control: how much
    of the answer the velocity carries)."""

    def __init__(self, cap: po.Capacity, nu, dt: float, bc_stream=None, bc_vorticity=None, bc_stream_border=None,
                 bc_vorticity_border=None, psi0: Optional[np.ndarray] = None, omega0: Optional[np.ndarray] = None,
                 source: Callable = zero_source, zero_velocity: bool = False):
        self.cap, self.nu, self.dt = cap, nu, float(dt)
        self.op = po.make_diffusion_ops(cap)
        self.M = int(np.prod(self.op.size))
        self.bc_stream = bc_stream if bc_stream is not None else po.Dirichlet(0.0)
        self.bc_vorticity = bc_vorticity if bc_vorticity is not None else po.Dirichlet(0.0)
        self.bc_stream_border = bc_stream_border if bc_stream_border is not None else po.BorderConditions({})
        self.bc_vorticity_border = bc_vorticity_border if bc_vorticity_border is not None else po.BorderConditions({})
        self.source = source
        self.zero_velocity = zero_velocity
        self.psi = np.zeros(2 * self.M) if psi0 is None else np.array(psi0, dtype=float)
        self.omega = np.zeros(2 * self.M) if omega0 is None else np.array(omega0, dtype=float)
        self.velocity = (np.zeros(self.M), np.zeros(self.M))
        self.time = 0.0
        self.states = [(0.0, self.psi.copy(), self.omega.copy())]
        # assemble_laplacian(operator, capacity, bc_stream, 1.0)   :105-117
        Ia, Ib = po.build_I_bc(self.op, self.bc_stream)
        Lw, Mx, P, Q = po._blocks(self.op)
        self.A_psi = sp.bmat([[Lw, Mx], [Ib * P, Ib * Q + Ia * sp.diags(cap.G)]], format="csr")

    # ---- ψ -------------------------------------------------------------------------------------------------------------
    def poisson_system(self, omega: np.ndarray, t: float) -> po.Solver:
        """[-V ωω; Γ g(C_γ, t)] and the border rows (no time)   :126-138, :195-198"""
        g = po.build_g_g(self.op, self.bc_stream, self.cap, t)
        b = np.concatenate([-self.cap.V * omega[: self.M], self.cap.G * g])
        s = po.Solver("Steady", "Monophasic", "Diffusion")
        s.A, s.b = po.BC_border_mono(self.A_psi, b, self.bc_stream_border, self.cap.mesh)
        return s

    def poisson(self, omega: np.ndarray, t: float) -> np.ndarray:
        s = self.poisson_system(omega, t)
        po.solve_system(s, method="\\")
        return s.x

    def velocity_of(self, psi: np.ndarray):
        """update_velocity!   :146-159"""
        g = po.grad(self.op, psi)
        u, v = g[self.M:].copy(), -g[: self.M]
        if self.zero_velocity:
            u, v = np.zeros(self.M), np.zeros(self.M)
        return u, v

    # ---- ω -------------------------------------------------------------------------------------------------------------
    def omega_system(self, u: np.ndarray, v: np.ndarray, omega_n: np.ndarray, t: float, scheme: str) -> po.Solver:
        """ConvectionOps(capacity, (u, v), [u; v]) and the unsteady advection-diffusion system from ω at t   :167-231"""
        cop = po.make_convection_ops(self.cap, (u, v), np.concatenate([u, v]))
        s = po.Solver("Unsteady", "Monophasic", "DiffusionAdvection")
        A = po.A_mono_unstead_advdiff(cop, self.cap, self.nu, self.bc_vorticity, self.dt, scheme)
        b = po.b_mono_unstead_advdiff(cop, self.source, self.cap, self.nu, self.bc_vorticity, omega_n, self.dt, t, scheme)
        s.A, s.b = po.BC_border_mono(A, b, self.bc_vorticity_border, self.cap.mesh)
        return s

    def omega_solve(self, u: np.ndarray, v: np.ndarray, omega_n: np.ndarray, t: float, scheme: str) -> np.ndarray:
        s = self.omega_system(u, v, omega_n, t, scheme)
        po.solve_system(s, method="\\")
        return s.x

    # ---- steps ---------------------------------------------------------------------------------------------------------
    def step_from(self, omega_n: np.ndarray, t: float, scheme: str = "BE"):
        """one step from given inputs -> ψ, u, v, ω_{n+1}"""
        psi = self.poisson(omega_n, t)
        u, v = self.velocity_of(psi)
        return psi, u, v, self.omega_solve(u, v, omega_n, t, scheme)

    def solve_stream(self) -> np.ndarray:
        self.psi = self.poisson(self.omega, self.time)
        self.velocity = self.velocity_of(self.psi)
        return self.psi

    def step(self, scheme: str = "BE") -> np.ndarray:
        if scheme not in ("BE", "CN"):
            raise ValueError("Unknown scheme.")
        self.psi, u, v, self.omega = self.step_from(self.omega, self.time, scheme)
        self.velocity = (u, v)
        self.time += self.dt
        self.states.append((self.time, self.psi.copy(), self.omega.copy()))
        return self.omega

    def run(self, steps: int, scheme: str = "BE"):
        for _ in range(steps):
            self.step(scheme)
        return self

    def run_until(self, t_end: float, scheme: str = "BE"):
        while self.time < t_end - 1e-12:
            self.step(scheme)
        return self
