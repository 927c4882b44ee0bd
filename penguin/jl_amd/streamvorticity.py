"""StreamVorticity -- src/solver/streamfunction_vorticity.jl: 2-D incompressible flow around cut-cell bodies in the
stream function - vorticity formulation,

    ∇²ψ = -ω,    u = ∂ψ/∂y,  v = -∂ψ/∂x,    ∂ω/∂t + (u·∇)ω = ν∇²ω + f.

Same names, keyword arguments and quirks as the reference; everything numeric is done by the library's composite handle
`pg_streamvort` (include/penguin_hip.h): ψ, ω, the velocity and the convection operators stay on the device from step to
step and come to the host only when an attribute is read.

Quirks kept (DESIGN.md "Stream function - vorticity"):
  * the ψ of state k is the one solved from the ω of state k-1 (`_step!` solves ψ first, :222, and pushes it with the new ω);
  * the interface velocity of the convection operators is the bulk velocity, uᵧ = [u; v] (:176-179);
  * border values are evaluated WITHOUT a time (BC_border_mono! is called without `t=`, :198, :231);
  * the reference calls b_mono_unstead_advdiff with 8 arguments for its 9 parameters (:228; `D` is missing -- a MethodError).
    What runs here is the evident intent, D = ν: under "BE" the value is never read, under "CN" it multiplies the explicit
    half of the diffusion.

Julia spellings: `solve_StreamVorticity!` -> solve_StreamVorticity_b, and so on.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Callable, Optional, Union

import numpy as np

from . import _lib as L
from ._lib import PenguinHipError
from .api import (BorderConditions, Capacity, ConvectionOps, DiffusionOps, Dirichlet, Phase, Solver, _border_descs, _dcoef, _eval,
                  _interface_desc, _krylov_opts, _padded_field, _step_info_check, _check_converged, _time_dependent, _UploadCache)

State = namedtuple("State", ["time", "ψ", "ω"])


def _zero_source(*args):
    return 0.0


class _BorrowedSolver(Solver):
    """A pg_solver that belongs to a pg_streamvort: system(), system_info(), A, b as for any Solver; never destroyed here."""

    def __init__(self, handle, nunk: int, owner):
        super().__init__("Steady", "Monophasic", "Diffusion")
        self._h = handle
        self._nunk = nunk
        self._owner = owner       # keeps the handle that owns the solver alive

    def __del__(self):
        pass


class StreamVorticity:
    """StreamVorticity(capacity, ν, Δt; bc_stream, bc_vorticity, bc_stream_border, bc_vorticity_border, ψ0, ω0, source)
    -- src/solver/streamfunction_vorticity.jl:73-98.

    ν: a number or a function ν(x, y, z) evaluated at C_ω (as build_I_D does).  Interface and border values: numbers or
    functions; border functions are called without a time.  `source(x, y, z, t)` is the body force of the vorticity
    equation.  `operator` (not in the reference, which builds it): a DiffusionOps of `capacity` to reuse.

    Fields: capacity, operator, ν, Δt, bc_*, ψ, ω, velocity = (u, v), time, states (State(time, ψ, ω) tuples, fetched from
    the device when read), Aψ, last_convection.  Assigning `s.ω = array` sets the vorticity the next step starts from."""

    def __init__(self, capacity: Capacity, ν: Union[float, Callable], Δt: float, bc_stream=None, bc_vorticity=None,
                 bc_stream_border: Optional[BorderConditions] = None, bc_vorticity_border: Optional[BorderConditions] = None,
                 ψ0: Optional[np.ndarray] = None, ω0: Optional[np.ndarray] = None, source: Callable = _zero_source,
                 operator: Optional[DiffusionOps] = None):
        L.init()
        self._h = C.c_void_p()
        bc_stream = Dirichlet(0.0) if bc_stream is None else bc_stream
        bc_vorticity = Dirichlet(0.0) if bc_vorticity is None else bc_vorticity
        bc_stream_border = BorderConditions({}) if bc_stream_border is None else bc_stream_border
        bc_vorticity_border = BorderConditions({}) if bc_vorticity_border is None else bc_vorticity_border
        self.capacity = capacity
        self.operator = DiffusionOps(capacity) if operator is None else operator
        if isinstance(self.operator, ConvectionOps):
            raise TypeError("StreamVorticity: operator must be a DiffusionOps (the convection operators are built from the "
                            "solver's own velocity)")
        self.ν, self.Δt = ν, float(Δt)
        self.bc_stream, self.bc_vorticity = bc_stream, bc_vorticity
        self.bc_stream_border, self.bc_vorticity_border = bc_stream_border, bc_vorticity_border
        self.source = source
        self.unconverged = 0
        self.last_run: Optional[L.pg_streamvort_run_info] = None
        self.last_step = None         # (pg_step_info of ψ, pg_step_info of ω) of the last step_StreamVorticity_b
        mesh = capacity.mesh
        M = self._M = int(np.prod(mesh.ext))
        D = _dcoef(Phase(capacity, self.operator, source, ν), M)
        nu = np.full(M, 1.0) if D is None else np.ascontiguousarray(D, dtype=np.float64)

        def state0(x, name):
            if x is None:
                return None
            x = np.ascontiguousarray(x, dtype=np.float64)
            if x.shape != (2 * M,):
                raise ValueError(f"{name} must have length 2*prod(n+1) = {2 * M}")
            return x

        ψ0, ω0 = state0(ψ0, "ψ0"), state0(ω0, "ω0")
        desc_s, keep_s = _interface_desc(bc_stream, capacity._cg, 0.0)           # build_g_g(.., t = s.time = 0)   :134
        desc_w, keep_w = _interface_desc(bc_vorticity, capacity._cg, self.Δt)    # g(0 + Δt); g(0) follows below (CN)
        bs, nbs, vals_s = _border_descs(bc_stream_border, mesh, None)            # no t   :198
        bw, nbw, vals_w = _border_descs(bc_vorticity_border, mesh, None)         # no t   :231
        p = lambda a: L.dptr(a) if a is not None else None
        L.check(L.lib().pg_streamvort_create(capacity._h, self.operator._h, L.dptr(nu), C.c_double(self.Δt), C.byref(desc_s),
                                             C.byref(desc_w), bs, C.c_int32(nbs), bw, C.c_int32(nbw), p(ψ0), p(ω0),
                                             C.byref(self._h)))
        if vals_s is not None:
            L.check(L.lib().pg_streamvort_set_border_values(self._h, C.c_int32(L.PG_SV_PSI), L.dptr(vals_s)))
        if vals_w is not None:
            L.check(L.lib().pg_streamvort_set_border_values(self._h, C.c_int32(L.PG_SV_OMEGA), L.dptr(vals_w)))
        # which data may change from step to step (any callable with a time parameter, as the other drivers decide it)
        self._dyn_f = source is not _zero_source and _time_dependent(source, 3)
        self._dyn_gs = _time_dependent(bc_stream.value, 3)
        self._dyn_gw = _time_dependent(bc_vorticity.value, 3)
        self._sent = _UploadCache()
        self._version = 0
        self._cache = {}
        self._conv = None
        self._have_velocity = False
        self._push_data(0.0, everything=True)

    # ---- data of closures ---------------------------------------------------------------------------------------------
    def _push_data(self, t: float, everything: bool = False) -> None:
        """Source and interface values at the reference's points and times (f, g_ω at t and t + Δt, g_ψ at t), sent when they
        differ from what the library holds.  `everything`: the constant ones too (once, after construction)."""
        lib, M, cap, dt = L.lib(), self._M, self.capacity, self.Δt
        full = lambda v: np.full(M, v) if isinstance(v, float) else v
        if self._dyn_f or (everything and self.source is not _zero_source):
            fn, fn1 = (_padded_field(_eval(self.source, cap._cw, tt, 3), M) for tt in (t, t + dt))
            zero = np.zeros(M)
            fn, fn1 = (fn if fn is not None else zero), (fn1 if fn1 is not None else zero)
            if self._sent.changed("f", fn, fn1) and (fn.any() or fn1.any() or not everything):
                L.check(lib.pg_streamvort_set_source(self._h, L.dptr(fn), L.dptr(fn1)))
        if self._dyn_gs:
            g = full(_eval(self.bc_stream.value, cap._cg, t, 3))
            if self._sent.changed("gs", g):
                L.check(lib.pg_streamvort_set_interface_values(self._h, C.c_int32(L.PG_SV_PSI), None, L.dptr(g)))
        if self._dyn_gw or (everything and callable(self.bc_vorticity.value)):
            g0, g1 = (full(_eval(self.bc_vorticity.value, cap._cg, tt, 3)) for tt in (t, t + dt))
            if self._sent.changed("gw", g0, g1):
                L.check(lib.pg_streamvort_set_interface_values(self._h, C.c_int32(L.PG_SV_OMEGA), L.dptr(g0), L.dptr(g1)))

    @property
    def _dynamic(self) -> bool:
        return self._dyn_f or self._dyn_gs or self._dyn_gw

    def _touch(self, velocity_changed: bool = True) -> None:
        self._version += 1
        self._cache.clear()
        if velocity_changed:
            self._conv = None          # update_velocity!: s.last_convection = nothing   :157

    # ---- fields -------------------------------------------------------------------------------------------------------
    def _get(self, field: int, index: int = -1) -> np.ndarray:
        key = (field, index)
        if key not in self._cache:
            n = self._M if field in (L.PG_SV_U, L.PG_SV_V) else 2 * self._M
            out = np.zeros(n)
            L.check(L.lib().pg_streamvort_get(self._h, C.c_int32(field), C.c_int64(index), L.dptr(out), C.c_int64(n)))
            self._cache[key] = out
        return self._cache[key]

    @property
    def ψ(self) -> np.ndarray:
        return self._get(L.PG_SV_PSI)

    @property
    def ω(self) -> np.ndarray:
        return self._get(L.PG_SV_OMEGA)

    @ω.setter
    def ω(self, value) -> None:
        value = np.ascontiguousarray(value, dtype=np.float64)
        if value.shape != (2 * self._M,):
            raise ValueError(f"ω must have length 2*prod(n+1) = {2 * self._M}")
        L.check(L.lib().pg_streamvort_set_omega(self._h, L.dptr(value)))
        self._touch(velocity_changed=False)

    @property
    def velocity(self):
        return (self._get(L.PG_SV_U), self._get(L.PG_SV_V))

    @property
    def time(self) -> float:
        return self._time(-1)

    def _time(self, index: int) -> float:
        t = C.c_double()
        L.check(L.lib().pg_streamvort_time(self._h, C.c_int64(index), C.byref(t)))
        return t.value

    @property
    def states(self):
        """[(time, ψ, ω), ...] starting with the initial state (:91); fetched from the device when read."""
        if "states" not in self._cache:
            n = C.c_int64()
            L.check(L.lib().pg_streamvort_num_states(self._h, C.byref(n)))
            self._cache["states"] = [State(self._time(k), self._get(L.PG_SV_PSI, k), self._get(L.PG_SV_OMEGA, k))
                                     for k in range(n.value)]
        return self._cache["states"]

    def _solver(self, which: int) -> Optional[Solver]:
        h = C.c_void_p()
        L.check(L.lib().pg_streamvort_solver(self._h, C.c_int32(which), C.byref(h)))
        return _BorrowedSolver(h, 2 * self._M, self) if h else None

    @property
    def psi_solver(self) -> Solver:
        """The steady solver of the Poisson system (borrowed): system(), system_info() as for any Solver."""
        return self._solver(L.PG_SV_PSI)

    @property
    def omega_solver(self) -> Optional[Solver]:
        """The solver of the last vorticity step (borrowed, replaced by every step; None before the first)."""
        return self._solver(L.PG_SV_OMEGA)

    @property
    def Aψ(self):
        """The Poisson matrix on its active rows / columns, embedded in 2M x 2M -- with the border rows of bc_stream_border
        applied (the reference stores the matrix before BC_border_mono! and applies the rows to a copy in every solve)."""
        return self.psi_solver.A

    @property
    def last_convection(self) -> Optional[ConvectionOps]:
        """ConvectionOps(capacity, (u, v), [u; v]) of the current velocity (:167-182): the same object on repeated reads
        until the next ψ solve; None before the first one.  A host-side view for inspection (C, K): the time loop uses the
        handle's own operators on the device."""
        if self._conv is None and self._have_velocity:
            u, v = self.velocity
            self._conv = ConvectionOps(self.capacity, (u, v), np.concatenate([u, v]))
        return self._conv

    def __del__(self):
        try:
            if self._h:
                L.lib().pg_streamvort_destroy(self._h)
        except Exception:
            pass


def _scheme(scheme: str) -> int:
    if scheme not in ("BE", "CN"):
        raise ValueError("Unknown scheme.")           # advectiondiffusion.jl:203-205
    return L.PG_SCHEME[scheme]


def _require(s) -> None:
    if not isinstance(s, StreamVorticity) or not s._h:
        raise PenguinHipError("StreamVorticity is not initialized. Call the constructor first.")


def solve_StreamVorticity_b(s: StreamVorticity, method="bicgstab", algorithm=None, **kwargs) -> np.ndarray:
    """solve_StreamVorticity!(s; ...) -- :273-275: the Poisson problem with the current ω, then the velocity.  Returns ψ."""
    _require(s)
    opts = _krylov_opts(method, kwargs)
    s._push_data(s.time)
    info = L.pg_step_info()
    L.check(L.lib().pg_streamvort_solve_stream(s._h, C.byref(opts), C.byref(info)))
    s._have_velocity = True
    s._touch()
    _step_info_check(s, info, "the stream-function solve")
    return s.ψ


def step_StreamVorticity_b(s: StreamVorticity, scheme: str = "BE", method="bicgstab", algorithm=None, **kwargs) -> np.ndarray:
    """step_StreamVorticity!(s; scheme, ...) -- :282-284: one time step.  Returns ω."""
    _require(s)
    sch = _scheme(scheme)
    opts = _krylov_opts(method, kwargs)
    s._push_data(s.time)
    ip, iw = L.pg_step_info(), L.pg_step_info()
    L.check(L.lib().pg_streamvort_step(s._h, C.c_int32(sch), C.byref(opts), C.byref(ip), C.byref(iw)))
    s._have_velocity = True
    s._touch()
    s.last_step = (ip, iw)            # pg_step_info of the stream-function and of the vorticity solve
    _step_info_check(s, ip, "the stream-function solve")
    _step_info_check(s, iw, "the vorticity solve")
    return s.ω


def run_StreamVorticity_b(s: StreamVorticity, steps: int, scheme: str = "BE", method="bicgstab", algorithm=None,
                          save_every: int = 1, **kwargs) -> StreamVorticity:
    """run_StreamVorticity!(s, steps; ...) -- :291-293.  Constant-in-time data: the loop runs inside the library
    (pg_streamvort_run) and every `save_every`-th state is kept (not in the reference, which keeps all: 1); closures with a
    time parameter: a loop of step_StreamVorticity_b with the data re-evaluated every step, every state kept."""
    _require(s)
    sch = _scheme(scheme)
    steps = int(steps)
    if steps <= 0:
        return s
    if s._dynamic:
        for _ in range(steps):
            step_StreamVorticity_b(s, scheme, method=method, algorithm=algorithm, **kwargs)
        return s
    opts = _krylov_opts(method, kwargs)
    run = L.pg_streamvort_run_info()
    L.check(L.lib().pg_streamvort_run(s._h, C.c_int64(steps), C.c_int32(sch), C.byref(opts), C.c_int32(save_every), C.byref(run)))
    s._have_velocity = True
    s._touch()
    s.last_run = run
    if run.unconverged:
        _check_converged(s, False, f"{run.unconverged} of {2 * run.steps} solves", run.worst_relres)
    return s


def run_until_StreamVorticity_b(s: StreamVorticity, t_end: float, scheme: str = "BE", method="bicgstab", algorithm=None,
                                save_every: int = 1, **kwargs) -> StreamVorticity:
    """run_until_StreamVorticity!(s, t_end; ...) -- :300-302: `while s.time < t_end - 1e-12` with fp64 `time += Δt`."""
    _require(s)
    _scheme(scheme)
    t, n = s.time, 0
    while t < t_end - 1e-12:          # the same additions the library performs
        t += s.Δt
        n += 1
    return run_StreamVorticity_b(s, n, scheme, method=method, algorithm=algorithm, save_every=save_every, **kwargs)
