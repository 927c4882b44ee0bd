"""Prescribed-motion diffusion through the HIP path -- the reference's
src/prescribedmotionsolver/diffusion.jl:16-35 (constructor), :100-225 (blocks), :227-268 (time loop) and
src/mesh.jl:129-146 (SpaceTimeMesh), with the same names and argument order.

    STmesh   = SpaceTimeMesh(mesh, [0.0, Δt])
    capacity = Capacity(body, STmesh)                       # body: MovingSphere / MovingHalfSpace
    operator = DiffusionOps(capacity)
    solver   = MovingDiffusionUnsteadyMono(Phase(capacity, operator, f, K), bc_b, bc, Δt, u0, mesh, "BE")
    solve_MovingDiffusionUnsteadyMono_b(solver, phase, body, Δt, Tstart, Tend, bc_b, bc, mesh, "BE")

Every time slab builds a new space-time capacity on the GPU (pg_capacity_create_spacetime), assembles the moving blocks
there (pg_solver_create_moving_mono) and solves; the host only evaluates the motion at the time-quadrature nodes and the
user's closures.  The level set of the reference is an arbitrary `body(x..., t)`; here it is a tagged moving body, as for
static capacities, or any closure wrapped in DeviceFunction: `Capacity(DeviceFunction(lambda x, y, t: ...), STmesh)` traces it
once and evaluates phi, its gradient and d phi / dt inside the space-time kernels (pg_capacity_create_spacetime_program,
DESIGN.md section 24); the drivers take it as `body`, and `DeviceFunction(fn, complement=True)` as `body_c`.  A marker polygon
that moves is a MovingFront (front.py): `Capacity(mf, STmesh)`, or `Capacity((front_n, front_np1), STmesh)` as the reference's
compute_spacetime_capacities is called, sends the markers at the slab's two times to pg_capacity_create_spacetime_polygon
(DESIGN.md section 26); the drivers take `mf` as `body` and `MovingFront(..., complement=True)` as `body_c`.  A plain callable
is refused (integrate it yourself and use SpaceTimeCapacity.from_arrays).
1-D and 2-D in space: the reference's 3-D+t selection `[1:end÷2]` drops the z direction."""
from __future__ import annotations

import ctypes as C
from typing import Callable, Optional, Sequence

import numpy as np

from . import _lib as L
from . import api
from ._lib import PenguinHipError
from .devfn import DeviceFunction, pg_program
from .front import MovingFront


class SpaceTimeMesh:
    """SpaceTimeMesh(spaceMesh, [t0, t1]) -- src/mesh.jl:129-146: nodes / centers / dims with the time dimension appended."""

    def __init__(self, spaceMesh: api.Mesh, time: Sequence[float], tag=None):
        if len(time) != 2:
            raise ValueError("SpaceTimeMesh: one time cell [t, t+Δt] (every call site of the moving solvers)")
        self.space = spaceMesh
        self.time = (float(time[0]), float(time[1]))
        self.nodes = tuple(spaceMesh.nodes) + (np.array(self.time),)
        self.centers = tuple(spaceMesh.centers) + (np.array([(self.time[0] + self.time[1]) / 2]),)
        self.dims = tuple(len(c) for c in self.centers)
        self.tag = tag if tag is not None else getattr(spaceMesh, "tag", None)
        self.N = spaceMesh.N + 1


def _ddt(fn: Callable, t: float, h: float) -> np.ndarray:
    return (np.atleast_1d(np.asarray(fn(t + h), dtype=np.float64)) - np.atleast_1d(np.asarray(fn(t - h), dtype=np.float64))) / (2 * h)


class MovingSphere:
    """f(x, t) = |x - center(t)| - radius(t), fluid where f <= 0 (complement: outside, the growing disc of
    examples/2D/SolidMoving/MovingHeat.jl:19).  dcenter / dradius: exact time derivatives (default: central differences);
    they only enter the space-time interface measure Γ."""

    def __init__(self, center: Callable, radius: Callable, complement: bool = False, dcenter: Optional[Callable] = None,
                 dradius: Optional[Callable] = None):
        self.center, self.radius, self.complement = center, radius, bool(complement)
        self.dcenter, self.dradius = dcenter, dradius
        self.kind = L.PG_BODY_BALL
        self.axis, self.sign = 0, 1.0

    def __call__(self, *xt):
        *x, t = xt
        c = np.atleast_1d(self.center(t))
        f = np.sqrt(sum((np.asarray(x[d]) - c[d]) ** 2 for d in range(len(c)))) - self.radius(t)
        return -f if self.complement else f

    def _state(self, t: float, N: int):
        c = np.atleast_1d(np.asarray(self.center(t), dtype=np.float64))
        if len(c) != N:
            raise ValueError("body dimension does not match the mesh")
        out = np.zeros(4)
        out[:N] = c
        out[3] = float(self.radius(t))
        return out

    def _rate(self, t: float, N: int, h: float):
        out = np.zeros(4)
        out[:N] = np.atleast_1d(self.dcenter(t)) if self.dcenter else _ddt(self.center, t, h)
        out[3] = float(self.dradius(t)) if self.dradius else float(_ddt(self.radius, t, h)[0])
        return out


MovingCircle = MovingSphere


class MovingHalfSpace:
    """f(x, t) = sign (x_axis - position(t)), fluid where f < 0 -- examples/1D/SolidMoving/MovingHeat.jl:18
    `body = (x,t,_=0) -> x - xf - c*sqrt(t)`."""

    def __init__(self, axis: int, position: Callable, sign: float = 1.0, complement: bool = False,
                 dposition: Optional[Callable] = None):
        self.axis, self.position, self.sign, self.complement = int(axis), position, (-1.0 if sign < 0 else 1.0), bool(complement)
        self.dposition = dposition
        self.kind = L.PG_BODY_HALFSPACE

    def __call__(self, *xt):
        *x, t = xt
        f = self.sign * (np.asarray(x[self.axis]) - self.position(t))
        return -f if self.complement else f

    def _state(self, t: float, N: int):
        out = np.zeros(4)
        out[0] = float(self.position(t))
        out[3] = 1.0
        return out

    def _rate(self, t: float, N: int, h: float):
        out = np.zeros(4)
        out[0] = float(self.dposition(t)) if self.dposition else float(_ddt(self.position, t, h)[0])
        return out


def time_rule(t0: float, t1: float, panels: int, order: int):
    x, w = np.polynomial.legendre.leggauss(order)
    edges = np.linspace(t0, t1, panels + 1)
    tau = np.concatenate([0.5 * (a + b) + 0.5 * (b - a) * x for a, b in zip(edges[:-1], edges[1:])])
    wt = np.concatenate([0.5 * (b - a) * w for a, b in zip(edges[:-1], edges[1:])])
    return tau, wt * ((t1 - t0) / wt.sum())        # (the weights add up to t1 - t0 to the last bit the ABI checks)


class SpaceTimeCapacity(api.Capacity):
    """Capacity(body, STmesh): first time layer of the (N+1)-D capacity, resident on the GPU.  `V`, `A`, `B`, `W`, `Γ`,
    `C_ω`, `C_γ`, `cell_types` are the layer's N-D fields (length M = prod(n_d+1)); `Vn_1` / `Vn` the time-face capacities
    A_(N+1) at t0 / t1 (the reference's names, diffusion.jl:113-114); `C_ω_st` / `C_γ_st` the (M, N+1) centroids with the
    time component; `A_st` the reference-layout A tuple (N+1 arrays of length 2M, second layer = time padding).
    time_panels x time_order: the composite Gauss-Legendre rule in time (space is exact)."""

    def __init__(self, body, mesh: SpaceTimeMesh, method: str = "VOFI", compute_centroids: bool = True,
                 time_panels: int = 16, time_order: int = 4, complement: bool = False, quadrature: Optional[str] = None):
        if quadrature is not None:
            raise PenguinHipError(f"Capacity(quadrature={quadrature!r}) on a SpaceTimeMesh: the keyword chooses the rule of a static "
                                  "3-D level set; space-time capacities are 1-D+t and 2-D+t and take no such keyword")
        if isinstance(body, api.FrontTracker):
            api.check_front_body(body, mesh)
        if isinstance(body, MovingFront) or (isinstance(body, (tuple, list)) and len(body) == 2
                                             and all(isinstance(f, api.FrontTracker) for f in body)):
            self._init_front(body, mesh, compute_centroids, time_panels, time_order, complement)
            return
        if complement:
            if not isinstance(body, DeviceFunction):
                raise PenguinHipError("Capacity(complement=True) is for DeviceFunction bodies; tagged bodies take complement=True themselves")
            body = DeviceFunction(body, complement=True)
        if isinstance(body, DeviceFunction):
            self._init_program(body, mesh, compute_centroids, time_panels, time_order)
            return
        if not hasattr(body, "_state"):
            raise PenguinHipError("Capacity(body, SpaceTimeMesh): pass a MovingSphere / MovingHalfSpace (an arbitrary moving "
                                  "level set needs SpaceTimeCapacity.from_arrays)")
        L.init()
        self.stmesh, self.mesh, self.body, self.compute_centroids = mesh, mesh.space, body, compute_centroids
        N = self.mesh.N
        t0, t1 = mesh.time
        tau, wt = time_rule(t0, t1, time_panels, time_order)
        h = 1e-6 * (t1 - t0)
        nodes = np.zeros((len(tau), 10))
        for k, (t, w) in enumerate(zip(tau, wt)):
            st, rt = body._state(float(t), N), body._rate(float(t), N, h)
            nodes[k] = [t, w, st[0], st[1], st[2], st[3], rt[0], rt[1], rt[2], rt[3]]
        self._nodes = np.ascontiguousarray(nodes)
        desc = L.pg_motion_desc()
        desc.body_kind = body.kind
        desc.flags = (L.PG_FLAG_COMPLEMENT if body.complement else 0) | (0 if compute_centroids else L.PG_FLAG_NO_CENTROIDS)
        desc.axis, desc.sign = int(body.axis), float(body.sign)
        desc.nq, desc.t0, desc.t1 = len(tau), t0, t1
        desc.nodes = L.dptr(self._nodes)
        b0, b1 = body._state(t0, N), body._state(t1, N)
        for i in range(4):
            desc.body0[i], desc.body1[i] = b0[i], b1[i]
        self._h = C.c_void_p()
        L.check(L.lib().pg_capacity_create_spacetime(self.mesh._h, C.byref(desc), C.byref(self._h)))
        self._cache = {}

    def _init_program(self, body: DeviceFunction, mesh: SpaceTimeMesh, compute_centroids: bool, time_panels: int, time_order: int):
        """body(x_1 .. x_N, t) traced: phi, its N spatial derivatives and d phi / dt are evaluated inside the space-time kernels
        (pg_capacity_create_spacetime_program).  The programs are compiled once per DeviceFunction, not once per slab."""
        L.init()
        self.stmesh, self.mesh, self.body, self.compute_centroids = mesh, mesh.space, body, compute_centroids
        N = self.mesh.N
        t0, t1 = mesh.time
        tau, wt = time_rule(t0, t1, time_panels, time_order)
        self._nodes = np.ascontiguousarray(np.column_stack([tau, wt]))
        self._h = C.c_void_p()
        self._cache = {}
        if N not in (1, 2):
            # (3-D+t: the entry's own refusal, in its words -- nothing is traced for it)
            z = pg_program()
            L.check(L.lib().pg_capacity_create_spacetime_program(self.mesh._h, C.byref(z), C.byref(z), C.byref(z), C.c_int32(0),
                                                                 C.c_double(t0), C.c_double(t1), C.c_int32(len(tau)),
                                                                 L.dptr(self._nodes), C.byref(self._h)))
        phi = body.moving_body_program(N)
        derivs = body.moving_gradient_programs(N)
        grad = (pg_program * N)(*derivs[:N])
        flags = (L.PG_FLAG_COMPLEMENT if body.complement else 0) | (0 if compute_centroids else L.PG_FLAG_NO_CENTROIDS)
        L.check(L.lib().pg_capacity_create_spacetime_program(self.mesh._h, C.byref(phi), grad, C.byref(derivs[N]), C.c_int32(flags),
                                                             C.c_double(t0), C.c_double(t1), C.c_int32(len(tau)),
                                                             L.dptr(self._nodes), C.byref(self._h)))

    def _init_front(self, body, mesh: SpaceTimeMesh, compute_centroids: bool, time_panels: int, time_order: int, complement: bool):
        """Capacity(mf, STmesh) with a MovingFront, or Capacity((front_n, front_np1), STmesh) -- the reference's
        compute_spacetime_capacities(mesh, front_n, front_np1, dt) (src/front_tracking.jl:1472): the markers at the slab's two
        times go to pg_capacity_create_spacetime_polygon, which moves every marker on a straight line in between.  cap.body is a
        MovingFront either way."""
        t0, t1 = mesh.time
        if isinstance(body, MovingFront):
            if complement:
                raise PenguinHipError("Capacity(MovingFront, complement=True): the MovingFront carries its own flag, "
                                      "MovingFront(..., complement=True)")
            p0, p1 = body.markers(t0), body.markers(t1)
        else:
            for f in body:
                if not f.is_closed:
                    raise PenguinHipError("Capacity((front_n, front_np1), SpaceTimeMesh): is_closed=False is not supported")
            p0, p1 = body[0].polygon(), body[1].polygon()
            if len(p0) != len(p1):
                raise PenguinHipError(f"Capacity((front_n, front_np1), SpaceTimeMesh): the fronts have {len(p0)} and {len(p1)} "
                                      "markers; both need the same count and order")
            body = MovingFront.from_fronts([p0, p1], [t0, t1], complement=complement)
        L.init()
        self.stmesh, self.mesh, self.body, self.compute_centroids = mesh, mesh.space, body, compute_centroids
        self.complement = body.complement
        tau, wt = time_rule(t0, t1, time_panels, time_order)
        self._nodes = np.ascontiguousarray(np.column_stack([tau, wt]))
        self._xy0 = np.ascontiguousarray(p0.reshape(-1), dtype=np.float64)
        self._xy1 = np.ascontiguousarray(p1.reshape(-1), dtype=np.float64)
        self._h = C.c_void_p()
        self._cache = {}
        flags = (L.PG_FLAG_COMPLEMENT if body.complement else 0) | (0 if compute_centroids else L.PG_FLAG_NO_CENTROIDS)
        L.check(L.lib().pg_capacity_create_spacetime_polygon(self.mesh._h, L.dptr(self._xy0), L.dptr(self._xy1),
                                                             C.c_int64(len(self._xy0) // 2), C.c_int32(flags), C.c_double(t0),
                                                             C.c_double(t1), C.c_int32(len(tau)), L.dptr(self._nodes),
                                                             C.byref(self._h)))

    @property
    def spacetime_kernel_ms(self):
        """measurement, program and polygon bodies: ({kernel: ms}, cells the cheap pass left to the list).  The times are those of this slab's
        six kernels when the capacity was built under `spacetime_kernel_timing(True)`, 0 otherwise and for a kernel not launched."""
        ms, n = (C.c_double * 6)(), C.c_int64(0)
        L.check(L.lib().pg_debug_capacity_spacetime_ms_parts(self._h, ms, C.byref(n)))
        names = ("k_st_classify", "k_st_cells", "k_st_sections", "k_st_sections_cut", "k_st_stagger", "k_st_stagger_cut")
        return dict(zip(names, (float(v) for v in ms))), int(n.value)

    @classmethod
    def from_arrays(cls, stmesh: SpaceTimeMesh, V, A, B, W, Gamma, C_omega, C_gamma, cell_types, Vn_1, Vn, body=None):
        """First-layer fields computed by the caller (arbitrary moving bodies).  C_omega / C_gamma: (M, N+1)."""
        mesh = stmesh.space
        N = mesh.N
        base = api.Capacity.from_arrays(mesh, V, A, B, W, Gamma, np.asarray(C_omega)[:, :N],
                                        np.asarray(C_gamma)[:, :N] if C_gamma is not None and len(C_gamma) else None,
                                        cell_types, body=body)
        self = cls.__new__(cls)
        self.__dict__.update(base.__dict__)
        base._h = None                                   # ownership moved
        self.stmesh = stmesh
        v0, v1 = np.ascontiguousarray(Vn_1, dtype=np.float64), np.ascontiguousarray(Vn, dtype=np.float64)
        ctw = np.ascontiguousarray(np.asarray(C_omega)[:, N], dtype=np.float64)
        ctg = np.ascontiguousarray(np.asarray(C_gamma)[:, N], dtype=np.float64) if C_gamma is not None and len(C_gamma) else None
        L.check(L.lib().pg_capacity_set_spacetime(self._h, C.c_double(stmesh.time[0]), C.c_double(stmesh.time[1]), L.dptr(v0),
                                                  L.dptr(v1), L.dptr(ctw), L.dptr(ctg) if ctg is not None else None))
        return self

    @property
    def Vn_1(self):
        return self._get(L.PG_CAP_ST_V0)

    @property
    def Vn(self):
        return self._get(L.PG_CAP_ST_V1)

    @property
    def C_ω_st(self):
        return np.column_stack([self.C_ω, self._get(L.PG_CAP_ST_CT_OMEGA)])

    @property
    def C_γ_st(self):
        if not self.compute_centroids:
            return np.zeros((0, self.N + 1))
        return np.column_stack([self.C_γ, self._get(L.PG_CAP_ST_CT_GAMMA)])

    @property
    def A_st(self):
        z = np.zeros_like(self.V)
        return tuple(np.concatenate([a, z]) for a in self.A) + (np.concatenate([self.Vn_1, self.Vn]),)

    # closures see the space-time centroids (build_source / build_g_g read capacity.C_ω / C_γ of the (N+1)-D capacity)
    def _cw(self):
        return self.C_ω_st

    def _cg(self):
        return self.C_γ_st


def spacetime_kernel_timing(on: bool) -> None:
    """measurement, off by default: bracket each of the six kernels of later program-body space-time capacities with events"""
    L.init()
    L.check(L.lib().pg_debug_spacetime_kernel_timing(C.c_int32(1 if on else 0)))


def _capacity_new(cls, body=None, mesh=None, *args, **kwargs):
    """Capacity(body, STmesh) of the reference: the same constructor name serves both mesh kinds."""
    if cls is api.Capacity and isinstance(mesh, SpaceTimeMesh):
        return object.__new__(SpaceTimeCapacity)
    return object.__new__(cls)


api.Capacity.__new__ = staticmethod(_capacity_new)


def _require_st_convection(phase: api.Phase):
    op = phase.operator
    if not (isinstance(op, api.ConvectionOps) and op._st):
        raise PenguinHipError("the moving advection-diffusion solver needs phase.operator = ConvectionOps(capacity, uₒ, uᵧ) of "
                              "the phase's space-time capacity (got a " + type(op).__name__ + ")")


def _create_step(s: api.Solver, phases: Sequence[api.Phase], bc_b, interface, Δt: float, Tᵢ: Optional[np.ndarray], mesh: api.Mesh,
                 scheme: str, t: float, t_border: Optional[float], from_previous: bool = False, advdiff: bool = False,
                 stefan: bool = False):
    """The system of one slab, one phase or two.  One phase, interface = bc_i: A_/b_mono_unstead_diff_moving +
    BC_border_mono!(A, b, bc_b, mesh; t) (diffusion.jl:29-33, 254-258); advdiff: A_/b_mono_unstead_advdiff_moving
    (advectiondiffusion.jl:24-31, 229-232), the same border rows.  Two phases, interface = ic: A_/b_diph_unstead_diff_moving +
    BC_border_diph!(A, b, bc_b, mesh) (diffusion.jl:281-288, 519-523); advdiff: A_/b_diph_unstead_advdiff_moving
    (advectiondiffusion.jl:255-262, 540-543); stefan: A_/b_diph_unstead_diff_moving_stef (liquidmotionsolver/diffusion.jl:
    445-651), the same border rows.  t_border: the time of the border rows -- b's t, or tₙ₊₁ in
    the liquid-motion Newton rebuilds (BC_border_mono!(...; t=tn1)); None: evaluated without t, as BC_border_diph! is called.
    from_previous: the state of s's present slab stays on the device (`previous`), Tᵢ is not read."""
    for ph in phases:
        cap = ph.capacity
        if not isinstance(cap, SpaceTimeCapacity):
            raise PenguinHipError("the moving solver needs a space-time capacity in every phase: "
                                  "Capacity(body, SpaceTimeMesh(mesh, [t, t+Δt]))")
        if cap.mesh is not mesh and tuple(cap.mesh.dims) != tuple(mesh.dims):
            raise ValueError("mesh does not match the capacity's space mesh")
        if advdiff:
            _require_st_convection(ph)
    M = int(np.prod(mesh.ext))
    sch = "CN" if scheme == "CN" else "BE"
    # build_g_g(operator, bc / jump, capacity): value(C_γ...) at the space-time interface centroids, no time argument (:172,
    # :423-424)
    if len(phases) == 1:
        desc, keep = api._interface_desc(interface, phases[0].capacity._cg, None)
    else:
        desc, keep = api._jump_desc(interface, *phases)
    Ds, fs = [], []
    for ph in phases:
        Ds.append(api._dcoef(ph, M))
        f1 = api._padded_field(api._eval(ph.source, ph.capacity._cw, float(t + Δt), 3), M)      # f(C_ω..., t+Δt)   :171, :416,418
        f0 = api._padded_field(api._eval(ph.source, ph.capacity._cw, float(t), 3), M) if sch == "CN" else None
        if sch == "CN" and f1 is not None and f0 is None:
            f0 = np.zeros(M)
        fs += [f0, f1]
    borders, nb, bvals = api._border_descs(bc_b, mesh, t_border)
    p = lambda a: L.dptr(a) if a is not None else None
    kind = "_advdiff" if advdiff else "_stefan" if stefan else ""
    create = getattr(L.lib(), "pg_solver_create_moving" + kind + ("_mono" if len(phases) == 1 else "_diph"))
    old, new = s._h, C.c_void_p()
    L.check(create(*[h for ph in phases for h in (ph.capacity._h, ph.operator._h)], C.byref(desc), borders, C.c_int32(nb),
                   *map(p, Ds), *map(p, fs), None if from_previous else p(Tᵢ), old if from_previous else None,
                   C.c_int32(L.PG_SCHEME[sch]), C.byref(new)))
    s._h = new
    if old:
        L.check(L.lib().pg_solver_destroy(old))
    if bvals is not None:
        L.check(L.lib().pg_solver_set_border_values(s._h, L.dptr(bvals)))
    # the device solver reads the capacities and operators: keep them alive as long as the handle
    s._keep = tuple(ph.capacity for ph in phases) + tuple(ph.operator for ph in phases)
    s._initial_done = False


def _solve_current(s: api.Solver, opts, what: str, save_states: bool, verbose: bool):
    info = L.pg_step_info()
    L.check(L.lib().pg_solver_initial_solve(s._h, C.byref(opts), C.byref(info)))
    api._step_info_check(s, info, what)
    s._initial_done = True
    s.ch.append(info)
    if save_states:
        s.x = s._fetch_state(-1)
        s.states.append(s.x)
    if verbose:
        print("Solver Extremum : ", float(info.extremum))


def _solve_slabs(s, phases, bodies, Δt, Tₛ, Tₑ, bc_b, interface, mesh, scheme, make_ops, advdiff, border_has_t, method,
                 geometry_method, verbose, max_steps, time_panels, time_order, save_states, kwargs):
    """The slab loop of the four prescribed-motion solvers (diffusion.jl:227-268, 501-535, advectiondiffusion.jl:201-242,
    510-553): phases[q] lives in bodies[q]; `make_ops(cap)` builds a slab's operator (DiffusionOps, or ConvectionOps from the
    same uₒ, uᵧ every slab); border_has_t: BC_border_mono!(...; t) against BC_border_diph!(...) without t."""
    if s is None or not s._h:
        raise PenguinHipError("Solver is not initialized. Call a solver constructor first.")
    opts = api._krylov_opts(method, kwargs)
    sch = "CN" if scheme == "CN" else "BE"
    t = float(Tₛ)
    if verbose:
        print(f"Time : {t}")
    _solve_current(s, opts, "the first solve", save_states, verbose)
    Tᵢ = s.x
    steps = 0
    while t < Tₑ:
        if max_steps is not None and steps >= max_steps:
            break
        t += Δt
        if verbose:
            print(f"Time : {t}")
        caps = [api.Capacity(b, SpaceTimeMesh(mesh, [t, t + Δt]), time_panels=time_panels, time_order=time_order,
                             compute_centroids=True, method=geometry_method) for b in bodies]
        phs = [api.Phase(cap, make_ops(cap), ph.source, ph.Diffusion_coeff) for cap, ph in zip(caps, phases)]
        _create_step(s, phs, bc_b, interface, float(Δt), Tᵢ, mesh, sch, t, t if border_has_t else None,
                     from_previous=not save_states, advdiff=advdiff)
        _solve_current(s, opts, f"the solve of the slab starting at t = {t}", save_states, verbose)
        Tᵢ = s.x
        steps += 1
    if not save_states:
        s.x = s._fetch_state(-1)
        s.states.append(s.x)
    return s


def MovingDiffusionUnsteadyMono(phase: api.Phase, bc_b, bc_i, Δt: float, Tᵢ: np.ndarray, mesh: api.Mesh, scheme: str,
                                verbose: bool = False) -> api.Solver:
    """MovingDiffusionUnsteadyMono(phase, bc_b, bc_i, Δt, Tᵢ, mesh, scheme) -- prescribedmotionsolver/diffusion.jl:16-35."""
    if verbose:
        print("Solver Creation:\n- Moving problem\n- Monophasic problem\n- Unsteady problem\n- Diffusion problem")
    s = api.Solver("Unsteady", "Monophasic", "Diffusion")
    Tᵢ = api._unsteady_prelude(s, 2, mesh, Tᵢ, phase=phase, bc_i=bc_i, dt=float(Δt))
    _create_step(s, [phase], bc_b, bc_i, float(Δt), Tᵢ, mesh, scheme, 0.0, 0.0)     # t = 0.0 in b and the border rows (:27-33)
    return s


def solve_MovingDiffusionUnsteadyMono_b(s: api.Solver, phase: api.Phase, body, Δt: float, Tₛ: float, Tₑ: float, bc_b, bc,
                                        mesh: api.Mesh, scheme: str, method="gmres", algorithm=None, geometry_method="VOFI",
                                        verbose: bool = False, max_steps: Optional[int] = None, time_panels: int = 16,
                                        time_order: int = 4, save_states: bool = True, **kwargs):
    """solve_MovingDiffusionUnsteadyMono!(s, phase, body, Δt, Tₛ, Tₑ, bc_b, bc, mesh, scheme; method, ...) --
    prescribedmotionsolver/diffusion.jl:227-268: the constructor's system first (states[1]); then `while t < Tₑ`:
    t += Δt, the capacity of the slab [t, t+Δt], new blocks and border rows at t, solve, push.
    `save_states=False` (not in the reference): the state is handed from slab to slab on the device and only the last one is
    fetched (`s.x`, `s.states[-1]`); the reference's `push!(s.states, s.x)` costs a device-to-host copy of 2M doubles per slab."""
    return _solve_slabs(s, [phase], [body], Δt, Tₛ, Tₑ, bc_b, bc, mesh, scheme, api.DiffusionOps, False, True, method,
                        geometry_method, verbose, max_steps, time_panels, time_order, save_states, kwargs)


def MovingAdvDiffusionUnsteadyMono(phase: api.Phase, bc_b, bc_i, Δt: float, Tᵢ: np.ndarray, mesh: api.Mesh, scheme: str,
                                   verbose: bool = False) -> api.Solver:
    """MovingAdvDiffusionUnsteadyMono(phase, bc_b, bc_i, Δt, Tᵢ, mesh, scheme) -- prescribedmotionsolver/advectiondiffusion.jl:15-33.
    phase.operator = ConvectionOps(capacity, uₒ, uᵧ) of the first slab's space-time capacity (2-D+t).  Convection enters A
    only in the cells with Vn = 0, Vn_1 ≠ 0 (psip_conv); elsewhere it is explicit, through the previous state in b.  The
    reference's quirks are kept: no bulk y-advection, ½K_x only (DESIGN.md "Moving advection-diffusion")."""
    if verbose:
        print("Solver Creation:\n- Moving problem\n- Monophasic problem\n- Unsteady problem\n- Advection-Diffusion problem")
    _require_st_convection(phase)
    s = api.Solver("Unsteady", "Monophasic", "DiffusionAdvection")
    Tᵢ = api._unsteady_prelude(s, 2, mesh, Tᵢ, phase=phase, bc_i=bc_i, dt=float(Δt))
    _create_step(s, [phase], bc_b, bc_i, float(Δt), Tᵢ, mesh, scheme, 0.0, 0.0, advdiff=True)    # t = 0.0 in b and the border rows
    return s


def solve_MovingAdvDiffusionUnsteadyMono_b(s: api.Solver, phase: api.Phase, body, Δt: float, Tₛ: float, Tₑ: float, bc_b, bc,
                                           mesh: api.Mesh, scheme: str, uₒ, uᵧ, method="gmres", algorithm=None,
                                           geometry_method="VOFI", verbose: bool = False, max_steps: Optional[int] = None,
                                           time_panels: int = 16, time_order: int = 4, save_states: bool = True, **kwargs):
    """solve_MovingAdvDiffusionUnsteadyMono!(s, phase, body, Δt, Tₛ, Tₑ, bc_b, bc, mesh, scheme, uₒ, uᵧ; method, ...) --
    prescribedmotionsolver/advectiondiffusion.jl:201-242: the loop of solve_MovingDiffusionUnsteadyMono_b with
    ConvectionOps(capacity, uₒ, uᵧ) rebuilt on every slab from the same uₒ, uᵧ (:225-227).  The explicit convection of b is
    formed on the device from the previous state, also with `save_states=False` (state handed over device to device)."""
    return _solve_slabs(s, [phase], [body], Δt, Tₛ, Tₑ, bc_b, bc, mesh, scheme, lambda cap: api.ConvectionOps(cap, uₒ, uᵧ), True,
                        True, method, geometry_method, verbose, max_steps, time_panels, time_order, save_states, kwargs)


# ---------------------------------------------------------------------------------------------------------------------
# two phases                                                          prescribedmotionsolver/diffusion.jl:272-535
# ---------------------------------------------------------------------------------------------------------------------
def MovingDiffusionUnsteadyDiph(phase1: api.Phase, phase2: api.Phase, bc_b, ic, Δt: float, Tᵢ: np.ndarray, mesh: api.Mesh,
                                scheme: str, verbose: bool = False) -> api.Solver:
    """MovingDiffusionUnsteadyDiph(phase1, phase2, bc_b, ic, Δt, Tᵢ, mesh, scheme) -- prescribedmotionsolver/diffusion.jl:272-290."""
    if verbose:
        print("Solver Creation:\n- Moving problem\n- Diphasic problem\n- Unsteady problem\n- Diffusion problem")
    s = api.Solver("Unsteady", "Diphasic", "Diffusion")
    Tᵢ = api._unsteady_prelude(s, 4, mesh, Tᵢ, dt=float(Δt))
    # t = 0.0 in b (:282, :285); BC_border_diph!(s.A, s.b, bc_b, mesh): no t (:288, :523)
    _create_step(s, [phase1, phase2], bc_b, ic, float(Δt), Tᵢ, mesh, scheme, 0.0, None)
    return s


def solve_MovingDiffusionUnsteadyDiph_b(s: api.Solver, phase1: api.Phase, phase2: api.Phase, body, body_c, Δt: float, Tₑ: float,
                                        bc_b, ic, mesh: api.Mesh, scheme: str, method="gmres", algorithm=None, verbose: bool = False,
                                        max_steps: Optional[int] = None, time_panels: int = 16, time_order: int = 4,
                                        save_states: bool = True, **kwargs):
    """solve_MovingDiffusionUnsteadyDiph!(s, phase1, phase2, body, body_c, Δt, Tₑ, bc_b, ic, mesh, scheme; method, ...) --
    prescribedmotionsolver/diffusion.jl:501-535: the constructor's system first (states[1]); then from t = 0.0 `while t < Tₑ`:
    t += Δt, the two capacities of the slab [t, t+Δt], new blocks and border rows, solve, push."""
    # t = 0.0 (:513); no geometry_method in the diphasic loops: the capacities' default
    return _solve_slabs(s, [phase1, phase2], [body, body_c], Δt, 0.0, Tₑ, bc_b, ic, mesh, scheme, api.DiffusionOps, False, False,
                        method, "VOFI", verbose, max_steps, time_panels, time_order, save_states, kwargs)


def MovingAdvDiffusionUnsteadyDiph(phase1: api.Phase, phase2: api.Phase, bc_b, ic, Δt: float, Tᵢ: np.ndarray, mesh: api.Mesh,
                                   scheme: str, verbose: bool = False) -> api.Solver:
    """MovingAdvDiffusionUnsteadyDiph(phase1, phase2, bc_b, ic, Δt, Tᵢ, mesh, scheme) --
    prescribedmotionsolver/advectiondiffusion.jl:246-264; both operators are space-time ConvectionOps."""
    if verbose:
        print("Solver Creation:\n- Moving problem\n- Diphasic problem\n- Unsteady problem\n- Advection-Diffusion problem")
    _require_st_convection(phase1)
    _require_st_convection(phase2)
    s = api.Solver("Unsteady", "Diphasic", "DiffusionAdvection")
    Tᵢ = api._unsteady_prelude(s, 4, mesh, Tᵢ, dt=float(Δt))
    _create_step(s, [phase1, phase2], bc_b, ic, float(Δt), Tᵢ, mesh, scheme, 0.0, None, advdiff=True)     # t = 0.0 in b
    return s


def solve_MovingAdvDiffusionUnsteadyDiph_b(s: api.Solver, phase1: api.Phase, phase2: api.Phase, body, body_c, Δt: float, Tₛ: float,
                                           Tₑ: float, bc_b, ic, mesh: api.Mesh, scheme: str, uₒ, uᵧ, method="gmres",
                                           algorithm=None, verbose: bool = False, max_steps: Optional[int] = None,
                                           time_panels: int = 16, time_order: int = 4, save_states: bool = True, **kwargs):
    """solve_MovingAdvDiffusionUnsteadyDiph!(s, phase1, phase2, body, body_c, Δt, Tₛ, Tₑ, bc_b, ic, mesh, scheme, uₒ, uᵧ; ...) --
    prescribedmotionsolver/advectiondiffusion.jl:510-553: from t = Tₛ (the diffusion twin starts at 0.0), both phases'
    ConvectionOps rebuilt per slab from the same uₒ, uᵧ (:535-538), BC_border_diph! without t."""
    return _solve_slabs(s, [phase1, phase2], [body, body_c], Δt, Tₛ, Tₑ, bc_b, ic, mesh, scheme,
                        lambda cap: api.ConvectionOps(cap, uₒ, uᵧ), True, False, method, "VOFI", verbose, max_steps, time_panels,
                        time_order, save_states, kwargs)
