"""Host-side mirror of Penguin.jl's API for the hot path
    Mesh -> Capacity -> DiffusionOps -> Phase -> DiffusionUnsteadyMono/Diph -> solve_*!
(src/Penguin.jl:25-75).  Same names, argument order and meaning as the reference; every numeric
operation is done by libpenguin_hip.so on the GPU through the C ABI (include/penguin_hip.h).
Closures never cross the ABI: they are evaluated here, at the reference's points and times
(C_ω for f and D, C_γ for interface values, mesh.centers for border values; t+Δt -- src/solver.jl:230-323,
441-448, src/solver/diffusion.jl:248-249) and passed as arrays.

Julia spellings that are not Python identifiers:  `∇`->grad, `∇₋`->div, `Wꜝ`->Winv (alias `Wꜝ` works
as an attribute), `solve_DiffusionUnsteadyMono!`->solve_DiffusionUnsteadyMono_b.
"""
from __future__ import annotations

import ctypes as C
import inspect
import math
import warnings
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Sequence, Union

import numpy as np

from . import _lib as L
from ._lib import PenguinHipError
from . import devfn as dev  # noqa: F401
from .devfn import DeviceFunction, pg_program
from .front import FrontTracker

Number = Union[int, float]

# =============================================================================== Mesh


class MeshTag:
    """src/mesh.jl:6-8; border_cells is materialised on first access (1.5 M tuples at 512^3)."""

    def __init__(self, mesh: "Mesh"):
        self._mesh = mesh
        self._cells = None

    @property
    def border_cells(self):
        if self._cells is None:
            idx, pos, _ = self._mesh._border_arrays()
            self._cells = [(tuple(int(v) for v in idx[q]), tuple(float(v) for v in pos[q])) for q in range(len(idx))]
        return self._cells


class Mesh:
    """Mesh(n, domain_size, x0) -- src/mesh.jl:47-78."""

    def __init__(self, n: Sequence[int], domain_size: Sequence[float], x0: Optional[Sequence[float]] = None):
        N = len(n)
        if len(domain_size) != N or (x0 is not None and len(x0) != N):
            raise ValueError("n, domain_size and x0 must have the same length")
        if x0 is None:
            x0 = (0.0,) * N
        self.N = N
        self._h = C.c_void_p()
        n_arr = np.asarray(n, dtype=np.int64)
        L_arr = np.asarray(domain_size, dtype=np.float64)
        x_arr = np.asarray(x0, dtype=np.float64)
        L.check(L.lib().pg_mesh_create(C.c_int32(N), L.iptr(n_arr), L.dptr(L_arr), L.dptr(x_arr), C.byref(self._h)))
        self.dims = tuple(int(v) for v in n)
        cen, nod = [], []
        for d in range(N):
            c = np.empty(self.dims[d])
            k = np.empty(self.dims[d] + 1)
            L.check(L.lib().pg_mesh_get_centers(self._h, d, L.dptr(c), C.c_int64(len(c))))
            L.check(L.lib().pg_mesh_get_nodes(self._h, d, L.dptr(k), C.c_int64(len(k))))
            cen.append(c)
            nod.append(k)
        self.centers = tuple(cen)
        self.nodes = tuple(nod)
        self.tag = MeshTag(self)

    def _border_arrays(self):
        nb = C.c_int64()
        L.check(L.lib().pg_mesh_num_border_cells(self._h, C.byref(nb)))
        nb = nb.value
        idx = np.empty((nb, self.N), dtype=np.int64)
        pos = np.empty((nb, self.N), dtype=np.float64)
        key = np.empty(nb, dtype=np.int32)
        L.check(L.lib().pg_mesh_get_border_cells(self._h, L.iptr(idx.reshape(-1)), L.dptr(pos.reshape(-1)),
                                                 key.ctypes.data_as(L.c_i32_p)))
        return idx, pos, key

    @property
    def ext(self):
        return tuple(d + 1 for d in self.dims)

    def __del__(self):
        try:
            if self._h:
                L.lib().pg_mesh_destroy(self._h)
        except Exception:
            pass


def nC(mesh: Mesh) -> int:
    """src/mesh.jl:86."""
    return int(np.prod(mesh.dims))


# =============================================================================== bodies


class Sphere:
    """Tagged level set f(x) = |x - c| - r (fluid where f <= 0), evaluated in-kernel.
    In 2-D a circle, in 1-D an interval.  `complement=True` gives -f (fluid outside)."""

    def __init__(self, center: Sequence[float], radius: float, complement: bool = False):
        self.center = tuple(float(v) for v in center)
        self.radius = float(radius)
        self.complement = bool(complement)

    def __call__(self, *x):
        s = sum((np.asarray(x[d]) - self.center[d]) ** 2 for d in range(len(self.center)))
        f = np.sqrt(s) - self.radius
        return -f if self.complement else f

    def _abi(self, N: int):
        if len(self.center) != N:
            raise ValueError("body dimension does not match the mesh")
        return L.PG_BODY_BALL, np.array(list(self.center) + [self.radius]), (L.PG_FLAG_COMPLEMENT if self.complement else 0)


Circle = Sphere


class MultiSphere:
    """Union of pairwise disjoint spheres of equal radius, f = min_s f_s (weak-scaling body)."""

    def __init__(self, centers: Sequence[Sequence[float]], radius: float):
        self.centers = [tuple(float(v) for v in c) for c in centers]
        self.radius = float(radius)

    def __call__(self, *x):
        return np.minimum.reduce([Sphere(c, self.radius)(*x) for c in self.centers])

    def _abi(self, N: int):
        flat = [self.radius, float(len(self.centers))]
        for c in self.centers:
            if len(c) != N:
                raise ValueError("body dimension does not match the mesh")
            flat += list(c)
        return L.PG_BODY_MULTIBALL, np.array(flat), 0


class HalfSpace:
    """Tagged level set f(x) = sign * (x[axis] - position) (fluid where f < 0), evaluated in-kernel: the reference's 1-D
    diphasic bodies `(x, _=0) -> (x - xint)` / `-(x - xint)` (test/convergence_test.jl:111-112,230-231) and their
    extrusions to 2-D / 3-D.  `axis` is 0-based; `complement=True` gives -f."""

    def __init__(self, axis: int, position: float, sign: float = 1.0, complement: bool = False):
        self.axis, self.position = int(axis), float(position)
        self.sign = -1.0 if sign < 0 else 1.0
        self.complement = bool(complement)

    def __call__(self, *x):
        f = self.sign * (np.asarray(x[self.axis]) - self.position)
        return -f if self.complement else f

    def _abi(self, N: int):
        if not 0 <= self.axis < N:
            raise ValueError("body axis does not exist on this mesh")
        return (L.PG_BODY_HALFSPACE, np.array([float(self.axis), self.position, self.sign]),
                (L.PG_FLAG_COMPLEMENT if self.complement else 0))


class Plane:
    """Tagged level set f(x) = normal . x - offset (fluid where f < 0), evaluated in-kernel: an oblique half space -- a tilted
    wall, an inclined two-phase interface -- in 1-D, 2-D and 3-D.  The normal is used as given (it need not have unit
    length, and is never normalised: f is the function the caller wrote); `complement=True` gives -f.  Every capacity of
    a cut cell is closed form."""

    def __init__(self, normal: Sequence[float], offset: float, complement: bool = False):
        self.normal = tuple(float(v) for v in normal)
        self.offset = float(offset)
        self.complement = bool(complement)

    @classmethod
    def through(cls, point: Sequence[float], normal: Sequence[float], complement: bool = False) -> "Plane":
        """the plane through `point` with the given normal: offset = normal . point"""
        if len(point) != len(normal):
            raise ValueError("Plane.through: point and normal must have the same dimension")
        return cls(normal, sum(float(n) * float(x) for n, x in zip(normal, point)), complement)

    def __call__(self, *x):
        f = sum(self.normal[d] * np.asarray(x[d]) for d in range(len(self.normal))) - self.offset
        return -f if self.complement else f

    def _abi(self, N: int):
        if len(self.normal) != N:
            raise PenguinHipError(f"PG_BODY_PLANE: a normal of {len(self.normal)} components on a {N}-D mesh")
        return (L.PG_BODY_PLANE, np.array(list(self.normal) + [self.offset]), (L.PG_FLAG_COMPLEMENT if self.complement else 0))


# =============================================================================== Capacity


class Ellipsoid:
    """Tagged level set f(x) = sqrt(sum ((x_d - c_d)/a_d)^2) - 1 with axis-aligned semi-axes a_d (fluid where f <= 0; an
    ellipse in 2-D).  `complement=True` gives -f."""

    def __init__(self, center: Sequence[float], semi_axes: Sequence[float], complement: bool = False):
        self.center = tuple(float(v) for v in center)
        self.semi_axes = tuple(float(v) for v in semi_axes)
        if len(self.center) != len(self.semi_axes) or min(self.semi_axes) <= 0.0:
            raise ValueError("Ellipsoid: one positive semi-axis per coordinate")
        self.complement = bool(complement)

    def __call__(self, *x):
        f = np.sqrt(sum(((np.asarray(x[d]) - self.center[d]) / self.semi_axes[d]) ** 2 for d in range(len(self.center)))) - 1.0
        return -f if self.complement else f

    def _abi(self, N: int):
        if len(self.center) != N:
            raise ValueError("body dimension does not match the mesh")
        return (L.PG_BODY_ELLIPSOID, np.array(list(self.center) + list(self.semi_axes)),
                (L.PG_FLAG_COMPLEMENT if self.complement else 0))


Ellipse = Ellipsoid


def check_front_body(front: FrontTracker, mesh) -> None:
    """what Capacity(front, mesh) refuses before it touches the device"""
    if not hasattr(mesh, "_h"):
        raise PenguinHipError("Capacity(FrontTracker, SpaceTimeMesh): one front has no motion; pass a MovingFront or the pair "
                              "(front_n, front_np1) for the space-time capacities of a moving front, or the spatial Mesh")
    if not front.is_closed:
        raise PenguinHipError("Capacity(FrontTracker): is_closed=False is not supported (the reference substitutes the convex hull "
                              "of the markers for an open front; close the front or pass the hull's markers)")
    if len(front.polygon()) < 3:
        raise PenguinHipError(f"Capacity(FrontTracker): a polygon needs at least 3 markers (got {len(front.polygon())})")
    if mesh.N != 2:
        raise PenguinHipError(f"Capacity(FrontTracker): a marker polygon is a 2-D body, the mesh is {mesh.N}-D")


class Capacity:
    """Capacity(body, mesh; method="VOFI", compute_centroids=true) -- src/capacity.jl:51-123.

    Fields A, B, W (N-tuples), V, Γ are the DIAGONALS of the reference's diagonal matrices (length
    M = prod(n_d+1)); C_ω, C_γ are (M,N) arrays; cell_types is the Float64 vector.  They are fetched
    from the GPU on first access.  `body` is a tagged body (Sphere / MultiSphere / Ellipsoid / HalfSpace / Plane) or any level set
    wrapped in DeviceFunction; in 3-D under the keyword `quadrature="height"`, the rule of csrc/pg_geom_program3.h:
    `Capacity(DeviceFunction(lambda x, y, z: ...), mesh, quadrature="height")` (without it a 3-D mesh is refused).  In 1-D
    and 2-D: `Capacity(DeviceFunction(lambda x, y: ...), mesh)` traces the closure and
    its derivatives and evaluates them inside the capacity kernels (fluid where it is <= 0; `complement=True`: where it is
    >= 0, the other phase; `cap.body` stays callable as the closure, negated for the complement).  A plain callable needs DeviceFunction or precomputed arrays: Capacity.from_arrays(...).
    `Capacity(front, mesh)` with a FrontTracker (2-D): the closed polygon of its markers, interior fluid, measured by the same
    kernels (src/capacity.jl:472-598); `complement=True`: the exterior."""

    def __init__(self, body, mesh: Mesh, method: str = "VOFI", compute_centroids: bool = True, complement: bool = False,
                 quadrature: Optional[str] = None):
        if method not in ("VOFI", "ImplicitIntegration"):
            raise ValueError('method must be "VOFI" or "ImplicitIntegration"')
        if quadrature is not None:
            # the 3-D rule of a traced level set is opt-in under its own name (csrc/pg_geom_program3.h)
            if quadrature != "height":
                raise PenguinHipError(f'Capacity(quadrature={quadrature!r}): the only rule to choose is "height", for a DeviceFunction body on a 3-D mesh')
            if not isinstance(body, DeviceFunction):
                raise PenguinHipError('Capacity(quadrature="height") is for DeviceFunction bodies: ' + type(body).__name__ + " bodies have their own rule")
            if mesh.N != 3:
                raise PenguinHipError(f'Capacity(quadrature="height") is the rule of a 3-D mesh; this mesh is {mesh.N}-D and needs no keyword')
        if isinstance(body, FrontTracker):
            self._init_front(body, mesh, compute_centroids, complement)
            return
        if complement:
            # the keyword of the Julia twin: the other phase of a DeviceFunction body (tagged bodies carry their own flag)
            if not isinstance(body, DeviceFunction):
                raise PenguinHipError("Capacity(complement=True) is for DeviceFunction bodies; tagged bodies take complement=True themselves")
            body = DeviceFunction(body, complement=True)
        program_body = isinstance(body, DeviceFunction)
        if not program_body and not hasattr(body, "_abi"):
            raise PenguinHipError(
                "Capacity: arbitrary level-set callables cannot be evaluated on the GPU; pass a tagged body "
                "(Sphere, MultiSphere, Ellipsoid, HalfSpace, Plane), wrap the closure in DeviceFunction (1-D and 2-D: it is "
                "traced and evaluated in the kernels) or use Capacity.from_arrays with precomputed capacities")
        if program_body and mesh.N == 3 and quadrature is None:
            raise PenguinHipError("Capacity(DeviceFunction): 3-D program bodies are not supported yet (1-D and 2-D) without "
                                  'quadrature="height", the keyword that chooses the 3-D rule')
        L.init()
        self.mesh = mesh
        self.body = body
        self.compute_centroids = compute_centroids
        if program_body:
            # fluid where body(x_1 .. x_N) <= 0; the N derivative programs come from the trace (devfn.differentiate)
            phi = body.body_program(mesh.N)
            grad = (pg_program * mesh.N)(*body.gradient_programs(mesh.N))
            self._h = C.c_void_p()
            create = L.lib().pg_capacity_create_program3 if mesh.N == 3 else L.lib().pg_capacity_create_program
            L.check(create(mesh._h, C.byref(phi), grad,
                           C.c_int32((0 if compute_centroids else L.PG_FLAG_NO_CENTROIDS)
                                     | (L.PG_FLAG_COMPLEMENT if body.complement else 0)),
                           C.byref(self._h)))
            self._cache = {}
            return
        kind, params, flags = body._abi(mesh.N)
        if not compute_centroids:
            flags |= L.PG_FLAG_NO_CENTROIDS
        self._h = C.c_void_p()
        params = np.ascontiguousarray(params, dtype=np.float64)
        L.check(L.lib().pg_capacity_create_levelset(mesh._h, C.c_int32(kind), L.dptr(params), C.c_int32(len(params)),
                                                    C.c_int32(flags), C.byref(self._h)))
        self._cache: Dict = {}

    def _init_front(self, front: FrontTracker, mesh: Mesh, compute_centroids: bool, complement: bool):
        """Capacity(front::FrontTracker, mesh) -- src/capacity.jl:472-598: the polygon of the markers is the body, its interior
        the fluid (complement=True: the exterior); cap.body is the front, callable as its signed distance"""
        check_front_body(front, mesh)
        L.init()
        self.mesh, self.body, self.compute_centroids = mesh, front, compute_centroids
        self.complement = bool(complement)
        xy = np.ascontiguousarray(front.polygon().reshape(-1), dtype=np.float64)
        self._h = C.c_void_p()
        L.check(L.lib().pg_capacity_create_polygon(mesh._h, L.dptr(xy), C.c_int64(len(xy) // 2),
                                                   C.c_int32((0 if compute_centroids else L.PG_FLAG_NO_CENTROIDS)
                                                             | (L.PG_FLAG_COMPLEMENT if complement else 0)),
                                                   C.byref(self._h)))
        self._cache = {}

    @classmethod
    def from_arrays(cls, mesh: Mesh, V, A, B, W, Gamma, C_omega, C_gamma, cell_types, body=None):
        L.init()
        self = cls.__new__(cls)
        self.mesh, self.body, self.compute_centroids = mesh, body, C_gamma is not None
        N = mesh.N
        keep = []

        def arr(a):
            a = np.ascontiguousarray(a, dtype=np.float64)
            keep.append(a)
            return a

        def ptrs(seq):
            p = (L.c_double_p * N)()
            for d in range(N):
                p[d] = L.dptr(arr(seq[d]))
            return p

        cw = [np.ascontiguousarray(np.asarray(C_omega)[:, d]) for d in range(N)]
        cg = [np.ascontiguousarray(np.asarray(C_gamma)[:, d]) for d in range(N)] if C_gamma is not None and len(C_gamma) else None
        self._h = C.c_void_p()
        L.check(L.lib().pg_capacity_create_from_arrays(
            mesh._h, L.dptr(arr(V)), ptrs(A), ptrs(B), ptrs(W), L.dptr(arr(Gamma)), ptrs(cw),
            ptrs(cg) if cg is not None else None, L.dptr(arr(cell_types)), C.byref(self._h)))
        self._cache = {}
        return self

    # ---- lazy field access -------------------------------------------------------------------
    def _get(self, field: int, d: int = 0) -> np.ndarray:
        key = (field, d)
        if key not in self._cache:
            M = int(np.prod(self.mesh.ext))
            out = np.zeros(M)
            L.check(L.lib().pg_capacity_get(self._h, C.c_int32(field), C.c_int32(d), L.dptr(out), C.c_int64(M)))
            self._cache[key] = out
        return self._cache[key]

    @property
    def N(self):
        return self.mesh.N

    @property
    def V(self):
        return self._get(L.PG_CAP_V)

    @property
    def Γ(self):
        return self._get(L.PG_CAP_GAMMA)

    Gamma = Γ

    @property
    def cell_types(self):
        return self._get(L.PG_CAP_CELL_TYPES)

    @property
    def A(self):
        return tuple(self._get(L.PG_CAP_A, d) for d in range(self.N))

    @property
    def B(self):
        return tuple(self._get(L.PG_CAP_B, d) for d in range(self.N))

    @property
    def W(self):
        return tuple(self._get(L.PG_CAP_W, d) for d in range(self.N))

    @property
    def C_ω(self):
        return np.stack([self._get(L.PG_CAP_C_OMEGA, d) for d in range(self.N)], axis=1)

    C_omega = C_ω

    @property
    def C_γ(self):
        if not self.compute_centroids:
            return np.zeros((0, self.N))  # capacity.jl:119
        return np.stack([self._get(L.PG_CAP_C_GAMMA, d) for d in range(self.N)], axis=1)

    C_gamma = C_γ

    # lazy coordinate getters: closures are only evaluated (and the M x N centroid arrays only fetched from the
    # GPU) when the user really passed a function -- constants never touch them
    def _cw(self):
        return self.C_ω

    def _cg(self):
        return self.C_γ

    @property
    def kernel_ms(self) -> float:
        ms = C.c_double()
        L.check(L.lib().pg_capacity_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    @property
    def kernel_ms_parts(self) -> Dict[str, float]:
        """device time of each capacity kernel between its own events (0.0: an empty work list launched nothing)"""
        ms = (C.c_double * 5)()
        L.check(L.lib().pg_capacity_kernel_ms_parts(self._h, ms))
        return dict(zip(("classify", "cut_cells", "sections", "stagger", "stagger_cut"), (float(v) for v in ms)))

    @property
    def polygon_ms_parts(self) -> Dict[str, float]:
        """a FrontTracker capacity: the five kernel times and the time of the edge lookup (`binning`), each between its own events"""
        ms = (C.c_double * 6)()
        L.check(L.lib().pg_capacity_polygon_ms_parts(self._h, ms))
        return dict(zip(("classify", "cut_cells", "sections", "stagger", "stagger_cut", "binning"), (float(v) for v in ms)))

    def __del__(self):
        try:
            if self._h:
                L.lib().pg_capacity_destroy(self._h)
        except Exception:
            pass


# =============================================================================== DiffusionOps


class DiffusionOps:
    """DiffusionOps(capacity) -- src/operators.jl:172-178.  G, H, Wꜝ are exported on demand as scipy CSC
    matrices (the time loop never forms them); V is the diagonal; size = (n_d+1,...)."""

    def __init__(self, capacity: Capacity):
        self.capacity = capacity
        self.size = capacity.mesh.ext
        self._h = C.c_void_p()
        L.check(L.lib().pg_diffops_create(capacity._h, C.byref(self._h)))
        self._mats: Dict[int, object] = {}

    def _export(self, which: int):
        if which not in self._mats:
            import scipy.sparse as sp

            N, M = self.capacity.N, int(np.prod(self.size))
            nnz = C.c_int64()
            L.check(L.lib().pg_diffops_export_csc(self._h, C.c_int32(which), None, None, None, C.byref(nnz)))
            ncols = N * M if which == L.PG_OP_WINV else M
            nrows = M if which >= L.PG_OP_C0 else N * M
            colptr = np.empty(ncols + 1, dtype=np.int64)
            rowval = np.empty(nnz.value, dtype=np.int64)
            nzval = np.empty(nnz.value)
            L.check(L.lib().pg_diffops_export_csc(self._h, C.c_int32(which), L.iptr(colptr), L.iptr(rowval), L.dptr(nzval),
                                                  C.byref(nnz)))
            self._mats[which] = sp.csc_matrix((nzval, rowval, colptr), shape=(nrows, ncols))
        return self._mats[which]

    @property
    def G(self):
        return self._export(L.PG_OP_G)

    @property
    def H(self):
        return self._export(L.PG_OP_H)

    @property
    def Winv(self):
        return self._export(L.PG_OP_WINV)

    @property
    def V(self):
        return self.capacity.V

    def __getattr__(self, name):
        if name == "Wꜝ":
            return self.Winv
        raise AttributeError(name)

    def __del__(self):
        try:
            if self._h:
                L.lib().pg_diffops_destroy(self._h)
        except Exception:
            pass


class ConvectionOps(DiffusionOps):
    """ConvectionOps(capacity, uₒ, uᵧ) -- src/operators.jl:194-210: C_d = δ_p[d]·diag(Σ_m[d] A_d uₒ_d)·Σ_m[d],
    K_d = diag(Σ_p[d] Hᵀuᵧ), plus G, H, Wꜝ, V, size as DiffusionOps.  uₒ: N arrays of length M, uᵧ: length N·M.

    On a space-time capacity (Capacity(body, SpaceTimeMesh(mesh, [t, t+Δt])), 2-D+t): uₒ = (uₒx, uₒy, uₒt), each of length
    2M, uᵧ of length 3·2M, as the reference's moving advection-diffusion solvers take them; `C` / `K` are then the three
    blocks those solvers slice (prescribedmotionsolver/advectiondiffusion.jl:94-95): C[1][L1,L1] = C_x of the first time
    layer, C[2][L2,L2] = C_y on the time padding (zero: A_y = 0 there), C[3][L1,L2] (zero: uₒt = 0 is required), and the same
    of K, where only K[1][L1,L1] = diag(Σ_p[x] Hᵀuᵧ) is used.  A non-zero uₒt or time block of uᵧ is refused."""

    def __init__(self, capacity: Capacity, uₒ, uᵧ):
        super().__init__(capacity)
        N, M = capacity.N, int(np.prod(capacity.mesh.ext))
        us = [np.ascontiguousarray(u, dtype=np.float64) for u in uₒ]
        ug = np.ascontiguousarray(uᵧ, dtype=np.float64)
        self._st = getattr(capacity, "stmesh", None) is not None          # a SpaceTimeCapacity (moving.py)
        if self._st:
            n1, M2 = N + 1, 2 * M
            if len(us) != n1 or any(u.shape != (M2,) for u in us) or ug.shape != (n1 * M2,):
                raise ValueError(f"ConvectionOps(space-time capacity): uₒ must be {n1} vectors of length {M2} (space "
                                 f"components, then time), uᵧ a vector of length {n1 * M2}")
            ptrs = (C.POINTER(C.c_double) * n1)(*[L.dptr(u) for u in us])
            L.check(L.lib().pg_diffops_set_velocity_spacetime(self._h, ptrs, L.dptr(ug)))
            return
        if len(us) != N or any(u.shape != (M,) for u in us) or ug.shape != (N * M,):
            raise ValueError(f"ConvectionOps: uₒ must be {N} vectors of length {M}, uᵧ a vector of length {N * M}")
        ptrs = (C.POINTER(C.c_double) * N)(*[L.dptr(u) for u in us])
        L.check(L.lib().pg_diffops_set_velocity(self._h, ptrs, L.dptr(ug)))

    def _st_blocks(self, first):
        import scipy.sparse as sp

        M = int(np.prod(self.capacity.mesh.ext))
        return (self._export(first),) + tuple(sp.csc_matrix((M, M)) for _ in range(2))

    @property
    def C(self):
        if self._st:
            return self._st_blocks(L.PG_OP_C0)
        return tuple(self._export(L.PG_OP_C0 + d) for d in range(self.capacity.N))

    @property
    def K(self):
        if self._st:
            return self._st_blocks(L.PG_OP_K0)
        return tuple(self._export(L.PG_OP_K0 + d) for d in range(self.capacity.N))


def grad(operator: DiffusionOps, p: np.ndarray) -> np.ndarray:
    """∇(operator, p) -- src/operators.jl:20-23."""
    M = int(np.prod(operator.size))
    p = np.ascontiguousarray(p, dtype=np.float64)
    out = np.empty(operator.capacity.N * M)
    L.check(L.lib().pg_diffops_grad(operator._h, L.dptr(p), L.dptr(out)))
    return out


def div(operator: DiffusionOps, qω: np.ndarray, qγ: np.ndarray) -> np.ndarray:
    """∇₋(operator, qω, qγ) -- src/operators.jl:30-34."""
    M = int(np.prod(operator.size))
    qω = np.ascontiguousarray(qω, dtype=np.float64)
    qγ = np.ascontiguousarray(qγ, dtype=np.float64)
    out = np.empty(M)
    L.check(L.lib().pg_diffops_div(operator._h, L.dptr(qω), L.dptr(qγ), L.dptr(out)))
    return out


# =============================================================================== boundary / phase


@dataclass
class Dirichlet:
    """src/boundary.jl:12-14."""
    value: Union[float, Callable]


@dataclass
class Neumann:
    """src/boundary.jl:25-27."""
    value: Union[float, Callable]


@dataclass
class Robin:
    """src/boundary.jl:38-42."""
    α: float
    β: float
    value: Union[float, Callable]


@dataclass
class Periodic:
    """src/boundary.jl:49-50."""


@dataclass
class ScalarJump:
    """src/boundary.jl:96-100."""
    α1: float
    α2: float
    value: Union[float, Callable]


@dataclass
class FluxJump:
    """src/boundary.jl:111-115."""
    β1: float
    β2: float
    value: Union[float, Callable]


class BorderConditions:
    """BorderConditions(Dict(:left => bc, ...)) -- src/boundary.jl:123-125.  Keys may be written
    "left" or ":left"; unknown keys (e.g. :front) are kept and silently ignored, as in the reference."""

    def __init__(self, borders: Dict[str, object]):
        self.borders = {str(k).lstrip(":"): v for k, v in borders.items()}


@dataclass
class InterfaceConditions:
    """src/boundary.jl:133-136."""
    scalar: Optional[ScalarJump]
    flux: Optional[FluxJump]


@dataclass
class Phase:
    """Phase(capacity, operator, source, Diffusion_coeff) -- src/phase.jl:12-17."""
    capacity: Capacity
    operator: DiffusionOps
    source: Callable
    Diffusion_coeff: Callable


# =============================================================================== closure evaluation


def _accepts(fn, nargs: int) -> bool:
    """Does fn have a method with `nargs` positional arguments?  (Julia: MethodError otherwise.)"""
    try:
        inspect.signature(fn).bind(*([0.0] * nargs))
        return True
    except TypeError:
        return False
    except ValueError:   # builtins without a signature
        return True


def _eval(fn, coords: np.ndarray, t: Optional[float], nargs_space: int):
    """Evaluate fn at the rows of coords (padded with zero columns up to nargs_space), vectorised when the
    callable accepts arrays.  Mirrors `try value(x..., t) catch value(x...)` (src/solver.jl:315-319,441-448).
    Returns a float when the callable returned a scalar for array input (constant data)."""
    if not callable(fn):
        return float(fn)
    if callable(coords):
        coords = coords()          # lazy: Capacity._cw / _cg
    cols = [coords[:, d] if d < coords.shape[1] else np.zeros(coords.shape[0]) for d in range(nargs_space)]
    if t is not None and _accepts(fn, nargs_space + 1):
        call = lambda c: fn(*c, t)
    elif _accepts(fn, nargs_space):
        call = lambda c: fn(*c)
    else:
        raise TypeError(f"{fn!r} accepts neither {nargs_space + 1} nor {nargs_space} positional arguments")
    try:
        out = call(cols)
    except Exception:
        # not vectorisable (branches, math.* calls): per-point loop with the same signature
        return np.array([call([c[i] for c in cols]) for i in range(coords.shape[0])], dtype=np.float64)
    if np.isscalar(out) or (isinstance(out, np.ndarray) and out.ndim == 0):
        return float(out)
    out = np.asarray(out, dtype=np.float64)
    if out.shape != (coords.shape[0],):
        out = np.broadcast_to(out, (coords.shape[0],)).copy()
    return np.ascontiguousarray(out)


def _padded_field(val, M: int) -> Optional[np.ndarray]:
    """scalar/array -> M array (None for an exact zero scalar)."""
    if isinstance(val, float):
        return None if val == 0.0 else np.full(M, val)
    return np.ascontiguousarray(val, dtype=np.float64)


# =============================================================================== time-separable data


def _space_value(φ, coords):
    """φ at the space coordinates `coords` (a sequence of scalars or arrays): a scalar φ as it is; a callable φ with all of
    them, or -- when it takes fewer, as a φ(x, y) handed the zero-padded z of a 2-D problem -- with the leading ones."""
    if not callable(φ):
        return float(φ)
    for n in range(len(coords), -1, -1):
        if _accepts(φ, n):
            return φ(*coords[:n])
    raise TypeError(f"{φ!r} accepts none of 0 .. {len(coords)} space coordinates")


class TimeSeparable:
    """Data of the form  Σ_k φ_k(x) · a_k(t),  k = 1 .. K <= 8:  TimeSeparable([(φ_1, a_1), (φ_2, a_2), ...]).

    φ_k is a scalar or a callable of the space coordinates only, a_k a callable t -> float.  The object is itself callable as
    ts(*coords, t) -- any number of coordinates followed by t -- and broadcasts over arrays, so it can be handed to anything
    that takes a closure (the constructors, which evaluate data at t = 0 on the host; the host-driven loop; a CPU reference).
    As Phase.source, as the value of the monophasic interface condition or of a Dirichlet border condition it lets the unsteady
    drivers keep the time loop on the device: the spatial parts are sent once, every step then costs K scalars (DESIGN.md
    "Time-separable data").  A pulse, a ramp, sinusoidal forcing, a uniform wall value g(t) are all of this form."""

    MAX_TERMS = 8     # PG_TD_MAX_TERMS

    def __init__(self, terms):
        terms = list(terms)
        if not 1 <= len(terms) <= self.MAX_TERMS:
            raise ValueError(f"TimeSeparable takes 1 .. {self.MAX_TERMS} terms (φ, a), not {len(terms)}")
        self.terms = []
        for term in terms:
            φ, a = term
            if not callable(a):
                raise TypeError(f"the time part of a term must be a callable t -> float, not {a!r}")
            self.terms.append((φ if callable(φ) else float(φ), a))

    def __call__(self, *args):
        if not args:
            raise TypeError("TimeSeparable is called as ts(*coords, t)")
        *coords, t = args
        out = 0.0
        for φ, a in self.terms:
            out = out + _space_value(φ, coords) * float(a(t))
        return out

    def __repr__(self):
        return f"TimeSeparable({len(self.terms)} terms)"


def _separable_table(coefs, Δt: float, Tₑ: float, max_steps: Optional[int] = None) -> np.ndarray:
    """The coefficient table of pg_solver_set_separable for the time parts `coefs` (callables t -> float, or a
    TimeSeparable): rows x 2 x K.  It walks the clock of the host-driven loop literally -- t = 0.0; while t < Tₑ: t += Δt,
    at most max_steps times -- and stores for each step the coefficients at the two times that loop evaluates its closures
    at: a_k(t) and a_k(t + Δt) with t ALREADY advanced (diffusion.jl:248-249, 287-290).  The library attaches no clock to the
    rows, so the quirk lives here alone."""
    if isinstance(coefs, TimeSeparable):
        coefs = [a for _, a in coefs.terms]
    coefs = list(coefs)
    rows = []
    t, steps = 0.0, 0
    while t < Tₑ:
        if max_steps is not None and steps >= max_steps:
            break
        t += Δt
        rows.append([[float(a(t)) for a in coefs], [float(a(t + Δt)) for a in coefs]])
        steps += 1
    return np.array(rows, dtype=np.float64).reshape(len(rows), 2, len(coefs))


_TD_SOURCE, _TD_INTERFACE, _TD_BORDER = 0, 1, 2      # PG_TD_*


def _separable_fields(ts: TimeSeparable, coords, nspace: int, M: int) -> np.ndarray:
    """K x M: the spatial parts of ts at the rows of coords (C_ω or C_γ, zero-padded to nspace columns)."""
    out = np.empty((len(ts.terms), M))
    for k, (φ, _) in enumerate(ts.terms):
        out[k] = _eval(lambda *c, φ=φ: _space_value(φ, c), coords, None, nspace)
    return out


def _separable_border(bc_b: "BorderConditions", mesh: "Mesh"):
    """Border values with TimeSeparable conditions as (modes K x nb in the mesh's border order, time parts): the terms of every
    distinct TimeSeparable on the cells of its borders, and -- the library takes EVERY border value from the modes -- one term
    with the coefficient 1 for the values that do not depend on time.  None when that makes more than 8 terms."""
    idx, pos, key = mesh._border_arrays()
    inv = {v: k for k, v in L.PG_KEY.items()}
    modes, coefs, where = [], [], {}
    const = np.zeros(len(key))
    for kval in np.unique(key):
        cond = bc_b.borders.get(inv[int(kval)])
        if cond is None:
            continue
        sel = key == kval
        v = getattr(cond, "value", 0.0)
        if isinstance(v, TimeSeparable):
            if id(v) not in where:
                where[id(v)] = len(modes)
                modes.extend(np.zeros(len(key)) for _ in v.terms)
                coefs.extend(a for _, a in v.terms)
            for k, (φ, _) in enumerate(v.terms):
                modes[where[id(v)] + k][sel] = _eval(lambda *c, φ=φ: _space_value(φ, c), pos[sel], None, mesh.N)
        elif callable(v):
            const[sel] = _eval(v, pos[sel], 0.0, mesh.N)      # (no time in it, or the caller said time_independent)
        elif v is not None:
            const[sel] = float(v)
    if np.any(const != 0.0):
        modes.append(const)
        coefs.append(lambda t: 1.0)
    if len(modes) > TimeSeparable.MAX_TERMS:
        return None
    return np.ascontiguousarray(np.array(modes)), coefs


def _install_separable(s: "Solver", which: int, phase: int, modes: np.ndarray, table: np.ndarray) -> None:
    modes = np.ascontiguousarray(modes, dtype=np.float64)
    table = np.ascontiguousarray(table, dtype=np.float64)
    L.check(L.lib().pg_solver_set_separable(s._h, C.c_int32(which), C.c_int32(phase), C.c_int32(modes.shape[0]), L.dptr(modes),
                                            C.c_int64(table.shape[0]), L.dptr(table)))


def _clear_separable(s: "Solver", nphase: int) -> None:
    """What an earlier call installed goes: every call of a driver starts its own clock at t = 0."""
    for which, phase in [(_TD_SOURCE, q) for q in range(nphase)] + ([(_TD_INTERFACE, 0)] if nphase == 1 else []) + [(_TD_BORDER, 0)]:
        L.check(L.lib().pg_solver_clear_separable(s._h, C.c_int32(which), C.c_int32(phase)))


# =============================================================================== device functions


def _program_times(Δt: float, Tₑ: float, max_steps: Optional[int]) -> np.ndarray:
    """rows x 2: the two times of every step, from the one walk of the loop's clock (_separable_table with a(t) = t)."""
    tab = _separable_table([lambda t: t], Δt, Tₑ, max_steps)
    return np.ascontiguousarray(tab.reshape(tab.shape[0], 2))


def _install_program(s: "Solver", which: int, phase: int, df: DeviceFunction, nspace: int, times: np.ndarray,
                     key: Optional[int] = None) -> None:
    prog = df.program_for(nspace)
    times = np.ascontiguousarray(times, dtype=np.float64)
    if key is None:
        L.check(L.lib().pg_solver_set_program(s._h, C.c_int32(which), C.c_int32(phase), C.byref(prog), C.c_int64(times.shape[0]),
                                              L.dptr(times)))
    else:
        L.check(L.lib().pg_solver_set_border_program(s._h, C.c_int32(key), C.byref(prog), C.c_int64(times.shape[0]),
                                                     L.dptr(times)))


def _program_border(bc_b: "BorderConditions", mesh: "Mesh", time_independent: bool):
    """Border values with DeviceFunction conditions as (values of every border cell without them -- constants and closures
    without a time parameter, 0 on the cells of a DeviceFunction --, [(key, DeviceFunction), ...]): one program per border key,
    applied to that key's cells."""
    progs: list = []
    static = _border_values(bc_b, mesh, 0.0, programs=progs, time_independent=time_independent)
    return static, progs


def _device_data(values) -> bool:
    """Can these time-dependent data stay on the device?  Every one a TimeSeparable or a DeviceFunction."""
    return bool(values) and all(isinstance(v, (TimeSeparable, DeviceFunction)) for v in values)


# =============================================================================== monitors


_MON_KINDS = {"sum": 0, "sumsq": 1}      # PG_MON_SUM, PG_MON_SUMSQ
MON_MAX = 8                              # PG_MON_MAX


def _block_offset(M: int, nunk: int, phase: int, kind: str) -> int:
    """Where the block (phase, kind) starts in the full unknown vector: [Tω, Tγ] (2M, monophasic) or [T1ω, T1γ, T2ω, T2γ]
    (4M, diphasic) -- the layout of Solver.x."""
    if kind not in ("omega", "gamma", "ω", "γ"):
        raise ValueError(f"kind must be 'omega' or 'gamma', not {kind!r}")
    if nunk not in (2 * M, 4 * M):
        raise ValueError(f"a solver on this mesh has 2*{M} or 4*{M} unknowns, not {nunk}")
    if phase not in (0, 1) or (phase == 1 and nunk == 2 * M):
        raise ValueError(f"phase {phase}: a {'monophasic' if nunk == 2 * M else 'diphasic'} solver has phase 0"
                         + ("" if nunk == 2 * M else " and phase 1"))
    return (2 * phase + (1 if kind in ("gamma", "γ") else 0)) * M


class Monitor:
    """A per-step observable Σ_i w_i x_i (kind="sum") or Σ_i w_i x_i² (kind="sumsq") of the state, evaluated on the device
    after every solve of an unsteady driver called with monitors=[...] (DESIGN.md "Monitors").  `weights` has the layout of
    Solver.x: 2M (monophasic) or 4M (diphasic) entries.  The values come back as one column of Solver.monitor_series."""

    def __init__(self, weights, kind: str = "sum", name: Optional[str] = None):
        if kind not in _MON_KINDS:
            raise ValueError(f"unknown monitor kind {kind!r}: 'sum' or 'sumsq'")
        self.kind = kind
        self.name = name
        self._w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)

    def _weights(self, nunk: int) -> np.ndarray:
        return self._w

    def __repr__(self):
        return f"{type(self).__name__}({self.name or self.kind})"


class VolumeIntegral(Monitor):
    """Σ_i V_i T_i over the bulk (ω) unknowns of one phase -- divided by Σ V when `mean` (the volume-weighted phase mean c̄ of
    the reference's examples/2D/Diffusion/Heat_2ph.jl); `square`: of T_i² instead."""

    def __init__(self, capacity: "Capacity", phase: int = 0, mean: bool = True, square: bool = False, name: Optional[str] = None):
        super().__init__(None, "sumsq" if square else "sum", name or f"{'mean' if mean else 'integral'}{'_sq' if square else ''}_{phase}")
        self.capacity, self.phase, self.mean = capacity, phase, mean

    def _weights(self, nunk: int) -> np.ndarray:
        V = np.asarray(self.capacity.V, dtype=np.float64)
        M = V.shape[0]
        w = np.zeros(nunk)
        off = _block_offset(M, nunk, self.phase, "omega")
        w[off:off + M] = V / V.sum() if self.mean else V
        return w


class InterfaceFlux(Monitor):
    """Σ_i [Id (Hᵀ W! G Tω + Hᵀ W! H Tγ)]_i, Id = diag D(C_ω): the interface flux the reference's Stefan and species solvers sum
    per step.  With d = D(C_ω) and q = W! H d = ∇(op, (0, d)) the sum is (Gᵀq)·Tω + (Hᵀq)·Tγ; the weights come from the device's
    own ∇ / ∇₋ once:  w_γ = ∇₋(op, 0, q) = Hᵀq,  w_ω = −∇₋(op, q, 0) − w_γ = Gᵀq."""

    def __init__(self, phase_obj: "Phase", phase: int = 0, name: Optional[str] = None):
        super().__init__(None, "sum", name or f"interface_flux_{phase}")
        self.phase_obj, self.phase = phase_obj, phase

    def _weights(self, nunk: int) -> np.ndarray:
        op = self.phase_obj.operator
        M = int(np.prod(op.size))
        off_w, off_g = _block_offset(M, nunk, self.phase, "omega"), _block_offset(M, nunk, self.phase, "gamma")
        d = _dcoef(self.phase_obj, M)
        d = np.ones(M) if d is None else np.asarray(d, dtype=np.float64)
        q = grad(op, np.concatenate([np.zeros(M), d]))
        zero = np.zeros_like(q)
        wγ = div(op, zero, q)
        wω = -div(op, q, zero) - wγ
        w = np.zeros(nunk)
        w[off_w:off_w + M] = wω
        w[off_g:off_g + M] = wγ
        return w


class Probe(Monitor):
    """The value of one unknown: unit weight on the cell `point_or_index` of block (phase, kind).  An int is the linear
    index of the cell (0-based, first coordinate fastest, n+1 cells per direction as in Solver.x), a tuple of ints its
    0-based multi-index, a tuple of floats a point -- the cell whose node interval holds it."""

    def __init__(self, mesh: "Mesh", point_or_index, kind: str = "omega", phase: int = 0, name: Optional[str] = None):
        super().__init__(None, "sum", name)
        ext = tuple(int(e) for e in mesh.ext)
        M = int(np.prod(ext))
        if isinstance(point_or_index, (int, np.integer)):
            lin = int(point_or_index)
        else:
            p = tuple(point_or_index)
            if len(p) != len(ext):
                raise ValueError(f"a point or multi-index of this mesh has {len(ext)} components, not {len(p)}")
            if all(isinstance(v, (int, np.integer)) for v in p):
                idx = [int(v) for v in p]
            else:
                idx = [int(np.clip(np.searchsorted(mesh.nodes[d], float(p[d]), side="right") - 1, 0, mesh.dims[d] - 1))
                       for d in range(len(ext))]
            if any(not 0 <= i < e for i, e in zip(idx, ext)):
                raise ValueError(f"multi-index {tuple(idx)} is outside the {ext} cells of the mesh")
            lin, stride = 0, 1
            for i, e in zip(idx, ext):
                lin += i * stride
                stride *= e
        if not 0 <= lin < M:
            raise ValueError(f"cell index {lin} is outside 0 .. {M - 1}")
        _block_offset(M, 4 * M, phase, kind)          # (kind and phase checked here; the solver's phase count later)
        self.M, self.cell, self.block_kind, self.phase = M, lin, kind, phase
        if self.name is None:
            self.name = f"probe_{kind}_{phase}_{lin}"

    def _weights(self, nunk: int) -> np.ndarray:
        w = np.zeros(nunk)
        w[_block_offset(self.M, nunk, self.phase, self.block_kind) + self.cell] = 1.0
        return w


def _check_monitor_args(monitors, save_every, verbose: bool, log: bool, nunk: Optional[int] = None):
    """The argument errors of monitors= / save_every=, raised before any call into the library.  Returns (list of
    monitors, save_every as an int or None)."""
    mons = [] if monitors is None else list(monitors)
    if len(mons) > MON_MAX:
        raise ValueError(f"at most {MON_MAX} monitors per solver (PG_MON_MAX), not {len(mons)}")
    for m in mons:
        if not isinstance(m, Monitor):
            raise TypeError(f"monitors must be Monitor objects (Monitor, VolumeIntegral, InterfaceFlux, Probe), not {m!r}")
        if m.kind not in _MON_KINDS:
            raise ValueError(f"unknown monitor kind {m.kind!r}: 'sum' or 'sumsq'")
        if nunk is not None and m._w is not None and m._w.shape[0] != nunk:
            raise ValueError(f"monitor weights must have the length of Solver.x, {nunk}, not {m._w.shape[0]}")
    if save_every is not None:
        if isinstance(save_every, bool) or not isinstance(save_every, (int, np.integer)) or save_every < 1:
            raise ValueError(f"save_every must be an integer >= 1, not {save_every!r}")
        if verbose or log:
            raise ValueError("save_every keeps the time loop on the device; verbose / log need the per-step branch: use one or the other")
        save_every = int(save_every)
    return mons, save_every


def _monitor_weights(mons, nunk: int) -> np.ndarray:
    """K x nunk, one row per monitor, lengths checked."""
    W = np.zeros((len(mons), nunk))
    for k, m in enumerate(mons):
        w = np.ascontiguousarray(m._weights(nunk), dtype=np.float64).reshape(-1)
        if w.shape[0] != nunk:
            raise ValueError(f"monitor weights must have the length of Solver.x, {nunk}, not {w.shape[0]}")
        W[k] = w
    return W


def _install_monitors(s: "Solver", mons) -> None:
    """Before the first solve of a driver: this call's monitors (row 0 of the series is then states[1] of the reference), or
    none -- what an earlier call on the same solver installed goes.  A solver that never had monitors is not touched."""
    if mons:
        W = _monitor_weights(mons, s._nunk)
        kinds = (C.c_int32 * len(mons))(*[_MON_KINDS[m.kind] for m in mons])
        L.check(L.lib().pg_solver_set_monitors(s._h, C.c_int32(len(mons)), kinds, L.dptr(W), C.c_int64(s._nunk)))
        s._monitors_installed = True
    elif s._monitors_installed:
        L.check(L.lib().pg_solver_clear_monitors(s._h))
        s._monitors_installed = False
    s.monitor_names = [m.name or f"monitor_{k}" for k, m in enumerate(mons)]
    s.monitor_series = np.zeros((0, len(mons)))
    s.monitor_times = np.zeros(0)


def _fetch_monitors(s: "Solver") -> None:
    if not s._monitors_installed:
        return
    K, rows = C.c_int32(0), C.c_int64(0)
    L.check(L.lib().pg_solver_monitor_info(s._h, C.byref(K), C.byref(rows), None, None))
    vals, times = np.zeros((rows.value, K.value)), np.zeros(rows.value)
    if rows.value > 0:
        L.check(L.lib().pg_solver_get_monitor_series(s._h, C.c_int64(0), rows, L.dptr(vals), L.dptr(times)))
    s.monitor_series, s.monitor_times = vals, times


def _fetch_kept_states(s: "Solver", save_every: int) -> None:
    """After pg_solver_run with save_every = k: the states it kept on the device (steps k, 2k, ...) follow the first solve's in
    s.states, s.state_steps says which step each belongs to, and the device copies are released."""
    n = C.c_int64(0)
    L.check(L.lib().pg_solver_num_states(s._h, C.byref(n)))
    for q in range(n.value):
        s.states.append(s._fetch_state(q))
        s.state_steps.append((q + 1) * save_every)
    L.check(L.lib().pg_solver_drop_states(s._h))


# =============================================================================== Solver


class Solver:
    """Penguin.Solver -- src/solver.jl:33-42.  `x` is the full 2M (mono) / 4M (diph) vector with zeros at
    eliminated unknowns (:186-187); `states` holds one such vector per solve when save_states is on."""

    def __init__(self, time_type: str, phase_type: str, equation_type: str):
        self.time_type, self.phase_type, self.equation_type = time_type, phase_type, equation_type
        self.x: Optional[np.ndarray] = None
        self.ch: list = []
        self.states: list = []
        self._h = C.c_void_p()
        self._nunk = 0
        self._initial_done = False
        self.last_run: Optional[L.pg_run_info] = None
        self.unconverged = 0          # solves that ended without meeting the tolerance (see _check_converged)
        # where the last unsteady solve took its time-dependent data from: "device" (every one a TimeSeparable or a
        # DeviceFunction: spatial parts and a coefficient table, or a program and a table of times, installed once, the loop
        # stays on the device), "host" (closures re-evaluated and uploaded every step), None (no time-dependent data, or no
        # unsteady solve yet)
        self.time_data: Optional[str] = None
        # monitors=[...] of the last unsteady solve: one row per completed solve (row 0: the first solve), one column per
        # monitor; the solver's time of each row; the monitors' names.  state_steps: with save_every=k, the step each entry of
        # `states` belongs to ([0, k, 2k, ...]); None otherwise.
        self.monitor_series: np.ndarray = np.zeros((0, 0))
        self.monitor_times: np.ndarray = np.zeros(0)
        self.monitor_names: list = []
        self.state_steps: Optional[list] = None
        self._monitors_installed = False

    # reduced system of the constructor (which=0) or of the loop (which=1): (A_csr, b, idx)
    def system(self, which: int = 0):
        import scipy.sparse as sp

        info = self.system_info(which)
        n, nnz = info.n_own, info.nnz
        rowptr = np.empty(n + 1, dtype=np.int64)
        col = np.empty(max(nnz, 1), dtype=np.int64)
        val = np.empty(max(nnz, 1))
        b = np.empty(max(n, 1))
        idx = np.empty(max(n, 1), dtype=np.int64)
        L.check(L.lib().pg_solver_get_system_csr(self._h, C.c_int32(which), L.iptr(rowptr), L.iptr(col), L.dptr(val),
                                                 L.dptr(b), L.iptr(idx)))
        A = sp.csr_matrix((val[:nnz], col[:nnz], rowptr), shape=(n, n + info.n_ghost))
        return A, b[:n], idx[:n]

    def row_scaling(self, which: int = 0) -> np.ndarray:
        """S = diag(|a_ii|^-1/2) of system `which` (0 constructor, 1 run): the weights of the convergence test
        ||S r|| <= reltol ||S b|| every Krylov method of the library is accepted on."""
        ds = np.empty(max(self.system_info(which).n_own, 1))
        L.check(L.lib().pg_solver_get_row_scaling(self._h, C.c_int32(which), L.dptr(ds)))
        return ds[: self.system_info(which).n_own]

    def guess_info(self) -> dict:
        """The extrapolated start of the loop's quiet steps (pg_solver_guess_info): older states kept, the ones the next
        step reads with their coefficients, and the sampled start residual without / with this step's extrapolation."""
        kept, ns = C.c_int32(0), C.c_int32(0)
        off = (C.c_int32 * 4)()
        cf = (C.c_double * 4)()
        ru, rw = C.c_double(0.0), C.c_double(0.0)
        L.check(L.lib().pg_solver_guess_info(self._h, C.byref(kept), C.byref(ns), off, cf, C.byref(ru), C.byref(rw)))
        return {"kept": kept.value, "offsets": list(off[: ns.value]), "coef": list(cf[: ns.value]), "rr_plain": ru.value,
                "rr_taken": rw.value}

    def row_const_info(self) -> dict:
        """Groups of 16 rows whose per-row constants are one value (pg_solver_row_const_info, PG_ROW_CONST): groups and
        qualifying groups of the full system's and of the loop system's table, for the compact loop the last step took."""
        out = (C.c_int64 * 4)()
        L.check(L.lib().pg_solver_row_const_info(self._h, out))
        return {"full_groups": int(out[0]), "full_const": int(out[1]), "loop_groups": int(out[2]), "loop_const": int(out[3])}

    def row_const_bconst_info(self) -> dict:
        """(tests) The bconst mark of row_const_info's full table (pg_debug_row_const_bconst): whether the last step's launch took
        one, the groups it marks, marks built so far and launches that took the standing one."""
        out = (C.c_int64 * 4)()
        L.check(L.lib().pg_debug_row_const_bconst(self._h, out))
        return {"valid": int(out[0]), "const": int(out[1]), "builds": int(out[2]), "uses": int(out[3])}

    def mg_info(self, precond="mg") -> dict:
        """The multigrid hierarchy of the constructor system (pg_solver_mg_info): levels (0 before the first solve with
        that `precond`), tail_level, rows and nnz per level, setup_ms, bytes.  precond: "mg" or "mg-cell" -- a solver holds
        one hierarchy per value."""
        return L.solver_mg_info(self._h, _precond_value(precond))

    def mg_step_info(self) -> list:
        """The two hierarchies of precond="mg-step" (pg_solver_mg_step_info): [constructor system, run system], each as mg_info
        reports (levels = 0 while no solve with the option has run on that matrix)."""
        return [L.solver_mg_step_info(self._h, which) for which in (0, 1)]

    def spectral_estimate(self, which: int = 0, run: bool = True) -> dict:
        """The spectral estimate behind precond="poly-est" of system `which` (0 constructor, 1 run system;
        pg_solver_spectral_estimate): steps, g_ritz, g_used, margin, admitted, gershgorin, gershgorin_admits, the smallest /
        largest real part and the largest |imaginary part| of the Ritz values, estimate_ms.  Runs the estimate if it has not
        run on that matrix; run=False only reports (steps = 0: none has run)."""
        return L.solver_spectral_estimate(self._h, which, run)

    def system_info(self, which: int = 0) -> L.pg_system_info:
        info = L.pg_system_info()
        L.check(L.lib().pg_solver_system_info(self._h, C.c_int32(which), C.byref(info)))
        return info

    @property
    def A(self):
        """The reference's s.A restricted to its active rows/cols, embedded in the full (2M x 2M) shape."""
        import scipy.sparse as sp

        Ar, _, idx = self.system(1 if self._initial_done and self._have_run else 0)
        n = self._nunk
        P = sp.csr_matrix((np.ones(len(idx)), (idx, np.arange(len(idx)))), shape=(n, len(idx)))
        return (P @ Ar[:, : len(idx)] @ P.T).tocsc()

    @property
    def b(self):
        _, b, idx = self.system(0)
        out = np.zeros(self._nunk)
        out[idx] = b
        return out

    _have_run = False

    def _fetch_state(self, index: int = -1) -> np.ndarray:
        out = np.zeros(self._nunk)
        L.check(L.lib().pg_solver_get_state(self._h, C.c_int64(index), L.dptr(out), C.c_int64(self._nunk)))
        return out

    def __del__(self):
        try:
            if self._h:
                L.lib().pg_solver_destroy(self._h)
        except Exception:
            pass


def _border_descs(bc_b: BorderConditions, mesh: Mesh, t: Optional[float]):
    """-> (ctypes array of pg_border_desc, per-border-cell values or None)."""
    descs = []
    need_values = False
    for name, cond in bc_b.borders.items():
        if name not in L.PG_KEY:
            continue  # unknown keys are silently ignored (examples/3D/Diffusion/Heat.jl:26 uses :front/:back)
        if isinstance(cond, Dirichlet):
            kind = L.PG_BC_DIRICHLET
        elif isinstance(cond, Periodic):
            kind = L.PG_BC_PERIODIC
        elif isinstance(cond, Neumann):
            kind = L.PG_BC_NEUMANN
        elif isinstance(cond, Robin):
            kind = L.PG_BC_ROBIN
        else:
            raise TypeError(f"unsupported border condition {cond!r}")
        value = 0.0
        v = getattr(cond, "value", 0.0)
        if callable(v):
            need_values = True
        elif v is not None:
            value = float(v)
        descs.append(L.pg_border_desc(L.PG_KEY[name], kind, value))
    arr = (L.pg_border_desc * max(len(descs), 1))(*descs)
    values = _border_values(bc_b, mesh, t) if need_values else None
    return arr, len(descs), values


def _border_values(bc_b: BorderConditions, mesh: Mesh, t: Optional[float], programs: Optional[list] = None,
                   time_independent: bool = False) -> np.ndarray:
    """eval_bc_value at every border cell (src/solver.jl:441-448): value(pos..., t) with the N unpadded
    coordinates of mesh.centers.  With a list `programs`, a key whose value is a time-dependent DeviceFunction is not
    evaluated: its cells stay 0 and (key, DeviceFunction) is appended to the list."""
    idx, pos, key = mesh._border_arrays()
    out = np.zeros(len(key))
    inv = {v: k for k, v in L.PG_KEY.items()}
    for kval in np.unique(key):
        cond = bc_b.borders.get(inv[int(kval)])
        if cond is None:
            continue
        sel = key == kval
        v = getattr(cond, "value", 0.0)
        if programs is not None and isinstance(v, DeviceFunction) and _time_dependent(v, mesh.N, time_independent):
            programs.append((int(kval), v))
        elif callable(v):
            out[sel] = _eval(v, pos[sel], t, mesh.N)
        elif v is not None:
            out[sel] = float(v)
    return out


class _UploadCache:
    """Data handed to the library at every step of a host-driven loop: a closure with a time parameter is re-evaluated every
    step, as the reference does, but what it returned is only sent when it differs from what the library already holds
    (`f = (x, y, z, t) -> 0.0`, the reference's own benchmark source, is time-dependent by its signature and constant by its
    values).  A step whose data did not change is a quiet step of the device loop (folded start, extrapolated start)."""

    def __init__(self):
        self._last = {}

    def changed(self, key, *arrays) -> bool:
        new = tuple(None if a is None else np.array(a, dtype=np.float64, copy=True) for a in arrays)
        old = self._last.get(key)
        same = old is not None and len(old) == len(new) and all(
            (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and np.array_equal(a, b))
            for a, b in zip(old, new))
        self._last[key] = new
        return not same


def _check_converged(s: "Solver", converged: bool, what: str, relres: float) -> None:
    """The device Krylov solve stands in for the reference's direct `\\` as well: a solve that stopped at maxiter or
    broke down must not pass silently (IterativeSolvers would hand back `ch.isconverged == false`)."""
    s.unconverged += 0 if converged else 1
    if not converged:
        warnings.warn(f"penguin.jl_amd: {what} did not converge (||r||/||b|| = {relres:.3e}); the state is not a "
                      "solution to the requested tolerance", RuntimeWarning, stacklevel=3)


def _step_info_check(s: "Solver", info: L.pg_step_info, what: str) -> None:
    _check_converged(s, bool(info.converged), what, info.resnorm / info.bnorm if info.bnorm > 0 else info.resnorm)


_PRECOND_NAMES = {"mg": L.PG_PRECOND_MG, "mg-cell": L.PG_PRECOND_MG_CELL, "poly-est": L.PG_PRECOND_POLY_EST,
                  "mg-step": L.PG_PRECOND_MG_STEP}


def _precond_value(precond) -> int:
    """pg_krylov_opts.precond of a `precond` keyword: an integer as it is, "mg" -> PG_PRECOND_MG, "mg-cell" -> PG_PRECOND_MG_CELL,
    "poly-est" -> PG_PRECOND_POLY_EST, "mg-step" -> PG_PRECOND_MG_STEP (names in any case)."""
    if isinstance(precond, str):
        if precond.lower() not in _PRECOND_NAMES:
            raise ValueError(f'precond must be an integer, "mg", "mg-cell", "poly-est" or "mg-step", not {precond!r}')
        return _PRECOND_NAMES[precond.lower()]
    return int(precond)


def _krylov_opts(method, kwargs) -> L.pg_krylov_opts:
    """method may be "bicgstab" / "cg" / "gmres" or a callable named like IterativeSolvers' (bicgstabl, cg, gmres...).
    gmres -> restarted GMRES on the device (restart kwarg, default 20; its iterations are Arnoldi steps, one product each, and that
    is the unit maxiter caps: a cycle that ends early is charged the steps it ran, the solve ends at iters >= maxiter); cg -> CG;
    bicgstabl WITH the keyword l (l=2, l=4, .., at most 8) -> BiCGStab(l) on the device (DESIGN.md "BiCGStab(l)": one rank, zero initial guess, plain -- the library refuses
    it together with precond = m >= 1, "mg", "mg-cell", "mg-step" or "poly-est"); `\\`, bicgstabl WITHOUT l and anything else -> BiCGStab.
    BiCGStab(l) counts BiCG sub-steps as its iterations, two products each -- the unit of BiCGStab's iterations, and the unit
    maxiter caps (no outer iteration starts at iters >= maxiter); products = 2 iters + the products that confirm the true residual.
    max_mv_products (IterativeSolvers' spelling of the cap) is accepted when maxiter is not given: maxiter = max_mv_products // 2.
    idrs WITH the keyword nshadow (nshadow=4, nshadow=8, .., at most 8; 0 means 8) -> IDR(s) on the device with s = nshadow shadow
    vectors (DESIGN.md "IDR(s)": one rank, plain -- refused with the same preconditioners as BiCGStab(l); with warm_start a steady
    re-solve and a time step start from the previous state); idrs WITHOUT nshadow -> BiCGStab.  IterativeSolvers spells the keyword
    `s`; it cannot be spelled that way here because the drivers' first positional parameter is `s` (the solver).  IDR(s) counts
    updates of x as its iterations, one product each; maxiter is passed unchanged and caps exactly that unit;
    products = iters + restarts + confirmations of the true residual (+ 1 for the product of a start from a previous state).
    reltol defaults to 1e-12: the parity target is the direct-solve path.
    precond: an integer as pg_krylov_opts.precond takes it (0 automatic, -1 off, m >= 1 the polynomial's degree), or "mg":
    the aggregation multigrid V-cycle (steady monophasic diffusion with a Dirichlet interface and the ψ solve of a
    StreamVorticity; the library refuses it anywhere else), or "mg-cell": the same V-cycle on the cell-aggregated hierarchy
    (steady monophasic diffusion, DarcyFlow included, with a Dirichlet, Robin or Neumann interface), or "poly-est": the
    polynomial preconditioner of precond = 0, admitted on an estimated spectral disc where Gershgorin refuses it (diphasic
    systems, Robin / Neumann interfaces of the unsteady diffusion solvers; one rank, BiCGStab, DiffusionOps, no moving body --
    refused anywhere else; Solver.spectral_estimate tells what the estimate found), or "mg-step": the cell-aggregated V-cycle
    inside the time loop of DiffusionUnsteadyMono / DarcyFlowUnsteady (Dirichlet, Robin or Neumann interface) and
    DiffusionUnsteadyDiph (BE and CN; DiffusionOps, one rank, BiCGStab) for steps far above h² -- one hierarchy per assembled matrix (Solver.mg_step_info), the
    iteration on the full system, warm-started from the previous state.  The library refuses it on steady and moving
    solvers, a ConvectionOps, a StreamVorticity, cg / gmres / bicgstabl with l, and where a coarse diagonal entry is not
    positive (DESIGN.md section 20 has the measured crossover)."""
    name = method if isinstance(method, str) else getattr(method, "__name__", "bicgstab")
    name = name.lower()
    restart = int(kwargs.get("restart", 0))
    if name == "bicgstabl":
        # the bare name keeps meaning BiCGStab (every existing call takes the path it took); the keyword l opts in
        if kwargs.get("l") is not None:
            m, restart = L.PG_METHOD["bicgstabl"], int(kwargs["l"])
        else:
            m = L.PG_METHOD["bicgstab"]
    elif name == "idrs" and kwargs.get("nshadow") is not None:
        # likewise: the bare name keeps meaning BiCGStab; the keyword nshadow opts in and travels in `restart`
        m, restart = L.PG_METHOD_IDRS, int(kwargs["nshadow"])
    else:
        m = L.PG_METHOD.get(name, L.PG_METHOD["bicgstab"])
    precond = _precond_value(kwargs.get("precond", 0))
    maxiter = int(kwargs.get("maxiter", 0))
    if m != L.PG_METHOD_IDRS and "maxiter" not in kwargs and kwargs.get("max_mv_products") is not None:
        maxiter = max(1, int(kwargs["max_mv_products"]) // 2)
    return L.pg_krylov_opts(m, float(kwargs.get("reltol", 1e-12)), float(kwargs.get("abstol", 0.0)),
                            maxiter, int(kwargs.get("check_every", 4)),
                            int(bool(kwargs.get("warm_start", True))), restart,
                            int(precond))


def DiffusionUnsteadyMono(phase: Phase, bc_b: BorderConditions, bc_i, Δt: float, Tᵢ: np.ndarray, scheme: str,
                          verbose: bool = False, _ops_kind=None) -> Solver:
    """DiffusionUnsteadyMono(phase, bc_b, bc_i, Δt, Tᵢ, scheme) -- src/solver/diffusion.jl:192-210."""
    _require_ops(phase, _ops_kind or DiffusionOps)
    if verbose:
        print("Solver creation:\n- Monophasic problem\n- Unsteady problem\n- Diffusion problem")
    s = Solver("Unsteady", "Monophasic", "Diffusion")
    cap, mesh = phase.capacity, phase.capacity.mesh
    Tᵢ = _unsteady_prelude(s, 2, mesh, Tᵢ, phase=phase, bc_i=bc_i, dt=float(Δt))
    M = s._ctx["M"]
    sch = "CN" if scheme == "CN" else "BE"   # diffusion.jl:200-206: anything but "CN" is BE
    desc, g_keep = _interface_desc(bc_i, cap._cg, float(Δt))      # b(t=0) uses g(0+Δt)  diffusion.jl:249
    D_arr = _dcoef(phase, M)
    f1 = _eval(phase.source, cap._cw, float(Δt), 3)        # f(0+Δt)
    f_arr = _padded_field(f1, M)
    borders, nb, bvals = _border_descs(bc_b, mesh, 0.0)    # ctor applies borders with t = 0  (:207)
    L.check(L.lib().pg_solver_create_unsteady_mono(
        cap._h, phase.operator._h, C.byref(desc), borders, C.c_int32(nb),
        L.dptr(D_arr) if D_arr is not None else None, L.dptr(f_arr) if f_arr is not None else None,
        C.c_double(Δt), L.dptr(Tᵢ) if Tᵢ is not None else None, C.c_int32(L.PG_SCHEME[sch]), C.byref(s._h)))
    if sch == "CN":
        f0 = _padded_field(_eval(phase.source, cap._cw, 0.0, 3), M)
        if f0 is not None:
            L.check(L.lib().pg_solver_set_source(s._h, 0, L.dptr(f0), None))
        if callable(bc_i.value):
            g0 = _eval(bc_i.value, cap._cg, 0.0, 3)
            g0 = np.full(M, g0) if isinstance(g0, float) else g0
            L.check(L.lib().pg_solver_set_interface_value(s._h, L.dptr(g0), None))
    if bvals is not None:
        L.check(L.lib().pg_solver_set_border_values(s._h, L.dptr(bvals)))
    s._ctor_scheme = sch
    return s


def _time_dependent(fn, nspace: int, time_independent: bool = False) -> bool:
    """May data(fn) change from one step to the next?  The reference re-evaluates every closure and re-applies the
    border rows on every step (diffusion.jl:286-296), so nothing is guessed from samples: any callable that accepts
    a time argument (nspace + 1 positional arguments) is time dependent and takes the host-driven loop.  Only
    constants, callables without a t parameter, or an explicit `time_independent=True` from the caller let the
    whole loop run on the device (pg_solver_run)."""
    if not callable(fn) or time_independent:
        return False
    return _accepts(fn, nspace + 1)


def solve_DiffusionUnsteadyMono_b(s: Solver, phase: Phase, Δt: float, Tₑ: float, bc_b: BorderConditions, bc,
                                  scheme: str, method="bicgstab", algorithm=None, save_states: bool = True,
                                  verbose: bool = False, max_steps: Optional[int] = None,
                                  time_independent: bool = False, monitors=None, save_every: Optional[int] = None, **kwargs):
    """solve_DiffusionUnsteadyMono!(s, phase, Δt, Tₑ, bc_b, bc, scheme; method, algorithm, kwargs...)
    -- src/solver/diffusion.jl:268-301, quirks kept: the first solve uses the constructor's system and is
    states[1]; A is rebuilt once with `scheme`; `while t < Tₑ` with fp64 `t += Δt`; data at t+Δt.
    `time_independent=True` (not in the reference): the caller asserts that no closure depends on t, which lets the
    loop stay on the device although the closures have a t parameter.
    `monitors=[...]` (not in the reference): observables evaluated on the device after every solve, in whichever branch runs
    (s.monitor_series, s.monitor_times, s.monitor_names).  `save_every=k`: the device loop keeps every k-th state; s.states
    holds the first solve's state and those, s.state_steps = [0, k, 2k, ...] (refused together with verbose / log)."""
    if s is None or not s._h:
        raise PenguinHipError("Solver is not initialized. Call a solver constructor first.")  # :269-271
    log = bool(kwargs.get("log", False))
    mons, save_every = _check_monitor_args(monitors, save_every, verbose, log, s._nunk)
    opts = _krylov_opts(method, kwargs)
    _install_monitors(s, mons)
    s.state_steps = [0] if save_every else None
    if save_every:
        s.states = []                 # states and state_steps describe THIS call, entry for entry
    cap, mesh, M = phase.capacity, phase.capacity.mesh, s._ctx["M"]
    sch = L.PG_SCHEME[scheme] if scheme in L.PG_SCHEME else L.PG_SCHEME["BE"]
    t = 0.0
    info = L.pg_step_info()
    L.check(L.lib().pg_solver_initial_solve(s._h, C.byref(opts), C.byref(info)))   # :275
    _step_info_check(s, info, "the first solve")
    s._initial_done = True
    if log:
        s.ch.append({"iters": info.iters, "resnorm": info.resnorm, "isconverged": bool(info.converged)})
    s.x = s._fetch_state()
    if save_states or save_every:
        s.states.append(s.x)
    if verbose:
        print("Time: ", t)
        print("Solver Extremum: ", info.extremum)
    # closures with a time parameter are re-evaluated every step, as the reference does (never sampled and guessed)
    dyn_f = _time_dependent(phase.source, 3, time_independent)
    dyn_g = _time_dependent(bc.value, 3, time_independent)
    dyn_b = any(_time_dependent(getattr(c, "value", None), mesh.N, time_independent) for c in bc_b.borders.values())
    steps = 0
    # every time-dependent datum a TimeSeparable: spatial parts and coefficient table go to the device once, and the loop
    # is the one constant data take -- no pg_solver_set_* call inside it.  One plain closure among them: the host-driven loop.
    _clear_separable(s, 1)
    dyn_data = ([phase.source] if dyn_f else []) + ([bc.value] if dyn_g else []) + \
        [c.value for c in bc_b.borders.values() if _time_dependent(getattr(c, "value", None), mesh.N, time_independent)]
    # ... or a DeviceFunction: its program goes once, and a kernel evaluates it every step.  One kind per slot; the border slot
    # takes TimeSeparable values or DeviceFunctions, not both.
    dyn_bv = dyn_data[int(dyn_f) + int(dyn_g):]
    border_sep = border_prog = None
    if dyn_b and _device_data(dyn_data):
        if all(isinstance(v, TimeSeparable) for v in dyn_bv):
            border_sep = _separable_border(bc_b, mesh)
        elif all(isinstance(v, DeviceFunction) for v in dyn_bv):
            border_prog = _program_border(bc_b, mesh, time_independent)
    device = _device_data(dyn_data) and (not dyn_b or border_sep is not None or border_prog is not None)
    s.time_data = "device" if device else ("host" if dyn_data else None)
    if device:
        table = lambda coefs: _separable_table(coefs, Δt, Tₑ, max_steps)
        if len(table([])) > 0:
            times = _program_times(Δt, Tₑ, max_steps)
            if dyn_f and isinstance(phase.source, DeviceFunction):
                _install_program(s, _TD_SOURCE, 0, phase.source, 3, times)
            elif dyn_f:
                _install_separable(s, _TD_SOURCE, 0, _separable_fields(phase.source, cap._cw, 3, M), table(phase.source))
            if dyn_g and isinstance(bc.value, DeviceFunction):
                _install_program(s, _TD_INTERFACE, 0, bc.value, 3, times)
            elif dyn_g:
                _install_separable(s, _TD_INTERFACE, 0, _separable_fields(bc.value, cap._cg, 3, M), table(bc.value))
            if border_sep is not None:
                _install_separable(s, _TD_BORDER, 0, border_sep[0], table(border_sep[1]))
            elif border_prog is not None:
                L.check(L.lib().pg_solver_set_border_values(s._h, L.dptr(border_prog[0])))
                for kval, df in border_prog[1]:
                    _install_program(s, _TD_BORDER, 0, df, mesh.N, times, key=kval)
    if device or not (dyn_f or dyn_g or dyn_b):
        if (save_states and not save_every) or verbose or log:
            while t < Tₑ:
                if max_steps is not None and steps >= max_steps:
                    break
                t += Δt
                if verbose:
                    print("Time: ", t)
                L.check(L.lib().pg_solver_step(s._h, C.c_int32(sch), C.byref(opts), C.byref(info)))
                _step_info_check(s, info, "a time-step solve")
                s._have_run = True
                if log:
                    s.ch.append({"iters": info.iters, "resnorm": info.resnorm, "isconverged": bool(info.converged)})
                s.x = s._fetch_state()
                if save_states:
                    s.states.append(s.x)
                if verbose:
                    print("Solver Extremum: ", info.extremum)
                steps += 1
        else:
            run = L.pg_run_info()
            L.check(L.lib().pg_solver_run(s._h, C.c_double(Tₑ), C.c_int32(sch), C.byref(opts), C.c_int32(0),
                                          C.c_int64(-1 if max_steps is None else max_steps), C.c_int32(save_every or 0),
                                          C.byref(run)))
            s._have_run = True
            s.last_run = run
            if run.unconverged_steps:
                _check_converged(s, False, f"{run.unconverged_steps} of {run.steps} time-step solves", run.worst_relres)
            s.x = s._fetch_state()
            if save_every:
                _fetch_kept_states(s, save_every)
        _fetch_monitors(s)
        return s
    # time-dependent data: host-driven loop, closures evaluated at the reference's points and times
    sent = _UploadCache()
    while t < Tₑ:
        if max_steps is not None and steps >= max_steps:
            break
        t += Δt                                                             # :287
        if verbose:
            print("Time: ", t)
        if dyn_f or scheme == "CN":
            fn = _padded_field(_eval(phase.source, cap._cw, t, 3), M)
            fn1 = _padded_field(_eval(phase.source, cap._cw, t + Δt, 3), M)   # f(t+Δt), t already advanced (:248)
            zero = np.zeros(M)
            fn, fn1 = (fn if fn is not None else zero), (fn1 if fn1 is not None else zero)
            if sent.changed("f", fn, fn1):
                L.check(L.lib().pg_solver_set_source(s._h, 0, L.dptr(fn), L.dptr(fn1)))
        if callable(bc.value) and (dyn_g or scheme == "CN"):
            gn, gn1 = _eval(bc.value, cap._cg, t, 3), _eval(bc.value, cap._cg, t + Δt, 3)
            gn = np.full(M, gn) if isinstance(gn, float) else gn
            gn1 = np.full(M, gn1) if isinstance(gn1, float) else gn1
            if sent.changed("g", gn, gn1):
                L.check(L.lib().pg_solver_set_interface_value(s._h, L.dptr(gn), L.dptr(gn1)))
        if dyn_b:
            bv = _border_values(bc_b, mesh, t)
            if sent.changed("b", bv):
                L.check(L.lib().pg_solver_set_border_values(s._h, L.dptr(bv)))   # :292
        L.check(L.lib().pg_solver_step(s._h, C.c_int32(sch), C.byref(opts), C.byref(info)))            # :294
        _step_info_check(s, info, "a time-step solve")
        s._have_run = True
        if log:
            s.ch.append({"iters": info.iters, "resnorm": info.resnorm, "isconverged": bool(info.converged)})
        s.x = s._fetch_state()
        steps += 1
        if save_every:                                   # (the host-driven loop thins what it keeps the same way)
            if steps % save_every == 0:
                s.states.append(s.x)
                s.state_steps.append(steps)
        elif save_states:
            s.states.append(s.x)
        if verbose:
            print("Solver Extremum: ", info.extremum)
    _fetch_monitors(s)
    return s


# ---- diphasic twins (config 5) ---------------------------------------------------------------------


def DiffusionUnsteadyDiph(phase1: Phase, phase2: Phase, bc_b: BorderConditions, ic: InterfaceConditions, Δt: float,
                          Tᵢ: np.ndarray, scheme: str, verbose: bool = False, _ops_kind=None) -> Solver:
    """DiffusionUnsteadyDiph(phase1, phase2, bc_b, ic, Δt, Tᵢ, scheme) -- src/solver/diffusion.jl:319-332."""
    _require_ops(phase1, _ops_kind or DiffusionOps)
    _require_ops(phase2, _ops_kind or DiffusionOps)
    if verbose:
        print("Solver creation:\n- Diphasic problem\n- Unsteady problem\n- Diffusion problem")
    s = Solver("Unsteady", "Diphasic", "Diffusion")
    mesh = phase1.capacity.mesh
    # (Tᵢ = None is not taken here: as an array it fails the length check)
    Tᵢ = _unsteady_prelude(s, 4, mesh, np.asarray(Tᵢ, dtype=np.float64), dt=float(Δt))
    M = s._ctx["M"]
    desc, jump_keep = _jump_desc(ic, phase1, phase2)
    D1, D2 = _dcoef(phase1, M), _dcoef(phase2, M)
    f1 = _padded_field(_eval(phase1.source, phase1.capacity._cw, float(Δt), 3), M)
    f2 = _padded_field(_eval(phase2.source, phase2.capacity._cw, float(Δt), 3), M)
    borders, nb, bvals = _border_descs(bc_b, mesh, None)   # BC_border_diph! is called without t (:330)
    sch = "CN" if scheme == "CN" else "BE"
    p = lambda a: L.dptr(a) if a is not None else None
    L.check(L.lib().pg_solver_create_unsteady_diph(
        phase1.capacity._h, phase1.operator._h, phase2.capacity._h, phase2.operator._h, C.byref(desc), borders,
        C.c_int32(nb), p(D1), p(D2), p(f1), p(f2), C.c_double(Δt), L.dptr(Tᵢ), C.c_int32(L.PG_SCHEME[sch]), C.byref(s._h)))
    if sch == "CN":
        for q, ph in enumerate((phase1, phase2)):
            f0 = _padded_field(_eval(ph.source, ph.capacity._cw, 0.0, 3), M)
            if f0 is not None:
                L.check(L.lib().pg_solver_set_source(s._h, q, L.dptr(f0), None))
    if bvals is not None:
        L.check(L.lib().pg_solver_set_border_values(s._h, L.dptr(bvals)))
    s._ctor_scheme = sch
    return s


def solve_DiffusionUnsteadyDiph_b(s: Solver, phase1: Phase, phase2: Phase, Δt: float, Tₑ: float,
                                  bc_b: BorderConditions, ic: InterfaceConditions, scheme: str, method="bicgstab",
                                  algorithm=None, save_states: bool = True, verbose: bool = False,
                                  max_steps: Optional[int] = None, time_independent: bool = False, monitors=None,
                                  save_every: Optional[int] = None, **kwargs):
    """solve_DiffusionUnsteadyDiph!(...) -- src/solver/diffusion.jl:422-454.  Sources with a time parameter are
    re-evaluated every step (`time_independent=True`: the caller asserts they are constant in time).  `monitors`, `save_every`:
    as solve_DiffusionUnsteadyMono_b (4M weights; save_every takes the device loop unless a plain closure is among the data)."""
    if s is None or not s._h:
        raise PenguinHipError("Solver is not initialized. Call a solver constructor first.")
    mons, save_every = _check_monitor_args(monitors, save_every, verbose, bool(kwargs.get("log", False)), s._nunk)
    opts = _krylov_opts(method, kwargs)
    _install_monitors(s, mons)
    s.state_steps = [0] if save_every else None
    if save_every:
        s.states = []                 # states and state_steps describe THIS call, entry for entry
    M = s._ctx["M"]
    sch = L.PG_SCHEME[scheme] if scheme in L.PG_SCHEME else L.PG_SCHEME["BE"]
    dyn = any(_time_dependent(ph.source, 3, time_independent) for ph in (phase1, phase2))
    t = 0.0
    info = L.pg_step_info()
    if verbose:
        print("Time: ", t)
    L.check(L.lib().pg_solver_initial_solve(s._h, C.byref(opts), C.byref(info)))
    _step_info_check(s, info, "the first solve")
    s._initial_done = True
    s.x = s._fetch_state()
    if save_states or save_every:
        s.states.append(s.x)
    if verbose:
        print("Solver Extremum: ", info.extremum)
    steps = 0
    # every time-dependent source a TimeSeparable: installed once, and no pg_solver_set_source inside the loop
    _clear_separable(s, 2)
    dyn_src = [(q, ph.source) for q, ph in enumerate((phase1, phase2)) if _time_dependent(ph.source, 3, time_independent)]
    device = _device_data([f for _, f in dyn_src])
    s.time_data = "device" if device else ("host" if dyn_src else None)
    if device:
        if len(_separable_table([], Δt, Tₑ, max_steps)) > 0:
            for q, f in dyn_src:
                if isinstance(f, DeviceFunction):
                    _install_program(s, _TD_SOURCE, q, f, 3, _program_times(Δt, Tₑ, max_steps))
                else:
                    _install_separable(s, _TD_SOURCE, q, _separable_fields(f, (phase1, phase2)[q].capacity._cw, 3, M),
                                       _separable_table(f, Δt, Tₑ, max_steps))
    # the whole loop in one call: separable data without a history asked for, as before; and save_every, whose history the
    # device keeps, on separable or constant data
    if (device and not (save_states or verbose or kwargs.get("log", False))) or (save_every and (device or not dyn_src)):
        run = L.pg_run_info()
        L.check(L.lib().pg_solver_run(s._h, C.c_double(Tₑ), C.c_int32(sch), C.byref(opts), C.c_int32(0),
                                      C.c_int64(-1 if max_steps is None else max_steps), C.c_int32(save_every or 0),
                                      C.byref(run)))
        s._have_run = True
        s.last_run = run
        if run.unconverged_steps:
            _check_converged(s, False, f"{run.unconverged_steps} of {run.steps} time-step solves", run.worst_relres)
        s.x = s._fetch_state()
        if save_every:
            _fetch_kept_states(s, save_every)
        _fetch_monitors(s)
        return s
    sent = _UploadCache()
    while t < Tₑ:
        if max_steps is not None and steps >= max_steps:
            break
        t += Δt
        if verbose:
            print("Time: ", t)
        if not device and (dyn or scheme == "CN"):
            for q, ph in enumerate((phase1, phase2)):
                fn = _padded_field(_eval(ph.source, ph.capacity._cw, t, 3), M)
                fn1 = _padded_field(_eval(ph.source, ph.capacity._cw, t + Δt, 3), M)
                zero = np.zeros(M)
                fn, fn1 = (fn if fn is not None else zero), (fn1 if fn1 is not None else zero)
                if sent.changed(("f", q), fn, fn1):
                    L.check(L.lib().pg_solver_set_source(s._h, q, L.dptr(fn), L.dptr(fn1)))
        L.check(L.lib().pg_solver_step(s._h, C.c_int32(sch), C.byref(opts), C.byref(info)))
        _step_info_check(s, info, "a time-step solve")
        s._have_run = True
        s.x = s._fetch_state()
        steps += 1
        if save_every:
            if steps % save_every == 0:
                s.states.append(s.x)
                s.state_steps.append(steps)
        elif save_states:
            s.states.append(s.x)
        if verbose:
            print("Solver Extremum: ", info.extremum)
    _fetch_monitors(s)
    return s


# =============================================================================== steady diffusion


def _interface_desc(bc_i, cg, t):
    """pg_bc_desc of a monophasic interface condition (value constant or evaluated at C_γ)."""
    if isinstance(bc_i, Dirichlet):
        kind, a, b = L.PG_BC_DIRICHLET, 0.0, 0.0
    elif isinstance(bc_i, Neumann):
        kind, a, b = L.PG_BC_NEUMANN, 0.0, 0.0
    elif isinstance(bc_i, Robin):
        kind, a, b = L.PG_BC_ROBIN, float(bc_i.α), float(bc_i.β)
    else:
        raise TypeError(f"unsupported interface condition {bc_i!r}")
    g_arr, gval = None, 0.0
    if callable(bc_i.value):
        g = _eval(bc_i.value, cg, t, 3)
        if isinstance(g, float):
            gval = g
        else:
            g_arr = g
    else:
        gval = float(bc_i.value)
    return L.pg_bc_desc(kind, a, b, gval, L.dptr(g_arr) if g_arr is not None else None), g_arr


def _jump_desc(ic: InterfaceConditions, phase1: Phase, phase2: Phase):
    """pg_jump_desc of a diphasic problem: g at C_γ of phase 1, h at C_γ of phase 2, both built WITHOUT t (diffusion.jl:397;
    the moving solvers: build_g_g(operator, jump, capacity), prescribedmotionsolver/diffusion.jl:423-424).  Returns the
    evaluated arrays too: the descriptor holds their addresses.  (What _eval returns is a contiguous float64 array already.)"""
    jump, flux = ic.scalar, ic.flux
    g = _eval(jump.value, phase1.capacity._cg, None, 3) if callable(jump.value) else float(jump.value)
    h = _eval(flux.value, phase2.capacity._cg, None, 3) if callable(flux.value) else float(flux.value)
    g_arr = None if isinstance(g, float) else g
    h_arr = None if isinstance(h, float) else h
    desc = L.pg_jump_desc(float(jump.α1), float(jump.α2), g if isinstance(g, float) else 0.0, float(flux.β1),
                          float(flux.β2), h if isinstance(h, float) else 0.0,
                          L.dptr(g_arr) if g_arr is not None else None, L.dptr(h_arr) if h_arr is not None else None)
    return desc, (g_arr, h_arr)


def _unsteady_prelude(s: Solver, K: int, mesh: Mesh, Tᵢ: Optional[np.ndarray], **ctx) -> Optional[np.ndarray]:
    """What every unsteady constructor does first: M = prod(n+1), the unknown count K*M (K = 2 mono, 4 diph), Tᵢ as a
    contiguous float64 vector of that length (None = zeros(K*M) without materialising it on the host, multi-GPU sizes) and
    s._ctx (M and what the caller adds)."""
    M = int(np.prod(mesh.ext))
    s._nunk = K * M
    if Tᵢ is not None:
        Tᵢ = np.ascontiguousarray(Tᵢ, dtype=np.float64)
        if Tᵢ.shape != (K * M,):
            raise ValueError(f"Tᵢ must have length {K}*prod(n+1) = {K * M}")
    s._ctx = dict(M=M, **ctx)
    return Tᵢ


def _dcoef(ph: Phase, M: int):
    D = _eval(ph.Diffusion_coeff, ph.capacity._cw, None, 3) if callable(ph.Diffusion_coeff) else float(ph.Diffusion_coeff)
    if isinstance(D, float):
        return None if D == 1.0 else np.full(M, D)
    return D


def DiffusionSteadyMono(phase: Phase, bc_b: BorderConditions, bc_i, verbose: bool = False, _ops_kind=None) -> Solver:
    """DiffusionSteadyMono(phase, bc_b, bc_i) -- src/solver/diffusion.jl:14-28."""
    _require_ops(phase, _ops_kind or DiffusionOps)
    if verbose:
        print("Solver creation:\n- Monophasic problem\n- Steady problem\n- Diffusion problem")
    s = Solver("Steady", "Monophasic", "Diffusion")
    cap, mesh = phase.capacity, phase.capacity.mesh
    M = int(np.prod(mesh.ext))
    s._nunk = 2 * M
    desc, g_keep = _interface_desc(bc_i, cap._cg, None)            # build_g_g without t  (:51)
    D_arr = _dcoef(phase, M)
    f_arr = _padded_field(_eval(phase.source, cap._cw, None, 3), M)  # build_source without t  (:50)
    borders, nb, bvals = _border_descs(bc_b, mesh, None)             # BC_border_mono!(A, b, bc_b, mesh)  (:25)
    p = lambda a: L.dptr(a) if a is not None else None
    L.check(L.lib().pg_solver_create_steady_mono(cap._h, phase.operator._h, C.byref(desc), borders, C.c_int32(nb),
                                                 p(D_arr), p(f_arr), C.byref(s._h)))
    if bvals is not None:
        L.check(L.lib().pg_solver_set_border_values(s._h, L.dptr(bvals)))
    s._ctx = dict(M=M, phase=phase)   # (the handle points into the phase's capacity and operators: they live as long as it)
    s._ctor_scheme = "STEADY"
    return s


def _solve_steady(s: Solver, method, kwargs, banner: str, verbose: bool):
    if s is None or not s._h:
        raise PenguinHipError("Solver is not initialized. Call a solver constructor first.")
    if verbose:
        print(banner)
    kwargs = dict(kwargs)
    kwargs.setdefault("warm_start", False)
    opts = _krylov_opts(method, kwargs)
    info = L.pg_step_info()
    L.check(L.lib().pg_solver_initial_solve(s._h, C.byref(opts), C.byref(info)))   # solve_system!(s; ...)
    _step_info_check(s, info, "the first solve")
    s._initial_done = True
    s.x = s._fetch_state()
    s.ch.append(dict(iters=info.iters, converged=bool(info.converged), resnorm=info.resnorm, bnorm=info.bnorm))
    return s


def solve_DiffusionSteadyMono_b(s: Solver, method="bicgstab", algorithm=None, verbose: bool = False, **kwargs):
    """solve_DiffusionSteadyMono!(s; method, algorithm, kwargs...) -- src/solver/diffusion.jl:60-71."""
    return _solve_steady(s, method, kwargs, "Solving the system:\n- Monophasic problem\n- Steady problem\n- Diffusion problem",
                         verbose)


def DiffusionSteadyDiph(phase1: Phase, phase2: Phase, bc_b: BorderConditions, ic: InterfaceConditions,
                        verbose: bool = False, _ops_kind=None) -> Solver:
    """DiffusionSteadyDiph(phase1, phase2, bc_b, ic) -- src/solver/diffusion.jl:88-101."""
    _require_ops(phase1, _ops_kind or DiffusionOps)
    _require_ops(phase2, _ops_kind or DiffusionOps)
    if verbose:
        print("Solver creation:\n- Diphasic problem\n- Steady problem\n- Diffusion problem")
    s = Solver("Steady", "Diphasic", "Diffusion")
    mesh = phase1.capacity.mesh
    M = int(np.prod(mesh.ext))
    s._nunk = 4 * M
    desc, jump_keep = _jump_desc(ic, phase1, phase2)
    p = lambda a: L.dptr(a) if a is not None else None
    D1, D2 = _dcoef(phase1, M), _dcoef(phase2, M)
    f1 = _padded_field(_eval(phase1.source, phase1.capacity._cw, None, 3), M)
    f2 = _padded_field(_eval(phase2.source, phase2.capacity._cw, None, 3), M)
    borders, nb, bvals = _border_descs(bc_b, mesh, None)
    L.check(L.lib().pg_solver_create_steady_diph(
        phase1.capacity._h, phase1.operator._h, phase2.capacity._h, phase2.operator._h, C.byref(desc), borders,
        C.c_int32(nb), p(D1), p(D2), p(f1), p(f2), C.byref(s._h)))
    if bvals is not None:
        L.check(L.lib().pg_solver_set_border_values(s._h, L.dptr(bvals)))
    s._ctx = dict(M=M, phase1=phase1, phase2=phase2)   # (as the monophasic constructor: the handle points into them)
    s._ctor_scheme = "STEADY"
    return s


def solve_DiffusionSteadyDiph_b(s: Solver, method="bicgstab", algorithm=None, verbose: bool = False, **kwargs):
    """solve_DiffusionSteadyDiph!(s; method, algorithm, kwargs...) -- src/solver/diffusion.jl:164-175."""
    return _solve_steady(s, method, kwargs, "Solving the system:\n- Diphasic problem\n- Steady problem\n- Diffusion problem",
                         verbose)


# =============================================================================== advection-diffusion
# src/solver/advectiondiffusion.jl: the diffusion drivers with conv_bulk = ΣC_d and conv_iface = ½ΣK_d added to the
# bulk rows; the library assembles them whenever the phase's operator is a ConvectionOps.  The reference's unsteady
# monophasic loop raises a MethodError after the first solve (8 arguments for the 9-parameter b_mono_unstead_advdiff,
# :272 vs :215) and its constructor leaves the border rows out; what runs here is the evident intent: the loop and the
# constructor of DiffusionUnsteadyMono with the advection-diffusion blocks.


def _require_ops(phase: Phase, kind):
    if not isinstance(phase.operator, kind) or (kind is DiffusionOps and isinstance(phase.operator, ConvectionOps)):
        raise TypeError(f"phase.operator must be a {kind.__name__}")   # Julia: MethodError on the ::{kind} argument


def AdvectionDiffusionSteadyMono(phase: Phase, bc_b: BorderConditions, bc_i, verbose: bool = False) -> Solver:
    """AdvectionDiffusionSteadyMono(phase, bc_b, bc_i) -- src/solver/advectiondiffusion.jl:13-27."""
    _require_ops(phase, ConvectionOps)
    s = DiffusionSteadyMono(phase, bc_b, bc_i, verbose=verbose, _ops_kind=ConvectionOps)
    s.equation_type = "DiffusionAdvection"
    return s


def solve_AdvectionDiffusionSteadyMono_b(s: Solver, method="bicgstab", algorithm=None, **kwargs):
    """solve_AdvectionDiffusionSteadyMono!(s; ...) -- src/solver/advectiondiffusion.jl:60-66."""
    return _solve_steady(s, method, kwargs, "", False)


def AdvectionDiffusionSteadyDiph(phase1: Phase, phase2: Phase, bc_b: BorderConditions, ic: InterfaceConditions,
                                 verbose: bool = False) -> Solver:
    """AdvectionDiffusionSteadyDiph(phase1, phase2, bc_b, ic) -- src/solver/advectiondiffusion.jl:80-93."""
    _require_ops(phase1, ConvectionOps)
    _require_ops(phase2, ConvectionOps)
    s = DiffusionSteadyDiph(phase1, phase2, bc_b, ic, verbose=verbose, _ops_kind=ConvectionOps)
    s.equation_type = "DiffusionAdvection"
    return s


def solve_AdvectionDiffusionSteadyDiph_b(s: Solver, method="bicgstab", algorithm=None, **kwargs):
    """solve_AdvectionDiffusionSteadyDiph!(s; ...) -- src/solver/advectiondiffusion.jl:141-147."""
    return _solve_steady(s, method, kwargs, "", False)


def AdvectionDiffusionUnsteadyMono(phase: Phase, bc_b: BorderConditions, bc_i, Δt: float, Tᵢ: np.ndarray, scheme: str,
                                   verbose: bool = False) -> Solver:
    """AdvectionDiffusionUnsteadyMono(phase, bc_b, bc_i, Δt, Tᵢ, scheme) -- src/solver/advectiondiffusion.jl:163-178."""
    _require_ops(phase, ConvectionOps)
    if scheme not in ("BE", "CN"):
        raise ValueError("Unknown scheme.")                       # :203-205
    s = DiffusionUnsteadyMono(phase, bc_b, bc_i, Δt, Tᵢ, scheme, verbose=verbose, _ops_kind=ConvectionOps)
    s.equation_type = "DiffusionAdvection"
    return s


def solve_AdvectionDiffusionUnsteadyMono_b(s: Solver, phase: Phase, Δt: float, Tₑ: float, bc_b: BorderConditions, bc,
                                           scheme: str, method="bicgstab", algorithm=None, **kwargs):
    """solve_AdvectionDiffusionUnsteadyMono!(...) -- src/solver/advectiondiffusion.jl:256-282 (intended loop)."""
    return solve_DiffusionUnsteadyMono_b(s, phase, Δt, Tₑ, bc_b, bc, scheme, method=method, algorithm=algorithm, **kwargs)


def AdvectionDiffusionUnsteadyDiph(phase1: Phase, phase2: Phase, bc_b: BorderConditions, ic: InterfaceConditions, Δt: float,
                                   Tᵢ: np.ndarray, scheme: str, verbose: bool = False) -> Solver:
    """AdvectionDiffusionUnsteadyDiph(phase1, phase2, bc_b, ic, Δt, Tᵢ, scheme) -- src/solver/advectiondiffusion.jl:299-311.

    Backward Euler only.  The reference's Crank-Nicolson right-hand side for this driver carries the convection terms
    but not the diffusion part of the explicit half step (:375-377), so it is neither Crank-Nicolson nor what the
    device loop computes (b from Â xⁿ with the one run matrix); rather than return a different answer silently, "CN"
    is refused.  As with the monophasic driver the border rows are applied from the constructor on (the reference's
    constructor leaves them out and its loop adds them, :404)."""
    _require_ops(phase1, ConvectionOps)
    _require_ops(phase2, ConvectionOps)
    if scheme not in ("BE", "CN"):
        raise ValueError("Unknown scheme.")                       # :343-345
    if scheme == "CN":
        raise PenguinHipError('AdvectionDiffusionUnsteadyDiph: scheme "CN" is not available on the HIP path (the reference\'s '
                              "right-hand side for it omits the diffusion term, advectiondiffusion.jl:375-377); use \"BE\"")
    s = DiffusionUnsteadyDiph(phase1, phase2, bc_b, ic, Δt, Tᵢ, "BE", verbose=verbose, _ops_kind=ConvectionOps)
    s.equation_type = "DiffusionAdvection"
    return s


def solve_AdvectionDiffusionUnsteadyDiph_b(s: Solver, phase1: Phase, phase2: Phase, Δt: float, Tₑ: float,
                                           bc_b: BorderConditions, ic: InterfaceConditions, scheme: str,
                                           method="bicgstab", algorithm=None, **kwargs):
    """solve_AdvectionDiffusionUnsteadyDiph!(...) -- src/solver/advectiondiffusion.jl:389-418 (BE, see the constructor)."""
    if scheme != "BE":
        raise PenguinHipError('solve_AdvectionDiffusionUnsteadyDiph!: only scheme "BE" is available on the HIP path')
    return solve_DiffusionUnsteadyDiph_b(s, phase1, phase2, Δt, Tₑ, bc_b, ic, "BE", method=method, algorithm=algorithm, **kwargs)


# =============================================================================== Darcy (src/solver/darcy.jl: aliases)


def DarcyFlow(phase: Phase, bc_b: BorderConditions, bc_i, verbose: bool = False) -> Solver:
    """DarcyFlow(phase, bc_b, bc_i) -- src/solver/darcy.jl:1-15: the steady monophasic diffusion system."""
    if verbose:
        print("Solver Creation:\n- Darcy Flow\n- Steady problem\n- Monophasic")
    return DiffusionSteadyMono(phase, bc_b, bc_i)


def solve_DarcyFlow_b(s: Solver, method="bicgstab", algorithm=None, **kwargs):
    """solve_DarcyFlow!(s; ...) -- src/solver/darcy.jl:17-24 (solve_system! + push!(s.states, s.x))."""
    _solve_steady(s, method, kwargs, "", False)
    s.states.append(s.x)
    return s


def solve_darcy_velocity(solver: Solver, Fluide: Phase, state_i: int = 1) -> np.ndarray:
    """solve_darcy_velocity(solver, Fluide; state_i=1) -- src/solver/darcy.jl:26-41: u = -∇(op, p) with p masked to NaN
    outside the fluid (pω where cell_types == 0; pγ where cell_types is 0 or 1).  state_i is 1-based as in Julia."""
    ct = Fluide.capacity.cell_types
    st = np.array(solver.states[state_i - 1], dtype=np.float64)
    half = st.shape[0] // 2
    pw, pg = st[:half].copy(), st[half:].copy()
    pw[ct == 0] = np.nan
    pg[ct == 0] = np.nan
    pg[ct == 1] = np.nan
    return -grad(Fluide.operator, np.concatenate([pw, pg]))


def DarcyFlowUnsteady(phase: Phase, bc_b: BorderConditions, bc_i, Δt: float, Tᵢ: np.ndarray, scheme: str,
                      verbose: bool = False) -> Solver:
    """DarcyFlowUnsteady(...) -- src/solver/darcy.jl:46-58: the unsteady monophasic diffusion system."""
    return DiffusionUnsteadyMono(phase, bc_b, bc_i, Δt, Tᵢ, scheme, verbose=verbose)


def solve_DarcyFlowUnsteady_b(s: Solver, phase: Phase, Δt: float, Tₑ: float, bc_b: BorderConditions, bc_i, scheme: str,
                              method="bicgstab", algorithm=None, **kwargs):
    """solve_DarcyFlowUnsteady!(...) -- src/solver/darcy.jl:60-91: the loop of solve_DiffusionUnsteadyMono! with the
    matrix rebuilt every step (same matrix: constant data)."""
    return solve_DiffusionUnsteadyMono_b(s, phase, Δt, Tₑ, bc_b, bc_i, scheme, method=method, algorithm=algorithm, **kwargs)


# =============================================================================== convergence metric


def lp_norm(errors, indices, pval, capacity: Capacity):
    """src/convergence.jl:4-15."""
    V = capacity.V
    if pval == math.inf:
        return float(np.max(np.abs(errors[indices]), initial=0.0))
    return float((np.sum(np.abs(errors[indices]) ** pval * V[indices]) / np.sum(V)) ** (1.0 / pval))


def _eval_points(u: Callable, C: np.ndarray) -> np.ndarray:
    """u at the rows of C: one call with coordinate arrays when the callable takes them (a few million centroids in 3-D),
    else point by point as `map(c -> u(c...), C)` does."""
    try:
        out = np.asarray(u(*[C[:, d] for d in range(C.shape[1])]), dtype=np.float64)
        if out.shape == (C.shape[0],):
            return out
    except Exception:
        pass
    return np.array([u(*c) for c in C], dtype=np.float64)


def check_convergence(u_analytical: Callable, solver: Solver, capacity: Capacity, p=2):
    """src/convergence.jl:45-93 (absolute norms)."""
    Cw = capacity.C_ω
    u_ana = _eval_points(u_analytical, Cw)
    u_num = solver.x[: len(solver.x) // 2]
    err = u_ana - u_num
    ct = capacity.cell_types
    sel = lambda m: np.flatnonzero(m)
    return (u_ana, u_num, lp_norm(err, sel((ct == 1) | (ct == -1)), p, capacity), lp_norm(err, sel(ct == 1), p, capacity),
            lp_norm(err, sel(ct == -1), p, capacity), lp_norm(err, sel(ct == 0), p, capacity))


def check_convergence_diph(u1_analytical: Callable, u2_analytical: Callable, solver: Solver, capacity1: Capacity,
                           capacity2: Capacity, p=2):
    """src/convergence.jl:114-234 (absolute norms): ((u1_ana, u2_ana), (u1_num, u2_num), global, full, cut, empty), each error
    entry a triple (phase 1, phase 2, max of both)."""
    M = len(capacity1.V)
    x = solver.states[-1] if solver.states else solver.x
    u_num = (x[:M], x[2 * M:3 * M])
    out_ana, errs = [], []
    for cap, ua, un in ((capacity1, u1_analytical, u_num[0]), (capacity2, u2_analytical, u_num[1])):
        ana = _eval_points(ua, cap.C_ω)
        err = ana - un
        ct = cap.cell_types
        sel = lambda m: np.flatnonzero(m)
        out_ana.append(ana)
        errs.append((lp_norm(err, sel((ct == 1) | (ct == -1)), p, cap), lp_norm(err, sel(ct == 1), p, cap),
                     lp_norm(err, sel(ct == -1), p, cap), lp_norm(err, sel(ct == 0), p, cap)))
    trip = lambda k: (errs[0][k], errs[1][k], max(errs[0][k], errs[1][k]))
    return tuple(out_ana), u_num, trip(0), trip(1), trip(2), trip(3)
