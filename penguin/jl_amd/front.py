"""FrontTracker -- the reference's marker front (src/front_tracking.jl:5-340) as a body: a closed polyline of markers whose
interior is the fluid.  `Capacity(front, mesh)` sends the markers to pg_capacity_create_polygon, where the capacity kernels
measure the polygon itself (penguin/jl_amd/csrc/pg_geom_polygon.h).  Everything in this file runs on the host in numpy: the
marker generators with the reference's formulas, `is_point_inside` and `sdf` -- the object is callable as front(x, y) and returns
the signed distance, negative inside, so that cap.body behaves like the other bodies.  The `_b` suffix stands for `!`.
MovingFront is a front that moves: a callable t -> markers, for Capacity(mf, SpaceTimeMesh(...)) and the moving solvers."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np


class FrontTracker:
    """FrontTracker(markers=None, is_closed=True) -- front_tracking.jl:5-22.  markers: [(x, y), ...]."""

    def __init__(self, markers: Optional[Sequence[Tuple[float, float]]] = None, is_closed: bool = True):
        self.markers: List[Tuple[float, float]] = []
        self.is_closed = bool(is_closed)
        if markers is not None:
            set_markers_b(self, markers)

    def __call__(self, x, y, *_):
        return sdf(self, x, y)

    def __repr__(self):
        return f"FrontTracker({len(self.markers)} markers, is_closed={self.is_closed})"

    def polygon(self) -> np.ndarray:
        """(M, 2) markers without the closing duplicate of the first"""
        p = np.asarray(self.markers, dtype=np.float64).reshape(-1, 2)
        if len(p) >= 2 and p[0, 0] == p[-1, 0] and p[0, 1] == p[-1, 1]:
            p = p[:-1]
        return np.ascontiguousarray(p)


def get_markers(ft: FrontTracker):
    return ft.markers


def set_markers_b(ft: FrontTracker, markers, is_closed: Optional[bool] = None) -> FrontTracker:
    ft.markers = [(float(x), float(y)) for x, y in markers]
    if is_closed is not None:
        ft.is_closed = bool(is_closed)
    return ft


def add_marker_b(ft: FrontTracker, x: float, y: float) -> FrontTracker:
    ft.markers.append((float(x), float(y)))
    return ft


def create_circle_b(ft: FrontTracker, center_x: float, center_y: float, radius: float, n_markers: int = 100) -> FrontTracker:
    """front_tracking.jl:91-104: marker i at the angle 2 pi (i / n), i = 0 .. n - 1"""
    m = []
    for i in range(n_markers):
        angle = 2.0 * math.pi * (i / n_markers)
        m.append((center_x + radius * math.cos(angle), center_y + radius * math.sin(angle)))
    return set_markers_b(ft, m, True)


def create_rectangle_b(ft: FrontTracker, min_x: float, min_y: float, max_x: float, max_y: float, n_markers: int = 100) -> FrontTracker:
    """front_tracking.jl:116-214: markers spread over the four sides in proportion to their lengths, none at a corner (the
    corners are cut), starting on the bottom side, counter-clockwise, closed by a duplicate of the first marker"""
    width, height = max_x - min_x, max_y - min_y
    perimeter = 2 * (width + height)
    total = n_markers - 4
    ppu = total / perimeter
    n_bottom = max(1, round(width * ppu))
    n_right = max(1, round(height * ppu))
    n_top = max(1, round(width * ppu))
    n_left = max(1, round(height * ppu))
    actual = n_bottom + n_right + n_top + n_left
    if actual < total:
        extra = total - actual
        if width >= height:
            eb = round(extra / 2)
            n_bottom += eb
            n_top += extra - eb
        else:
            er = round(extra / 2)
            n_right += er
            n_left += extra - er
    elif actual > total:
        excess = actual - total
        if width >= height:
            eb = round(excess / 2)
            n_bottom = max(1, n_bottom - eb)
            n_top = max(1, n_top - (excess - eb))
        else:
            er = round(excess / 2)
            n_right = max(1, n_right - er)
            n_left = max(1, n_left - (excess - er))
    m = []
    for i in range(1, n_bottom + 1):
        m.append((min_x + i / (n_bottom + 1) * width, min_y))
    for i in range(1, n_right + 1):
        m.append((max_x, min_y + i / (n_right + 1) * height))
    for i in range(1, n_top + 1):
        m.append((max_x - i / (n_top + 1) * width, max_y))
    for i in range(1, n_left + 1):
        m.append((min_x, max_y - i / (n_left + 1) * height))
    m.append(m[0])
    return set_markers_b(ft, m, True)


def create_ellipse_b(ft: FrontTracker, center_x: float, center_y: float, radius_x: float, radius_y: float,
                     n_markers: int = 100) -> FrontTracker:
    """front_tracking.jl:221-226: the angles range(0, 2 pi, length = n + 1) without the last"""
    step = 2.0 * math.pi / n_markers
    m = [(center_x + radius_x * math.cos(i * step), center_y + radius_y * math.sin(i * step)) for i in range(n_markers)]
    return set_markers_b(ft, m, True)


def create_crystal_b(ft: FrontTracker, center_x: float, center_y: float, base_radius: float, n_lobes: int = 6,
                     amplitude: float = 0.2, n_markers: int = 100) -> FrontTracker:
    """front_tracking.jl:240-266: r = base_radius (1 + amplitude cos(n_lobes theta)), theta = 2 pi (i - 1) / n, closed by a duplicate
    of the first marker"""
    m = []
    for i in range(1, n_markers + 1):
        theta = 2.0 * math.pi * (i - 1) / n_markers
        r = base_radius * (1.0 + amplitude * math.cos(n_lobes * theta))
        m.append((center_x + r * math.cos(theta), center_y + r * math.sin(theta)))
    m.append(m[0])
    return set_markers_b(ft, m, True)


def is_point_inside(ft: FrontTracker, x, y):
    """even-odd, with the crossing rule of the kernels: edge (p, q) crosses the line at height y iff (p_y <= y) != (q_y <= y),
    and the point is inside iff an odd number of crossings lie at or left of x.  Arrays broadcast."""
    p = ft.polygon()
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    if len(p) < 3:
        return np.zeros(x.shape, dtype=bool) if x.shape else False
    q = np.roll(p, -1, axis=0)
    X, Y = x[..., None], y[..., None]
    cross = (p[:, 1] <= Y) != (q[:, 1] <= Y)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = p[:, 0] + (Y - p[:, 1]) * (q[:, 0] - p[:, 0]) / (q[:, 1] - p[:, 1])
    c = np.clip(c, np.minimum(p[:, 0], q[:, 0]), np.maximum(p[:, 0], q[:, 0]))
    inside = (np.count_nonzero(cross & (c <= X), axis=-1) % 2) == 1
    return inside if x.shape else bool(inside)


def sdf(ft: FrontTracker, x, y):
    """signed distance to the front, negative inside (front_tracking.jl:325-340); inf without a geometry"""
    p = ft.polygon()
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    if len(p) < 3:
        return np.full(x.shape, np.inf) if x.shape else math.inf
    q = np.roll(p, -1, axis=0)
    if not ft.is_closed:
        p, q = p[:-1], q[:-1]
    X, Y = x[..., None], y[..., None]
    ex, ey = q[:, 0] - p[:, 0], q[:, 1] - p[:, 1]
    ee = ex * ex + ey * ey
    t = np.clip(((X - p[:, 0]) * ex + (Y - p[:, 1]) * ey) / np.where(ee > 0.0, ee, 1.0), 0.0, 1.0)
    dist = np.min(np.hypot(X - (p[:, 0] + t * ex), Y - (p[:, 1] + t * ey)), axis=-1)
    out = np.where(is_point_inside(ft, x, y), -dist, dist)
    return out if x.shape else float(out)


class MovingFront:
    """MovingFront(markers_of_t, complement=False): a marker polygon that moves.  `markers_of_t(t)` returns the (M, 2) markers at
    time t, the same count and order at every t.  `Capacity(mf, SpaceTimeMesh(mesh, [t, t + Δt]))` evaluates it at the slab's two
    times only and moves every marker on a straight line at constant speed in between -- the reference's interpolate_front
    (src/front_tracking.jl:2289-2307) inside compute_spacetime_capacities (:1472); the prescribed-motion drivers take it as
    `body`, and `MovingFront(..., complement=True)` (fluid outside) as `body_c`.  Callable as mf(x, y, t): the signed distance to
    the polygon of `markers_of_t(t)`, negative in the fluid."""

    def __init__(self, markers_of_t, complement: bool = False):
        if not callable(markers_of_t):
            raise TypeError("MovingFront: markers_of_t must be callable, t -> (M, 2) markers (two fronts: MovingFront.from_fronts)")
        self.markers_of_t, self.complement = markers_of_t, bool(complement)
        self._count = None

    def markers(self, t: float) -> np.ndarray:
        """the (M, 2) markers at t, as float64; the count must not change between calls"""
        p = np.ascontiguousarray(np.asarray(self.markers_of_t(float(t)), dtype=np.float64))
        if p.ndim != 2 or p.shape[1] != 2:
            raise ValueError(f"MovingFront: markers_of_t(t) must return an (M, 2) array, got shape {p.shape}")
        if self._count is None:
            self._count = len(p)
        elif len(p) != self._count:
            raise ValueError(f"MovingFront: {len(p)} markers at t = {t}, {self._count} before: the count and order must not change")
        return p

    def at(self, t: float) -> FrontTracker:
        return FrontTracker([tuple(r) for r in self.markers(t)])

    def __call__(self, x, y, t, *_):
        d = sdf(self.at(t), x, y)
        return -d if self.complement else d

    def __repr__(self):
        return f"MovingFront({self._count if self._count is not None else '?'} markers, complement={self.complement})"

    @classmethod
    def rigid(cls, front, shift=None, angle=None, about=(0.0, 0.0), complement: bool = False) -> "MovingFront":
        """the markers of `front` (a FrontTracker or an (M, 2) array) turned by angle(t) about `about`, then moved by shift(t)"""
        base = front.polygon() if isinstance(front, FrontTracker) else np.asarray(front, dtype=np.float64).reshape(-1, 2)
        c = np.asarray(about, dtype=np.float64)

        def markers_of_t(t):
            a = float(angle(t)) if angle is not None else 0.0
            d = np.asarray(shift(t), dtype=np.float64) if shift is not None else np.zeros(2)
            ca, sa = math.cos(a), math.sin(a)
            r = base - c
            return np.column_stack([c[0] + ca * r[:, 0] - sa * r[:, 1] + d[0], c[1] + sa * r[:, 0] + ca * r[:, 1] + d[1]])
        return cls(markers_of_t, complement)

    @classmethod
    def from_fronts(cls, fronts, times, complement: bool = False) -> "MovingFront":
        """piecewise linear in time through the given fronts (FrontTrackers or (M, 2) arrays) at the ascending `times`; exactly
        fronts[i] at times[i]"""
        P = [f.polygon() if isinstance(f, FrontTracker) else np.asarray(f, dtype=np.float64).reshape(-1, 2) for f in fronts]
        T = [float(t) for t in times]
        if len(P) != len(T) or len(P) < 2:
            raise ValueError("MovingFront.from_fronts: as many times as fronts, at least two")
        if any(b <= a for a, b in zip(T[:-1], T[1:])):
            raise ValueError("MovingFront.from_fronts: the times must ascend")
        if any(p.shape != P[0].shape for p in P):
            raise ValueError("MovingFront.from_fronts: every front needs the same number of markers")

        def markers_of_t(t):
            if not T[0] <= t <= T[-1]:
                raise ValueError(f"MovingFront.from_fronts: t = {t} outside [{T[0]}, {T[-1]}]")
            for i, ti in enumerate(T):
                if t == ti:
                    return P[i].copy()
            i = int(np.searchsorted(T, t)) - 1
            s = (t - T[i]) / (T[i + 1] - T[i])
            return P[i] + s * (P[i + 1] - P[i])
        return cls(markers_of_t, complement)
