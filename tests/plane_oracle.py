"""CPU reference for oblique half spaces, f(x) = n.x - offset with the fluid where f < 0: a duck-typed body for
oracle.penguin_oracle.make_capacity (`box`, `section`), in a formulation that shares nothing with the kernels' (pg_geom.h
integrates exact sections along the dominant axis with Simpson's rule):

  classification  the rule of the ABI, verbatim: far = sum_d (n_d > 0 ? n_d hi_d : n_d lo_d), near the same with lo and hi
                  swapped; FULL if far <= offset, EMPTY if near >= offset, CUT otherwise; complement: n -> -n, offset -> -offset
  N = 1           the crossing point
  N = 2           Sutherland-Hodgman clipping of the rectangle by the half plane, shoelace formula
  N = 3           the box corners on the fluid side and the edge / plane intersection points go into scipy.spatial.ConvexHull;
                  volume and centroid from the hull's simplices about the mean point; the interface polygon is measured in an
                  in-plane basis
  sections        the same class one dimension down

Coordinates are taken relative to the box corner whose level is nearest the plane, so that a cut of 1e-16 of a cell (a plane
through a mesh node, up to rounding) still has a polygon / polytope with distinct vertices.
"""
from __future__ import annotations

import itertools
import math
from typing import Sequence

import numpy as np

from oracle.geometry import CUT, EMPTY, FULL, BoxMeasure, _prod


def classify(n: Sequence[float], off: float, lo: Sequence[float], hi: Sequence[float]):
    far = 0.0
    near = 0.0
    for d in range(len(n)):
        a, b = n[d] * lo[d], n[d] * hi[d]
        far = far + (b if n[d] > 0.0 else a)
        near = near + (a if n[d] > 0.0 else b)
    if far <= off:
        return FULL, near, far
    if near >= off:
        return EMPTY, near, far
    return CUT, near, far


def _local_frame(n, off, near, far, lo, hi):
    """origin (the near or the far corner), the box corners relative to it with their levels g = n.p - alpha (fluid: g <= 0)"""
    N = len(n)
    from_far = (far - off) < (off - near)
    origin = [(hi[d] if (n[d] > 0.0) == from_far else lo[d]) for d in range(N)]
    alpha = (off - far) if from_far else (off - near)
    corners = {}
    for bits in itertools.product((0, 1), repeat=N):
        p = tuple((hi[d] if bits[d] else lo[d]) - origin[d] for d in range(N))
        corners[bits] = (p, sum(n[d] * p[d] for d in range(N)) - alpha)
    return origin, corners


def _cross(a, ga, b, gb):
    t = ga / (ga - gb)
    return tuple(a[d] + t * (b[d] - a[d]) for d in range(len(a)))


def _cut2(n, off, near, far, lo, hi):
    origin, corners = _local_frame(n, off, near, far, lo, hi)
    ring = [corners[b] for b in ((0, 0), (1, 0), (1, 1), (0, 1))]
    poly, chord = [], []
    for k in range(4):                                            # Sutherland-Hodgman, one clip line
        (a, ga), (b, gb) = ring[k], ring[(k + 1) % 4]
        if ga <= 0.0:
            poly.append(a)
            if ga == 0.0:
                chord.append(a)
        if (ga < 0.0 and gb > 0.0) or (ga > 0.0 and gb < 0.0):
            x = _cross(a, ga, b, gb)
            poly.append(x)
            chord.append(x)
    area = mx = my = 0.0
    for k in range(len(poly)):                                     # shoelace
        (x0, y0), (x1, y1) = poly[k], poly[(k + 1) % len(poly)]
        w = x0 * y1 - x1 * y0
        area += w
        mx += (x0 + x1) * w
        my += (y0 + y1) * w
    area *= 0.5
    cen = (origin[0] + mx / (6.0 * area), origin[1] + my / (6.0 * area)) if area > 0.0 else None
    gamma, cg = 0.0, None
    if len(chord) >= 2:
        p, q = chord[0], chord[-1]
        gamma = math.hypot(q[0] - p[0], q[1] - p[1])
        cg = (origin[0] + 0.5 * (p[0] + q[0]), origin[1] + 0.5 * (p[1] + q[1]))
    return area, cen, gamma, cg


_EDGES3 = [(a, b) for a in itertools.product((0, 1), repeat=3) for b in itertools.product((0, 1), repeat=3)
           if a < b and sum(abs(a[d] - b[d]) for d in range(3)) == 1]


def _cut3(n, off, near, far, lo, hi, want_surface=True):
    from scipy.spatial import ConvexHull, QhullError

    origin, corners = _local_frame(n, off, near, far, lo, hi)
    pts = [p for p, g in corners.values() if g <= 0.0]
    ring = [p for p, g in corners.values() if g == 0.0]
    for a, b in _EDGES3:
        (pa, ga), (pb, gb) = corners[a], corners[b]
        if (ga < 0.0 and gb > 0.0) or (ga > 0.0 and gb < 0.0):
            x = _cross(pa, ga, pb, gb)
            pts.append(x)
            ring.append(x)
    P = np.array(pts)
    scale = float(np.max(np.abs(P)))
    Q = P / scale
    try:
        hull = ConvexHull(Q)
    except QhullError:
        hull = ConvexHull(Q, qhull_options="QJ")
    c0 = Q[hull.vertices].mean(axis=0)
    vol = 0.0
    mom = np.zeros(3)
    for tri in hull.simplices:                                     # tetrahedra (c0, triangle)
        a, b, c = Q[tri[0]] - c0, Q[tri[1]] - c0, Q[tri[2]] - c0
        v = abs(float(np.dot(a, np.cross(b, c)))) / 6.0
        vol += v
        mom += v * (c0 + 0.25 * (a + b + c))
    cen = tuple(origin[d] + scale * mom[d] / vol for d in range(3)) if vol > 0.0 else None
    vol *= scale ** 3
    gamma, cg = 0.0, None
    if want_surface and len(ring) >= 3:
        R = np.array(ring)
        nn = np.array(n) / np.linalg.norm(n)
        u = np.cross(nn, np.eye(3)[int(np.argmin(np.abs(nn)))])
        u /= np.linalg.norm(u)
        w = np.cross(nn, u)
        r0 = R.mean(axis=0)
        s = float(np.max(np.abs(R - r0))) or 1.0
        uv = np.stack([(R - r0) @ u, (R - r0) @ w], axis=1) / s
        uv = uv[np.argsort(np.arctan2(uv[:, 1], uv[:, 0]))]
        area = mu = mv = 0.0
        for k in range(len(uv)):
            (x0, y0), (x1, y1) = uv[k], uv[(k + 1) % len(uv)]
            t = x0 * y1 - x1 * y0
            area += t
            mu += (x0 + x1) * t
            mv += (y0 + y1) * t
        area *= 0.5
        if area > 0.0:
            gamma = area * s * s
            pc = r0 + s * (mu / (6.0 * area)) * u + s * (mv / (6.0 * area)) * w
            cg = tuple(origin[d] + float(pc[d]) for d in range(3))
    return vol, cen, gamma, cg


class ObliqueHalfSpace:
    def __init__(self, normal: Sequence[float], offset: float, complement: bool = False):
        self.normal = tuple(float(v) for v in normal)
        self.offset = float(offset)
        self.complement = bool(complement)
        self.N = len(self.normal)
        s = -1.0 if self.complement else 1.0
        self._n = tuple(s * v for v in self.normal)               # what the measures use
        self._off = s * self.offset

    def __call__(self, *x):
        f = sum(self.normal[d] * x[d] for d in range(self.N)) - self.offset
        return -f if self.complement else f

    def box(self, lo, hi, want_surface: bool = True) -> BoxMeasure:
        N = self.N
        n, off = self._n, self._off
        ext = [hi[d] - lo[d] for d in range(N)]
        ctr = tuple(0.5 * (lo[d] + hi[d]) for d in range(N))
        zero = tuple(0.0 for _ in range(N))
        t, near, far = classify(n, off, lo, hi)
        if any(e <= 0.0 for e in ext):
            return BoxMeasure(t, 0.0, ctr, 0.0, zero)
        if t != CUT:
            return BoxMeasure(t, _prod(ext) if t == FULL else 0.0, ctr, 0.0, zero)
        if N == 1:
            x = off / n[0]
            x = min(max(x, lo[0]), hi[0])
            a, b = (lo[0], x) if n[0] > 0.0 else (x, hi[0])
            return BoxMeasure(CUT, b - a, (0.5 * (a + b),), 1.0, (x,))
        if N == 2:
            vol, cen, gamma, cg = _cut2(n, off, near, far, lo, hi)
        else:
            vol, cen, gamma, cg = _cut3(n, off, near, far, lo, hi, want_surface)
        return BoxMeasure(CUT, vol, cen if cen is not None else ctr, gamma, cg if cg is not None else zero)

    def section(self, d: int, s: float, lo, hi) -> float:
        N = self.N
        n, off = self._n, self._off
        plo, phi = list(lo), list(hi)
        plo[d] = s
        phi[d] = s
        t, _, _ = classify(n, off, plo, phi)                      # the N-D rule on the flattened box
        if N == 1:
            return 1.0 if t == FULL else 0.0                      # a point: fluid iff f <= 0
        others = [k for k in range(N) if k != d]
        full = _prod([hi[k] - lo[k] for k in others])
        if t != CUT:
            return full if t == FULL else 0.0
        sub = ObliqueHalfSpace([n[k] for k in others], off - n[d] * s)
        return sub.box([lo[k] for k in others], [hi[k] for k in others], want_surface=False).vol
