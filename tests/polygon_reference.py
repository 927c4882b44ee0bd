"""CPU arbiter for marker-polygon bodies (penguin/jl_amd/csrc/pg_geom_polygon.h): a duck-typed body for
oracle.penguin_oracle.make_capacity (`box`, `section`, the protocol of tests/plane_oracle.py) in EXACT rational arithmetic
(fractions.Fraction of the float inputs), by methods that share nothing with the product's Green sums:

  box area, moments   Sutherland-Hodgman clipping of the whole polygon against the box, then the shoelace sums about the box's
                      lower corner; the exterior phase is the box minus the interior
  sections            exact crossings, sorted
  front               exact Liang-Barsky pieces; the one square root per piece in mpmath at 30 digits

and the product's rules, restated:

  crossing   edge (p, q) crosses the line x_d = s iff (p_d <= s) != (q_d <= s), at p_o + (s - p_d)(q_o - p_o) / (q_d - p_d)
  inside     even-odd: an odd number of crossings of the line x_1 = y at or left of x
  section    parity at lo_o from the crossings <= lo_o, then the crossings strictly inside (lo_o, hi_o); none: the full extent or 0
  box type   CUT iff a piece (an edge clipped to the closed box) of positive length has its midpoint strictly inside the open box;
             otherwise FULL or EMPTY by the centre: touching is not cutting
  front      the pieces whose midpoint m has lo <= m < hi belong to the box, whatever its type
  orientation is normalised to counter-clockwise; a closing duplicate of the first marker is dropped
"""
from __future__ import annotations

from fractions import Fraction as Fr

import mpmath as mp
import numpy as np

from oracle.geometry import CUT, EMPTY, FULL, BoxMeasure

mp.mp.dps = 30


def _mpf(fr: Fr):
    return mp.mpf(fr.numerator) / mp.mpf(fr.denominator)


class PolygonBody:
    def __init__(self, markers, complement: bool = False):
        pts = [(float(x), float(y)) for x, y in markers]
        if len(pts) >= 2 and pts[0] == pts[-1]:
            pts = pts[:-1]
        assert len(pts) >= 3
        ex = [(Fr(x), Fr(y)) for x, y in pts]
        area2 = sum(ex[k][0] * ex[(k + 1) % len(ex)][1] - ex[(k + 1) % len(ex)][0] * ex[k][1] for k in range(len(ex)))
        assert area2 != 0
        if area2 < 0:
            pts = [pts[0]] + pts[:0:-1]
            ex = [ex[0]] + ex[:0:-1]
            area2 = -area2
        self.N = 2
        self.complement = bool(complement)
        self.pts = pts
        self.P = np.array(pts)                       # floats, for exact comparisons that select candidates
        self.Q = np.roll(self.P, -1, axis=0)
        self.ex = ex
        self.area = area2 / 2                         # exact
        self.M = len(pts)

    def perimeter(self):
        return float(sum(mp.sqrt(_mpf((q[0] - p[0]) ** 2 + (q[1] - p[1]) ** 2)) for p, q in self._edges(range(self.M))))

    def _edges(self, ks):
        for k in ks:
            yield self.ex[k], self.ex[(k + 1) % self.M]

    # ---- crossings ------------------------------------------------------------------------------------------------------------
    def _crossings(self, d, s):
        """exact coordinates on the other axis of the edges that cross x_d = s"""
        o = 1 - d
        ks = np.flatnonzero((self.P[:, d] <= s) != (self.Q[:, d] <= s))
        S = Fr(s)
        return [p[o] + (S - p[d]) * (q[o] - p[o]) / (q[d] - p[d]) for p, q in self._edges(ks)]

    def inside(self, x, y):
        X = Fr(x)
        return sum(1 for c in self._crossings(1, y) if c <= X) % 2 == 1

    def __call__(self, x, y, *_):
        return (1.0 if self.inside(x, y) else -1.0) * (1.0 if self.complement else -1.0)

    def _section_exact(self, d, s, a, z):
        """fluid length of {x_d = s} and [a, z] (Fractions), and whether a crossing lies strictly inside"""
        cs = self._crossings(d, s)
        fluid = (sum(1 for c in cs if c <= a) % 2 == 1) != self.complement
        mid = sorted(c for c in cs if a < c < z)
        length, last = Fr(0), a
        for c in mid:
            if fluid:
                length += c - last
            fluid = not fluid
            last = c
        if fluid:
            length += z - last
        return length, bool(mid)

    def section(self, d, s, lo, hi) -> float:
        o = 1 - d
        if not hi[o] - lo[o] > 0.0:
            return 0.0
        length, cut = self._section_exact(d, float(s), Fr(lo[o]), Fr(hi[o]))
        if not cut:
            return (hi[o] - lo[o]) if length > 0 else 0.0
        return float(length)

    # ---- boxes ----------------------------------------------------------------------------------------------------------------
    def _pieces(self, lo, hi):
        """exact Liang-Barsky: the pieces of positive length of the edges inside the closed box"""
        P, Q = self.P, self.Q
        near = np.flatnonzero((np.maximum(P[:, 0], Q[:, 0]) >= lo[0]) & (np.minimum(P[:, 0], Q[:, 0]) <= hi[0]) &
                              (np.maximum(P[:, 1], Q[:, 1]) >= lo[1]) & (np.minimum(P[:, 1], Q[:, 1]) <= hi[1]))
        L, H = (Fr(lo[0]), Fr(lo[1])), (Fr(hi[0]), Fr(hi[1]))
        out = []
        for p, q in self._edges(near):
            t0, t1 = Fr(0), Fr(1)
            ok = True
            for ax in (0, 1):
                dlt = q[ax] - p[ax]
                for pp, qq in ((-dlt, p[ax] - L[ax]), (dlt, H[ax] - p[ax])):
                    if pp == 0:
                        ok = ok and qq >= 0
                    elif pp < 0:
                        t0 = max(t0, qq / pp)
                    else:
                        t1 = min(t1, qq / pp)
            if ok and t1 > t0:
                a = (p[0] + t0 * (q[0] - p[0]), p[1] + t0 * (q[1] - p[1]))
                b = (p[0] + t1 * (q[0] - p[0]), p[1] + t1 * (q[1] - p[1]))
                out.append((a, b))
        return out, L, H

    def _clipped_polygon(self, L, H):
        poly = self.ex
        for ax, bound, ge in ((0, L[0], True), (0, H[0], False), (1, L[1], True), (1, H[1], False)):
            out = []
            n = len(poly)
            for k in range(n):
                a, b = poly[k], poly[(k + 1) % n]
                ina = a[ax] >= bound if ge else a[ax] <= bound
                inb = b[ax] >= bound if ge else b[ax] <= bound
                if ina:
                    out.append(a)
                if ina != inb:
                    t = (bound - a[ax]) / (b[ax] - a[ax])
                    pt = [a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1])]
                    pt[ax] = bound
                    out.append(tuple(pt))
            poly = out
            if not poly:
                break
        return poly

    def box(self, lo, hi, want_surface: bool = True) -> BoxMeasure:
        lo, hi = [float(v) for v in lo], [float(v) for v in hi]
        ctr = (0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]))
        zero = (0.0, 0.0)
        degenerate = not (hi[0] - lo[0] > 0.0 and hi[1] - lo[1] > 0.0)
        pieces, L, H = ([], None, None) if degenerate else self._pieces(lo, hi)
        cut = False
        gamma, gm = mp.mpf(0), [mp.mpf(0), mp.mpf(0)]
        for a, b in pieces:
            m = ((a[0] + b[0]) / 2, (a[1] + b[1]) / 2)
            if L[0] < m[0] < H[0] and L[1] < m[1] < H[1]:
                cut = True
            if want_surface and L[0] <= m[0] < H[0] and L[1] <= m[1] < H[1]:
                ln = mp.sqrt(_mpf((b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2))
                gamma += ln
                gm[0] += ln * _mpf(m[0])
                gm[1] += ln * _mpf(m[1])
        if cut:
            t = CUT
        else:
            t = FULL if self.inside(Fr(lo[0]) / 2 + Fr(hi[0]) / 2, ctr[1]) != self.complement else EMPTY
        G = float(gamma)
        cg = (float(gm[0] / gamma), float(gm[1] / gamma)) if gamma > 0 else zero
        if degenerate:
            return BoxMeasure(t, 0.0, ctr, 0.0, zero)
        if t != CUT:
            return BoxMeasure(t, (hi[0] - lo[0]) * (hi[1] - lo[1]) if t == FULL else 0.0, ctr, G, cg)
        poly = self._clipped_polygon(L, H)
        area = m0 = m1 = Fr(0)
        for k in range(len(poly)):                                   # shoelace about the lower corner
            x0, y0 = poly[k][0] - L[0], poly[k][1] - L[1]
            x1, y1 = poly[(k + 1) % len(poly)][0] - L[0], poly[(k + 1) % len(poly)][1] - L[1]
            w = x0 * y1 - x1 * y0
            area += w
            m0 += (x0 + x1) * w
            m1 += (y0 + y1) * w
        area, m0, m1 = area / 2, m0 / 6, m1 / 6
        if self.complement:
            ex0, ex1 = H[0] - L[0], H[1] - L[1]
            area, m0, m1 = ex0 * ex1 - area, ex0 * ex0 * ex1 / 2 - m0, ex0 * ex1 * ex1 / 2 - m1
        cen = (float(L[0] + m0 / area), float(L[1] + m1 / area)) if area > 0 else ctr
        return BoxMeasure(CUT, float(area), cen, G, cg)
