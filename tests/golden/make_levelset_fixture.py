"""Writes tests/golden/levelset_cells.json: cut-cell capacities of three level-set bodies at 30 digits (mpmath), the arbiter of
the traced-level-set bodies (penguin/jl_amd/csrc/pg_geom_program.h, tests/test_levelset_host.py, tests/test_gpu_levelset.py).

    python tests/golden/make_levelset_fixture.py          (a few minutes)

The route shares nothing with the device's.  The device picks the height direction per cell from the gradient, finds roots by
regula falsi on 9 samples and integrates with Gauss-Legendre in double precision.  Here every body is a union of conics
a x^2 + b xy + c y^2 + d x + e y + f <= 0 whose coefficients are expanded at 30 digits from the very doubles the traced closure
holds; the fluid part of a vertical line is the union of the conics' chords, from the quadratic formula; a box is ALWAYS
integrated along x with mpmath.quad (tanh-sinh, which takes the square-root endpoint singularities of chords and arc length in
its stride) between breakpoints that are the box ends, the crossings of the conics with the two horizontal edges, the abscissae
of vertical tangency and the abscissae where two conics meet (the kink of a union) -- all roots of quadratics, taken in closed
form at 30 digits rather than iterated.  The interface measure is the arc length int |grad phi| / |phi_y| dx over the branches
inside the box that no other conic covers.  Only the classification is restated from the device: the lattice of 9 samples per
edge and the centre, evaluated at 30 digits.  B_d and W_d are taken at the fixture's own centroids, rounded to double.

The capacities are assembled by oracle.penguin_oracle.make_capacity from `box` and `section` below."""
from __future__ import annotations

import json
import sys
from pathlib import Path

import mpmath as mp
import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

from oracle import penguin_oracle as po  # noqa: E402
from oracle.geometry import CUT, EMPTY, FULL, BoxMeasure  # noqa: E402

mp.mp.dps = 30
M = mp.mpf


class Conic:
    def __init__(self, a, b, c, d, e, f):
        self.a, self.b, self.c, self.d, self.e, self.f = a, b, c, d, e, f

    @classmethod
    def ellipse(cls, cx, cy, ax, ay, cos_t, sin_t):
        """((C (x - cx) + S (y - cy)) / ax)^2 + ((C (y - cy) - S (x - cx)) / ay)^2 - 1 with the doubles C, S as given"""
        cx, cy, ax, ay, C, S = (M(v) for v in (cx, cy, ax, ay, cos_t, sin_t))
        p, q = 1 / ax ** 2, 1 / ay ** 2
        a, b, c = p * C * C + q * S * S, 2 * C * S * (p - q), p * S * S + q * C * C
        return cls(a, b, c, -2 * a * cx - b * cy, -2 * c * cy - b * cx, a * cx * cx + b * cx * cy + c * cy * cy - 1)

    @classmethod
    def disc(cls, cx, cy, r):
        cx, cy, r = M(cx), M(cy), M(r)
        return cls(M(1), M(0), M(1), -2 * cx, -2 * cy, cx * cx + cy * cy - r * r)

    def phi(self, x, y):
        return self.a * x * x + self.b * x * y + self.c * y * y + self.d * x + self.e * y + self.f

    def grad(self, x, y):
        return 2 * self.a * x + self.b * y + self.d, self.b * x + 2 * self.c * y + self.e

    @staticmethod
    def _roots(A, B, Cc):
        disc = B * B - 4 * A * Cc
        if disc < 0:
            return None
        s = mp.sqrt(disc)
        return (-B - s) / (2 * A), (-B + s) / (2 * A)

    def chord_y(self, x):
        return self._roots(self.c, self.b * x + self.e, self.a * x * x + self.d * x + self.f)

    def chord_x(self, y):
        return self._roots(self.a, self.b * y + self.d, self.c * y * y + self.e * y + self.f)

    def x_tangency(self):
        """abscissae where the chord in y closes: the discriminant of chord_y as a quadratic in x"""
        r = self._roots(self.b ** 2 - 4 * self.a * self.c, 2 * self.b * self.e - 4 * self.c * self.d, self.e ** 2 - 4 * self.c * self.f)
        return sorted(r) if r else []


def meet(p: Conic, q: Conic):
    """abscissae where the boundaries of two conics cross: sign changes of q at the chord ends of p, bracketed on a fine grid
    and refined at 30 digits"""
    out = []
    lo, hi = p.x_tangency()
    for branch in (0, 1):
        def g(x):
            ch = p.chord_y(x)
            return q.phi(x, ch[branch]) if ch else M(1)
        n = 256
        xs = [lo + (hi - lo) * (M(k) + M(1) / 2) / n for k in range(n)]
        vs = [g(x) for x in xs]
        for k in range(n - 1):
            if vs[k] * vs[k + 1] < 0:
                out.append(mp.findroot(g, (xs[k], xs[k + 1]), solver="illinois", tol=M(10) ** -50, maxsteps=200))
    return out


def union(ivs):
    ivs = sorted(iv for iv in ivs if iv is not None and iv[1] > iv[0])
    out = []
    for lo, hi in ivs:
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


class MpBody:
    """fluid = union of the conics (complement: the rest of the plane, boundary included on both sides as phi <= 0 / -phi <= 0)"""

    def __init__(self, prims, complement=False):
        self.prims, self.complement = prims, complement
        self.kinks = [x for i, p in enumerate(prims) for q in prims[i + 1:] for x in meet(p, q)]

    def phi(self, x, y):
        v = min(p.phi(x, y) for p in self.prims)
        return -v if self.complement else v

    def __call__(self, x, y):
        return float(self.phi(M(float(x)), M(float(y))))

    # ---- the device's lattice rule, at 30 digits
    def box_type(self, lo, hi):
        x0, y0, x1, y1 = M(lo[0]), M(lo[1]), M(hi[0]), M(hi[1])
        xs = [x0 + (x1 - x0) * (M(k) / 8) for k in range(8)] + [x1]
        ys = [y0 + (y1 - y0) * (M(k) / 8) for k in range(8)] + [y1]
        pts = [(x, y0) for x in xs] + [(x, y1) for x in xs] + [(x0, y) for y in ys[1:8]] + [(x1, y) for y in ys[1:8]]
        pts.append(((x0 + x1) / 2, (y0 + y1) / 2))
        vals = [self.phi(x, y) for x, y in pts]
        if all(v <= 0 for v in vals):
            return FULL
        if all(v >= 0 for v in vals):               # (FULL first: touching from outside is EMPTY, as the closed-form kinds)
            return EMPTY
        return CUT

    def _chords(self, x, y0, y1):
        return union([(max(ch[0], y0), min(ch[1], y1)) for ch in (p.chord_y(x) for p in self.prims) if ch])

    def box(self, lo, hi, want_surface=True) -> BoxMeasure:
        t = self.box_type(lo, hi)
        x0, y0, x1, y1 = M(lo[0]), M(lo[1]), M(hi[0]), M(hi[1])
        centre = (float((x0 + x1) / 2), float((y0 + y1) / 2))
        area = (x1 - x0) * (y1 - y0)
        if t != CUT or not (x1 > x0 and y1 > y0):
            return BoxMeasure(t, float(area) if t == FULL and area > 0 else 0.0, centre, 0.0, (0.0, 0.0))
        bps = {x0, x1}
        for p in self.prims:
            cand = list(p.x_tangency())
            for ye in (y0, y1):
                cand += list(p.chord_x(ye) or ())
            bps.update(v for v in cand if x0 < v < x1)
        bps.update(v for v in self.kinks if x0 < v < x1)
        bps = sorted(bps)
        V = mx = my = G = gx = gy = M(0)
        for a, b in zip(bps[:-1], bps[1:]):
            if not b > a:
                continue
            cache = {}

            def chords(x):
                if x not in cache:
                    cache[x] = self._chords(x, y0, y1)
                return cache[x]
            V += mp.quad(lambda x: sum(h - l for l, h in chords(x)), [a, b])
            mx += mp.quad(lambda x: x * sum(h - l for l, h in chords(x)), [a, b])
            my += mp.quad(lambda x: sum(h * h - l * l for l, h in chords(x)) / 2, [a, b])
            if not want_surface:
                continue
            xm = (a + b) / 2
            for p in self.prims:
                ch = p.chord_y(xm)
                if not ch:
                    continue
                for branch in (0, 1):
                    ym = ch[branch]
                    if not (y0 < ym < y1) or any(q.phi(xm, ym) <= 0 for q in self.prims if q is not p):
                        continue

                    def w(x, p=p, branch=branch):
                        ch = p.chord_y(x)
                        if not ch or ch[1] == ch[0]:   # (a node an ulp of 30 digits from a tangency: its weight is below 1e-30)
                            return M(0), M(0)
                        y = ch[branch]
                        g0, g1 = p.grad(x, y)
                        return mp.sqrt(g0 * g0 + g1 * g1) / abs(g1), y
                    G += mp.quad(lambda x: w(x)[0], [a, b])
                    gx += mp.quad(lambda x: x * w(x)[0], [a, b])
                    gy += mp.quad(lambda x: w(x)[0] * w(x)[1], [a, b])
        if self.complement:
            mx, my = area * (x0 + x1) / 2 - mx, area * (y0 + y1) / 2 - my
            V = area - V
        cen = (float(mx / V), float(my / V)) if V > 0 else centre
        cg = (float(gx / G), float(gy / G)) if G > 0 else (0.0, 0.0)
        return BoxMeasure(CUT, float(V), cen, float(G), cg)

    def section(self, d, s, lo, hi) -> float:
        s = M(s)
        o = 1 - d
        a, b = M(lo[o]), M(hi[o])
        ivs = union([(max(ch[0], a), min(ch[1], b)) for ch in ((p.chord_y(s) if d == 0 else p.chord_x(s)) for p in self.prims) if ch])
        m = sum(h - l for l, h in ivs)
        return float((b - a) - m if self.complement else m)


def cases():
    c, s = float(np.cos(0.5)), float(np.sin(0.5))           # the doubles tests/levelset_cases.rotated_ellipse holds
    ell = Conic.ellipse(2.01, 1.97, 1.3, 0.6, c, s)
    discs = [Conic.disc(1.6, 2.01, 0.8), Conic.disc(2.5, 2.2, 0.7)]
    return {
        "ellipse_16": (MpBody([ell]), (16, 16), (4.0, 4.0), (0.0, 0.0)),
        "ellipse_17x13": (MpBody([ell]), (17, 13), (4.0, 3.0), (-0.3, 0.2)),
        "discs_24": (MpBody(discs), (24, 24), (4.0, 4.0), (0.0, 0.0)),
        "ellipse_complement_16": (MpBody([ell], complement=True), (16, 16), (4.0, 4.0), (0.0, 0.0)),
    }


def main(only=None):
    out = {"digits": mp.mp.dps, "cases": {}}
    path = ROOT / "tests" / "golden" / "levelset_cells.json"
    if only and path.exists():
        out = json.loads(path.read_text())
    for name, (body, n, L, x0) in cases().items():
        if only and name not in only:
            continue
        cap = po.make_capacity(body, po.Mesh(n, L, x0))
        out["cases"][name] = {
            "n": list(n), "L": list(L), "x0": list(x0),
            "V": cap.V.tolist(), "G": cap.G.tolist(), "cell_types": cap.cell_types.tolist(),
            "A": [a.tolist() for a in cap.A], "B": [a.tolist() for a in cap.B], "W": [a.tolist() for a in cap.W],
            "C_w": cap.C_w.ravel().tolist(), "C_g": cap.C_g.ravel().tolist(),
        }
        print(name, "cut cells:", int((cap.cell_types == CUT).sum()), flush=True)
    path.write_text(json.dumps(out, separators=(",", ":")) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
