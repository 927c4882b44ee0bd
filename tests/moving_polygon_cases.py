"""Shared by tests/test_moving_polygon_host.py and tests/test_gpu_moving_polygon.py: the moving marker polygons of the suite, the
host (g++) build of the interpolating view (tests/spacetime_polygon_host.cpp), the arbiter's slab capacities (computed once per
case and process) and the bars.

Bars.  Units are those of tests/levelset_cases.py, 2^-52 (|x0| + L) / h, with the slab integrals divided by dt and the time
centroids by dt (tests/spacetime_program_reference.slab_ratios).  The bar of a quantity and case is 10 times the worst the HOST
build shows on the CPU against the arbiter (tests/spacetime_polygon_reference.py), plus (nq + 3) 2^-53 relative for the order of
the sum over the time nodes; the margin of 10 is there because the wave's butterfly and the kernels' strides are not the host's
order.  No floor.  The GPU is held to the same bars and never sets them."""
from __future__ import annotations

import ctypes as C
import functools
import math
import subprocess
from pathlib import Path

import numpy as np

from oracle import penguin_oracle as po
from penguin.jl_amd import front as ft
from tests import spacetime_polygon_reference as spr
from tests.levelset_cases import unit
from tests.spacetime_program_reference import Layer, slab_ratios

ROOT = Path(__file__).resolve().parent.parent
QUANTITIES = ("V", "A", "B", "W", "G", "Cw", "Cg", "Vn_1", "Vn")
T0, DT = 0.1, 0.05


def _poly(front):
    return front.polygon()


def rigid(base, shift, angle, about):
    """markers(t) of penguin.jl_amd.front.MovingFront.rigid"""
    return ft.MovingFront.rigid(base, shift=shift, angle=angle, about=about).markers_of_t


_HEPTAGON = _poly(ft.create_circle_b(ft.FrontTracker(), 1.71, 2.21, 1.0, 7))
_CRYSTAL = _poly(ft.create_crystal_b(ft.FrontTracker(), 2.01, 1.97, 1.0, 6, 0.3, 96))
_FINE = _poly(ft.create_circle_b(ft.FrontTracker(), 2.01, 2.01, 1.0, 2000))


def _heptagon(t):
    return rigid(_HEPTAGON, lambda t: (1.3 * (t - T0), -0.7 * (t - T0)), lambda t: 2.0 * (t - T0), (1.71, 2.21))(t)


def _crystal(t):
    c = np.array([2.01, 1.97])
    return c + (1.0 + 2.2 * (t - T0)) * (_CRYSTAL - c)


def _triangle(t):
    return rigid(np.array([(0.73, 1.12), (3.31, 1.27), (2.13, 3.43)]), lambda t: (-0.9 * (t - T0), 1.1 * (t - T0)),
                 lambda t: -1.5 * (t - T0), (2.0, 2.0))(t)


def _fine(t):
    return _FINE + np.array([1.7 * (t - T0), 0.9 * (t - T0)])


def _leaving(t):
    return rigid(_HEPTAGON, lambda t: (0.9 + 9.0 * (t - T0), 0.13 - 3.0 * (t - T0)), lambda t: 0.3, (1.71, 2.21))(t)


def _aligned(t):
    r = np.array([(1.125, 1.125), (2.625, 1.125), (2.625, 3.125), (1.125, 3.125)])
    return r + np.array([7.5 * (t - T0), 0.0])               # 1.5 cells along x during the slab, the edges stay on node lines


HEPT_MESH = ((12, 10), (4.0, 4.0), (-0.3, 0.2))
SQ16 = ((16, 16), (4.0, 4.0), (0.0, 0.0))
# name -> (markers(t), n, L, x0, complement, (time_panels, time_order))
CASES = {
    "heptagon_nq3": (_heptagon, *HEPT_MESH, False, (1, 3)),
    "heptagon_nq64": (_heptagon, *HEPT_MESH, False, (16, 4)),
    "heptagon_nq80": (_heptagon, *HEPT_MESH, False, (20, 4)),
    "crystal_16": (_crystal, *SQ16, False, (2, 4)),
    "triangle": (_triangle, *HEPT_MESH, False, (2, 2)),
    "fine_2000_8": (_fine, (8, 8), (4.0, 4.0), (0.0, 0.0), False, (2, 2)),
    "complement_heptagon": (_heptagon, *HEPT_MESH, True, (2, 4)),
    "leaving": (_leaving, *HEPT_MESH, False, (2, 2)),
    "aligned_rect_16": (_aligned, *SQ16, False, (2, 2)),
}
ALIGNED = ("aligned_rect_16",)
ARBITRATED = [c for c in CASES if c not in ALIGNED]


def nq_of(name):
    return CASES[name][5][0] * CASES[name][5][1]


def ends(name):
    f = CASES[name][0]
    return np.asarray(f(T0), dtype=float), np.asarray(f(T0 + DT), dtype=float)


def rule(name):
    return spr.time_rule(T0, T0 + DT, *CASES[name][5])


# ---- the host build ------------------------------------------------------------------------------------------------------------------

def build_host_lib():
    out = ROOT / "tests" / "_build" / "libspacetime_polygon_host.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "spacetime_polygon_host.cpp"
    deps = [src] + [ROOT / "penguin" / "jl_amd" / "csrc" / n for n in ("pg_geom_polygon.h", "pg_geom.h")]
    if not out.exists() or out.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out), str(src)], check=True)
    lib = C.CDLL(str(out))
    lib.stp_new.restype = C.c_void_p
    lib.stp_section.restype = C.c_double
    lib.stp_free.argtypes = [C.c_void_p]
    return lib


def host_slab(lib, name):
    _, n, L, x0, comp, _ = CASES[name]
    p0, p1 = ends(name)
    tau, wt = rule(name)
    return spr.HostSlab(lib, p0, p1, po.Mesh(n, L, x0), L, T0, T0 + DT, tau, wt, comp)


def host_capacity(lib, name, cheap_pass=True):
    return spr.host_slab_capacity(host_slab(lib, name), cheap_pass)


def arbiter(name):
    _, _, _, _, comp, _ = CASES[name]
    return spr.MovingPolygonArbiter(*ends(name), T0, T0 + DT, comp)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the arbiter's first layer of a case, with its own Gamma and C_gamma: computed once per process, never changed"""
    _, n, L, x0, _, pr = CASES[name]
    mesh = po.Mesh(n, L, x0)
    arb = arbiter(name)
    M = int(np.prod(mesh.ext))
    lay = Layer(spr.slab_reference(arb, mesh, *pr), 2, M)
    G, Cg = spr.arbiter_front(arb, mesh, *rule(name))
    lay.G, lay.C_g_st, lay.C_g = G, Cg, Cg[:, :2]
    return lay


def check_generic(name):
    """no marker on a node line or on a line through a C_omega, and no edge along either, at any node time or face: then no
    comparison depends on which side of a line a coincident point is counted, and nothing is left out"""
    _, n, L, x0, _, _ = CASES[name]
    mesh = po.Mesh(n, L, x0)
    arb, ref = arbiter(name), reference(name)
    tau, _ = rule(name)
    for d in range(2):
        lines = np.unique(np.concatenate([np.asarray(mesh.nodes[d], dtype=float), ref.C_w_st[:, d]]))
        for t in [T0, T0 + DT, *tau]:
            v = arb.vertices(float(t))
            assert not np.isin(v[:, d], lines).any(), (name, d, t)
            assert np.all(v[:, d] != np.roll(v[:, d], -1)), (name, "an axis-aligned edge", d, t)


# ---- bars -----------------------------------------------------------------------------------------------------------------------------
# MEASURED: the worst ratio of each quantity, in the units above, of the HOST build (g++ -O2 -ffp-contract=off, the kernels' slab
# rule with the wave's order of summation) against the arbiter, on this project's CPU runs (tests/test_moving_polygon_host.py
# prints them again).  The bar is 10 times the figure plus the order term, with no floor.
MEASURED = {
    "heptagon_nq3": {"V": 0.727, "A": 0.465, "B": 2.91, "W": 1.16, "G": 0.407, "Cw": 0.93, "Cg": 0.93, "Vn_1": 0.727, "Vn": 0.727},
    "heptagon_nq64": {"V": 0.727, "A": 0.465, "B": 2.66, "W": 1.44, "G": 0.116, "Cw": 2.33, "Cg": 0.465, "Vn_1": 0.727, "Vn": 0.727},
    "heptagon_nq80": {"V": 0.727, "A": 0.581, "B": 5.49, "W": 1.38, "G": 0.116, "Cw": 2.33, "Cg": 0.93, "Vn_1": 0.727, "Vn": 0.727},
    "crystal_16": {"V": 0.0312, "A": 0.125, "B": 1.23, "W": 1.44, "G": 0.125, "Cw": 1.0, "Cg": 1.0, "Vn_1": 0.516, "Vn": 0.0625},
    "triangle": {"V": 0.727, "A": 0.465, "B": 15.0, "W": 0.745, "G": 0.698, "Cw": 3.26, "Cg": 0.465, "Vn_1": 0.727, "Vn": 0.727},
    "fine_2000_8": {"V": 0.156, "A": 0.125, "B": 0.625, "W": 1.06, "G": 0.75, "Cw": 1.0, "Cg": 0.5, "Vn_1": 0.281, "Vn": 0.25},
    "complement_heptagon": {"V": 0.799, "A": 0.581, "B": 1.08, "W": 0.963, "G": 0.174, "Cw": 0.93, "Cg": 0.465, "Vn_1": 0.799, "Vn": 0.799},
    "leaving": {"V": 0.509, "A": 0.349, "B": 2.1, "W": 0.945, "G": 0.93, "Cw": 6.05, "Cg": 0.93, "Vn_1": 0.727, "Vn": 0.436},
    "aligned_rect_16": {"V": 0.0, "A": 0.0, "B": 0.0, "W": 0.531, "G": 0.25, "Cw": 0.5, "Cg": 0.5, "Vn_1": 0.0, "Vn": 0.0},
}
# The largest figure is B = 15 of the triangle, consistent with its C_omega figure (3.26) times the slope of its long edges: B is
# the section through C_omega, and along a shallow edge a centroid off by an ulp moves the crossing by several.  Every figure is below 10 times the largest static one (4.7, tests/polygon_cases.py), as a
# positive-weight time average of the static errors must be.


def bars(name):
    _, n, L, x0, _, _ = CASES[name]
    u, _ = unit(x0, L, n)
    order = (nq_of(name) + 3) * 2.0 ** -53 / u
    return {q: 10.0 * MEASURED[name][q] + order for q in QUANTITIES}


def case_ratios(name, got, ref=None):
    _, n, L, x0, _, _ = CASES[name]
    return slab_ratios(got, ref or reference(name), x0, L, n, DT)


def check(name, got, what=""):
    """print every figure, then hold each to its bar; the aligned case: V, Gamma, Vn_1 and Vn only"""
    r, b = case_ratios(name, got), bars(name)
    held = ("V", "G", "Vn_1", "Vn") if name in ALIGNED else QUANTITIES
    print(f"[moving-polygon {what}{name}] " + "  ".join(f"{q} {r[q]:.3g}/{b[q]:.3g}" for q in held))
    bad = {q: (r[q], b[q]) for q in held if not r[q] <= b[q]}
    assert not bad, f"{name}: over the bar (measured, bar) in units of 2^-52 (|x0| + L) / h: {bad}"
    return r


# ---- analytic sums ---------------------------------------------------------------------------------------------------------------------

def shoelace(p):
    p = np.asarray(p, dtype=np.longdouble).reshape(-1, 2)
    q = np.roll(p, -1, axis=0)
    return abs(np.sum((p[:, 0] - p[0, 0]) * (q[:, 1] - p[0, 1]) - (q[:, 0] - p[0, 0]) * (p[:, 1] - p[0, 1]))) / 2


def sum_tol(terms, ncut, *extra):
    """(cut cells + 3) 2^-52 of the summed absolute terms: one rounding per cut cell's value and per partial sum of the longdouble
    total, and 3 for the closed form.  Derived, not measured."""
    return (ncut + 3) * np.longdouble(2.0) ** -52 * (np.sum(np.abs(np.asarray(terms, dtype=np.longdouble))) + sum(abs(e) for e in extra))


def lsum(a):
    return np.sum(np.asarray(a, dtype=np.longdouble))


# ---- the motions of the solves: 1 + 4 slabs of DT from t = 0 ---------------------------------------------------------------------------
# (found by a search over velocities, turning rates and offsets with the host build: a turning polygon clips cell corners often, and
# most motions leave a sliver in one of the five slabs)
def solve_heptagon(t):
    return rigid(_HEPTAGON, lambda t: (-0.67 * t, -0.02 + 0.15 * t), lambda t: 1.61 * t, (1.71, 2.21))(t)


_K = np.arange(10)
_STAR = np.column_stack([2.01 + np.where(_K % 2 == 0, 1.0, 0.55) * np.cos(2 * np.pi * _K / 10),
                         1.97 + np.where(_K % 2 == 0, 1.0, 0.55) * np.sin(2 * np.pi * _K / 10)])


def solve_star(t):
    """a five-pointed star (non-convex, 10 markers), turning"""
    return rigid(_STAR, lambda t: (0.07 + 0.7 * t, -0.03 + 0.73 * t), lambda t: 2.44 * t, (2.01, 1.97))(t)


# name -> (markers(t), n, L, x0)
SOLVES = {"mono_12x10": (solve_heptagon, *HEPT_MESH), "diph_16": (solve_star, *SQ16), "advdiff_16": (solve_star, *SQ16)}
SOLVE_SLABS = [(k * DT, (k + 1) * DT) for k in range(5)]
SLIVER = 1e-4                                                # no space-time cut cell of a solve is below this part of a full one


def smallest_cut_fraction(cap, n, L):
    """the smallest V of a CUT cell as a part of a full cell's h0 h1 dt (cap: anything with V and cell_types of one slab)"""
    ct, V = np.asarray(cap.cell_types), np.asarray(cap.V)
    return float(np.min(V[ct == -1.0]) / (L[0] / n[0] * L[1] / n[1] * DT))
