"""Shared by tests/test_polygon_host.py and tests/test_gpu_polygon.py: the marker polygons of the suite, the host (g++) build of
penguin/jl_amd/csrc/pg_geom_polygon.h wrapped as a duck-typed body for oracle.penguin_oracle.make_capacity (`box`, `section`),
the arbiter's capacities (computed once per case and process) and the bars.

Bars.  Every difference is normalised as in tests/levelset_cases.py (dV / h^2, dA dB dGamma / h, dW / h^2, dC / h with h the
smallest spacing; centroids only where the fluid fraction exceeds 1e-3) and expressed in units of 2^-52 (|x0| + L) / h.  The bar
of a quantity and case is 10 times the worst the HOST build shows on the CPU against the exact arbiter
(tests/polygon_reference.py), with no floor: where the host build agrees exactly the bar is 0.  The GPU is held to the same bars
and never sets them."""
from __future__ import annotations

import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

from oracle import penguin_oracle as po
from oracle.geometry import BoxMeasure
from penguin.jl_amd import front as ft
from tests.levelset_cases import QUANTITIES, ratios
from tests.polygon_reference import PolygonBody

ROOT = Path(__file__).resolve().parent.parent
P = C.POINTER(C.c_double)


def circle(cx, cy, r, n):
    return ft.create_circle_b(ft.FrontTracker(), cx, cy, r, n)


def _heptagon():
    return circle(2.01, 2.01, 1.0, 7)


def _crystal():
    return ft.create_crystal_b(ft.FrontTracker(), 2.01, 1.97, 1.0, 6, 0.3, 96)


def _rect():
    return ft.FrontTracker([(0.9, 1.3), (3.1, 1.3), (3.1, 2.7), (0.9, 2.7)])


def _square(a=1.0, b=3.0):
    return ft.FrontTracker([(a, a), (b, a), (b, b), (a, b)])


SQ = ((4.0, 4.0), (0.0, 0.0))
# name -> (front factory, n, L, x0, complement)
CASES = {
    "circle_16": (lambda: circle(2.01, 2.01, 1.0, 40), (16, 16), *SQ, False),
    "heptagon_24": (_heptagon, (24, 24), *SQ, False),
    "crystal_24": (_crystal, (24, 24), *SQ, False),
    "fine_circle_8": (lambda: circle(2.01, 2.01, 1.0, 2000), (8, 8), *SQ, False),
    "rect_16": (_rect, (16, 16), *SQ, False),
    "shifted_17x13": (lambda: circle(2.01, 2.01, 1.0, 40), (17, 13), (4.0, 4.0), (-0.3, 0.2), False),
    "complement_16": (lambda: circle(2.01, 2.01, 1.0, 40), (16, 16), *SQ, True),
    "aligned_square_16": (_square, (16, 16), *SQ, False),
    "node_square_16": (lambda: _square(1.125, 3.125), (16, 16), *SQ, False),
}
# The two squares: markers on nodes, edges on node lines.  Mesh() puts the nodes at x0 + (j + 1/2) h, so on 16^2 over [0, 4]^2 it
# is the square [1.125, 3.125]^2 (node_square_16) whose edges lie on node lines; [1, 3]^2 (aligned_square_16) lies on the lines
# through the cell centres.  Both are held to the same short list: cell types, V, sum Gamma = the perimeter, every array finite.
# A and B on faces that coincide with a polygon edge are defined by the crossing rule (the face x = s belongs to the side
# p_x <= s) and documented, not arbitrated.
SQUARES = ("aligned_square_16", "node_square_16")
ARBITRATED = [c for c in CASES if c not in SQUARES]


# ---- the host build as an oracle body ------------------------------------------------------------------------------------------------

def build_host_lib():
    out = ROOT / "tests" / "_build" / "libpolygon_host.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "polygon_host.cpp"
    deps = [src] + [ROOT / "penguin" / "jl_amd" / "csrc" / n for n in ("pg_geom_polygon.h", "pg_geom.h")]
    if not out.exists() or out.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out), str(src)], check=True)
    lib = C.CDLL(str(out))
    lib.poly_new.restype = C.c_void_p
    lib.poly_section_c.restype = C.c_double
    lib.poly_free.argtypes = [C.c_void_p]
    return lib


def _arr(v):
    return np.ascontiguousarray(v, dtype=float)


def host_new(lib, markers, n, nodes, complement=False):
    """(handle or None, message)"""
    xy = _arr(np.asarray(markers, dtype=float).reshape(-1))
    msg = C.create_string_buffer(512)
    h = lib.poly_new(xy.ctypes.data_as(P) if len(xy) else None, C.c_int64(len(xy) // 2), int(bool(complement)), int(n[0]), int(n[1]),
                     _arr(nodes[0]).ctypes.data_as(P), _arr(nodes[1]).ctypes.data_as(P), msg, 512)
    return h, msg.value.decode()


class HostPolygon:
    """a FrontTracker's markers measured by the host build on one mesh: `box` and `section` as oracle.geometry's bodies have them,
    with the one rule the capacity kernels add to the primitives: the measure of a FULL mesh cell, and what a wholly fluid
    section returns, come from the mesh spacing L_d / n_d and not from differences of node coordinates (pg_capacity.hip,
    full_measure) -- the arbiter takes node differences, so that rule's rounding is part of what the bars are measured from"""

    def __init__(self, lib, front, mesh: po.Mesh, L, complement=False, lanes=16):
        self.lib, self.N, self.lanes = lib, 2, lanes
        self.h, why = host_new(lib, front.markers, mesh.dims, mesh.nodes, complement)
        assert self.h, why
        self.h = C.c_void_p(self.h)
        self.spacing = tuple(float(L[d]) / mesh.dims[d] for d in range(2))
        self.cell_of = [{float(x): i for i, x in enumerate(mesh.nodes[d])} for d in range(2)]
        self.nodes = [np.asarray(mesh.nodes[d], dtype=float) for d in range(2)]

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.poly_free(self.h)

    def _is_mesh_cell(self, lo, hi):
        for d in range(2):
            i = self.cell_of[d].get(float(lo[d]))
            if i is None or i + 1 >= len(self.nodes[d]) or self.nodes[d][i + 1] != hi[d]:
                return False
        return True

    def box(self, lo, hi, want_surface=True) -> BoxMeasure:
        out = np.zeros(9)
        lo, hi = _arr(list(lo) + [0.0]), _arr(list(hi) + [0.0])
        self.lib.poly_box(self.h, lo.ctypes.data_as(P), hi.ctypes.data_as(P), int(want_surface), self.lanes, out.ctypes.data_as(P))
        vol = float(out[1])
        if int(out[0]) == 1 and self._is_mesh_cell(lo, hi):
            vol = self.spacing[0] * self.spacing[1]
        return BoxMeasure(int(out[0]), vol, tuple(out[2:4]), float(out[5]), tuple(out[6:8]))

    def section(self, d, s, lo, hi) -> float:
        lo, hi = _arr(list(lo) + [0.0]), _arr(list(hi) + [0.0])
        return self.lib.poly_section_c(self.h, d, C.c_double(s), lo.ctypes.data_as(P), hi.ctypes.data_as(P),
                                       C.c_double(self.spacing[1 - d]))


def host_capacity(lib, name):
    make, n, L, x0, comp = CASES[name]
    mesh = po.Mesh(n, L, x0)
    return po.make_capacity(HostPolygon(lib, make(), mesh, L, comp), mesh)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the arbiter's capacities of a case: computed once per process, never changed"""
    make, n, L, x0, comp = CASES[name]
    return po.make_capacity(PolygonBody(make().markers, comp), po.Mesh(n, L, x0))


# ---- sum identities -------------------------------------------------------------------------------------------------------------------

def shoelace_and_perimeter(markers):
    p = np.asarray(markers, dtype=np.longdouble).reshape(-1, 2)
    if len(p) >= 2 and p[0, 0] == p[-1, 0] and p[0, 1] == p[-1, 1]:
        p = p[:-1]
    q = np.roll(p, -1, axis=0)
    area = abs(np.sum((p[:, 0] - p[0, 0]) * (q[:, 1] - p[0, 1]) - (q[:, 0] - p[0, 0]) * (p[:, 1] - p[0, 1]))) / 2
    return area, np.sum(np.sqrt((q[:, 0] - p[:, 0]) ** 2 + (q[:, 1] - p[:, 1]) ** 2))


def check_identities(name, cap, what=""):
    """sum V = the shoelace area (the box minus it for the exterior) and sum Gamma = the perimeter, each within
    (cut cells + 3) 2^-52 (sum of absolute terms): one rounding per cut cell's value and per partial sum of the longdouble total,
    and 3 for the shoelace sum, the perimeter and the box.  Derived, not measured."""
    make, n, L, x0, comp = CASES[name]
    area, perimeter = shoelace_and_perimeter(make().markers)
    V = np.asarray(cap.V, dtype=np.longdouble)
    G = np.asarray(cap.G if hasattr(cap, "G") else cap.Γ, dtype=np.longdouble)
    ncut = int(np.count_nonzero(np.asarray(cap.cell_types) == -1))
    want = (np.longdouble(L[0]) * L[1] - area) if comp else area
    eps = np.longdouble(2.0) ** -52
    tol_v = (ncut + 3) * eps * (np.sum(np.abs(V)) + area + (L[0] * L[1] if comp else 0.0))
    tol_g = (ncut + 3) * eps * (np.sum(np.abs(G)) + perimeter)
    dv, dg = abs(np.sum(V) - want), abs(np.sum(G) - perimeter)
    print(f"[polygon {what}{name}] sum V off by {float(dv):.3g} (bound {float(tol_v):.3g}), sum Gamma off by {float(dg):.3g} "
          f"(bound {float(tol_g):.3g}), {ncut} cut cells")
    assert dv <= tol_v and dg <= tol_g, (name, float(dv), float(tol_v), float(dg), float(tol_g))


# ---- bars -----------------------------------------------------------------------------------------------------------------------------
# MEASURED: the worst ratio of each quantity, in units of 2^-52 (|x0| + L) / h, of the HOST build (g++ -O2 -ffp-contract=off, the
# kernels' 16-lane summation order) against the exact arbiter, on this project's CPU runs (tests/test_polygon_host.py prints them
# again).  The bar is 10 times the figure, with no floor.
MEASURED = {
    "circle_16": {"V": 0.0625, "G": 0.25, "A": 0.219, "B": 1.2, "W": 0.109, "Cw": 0.5, "Cg": 0.5},
    "heptagon_24": {"V": 0.68, "G": 0.273, "A": 0.344, "B": 4.7, "W": 0.914, "Cw": 3.75, "Cg": 0.5},
    "crystal_24": {"V": 0.68, "G": 0.297, "A": 0.344, "B": 0.891, "W": 0.352, "Cw": 0.5, "Cg": 0.5},
    "fine_circle_8": {"V": 0.0938, "G": 0.25, "A": 0.188, "B": 0.312, "W": 0.25, "Cw": 0.5, "Cg": 0.25},
    "rect_16": {"V": 0, "G": 0, "A": 0, "B": 0, "W": 0.25, "Cw": 0.25, "Cg": 0.125},
    "shifted_17x13": {"V": 0.614, "G": 0.243, "A": 0.407, "B": 0.407, "W": 0.402, "Cw": 0.465, "Cg": 0.465},
    "complement_16": {"V": 0.0625, "G": 0.25, "A": 0.234, "B": 0.844, "W": 0.25, "Cw": 0.5, "Cg": 0.5},
    "aligned_square_16": {"V": 0, "G": 0, "A": 0, "B": 0, "W": 0, "Cw": 0, "Cg": 0},
    "node_square_16": {"V": 0, "G": 0, "A": 0, "B": 0, "W": 0, "Cw": 0, "Cg": 0},
}
BARS = {name: {q: 10.0 * v for q, v in m.items()} for name, m in MEASURED.items()}


def check(name, got, ref, what=""):
    """print every figure, then hold each to its bar"""
    _, n, L, x0, _ = CASES[name]
    r = ratios(got, ref, x0, L, n)
    print(f"[polygon {what}{name}] " + "  ".join(f"{q} {r[q]:.3g}/{BARS[name][q]:.3g}" for q in QUANTITIES))
    bad = {q: (r[q], BARS[name][q]) for q in QUANTITIES if not r[q] <= BARS[name][q]}
    assert not bad, f"{name}: over the bar (measured, bar) in units of 2^-52 (|x0| + L) / h: {bad}"
    return r
