"""Shared by tests/test_levelset_host.py, tests/test_gpu_levelset.py and tests/golden/make_levelset_fixture.py: the traced
level-set bodies of the suite, the host (g++) build of penguin/jl_amd/csrc/pg_geom_program.h wrapped as a duck-typed body for
oracle.penguin_oracle.make_capacity (`box`, `section`), and the bars.

Bars.  Every difference is normalised by the measure of a full cell, face or edge (dV / h^2, dA dB dGamma / h, dW / h^2,
dC / h, with h = min_d h_d; centroids only where the fluid fraction exceeds 1e-3) and held to c * 2^-52 * (|x0| + L) / h: a root
is known to one ulp of its coordinate.  c is 10 times the worst ratio the HOST build shows here on the CPU against the arbiter
named (DESIGN.md section 23 has the measured worsts); the GPU is held to the same c and never sets it."""
from __future__ import annotations

import ctypes as C
import json
import subprocess
from pathlib import Path

import numpy as np

from oracle.geometry import BoxMeasure
from penguin.jl_amd.devfn import DeviceFunction, pg_program

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests" / "golden" / "levelset_cells.json"
P = C.POINTER(C.c_double)
QUANTITIES = ("V", "A", "B", "W", "G", "Cw", "Cg")


# ---- bodies (closures of numpy operations: traced by DeviceFunction, called with arrays by the oracle) ---------------------------

def rotated_ellipse(cx=2.01, cy=1.97, a=1.3, b=0.6, angle=0.5, sign=1.0):
    c, s = float(np.cos(angle)), float(np.sin(angle))

    def phi(x, y):
        X = c * (x - cx) + s * (y - cy)
        Y = c * (y - cy) - s * (x - cx)
        return sign * ((X / a) ** 2 + (Y / b) ** 2 - 1.0)
    return phi


def two_discs(x, y):
    return np.minimum(np.sqrt((x - 1.6) ** 2 + (y - 2.01) ** 2) - 0.8, np.sqrt((x - 2.5) ** 2 + (y - 2.2) ** 2) - 0.7)


def circle(cx=2.01, cy=2.01, r=1.0):
    return lambda x, y: np.sqrt((x - cx) ** 2 + (y - cy) ** 2) - r


def ellipse_sqrt(cx, cy, a, b):
    """the level set of oracle.geometry.Ellipsoid: sqrt(sum ((x_d - c_d) / a_d)^2) - 1"""
    return lambda x, y: np.sqrt(((x - cx) / a) ** 2 + ((y - cy) / b) ** 2) - 1.0


def plane(nx, ny, off):
    return lambda x, y: nx * x + ny * y - off


# ---- the host build as an oracle body -----------------------------------------------------------------------------------------------

def build_host_lib():
    out = ROOT / "tests" / "_build" / "liblevelset_host.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "levelset_host.cpp"
    deps = [src] + [ROOT / "penguin" / "jl_amd" / "csrc" / n for n in ("pg_geom_program.h", "pg_geom.h", "pg_program.h")]
    if not out.exists() or out.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out), str(src)], check=True)
    lib = C.CDLL(str(out))
    lib.ls_section.restype = C.c_double
    return lib


def _arr(v):
    return np.ascontiguousarray(v, dtype=float)


class HostBody:
    """A DeviceFunction's programs measured by the host build: `box` and `section` as oracle.geometry's bodies have them."""

    def __init__(self, lib, fn, N, complement=False):
        self.lib, self.N, self.comp = lib, N, int(bool(complement))
        self.df = fn if isinstance(fn, DeviceFunction) else DeviceFunction(fn)
        self.phi = self.df.body_program(N)
        self.grad = (pg_program * N)(*self.df.gradient_programs(N))

    def __call__(self, *x):
        v = self.df(*x)
        return -v if self.comp else v

    def box(self, lo, hi, want_surface=True) -> BoxMeasure:
        out = np.zeros(9)
        lo, hi = _arr(list(lo) + [0.0] * (3 - self.N)), _arr(list(hi) + [0.0] * (3 - self.N))
        self.lib.ls_box(self.N, self.comp, C.byref(self.phi), self.grad, lo.ctypes.data_as(P), hi.ctypes.data_as(P),
                        int(want_surface), out.ctypes.data_as(P))
        return BoxMeasure(int(out[0]), float(out[1]), tuple(out[2:2 + self.N]), float(out[5]), tuple(out[6:6 + self.N]))

    def section(self, d, s, lo, hi) -> float:
        lo, hi = _arr(list(lo) + [0.0] * (3 - self.N)), _arr(list(hi) + [0.0] * (3 - self.N))
        return self.lib.ls_section(self.N, self.comp, C.byref(self.phi), self.grad, d, C.c_double(s), lo.ctypes.data_as(P),
                                   hi.ctypes.data_as(P), C.c_double(-1.0))


# ---- comparisons ------------------------------------------------------------------------------------------------------------------

def unit(mesh_x0, mesh_L, mesh_n):
    """2^-52 (|x0| + L) / h with h the smallest spacing: the size of one ulp of a coordinate in units of h"""
    h = min(L / n for L, n in zip(mesh_L, mesh_n))
    return 2.0 ** -52 * max(abs(x) + L for x, L in zip(mesh_x0, mesh_L)) / h, h


def ratios(got, ref, x0, L, n):
    """worst normalised difference of each quantity, in units of 2^-52 (|x0| + L) / h.  got / ref: anything with V, A, B, W, the
    interface measure (G or Γ), C_w / C_ω, C_g / C_γ"""
    u, h = unit(x0, L, n)
    N = len(n)

    def f(o, *names):
        for k in names:
            if hasattr(o, k):
                return getattr(o, k)
        raise AttributeError(names[0])

    full = float(np.prod([Ld / nd for Ld, nd in zip(L, n)]))
    V, Vr = np.asarray(f(got, "V")), np.asarray(f(ref, "V"))
    face = h ** (N - 1)
    out = {"V": np.max(np.abs(V - Vr)) / full / u,
           "G": np.max(np.abs(np.asarray(f(got, "G", "Γ")) - np.asarray(f(ref, "G", "Γ")))) / face / u}
    for name in ("A", "B", "W"):
        scale = full if name == "W" else face
        out[name] = max(np.max(np.abs(np.asarray(f(got, name)[d]) - np.asarray(f(ref, name)[d]))) for d in range(N)) / scale / u
    keep = Vr > 1e-3 * full
    Cw, Cwr = np.asarray(f(got, "C_w", "C_ω")), np.asarray(f(ref, "C_w", "C_ω"))
    out["Cw"] = (np.max(np.abs(Cw - Cwr)[keep]) if keep.any() else 0.0) / h / u
    Gr = np.asarray(f(ref, "G", "Γ"))
    keepg = keep & (Gr > 1e-3 * face)
    Cg, Cgr = np.asarray(f(got, "C_g", "C_γ")), np.asarray(f(ref, "C_g", "C_γ"))
    out["Cg"] = (np.max(np.abs(Cg - Cgr)[keepg]) if keepg.any() else 0.0) / h / u
    return {k: float(v) for k, v in out.items()}


class FixtureCase:
    def __init__(self, name, d):
        self.name = name
        self.n, self.L, self.x0 = tuple(d["n"]), tuple(d["L"]), tuple(d["x0"])
        N = len(self.n)
        self.V, self.G, self.cell_types = np.array(d["V"]), np.array(d["G"]), np.array(d["cell_types"])
        self.A = tuple(np.array(a) for a in d["A"])
        self.B = tuple(np.array(a) for a in d["B"])
        self.W = tuple(np.array(a) for a in d["W"])
        self.C_w = np.array(d["C_w"]).reshape(-1, N)
        self.C_g = np.array(d["C_g"]).reshape(-1, N)


def load_fixture():
    raw = json.loads(FIXTURE.read_text())
    return {k: FixtureCase(k, v) for k, v in raw["cases"].items()}


FIXTURE_BODIES = {
    "ellipse_16": (lambda: rotated_ellipse(), False),
    "ellipse_17x13": (lambda: rotated_ellipse(), False),
    "discs_24": (lambda: two_discs, False),
    "ellipse_complement_16": (lambda: rotated_ellipse(), True),
}

# ---- bars ---------------------------------------------------------------------------------------------------------------------------
# MEASURED: the worst ratio of each quantity, in units of 2^-52 (|x0| + L) / h, of the HOST build (g++ -O2 -ffp-contract=off,
# glibc's libm) against the arbiter named, on this project's CPU runs (tests/test_levelset_host.py prints them again).  The bar
# of a quantity is c = 10 times the measured worst of those units -- the 10 is for the device's libm -- with no floor: where the
# host build agrees with its arbiter exactly (1-D half line: every figure 0) the bar is 0 and the comparison is exact.  The GPU
# is held to the same c.
#   fixture cases: against tests/golden/levelset_cells.json (30 digits).  discs_24 has two cells with a KINK of the interface
#     inside (the discs meet at (1.838.., 1.246..) and (1.916.., 2.586..)): no breakpoint falls on the kink, Gauss-Legendre runs
#     across it and those two cells, and the staggered boxes that contain a kink, are 1e-3 .. 1e-5 of a cell off -- the documented
#     accuracy of the kind at a kink.  "discs_24_smooth" is the same case without the entries of those cells and of their upper
#     neighbours (A, B, W of a cell reach one cell down): rounding level like the rest.
#   circle, ellipse0: against oracle.geometry.Ball at 12^2 16^2 24^2 48^2 and Ellipsoid at 16^2 24^2 48^2, through .box and
#     .section.  B, W and C_w are the closed forms' own loss in thin cells, not the quadrature's.
#   plane: against tests/plane_oracle.py, 0.6 x - 0.8 y - 0.31 at 16^2 and 24^2 and x - 1.375 (on a node line) at 16^2, both phases.
MEASURED = {
    "ellipse_16": {"V": 5.94, "G": 406.0, "A": 0.562, "B": 6.88, "W": 7.09, "Cw": 8.0, "Cg": 336.0},
    "ellipse_17x13": {"V": 0.154, "G": 0.669, "A": 0.378, "B": 0.68, "W": 0.463, "Cw": 0.465, "Cg": 0.465},
    "discs_24": {"V": 6.56e10, "G": 6.15e11, "A": 0.422, "B": 8.54e8, "W": 5.59e11, "Cw": 1.91e10, "Cg": 2.87e11},
    "discs_24_smooth": {"V": 0.211, "G": 1.09, "A": 0.422, "B": 0.633, "W": 0.527, "Cw": 0.5, "Cg": 0.5},
    "ellipse_complement_16": {"V": 5.86, "G": 406.0, "A": 0.547, "B": 51.2, "W": 13.6, "Cw": 16.5, "Cg": 336.0},
    "circle": {"V": 2.57, "G": 0.572, "A": 0.5, "B": 8510.0, "W": 243.0, "Cw": 3900.0, "Cg": 23.2},
    "ellipse0": {"V": 2.36, "G": 1.37, "A": 1.12, "B": 31900.0, "W": 504.0, "Cw": 15900.0, "Cg": 0.5},
    "plane": {"V": 0.516, "G": 1.16, "A": 0.5, "B": 1.0, "W": 0.609, "Cw": 0.5, "Cg": 0.75},
    "halfspace1d": {"V": 0.0, "G": 0.0, "A": 0.0, "B": 0.0, "W": 0.0, "Cw": 0.0, "Cg": 0.0},
}
BARS = {name: {q: 10.0 * v for q, v in m.items()} for name, m in MEASURED.items()}

# In discs_24 the bars of V, B, W, G, C_w, C_g are those of the two kink cells and say nothing else; what the kink may cost is
# bounded from the rule itself.  One Gauss-Legendre rule of n = 16 nodes runs over a piece of width <= h whose integrand, the
# height of the fluid column, has a jump J of its slope at the kink.  The rule is exact for the smooth part; for the hinge
# J max(u - u*, 0) its error is at most J h^2 / (2 n^2) times a constant below 2.5 (the nodes' spacing is at most 2.5 h / n near
# the middle of the interval): with J <= 2 (each disc's boundary is a graph of slope <= 1 over the axis the gradient picks)
# that is 2 * 2.5 / 512 < 1e-2 h^2 for V and W.  For the interface the integrand itself, |grad phi| / |d phi / d v| in [1, sqrt 2],
# JUMPS at the kink: the error is at most the jump times the largest weight, (sqrt 2 - 1) * 0.19 h / 2 < 4e-2 h.
KINK_ABS = {"V": 1e-2, "W": 1e-2, "G": 4e-2}     # of h^2, h^2, h

KINK_CELLS = ((13, 8), (11, 15))                 # 0-based (i, j) of the two cells of discs_24 that hold a kink


class Masked:
    """the capacities of `cap` with the entries of the kink cells of discs_24 and of their upper neighbours replaced by `ref`'s"""

    def __init__(self, cap, ref, ext):
        drop = np.zeros(ext[0] * ext[1], dtype=bool)
        for i, j in KINK_CELLS:
            for di, dj in ((0, 0), (1, 0), (0, 1)):
                drop[(j + dj) * ext[0] + i + di] = True

        def pick(o, *names):
            for k in names:
                if hasattr(o, k):
                    return getattr(o, k)
            raise AttributeError(names[0])

        def mix(a, b):
            a = np.array(a, dtype=float, copy=True)
            a[drop] = np.asarray(b)[drop]
            return a
        self.V = mix(pick(cap, "V"), ref.V)
        self.G = mix(pick(cap, "G", "Γ"), ref.G)
        self.A, self.B, self.W = (tuple(mix(pick(cap, k)[d], getattr(ref, k)[d]) for d in range(2)) for k in ("A", "B", "W"))
        self.C_w = mix(pick(cap, "C_w", "C_ω"), ref.C_w)
        self.C_g = mix(pick(cap, "C_g", "C_γ"), ref.C_g)


def check(name, got, ref, x0, L, n, what=""):
    """print every figure, then hold each to its bar"""
    r = ratios(got, ref, x0, L, n)
    print(f"[levelset {what}{name}] " + "  ".join(f"{q} {r[q]:.3g}/{BARS[name][q]:.3g}" for q in QUANTITIES))
    bad = {q: (r[q], BARS[name][q]) for q in QUANTITIES if not r[q] <= BARS[name][q]}
    assert not bad, f"{name}: over the bar (measured, bar) in units of 2^-52 (|x0| + L) / h: {bad}"
    return r


def check_kink(got, ref, L, n, what=""):
    """discs_24 with its kink cells in: V and W to KINK_ABS of a full cell, the interface measure to KINK_ABS of an edge"""
    h = L[0] / n[0]

    def pick(o, *names):
        return next(getattr(o, k) for k in names if hasattr(o, k))
    fig = {"V": np.max(np.abs(np.asarray(pick(got, "V")) - ref.V)) / h ** 2,
           "W": max(np.max(np.abs(np.asarray(pick(got, "W")[d]) - ref.W[d])) for d in range(2)) / h ** 2,
           "G": np.max(np.abs(np.asarray(pick(got, "G", "Γ")) - ref.G)) / h}
    print(f"[levelset {what}kink cells] " + "  ".join(f"{q} {fig[q]:.3g}/{KINK_ABS[q]:.3g}" for q in fig))
    bad = {q: (fig[q], KINK_ABS[q]) for q in fig if not fig[q] <= KINK_ABS[q]}
    assert not bad, f"kink cells over the bar (measured, bar): {bad}"
