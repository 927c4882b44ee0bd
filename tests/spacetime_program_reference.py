"""Shared by tests/test_spacetime_program_host.py and tests/test_gpu_spacetime_program.py: the moving traced bodies of the suite,
the host (g++) build of penguin/jl_amd/csrc/pg_geom_program.h for a body phi(x, t) (tests/spacetime_program_host.cpp), the numpy
restatement of the slab rule on top of it, the cheap rule of k_st_classify through the same build, and the bars.

`slab_capacity` follows oracle/spacetime.py:make_spacetime_capacity line by line -- the same loops, padding, prev_i / next_i and
skip of W between two EMPTY cells -- with "the body at node k" = the program body at tau[k] measured by the host build, and the
normal speed - d_t phi / |grad phi| at the spatial interface centroid.  `C_w` may be supplied by the caller for B and W: the
section through a centroid moves with the centroid, which is not what a comparison of B and W is about.

Bars (the issue's rule).  Every difference is normalised as in tests/levelset_cases.py (a full cell, face or edge, times dt for
slab integrals; centroids where the fluid fraction exceeds 1e-3) in units of 2^-52 (|x0| + L) / h.  The bar of a quantity is twice
what tests/levelset_cases.py records against the fixture arbiter, worst over its smooth cases (MEASURED of ellipse_16,
ellipse_17x13, discs_24_smooth, ellipse_complement_16; the parent's values, not re-measured), plus (nq + 3) 2^-53 for the order of
summation: both sides sit within that bar of the truth, and a positive-weight time average cannot exceed the worst node."""
from __future__ import annotations

import ctypes as C
import itertools
import math
import subprocess
from pathlib import Path

import numpy as np

from oracle import geometry as og
from oracle import penguin_oracle as po
from oracle import spacetime as ost
from penguin.jl_amd.devfn import DeviceFunction, pg_program
from tests import levelset_cases as lc

ROOT = Path(__file__).resolve().parent.parent
P = C.POINTER(C.c_double)
SMOOTH_FIXTURE_CASES = ("ellipse_16", "ellipse_17x13", "discs_24_smooth", "ellipse_complement_16")
QUANTITIES = ("V", "A", "B", "W", "G", "Cw", "Cg", "Vn_1", "Vn")


# ---- bodies: closures of numpy operations of (x.., t) -----------------------------------------------------------------------------

def rotating_ellipse(cx=2.013, cy=1.968, a=1.1, b=0.6, omega=2.0):
    """(X / a)^2 + (Y / b)^2 - 1 with (X, Y) the coordinates turned by omega t about (cx, cy), a point off the cell lattice,
    written with the double angle: p (dx^2 + dy^2) + q (cos 2wt (dx^2 - dy^2) + 2 sin 2wt dx dy) - 1.  The program format repeats
    a subexpression every time it occurs, and the obvious form (`rotating_ellipse_naive`) has a d/dt of more than 96 instructions."""
    p, q = 0.5 * (1.0 / a ** 2 + 1.0 / b ** 2), 0.5 * (1.0 / a ** 2 - 1.0 / b ** 2)

    def phi(x, y, t):
        dx, dy = x - cx, y - cy
        return p * (dx * dx + dy * dy) + q * (np.cos(2.0 * omega * t) * (dx * dx - dy * dy) + 2.0 * np.sin(2.0 * omega * t) * dx * dy) - 1.0
    return phi


def rotating_ellipse_naive(cx=2.013, cy=1.968, a=1.1, b=0.6, omega=2.0):
    def phi(x, y, t):
        c, s = np.cos(omega * t), np.sin(omega * t)
        X = c * (x - cx) + s * (y - cy)
        Y = c * (y - cy) - s * (x - cx)
        return (X / a) ** 2 + (Y / b) ** 2 - 1.0
    return phi


def pulsating_superellipse(cx=2.013, cy=1.968, a=1.2, b=0.8, amp=0.3, freq=5.0):
    """((x - cx) / a)^4 + ((y - cy) / b)^4 = 1 + amp sin(freq t)"""
    def phi(x, y, t):
        return ((x - cx) / a) ** 4 + ((y - cy) / b) ** 4 - (1.0 + amp * np.sin(freq * t))
    return phi


def wall_1d(x, t):
    return x - (0.37 + 0.2 * np.sin(3.0 * t))


WALL_POS, WALL_DPOS = (lambda t: 0.37 + 0.2 * np.sin(3.0 * t)), (lambda t: 0.6 * np.cos(3.0 * t))


def moving_disc(x, y, t):
    return np.sqrt((x - (2.013 + 0.8 * t)) ** 2 + (y - (1.968 - 0.5 * t)) ** 2) - (1.0 + 0.4 * t)


DISC_CEN, DISC_DCEN = (lambda t: (2.013 + 0.8 * t, 1.968 - 0.5 * t)), (lambda t: (0.8, -0.5))
DISC_RAD, DISC_DRAD = (lambda t: 1.0 + 0.4 * t), (lambda t: 0.4)


def growing_disc(x, y, t):
    """fixed centre, r(t) = 0.8 + 0.3 t, as x^2 + y^2 - r^2: the slab integral of its area is a cubic in t, exact for any Gauss rule
    of two or more points"""
    return (x - 2.013) * (x - 2.013) + (y - 1.968) * (y - 1.968) - (0.8 + 0.3 * t) * (0.8 + 0.3 * t)


def wavy_wall(x, y, t):
    """an oscillating wavy wall: the fluid below y = 2.1 + 0.3 sin(2 x) cos(6 t)"""
    return y - (2.1 + 0.3 * np.sin(2.0 * x) * np.cos(6.0 * t))


def approaching_discs(x, y, t):
    """two discs of radius 0.6 approaching each other at 0.6 each (disjoint during the slabs of the tests: no kink of the interface;
    the line where the two branches of min meet, x = 2.0605, passes through no cell centre of the meshes used -- on a centre the
    entry's derivative check meets the kink of min and refuses, rightly)"""
    a, b, c = x - (1.25 + 0.6 * t), x - (2.871 - 0.6 * t), y - 1.968
    return np.minimum(a * a + c * c - 0.36, b * b + c * c - 0.36)


# name: (closure, complement, n, L, x0) -- 12 x 10 and 16 x 16 with an offset origin, 10 cells in 1-D
MESH_A, MESH_B, MESH_1D = ((12, 10), (4.0, 4.0), (0.1, 0.05)), ((16, 16), (4.0, 4.0), (-0.2, 0.15)), ((10,), (1.0,), (0.0,))
CASES = {
    "ellipse": (rotating_ellipse(), False) + MESH_A,
    "ellipse_complement": (rotating_ellipse(), True) + MESH_B,
    "superellipse": (pulsating_superellipse(), False) + MESH_B,
    "wall": (wall_1d, False) + MESH_1D,
    "disc": (moving_disc, False) + MESH_A,
    "growing_disc": (growing_disc, False) + MESH_B,
    "wavy_wall": (wavy_wall, False) + MESH_A,
    "approaching_discs": (approaching_discs, False) + MESH_B,
}
T0, DT = 0.1, 0.05
RULES = {3: (3, 1), 16: (4, 4), 64: (16, 4), 80: (20, 4)}      # nq: (panels, order)


def time_rule(t0, t1, panels, order):
    """penguin.jl_amd.moving.time_rule, restated"""
    x, w = np.polynomial.legendre.leggauss(order)
    edges = np.linspace(t0, t1, panels + 1)
    tau = np.concatenate([0.5 * (a + b) + 0.5 * (b - a) * x for a, b in zip(edges[:-1], edges[1:])])
    wt = np.concatenate([0.5 * (b - a) * w for a, b in zip(edges[:-1], edges[1:])])
    return tau, wt * ((t1 - t0) / wt.sum())


# ---- the host build ---------------------------------------------------------------------------------------------------------------

def build_host_lib():
    out = ROOT / "tests" / "_build" / "libspacetime_program_host.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "spacetime_program_host.cpp"
    deps = [src] + [ROOT / "penguin" / "jl_amd" / "csrc" / n for n in ("pg_geom_program.h", "pg_geom.h", "pg_program.h")]
    if not out.exists() or out.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out), str(src)], check=True)
    return C.CDLL(str(out))


def _arr(v):
    return np.ascontiguousarray(v, dtype=float)


def _pad3(v):
    return _arr(list(v) + [0.0] * (3 - len(v)))


class HostMovingBody:
    """A DeviceFunction phi(x.., t) measured by the host build at given times."""

    def __init__(self, lib, fn, N, complement=False):
        self.lib, self.N = lib, N
        self.df = fn if isinstance(fn, DeviceFunction) else DeviceFunction(fn)
        self.comp = int(bool(complement) != bool(self.df.complement))
        self.phi = self.df.moving_body_program(N)
        self.derivs = (pg_program * (N + 1))(*self.df.moving_gradient_programs(N))

    def box_nodes(self, times, lo, hi, want_surface=True) -> np.ndarray:
        """rows of (type, vol, cen[3], gamma, cg[3], v_n)"""
        times = _arr(times)
        out = np.zeros((len(times), 10))
        lo, hi = _pad3(lo), _pad3(hi)
        self.lib.stp_box_nodes(self.N, self.comp, C.byref(self.phi), self.derivs, len(times), times.ctypes.data_as(P),
                               lo.ctypes.data_as(P), hi.ctypes.data_as(P), int(want_surface), out.ctypes.data_as(P))
        return out

    def section_nodes(self, times, d, s, lo, hi) -> np.ndarray:
        times = _arr(times)
        out = np.zeros(len(times))
        lo, hi = _pad3(lo), _pad3(hi)
        self.lib.stp_section_nodes(self.N, self.comp, C.byref(self.phi), self.derivs, len(times), times.ctypes.data_as(P), d,
                                   C.c_double(s), lo.ctypes.data_as(P), hi.ctypes.data_as(P), C.c_double(-1.0), out.ctypes.data_as(P))
        return out

    def far(self, lo, hi, t0, t1) -> int:
        lo, hi = _pad3(lo), _pad3(hi)
        return int(self.lib.stp_far(self.N, self.comp, C.byref(self.phi), self.derivs, lo.ctypes.data_as(P), hi.ctypes.data_as(P),
                                    C.c_double(t0), C.c_double(t1)))


# ---- the slab rule ----------------------------------------------------------------------------------------------------------------

def _cells(n, N, rng=None):
    rng = rng or [range(1, n[d] + 1) for d in range(N)]
    for rev in itertools.product(*reversed(rng)):
        yield tuple(reversed(rev))


def slab_capacity(body: HostMovingBody, mesh: po.Mesh, t0: float, t1: float, tau, wt, C_w=None) -> po.Capacity:
    """oracle/spacetime.py:make_spacetime_capacity for a program body, on the time rule (tau, wt).  C_w (M x N or more columns):
    the centroids B and W are taken at, instead of this function's own."""
    N = mesh.N
    assert N in (1, 2)
    n, ext, nodes = mesh.dims, mesh.ext, mesh.nodes
    M = int(np.prod(ext))
    tau, wt = np.asarray(tau, dtype=float), np.asarray(wt, dtype=float)
    nq = len(tau)
    times = np.concatenate([tau, [t0, t1]])
    st = ost.SpaceTimeMesh(mesh, [t0, t1])
    M2 = 2 * M
    V, G, ct = np.zeros(M2), np.zeros(M2), np.zeros(M2)
    Cw, Cg = np.zeros((M2, N + 1)), np.zeros((M2, N + 1))
    A = tuple(np.zeros(M2) for _ in range(N + 1))
    B = tuple(np.zeros(M2) for _ in range(N + 1))
    W = tuple(np.zeros(M2) for _ in range(N + 1))
    dt = t1 - t0
    for I in _cells(n, N):
        li = po.lin_index(ext, I)
        lo = [float(nodes[d][I[d] - 1]) for d in range(N)]
        hi = [float(nodes[d][I[d]]) for d in range(N)]
        rows = body.box_nodes(times, lo, hi)
        m0, m1 = rows[nq], rows[nq + 1]
        types = {int(m0[0]), int(m1[0])}
        v = gam = momt = gmt = 0.0
        mom, gm = np.zeros(N), np.zeros(N)
        for k in range(nq):
            m = rows[k]
            types.add(int(m[0]))
            v += wt[k] * m[1]
            momt += wt[k] * m[1] * tau[k]
            mom += wt[k] * m[1] * m[2:2 + N]
            if m[5] > 0.0:
                vn = m[9]
                ws = wt[k] * m[5] * math.sqrt(1.0 + vn * vn)
                gam += ws
                gmt += ws * tau[k]
                gm += ws * m[6:6 + N]
        ctr = [0.5 * (lo[d] + hi[d]) for d in range(N)]
        if types == {og.FULL}:
            vol = float(np.prod([hi[d] - lo[d] for d in range(N)]))
            V[li], A[N][li], A[N][M + li], ct[li] = vol * dt, vol, vol, og.FULL
            Cw[li, :N], Cw[li, N] = ctr, 0.5 * (t0 + t1)
        elif types == {og.EMPTY}:
            ct[li] = og.EMPTY
            Cw[li, :N], Cw[li, N] = ctr, 0.5 * (t0 + t1)
        else:
            ct[li] = og.CUT
            V[li], A[N][li], A[N][M + li], G[li] = v, m0[1], m1[1], gam
            Cw[li, :N], Cw[li, N] = (mom / v, momt / v) if v > 0.0 else (ctr, 0.5 * (t0 + t1))
            if gam > 0.0:
                Cg[li, :N], Cg[li, N] = gm / gam, gmt / gam
    Cu = Cw if C_w is None else np.asarray(C_w)
    for d in range(N):
        rng = [range(1, (n[k] + 2) if k == d else (n[k] + 1)) for k in range(N)]
        for I in _cells(n, N, rng):
            li = po.lin_index(ext, I)
            lo = [float(nodes[k][min(I[k], n[k]) - 1]) for k in range(N)]
            hi = [float(nodes[k][min(I[k], n[k])]) for k in range(N)]
            s = float(nodes[d][I[d] - 1])
            A[d][li] = float(np.sum(wt * body.section_nodes(tau, d, s, lo, hi)))
    for I in _cells(n, N):
        li = po.lin_index(ext, I)
        lo = [float(nodes[d][I[d] - 1]) for d in range(N)]
        hi = [float(nodes[d][I[d]]) for d in range(N)]
        for d in range(N):
            B[d][li] = float(np.sum(wt * body.section_nodes(tau, d, float(Cu[li, d]), lo, hi)))
    for d in range(N):
        rng = [range(1, (n[k] + 2) if k == d else (n[k] + 1)) for k in range(N)]
        for I in _cells(n, N, rng):
            li = po.lin_index(ext, I)
            prev_i, next_i = max(I[d] - 1, 1), min(I[d], n[d])            # capacity.jl:401-402
            lp = po.lin_index(ext, tuple(prev_i if k == d else I[k] for k in range(N)))
            ln = po.lin_index(ext, tuple(next_i if k == d else I[k] for k in range(N)))
            lo = [float(Cu[lp, k]) if k == d else float(nodes[k][I[k] - 1]) for k in range(N)]
            hi = [float(Cu[ln, k]) if k == d else float(nodes[k][I[k]]) for k in range(N)]
            if ct[lp] == og.EMPTY and ct[ln] == og.EMPTY:
                continue
            W[d][li] = float(np.sum(wt * body.box_nodes(tau, lo, hi, want_surface=False)[:, 1]))
    return po.Capacity(A, B, V, W, Cw, Cg, G, ct, st, body)


def all_nodes_types(body: HostMovingBody, mesh: po.Mesh, t0, t1, tau):
    """(type under the all-nodes rule, what the cheap rule says: 1 / -1 / 0) of every real cell, by linear index"""
    N, n, ext, nodes = mesh.N, mesh.dims, mesh.ext, mesh.nodes
    times = np.concatenate([np.asarray(tau, dtype=float), [t0, t1]])
    out = {}
    for I in _cells(n, N):
        lo = [float(nodes[d][I[d] - 1]) for d in range(N)]
        hi = [float(nodes[d][I[d]]) for d in range(N)]
        ts = set(int(v) for v in body.box_nodes(times, lo, hi, want_surface=False)[:, 0])
        typ = og.FULL if ts == {og.FULL} else og.EMPTY if ts == {og.EMPTY} else og.CUT
        out[po.lin_index(ext, I)] = (typ, body.far(lo, hi, t0, t1))
    return out


# ---- comparisons ------------------------------------------------------------------------------------------------------------------

class Layer:
    """the first time layer of a capacity in the names lc.ratios reads, from a product capacity or a po.Capacity of the slab"""

    def __init__(self, cap, N, M):
        if isinstance(cap, po.Capacity):
            self.V, self.G, self.cell_types = cap.V[:M], cap.G[:M], cap.cell_types[:M]
            self.A, self.B, self.W = (tuple(a[:M] for a in f[:N]) for f in (cap.A, cap.B, cap.W))
            self.Vn_1, self.Vn = cap.A[N][:M], cap.A[N][M:]
            self.C_w_st, self.C_g_st = cap.C_w[:M], (cap.C_g[:M] if cap.C_g.shape[0] else np.zeros((M, N + 1)))
        else:
            self.V, self.G, self.cell_types = cap.V, cap.Γ, cap.cell_types
            self.A, self.B, self.W, self.Vn_1, self.Vn = cap.A, cap.B, cap.W, cap.Vn_1, cap.Vn
            self.C_w_st, self.C_g_st = cap.C_ω_st, cap.C_γ_st
        self.C_w, self.C_g = self.C_w_st[:, :N], self.C_g_st[:, :N]


def bars(nq: int, x0, L, n, source=None):
    """per quantity, in units of 2^-52 (|x0| + L) / h.  source: a dict of recorded figures to double (default: MEASURED, worst over
    the smooth fixture cases)"""
    u, _ = lc.unit(x0, L, n)
    order = (nq + 3) * 2.0 ** -53 / u
    base = source or {q: max(lc.MEASURED[c][q] for c in SMOOTH_FIXTURE_CASES) for q in lc.QUANTITIES}
    out = {q: 2.0 * base[q] + order for q in lc.QUANTITIES}
    out["Vn_1"] = out["Vn"] = 2.0 * base["V"] + order
    return out


def slab_ratios(got: Layer, ref: Layer, x0, L, n, dt):
    """lc.ratios with the slab integrals divided by dt, plus the face volumes; the time components of the centroids, divided by
    dt, are held to the same units as the spatial ones divided by h (their error is that of the V(tau_k) and Gamma(tau_k) they
    average) and the worse of the two is reported"""
    N = len(n)

    class Scaled:
        def __init__(self, o):
            self.V, self.G = o.V / dt, o.G / dt
            self.A, self.B, self.W = (tuple(a / dt for a in f) for f in (o.A, o.B, o.W))
            self.C_w, self.C_g = o.C_w, o.C_g

    r = lc.ratios(Scaled(got), Scaled(ref), x0, L, n)
    u, h = lc.unit(x0, L, n)
    full = float(np.prod([Ld / nd for Ld, nd in zip(L, n)]))
    r["Vn_1"] = float(np.max(np.abs(got.Vn_1 - ref.Vn_1)) / full / u)
    r["Vn"] = float(np.max(np.abs(got.Vn - ref.Vn)) / full / u)
    keep = ref.V / dt > 1e-3 * full
    keepg = keep & (ref.G / dt > 1e-3 * h ** (N - 1))
    for q, a, b, k in (("Cw", got.C_w_st, ref.C_w_st, keep), ("Cg", got.C_g_st, ref.C_g_st, keepg)):
        if k.any():
            r[q] = max(r[q], float(np.max(np.abs(a[:, N] - b[:, N])[k]) / dt / u))
    return r


def check(name, got: Layer, ref: Layer, x0, L, n, dt, nq, source=None, what=""):
    """print every figure, then hold each to its bar"""
    r, b = slab_ratios(got, ref, x0, L, n, dt), bars(nq, x0, L, n, source)
    print(f"[spacetime-program {what}{name} nq={nq}] " + "  ".join(f"{q} {r[q]:.3g}/{b[q]:.3g}" for q in QUANTITIES))
    bad = {q: (r[q], b[q]) for q in QUANTITIES if not r[q] <= b[q]}
    assert not bad, f"{name}: over the bar (measured, bar) in units of 2^-52 (|x0| + L) / h: {bad}"
    return r
