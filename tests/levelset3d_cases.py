"""Shared by tests/test_levelset3d_host.py, tests/test_gpu_levelset3d.py and tests/golden/make_levelset3d_fixture.py: the traced
3-D level-set bodies of the suite, the host (g++) build of penguin/jl_amd/csrc/pg_geom_program3.h wrapped as a duck-typed body
for oracle.penguin_oracle.make_capacity (`box`, `section`), the closed-form test of which cut cells are IRREGULAR, and the bars.

Units.  Every difference is normalised by the measure of a full cell, face or edge (dV dW / h^3, dA dB dGamma / h^2, dC / h; the
centroids only where the fluid fraction exceeds 1e-3) and given in u = 2^-52 (|x0| + L) / h, DESIGN.md section 23's unit.

Classes.  A box is IRREGULAR when, with the axes (u, v, w) the rule picks from the gradient at the box centre, the trace of the
interface on a face v = const has an extreme point in w inside the box (there d_u phi = 0: the trace is no graph u = g(w)) or
d_v phi vanishes on the interface inside the box.  For the bodies here both sets are circles, so the test is closed form
(`irregular_box`).  An irregular box carries a square-root singularity inside an outer Gauss-Legendre piece; the rule integrates
across it.  V, Gamma, C_w, C_g of a cell follow the cell's class; B_d (a section through the centroid)
follows the cell's or the section's own; W_d follows the staggered box's own class or that of either cell whose centroid bounds
it; A_d follows the face's: a face is the 2-D rule, irregular when the in-plane derivative along its height axis vanishes on the
interface inside the face (`irregular_section`: the small slices near the poles of a body a few cells wide)."""
from __future__ import annotations

import base64
import ctypes as C
import json
import math
import subprocess
import zlib
from pathlib import Path

import numpy as np

from oracle import penguin_oracle as po
from oracle.geometry import BoxMeasure
from penguin.jl_amd.devfn import DeviceFunction, pg_program
from tests.levelset_cases import unit

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests" / "golden" / "levelset3d_cells.json"
P = C.POINTER(C.c_double)

# ---- bodies -----------------------------------------------------------------------------------------------------------------------

PLANE_N, PLANE_OFF = (0.6, -0.64, 0.48), 0.37
PLANE_MESH = ((9, 8, 7), (3.0, 2.5, 2.0), (-0.7, 0.3, -1.1))           # n, L, x0
BALL_C, BALL_R = (2.01, 1.97, 2.03), 1.0
ELL_C, ELL_A = (2.01, 1.97, 2.03), (1.3, 0.8, 1.05)
TORUS_C, TORUS_R, TORUS_r = (2.03, 1.96, 2.07), 1.2, 0.5
TORUS_MESH = ((12, 12, 12), (4.0, 4.0, 4.0), (0.0, 0.0, 0.0))


def plane(n=PLANE_N, off=PLANE_OFF):
    return lambda x, y, z: n[0] * x + n[1] * y + n[2] * z - off


def ball(c=BALL_C, r=BALL_R):
    return lambda x, y, z: np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r


def ellipsoid(c=ELL_C, a=ELL_A):
    """the level set of oracle.geometry.Ellipsoid"""
    return lambda x, y, z: np.sqrt(((x - c[0]) / a[0]) ** 2 + ((y - c[1]) / a[1]) ** 2 + ((z - c[2]) / a[2]) ** 2) - 1.0


def torus(c=TORUS_C, R=TORUS_R, r=TORUS_r):
    return lambda x, y, z: (np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2) - R) ** 2 + (z - c[2]) ** 2 - r * r


def rotated_ellipsoid(c=(2.02, 1.97, 2.05), a=(1.4, 0.9, 1.1), alpha=0.5, beta=0.35):
    """an ellipsoid turned by alpha about z, then by beta about x: sum_i (m_i . (x - c))^2 - 1 with the rows m_i of the rotation
    divided by the semi-axes (the rows are folded to numbers here: the traced program holds no repeated subexpression)"""
    ca, sa, cb, sb = math.cos(alpha), math.sin(alpha), math.cos(beta), math.sin(beta)
    Rz = np.array([[ca, sa, 0.0], [-sa, ca, 0.0], [0.0, 0.0, 1.0]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cb, sb], [0.0, -sb, cb]])
    m = (Rx @ Rz) / np.array(a)[:, None]
    k = m @ np.array(c)

    def phi(x, y, z):
        out = -1.0
        for i in range(3):
            u = float(m[i, 0]) * x + float(m[i, 1]) * y + float(m[i, 2]) * z - float(k[i])
            out = out + u * u
        return out
    phi.axes = a
    return phi


# ---- the host build as an oracle body ---------------------------------------------------------------------------------------------

def build_host_lib():
    out = ROOT / "tests" / "_build" / "liblevelset3d_host.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "levelset3d_host.cpp"
    deps = [src] + [ROOT / "penguin" / "jl_amd" / "csrc" / n for n in ("pg_geom_program3.h", "pg_geom_program.h", "pg_geom.h", "pg_program.h")]
    if not out.exists() or out.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out), str(src)], check=True)
    lib = C.CDLL(str(out))
    lib.ls3_section.restype = C.c_double
    return lib


def _arr(v):
    return np.ascontiguousarray(v, dtype=float)


class HostBody3:
    """A DeviceFunction's 3-D programs measured by the host build: `box` and `section` as oracle.geometry's bodies have them."""

    def __init__(self, lib, fn, complement=False):
        self.lib, self.N, self.comp = lib, 3, int(bool(complement))
        self.df = fn if isinstance(fn, DeviceFunction) else DeviceFunction(fn)
        self.phi = self.df.body_program(3)
        self.grad = (pg_program * 3)(*self.df.gradient_programs(3))

    def __call__(self, *x):
        v = self.df(*x)
        return -v if self.comp else v

    def box(self, lo, hi, want_surface=True, qlane=0, qstride=1) -> BoxMeasure:
        out = np.zeros(9)
        lo, hi = _arr(lo), _arr(hi)
        self.lib.ls3_box(self.comp, C.byref(self.phi), self.grad, lo.ctypes.data_as(P), hi.ctypes.data_as(P), int(want_surface),
                         qlane, qstride, out.ctypes.data_as(P))
        return BoxMeasure(int(out[0]), float(out[1]), tuple(out[2:5]), float(out[5]), tuple(out[6:9]))

    def section(self, d, s, lo, hi) -> float:
        lo, hi = _arr(lo), _arr(hi)
        return self.lib.ls3_section(self.comp, C.byref(self.phi), self.grad, d, C.c_double(s), lo.ctypes.data_as(P),
                                    hi.ctypes.data_as(P), C.c_double(-1.0))


# ---- irregular boxes, in closed form ----------------------------------------------------------------------------------------------
# A body is described in coordinates X_d = (x_d - c_d) / a_d in which its critical sets {phi = 0, d phi / d x_a = 0} are circles
# (an axis-aligned scaling keeps "extreme along an axis" and "derivative along an axis vanishes").  A circle: (p, X_p, (centre
# over the two other axes, ascending), radius).

def _sphere_circles(a):
    return [(a, 0.0, (0.0, 0.0), 1.0)]


def _torus_circles(a, R=TORUS_R, r=TORUS_r):
    if a == 2:
        return [(2, 0.0, (0.0, 0.0), R + r), (2, 0.0, (0.0, 0.0), R - r)]
    # the plane x_a = 0 cuts the tube in two circles around (+-R, 0) in (the other horizontal axis, z); the top and bottom
    # circles of the torus, where the horizontal part of the gradient vanishes altogether
    return [(a, 0.0, (R, 0.0), r), (a, 0.0, (-R, 0.0), r), (2, r, (0.0, 0.0), R), (2, -r, (0.0, 0.0), R)]


class Shape:
    def __init__(self, kind, c, a=(1.0, 1.0, 1.0), R=TORUS_R, r=TORUS_r):
        self.kind, self.c, self.a, self.R, self.r = kind, tuple(c), tuple(a), R, r

    def grad(self, x):
        X = [(x[d] - self.c[d]) / self.a[d] for d in range(3)]
        if self.kind == "sphere":
            return [X[d] / self.a[d] for d in range(3)]         # up to the positive factor 1 / |X|
        rho = math.hypot(X[0], X[1])
        k = (rho - self.R) / rho if rho > 0.0 else 0.0
        return [k * X[0], k * X[1], X[2]]                       # up to a positive factor

    def circles(self, a):
        return _sphere_circles(a) if self.kind == "sphere" else _torus_circles(a, self.R, self.r)


def axis_order(g):
    """(u, v, w) as pg_geom_program3.h picks them from |grad phi| at the box centre (ties: the later axis)"""
    g = [abs(t) for t in g]
    v = 0
    if g[1] >= g[0]:
        v = 1
    if g[2] >= g[v]:
        v = 2
    a, b = (1 if v == 0 else 0), (1 if v == 2 else 2)
    u = a if g[a] > g[b] else b
    return u, v, (b if u == a else a)


def _circle_meets_rect(c, rad, lo, hi):
    dx = max(lo[0] - c[0], 0.0, c[0] - hi[0])
    dy = max(lo[1] - c[1], 0.0, c[1] - hi[1])
    far = max(math.hypot(x - c[0], y - c[1]) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]))
    return math.hypot(dx, dy) <= rad <= far


def irregular_box(shape: Shape, lo, hi) -> bool:
    cen = [0.5 * (lo[d] + hi[d]) for d in range(3)]
    u, v, w = axis_order(shape.grad(cen))
    Lo = [(lo[d] - shape.c[d]) / shape.a[d] for d in range(3)]
    Hi = [(hi[d] - shape.c[d]) / shape.a[d] for d in range(3)]
    for p, Xp, c2, rad in shape.circles(v):                    # d_v phi = 0 on the interface inside the box
        q = [d for d in range(3) if d != p]
        if Lo[p] <= Xp <= Hi[p] and _circle_meets_rect(c2, rad, [Lo[q[0]], Lo[q[1]]], [Hi[q[0]], Hi[q[1]]]):
            return True
    for p, Xp, c2, rad in shape.circles(u):                    # d_u phi = 0 on the trace of a face v = const, inside the box
        q = [d for d in range(3) if d != p]
        if not Lo[p] <= Xp <= Hi[p]:
            continue
        for v0 in (Lo[v], Hi[v]):
            if p == v:
                if Xp == v0 and _circle_meets_rect(c2, rad, [Lo[q[0]], Lo[q[1]]], [Hi[q[0]], Hi[q[1]]]):
                    return True
                continue
            o = q[1] if q[0] == v else q[0]                     # the circle's other in-plane axis
            cv, co = (c2[0], c2[1]) if q[0] == v else (c2[1], c2[0])
            s2 = rad * rad - (v0 - cv) ** 2
            if s2 < 0.0:
                continue
            for sg in (-1.0, 1.0):
                if Lo[o] <= co + sg * math.sqrt(s2) <= Hi[o]:
                    return True
    return False


def irregular_section(shape: Shape, d, s, lo, hi) -> bool:
    """the 2-D rule on the face {x_d = s} of the box: heights run along the in-plane axis with the larger derivative at the face's
    centre; irregular when that derivative vanishes on the interface inside the face"""
    cen = [0.5 * (lo[q] + hi[q]) for q in range(3)]
    cen[d] = s
    g = [abs(t) for t in shape.grad(cen)]
    a, b = (1 if d == 0 else 0), (1 if d == 2 else 2)
    v = a if g[a] > g[b] else b
    Lo = [(lo[q] - shape.c[q]) / shape.a[q] for q in range(3)]
    Hi = [(hi[q] - shape.c[q]) / shape.a[q] for q in range(3)]
    S = (s - shape.c[d]) / shape.a[d]
    for p, Xp, c2, rad in shape.circles(v):
        q = [t for t in range(3) if t != p]
        if p == d:
            if Xp == S and _circle_meets_rect(c2, rad, [Lo[q[0]], Lo[q[1]]], [Hi[q[0]], Hi[q[1]]]):
                return True
            continue
        if not Lo[p] <= Xp <= Hi[p]:
            continue
        o = q[1] if q[0] == d else q[0]
        cd, co = (c2[0], c2[1]) if q[0] == d else (c2[1], c2[0])
        s2 = rad * rad - (S - cd) ** 2
        if s2 >= 0.0 and any(Lo[o] <= co + sg * math.sqrt(s2) <= Hi[o] for sg in (-1.0, 1.0)):
            return True
    return False


def class_masks(shape: Shape, mesh, ref):
    """irregular-entry masks (cells, A_d, B_d, W_d) for the capacities `ref` (an oracle Capacity or a FixtureCase)"""
    n, L, x0 = mesh
    ext = tuple(k + 1 for k in n)
    M = int(np.prod(ext))
    nodes = [np.asarray(a, dtype=float) for a in po.Mesh(n, L, x0).nodes]
    ct = np.asarray(ref.cell_types)
    Cw = np.asarray(getattr(ref, "C_w", None) if hasattr(ref, "C_w") else ref.C_ω)
    cell = np.zeros(M, dtype=bool)
    idx = lambda i, j, k: (k * ext[1] + j) * ext[0] + i
    for k in range(n[2]):
        for j in range(n[1]):
            for i in range(n[0]):
                li = idx(i, j, k)
                if ct[li] == -1:
                    cell[li] = irregular_box(shape, [nodes[0][i], nodes[1][j], nodes[2][k]], [nodes[0][i + 1], nodes[1][j + 1], nodes[2][k + 1]])
    W = [np.zeros(M, dtype=bool) for _ in range(3)]
    A = [np.zeros(M, dtype=bool) for _ in range(3)]
    B = [np.zeros(M, dtype=bool) for _ in range(3)]
    for d in range(3):
        for k in range(n[2]):
            for j in range(n[1]):
                for i in range(n[0]):
                    I = [i, j, k]
                    li = idx(i, j, k)
                    if ct[li] == -1:
                        lo = [nodes[q][I[q]] for q in range(3)]
                        hi = [nodes[q][I[q] + 1] for q in range(3)]
                        B[d][li] = cell[li] or irregular_section(shape, d, Cw[li, d], lo, hi)
                        A[d][li] = irregular_section(shape, d, lo[d], lo, hi)
                        Iu = list(I)
                        Iu[d] += 1                              # the upper face is the lower face of the next entry
                        A[d][idx(*Iu)] = A[d][idx(*Iu)] or irregular_section(shape, d, hi[d], lo, hi)
                    if I[d] == 0:
                        continue
                    Ip = list(I)
                    Ip[d] -= 1
                    lp = idx(*Ip)
                    if ct[li] == 0 and ct[lp] == 0:
                        continue
                    lo = [nodes[q][I[q]] for q in range(3)]
                    hi = [nodes[q][I[q] + 1] for q in range(3)]
                    lo[d], hi[d] = Cw[lp, d], Cw[li, d]
                    W[d][li] = cell[li] or cell[lp] or ((ct[li] == -1 or ct[lp] == -1) and irregular_box(shape, lo, hi))
    return cell, A, B, W


# ---- comparisons ------------------------------------------------------------------------------------------------------------------

def _f(o, *names):
    for k in names:
        if hasattr(o, k):
            return getattr(o, k)
    raise AttributeError(names[0])


def diffs(got, ref, mesh, keep=None):
    """|got - ref| of every entry, normalised by a full cell / face / edge: {"V": (M,), "A": (3, M), ..., "Cw": (M,)}; `keep`: a mask
    of the entries `ref` holds (a sparse fixture)"""
    n, L, x0 = mesh
    h = min(Ld / nd for Ld, nd in zip(L, n))
    full = float(np.prod([Ld / nd for Ld, nd in zip(L, n)]))
    face = h * h
    Vr = np.asarray(_f(ref, "V"))
    out = {"V": np.abs(np.asarray(_f(got, "V")) - Vr) / full,
           "G": np.abs(np.asarray(_f(got, "G", "Γ")) - np.asarray(_f(ref, "G", "Γ"))) / face}
    for name in ("A", "B", "W"):
        scale = full if name == "W" else face
        out[name] = np.stack([np.abs(np.asarray(_f(got, name)[d]) - np.asarray(_f(ref, name)[d])) for d in range(3)]) / scale
    fluid = Vr > 1e-3 * full
    out["Cw"] = np.where(fluid, np.max(np.abs(np.asarray(_f(got, "C_w", "C_ω")) - np.asarray(_f(ref, "C_w", "C_ω"))), axis=1), 0.0) / h
    if hasattr(ref, "C_g") or hasattr(ref, "C_γ"):
        surf = fluid & (np.asarray(_f(ref, "G", "Γ")) > 1e-3 * face)
        out["Cg"] = np.where(surf, np.max(np.abs(np.asarray(_f(got, "C_g", "C_γ")) - np.asarray(_f(ref, "C_g", "C_γ"))), axis=1), 0.0) / h
    if keep is not None:
        for q in out:
            out[q] = np.where(keep, out[q], 0.0)
    return out


def worsts(d, cell_irr=None, A_irr=None, B_irr=None, W_irr=None):
    """(regular, irregular) worst of every quantity; without masks everything is regular"""
    reg, irr = {}, {}
    for q, a in d.items():
        if cell_irr is None:
            m = np.zeros(a.shape, dtype=bool)
        elif q == "W":
            m = np.stack(W_irr)
        elif q == "A":
            m = np.stack(A_irr)
        elif q == "B":
            m = np.stack(B_irr)
        else:
            m = cell_irr
        reg[q] = float(np.max(np.where(m, 0.0, a)))
        irr[q] = float(np.max(np.where(m, a, 0.0)))
    return reg, irr


def check(name, got, ref, mesh, shape=None, what="", keep=None):
    """print every figure, then hold each to its bar: regular entries in units of u to BARS[name], irregular ones as fractions
    of a cell / face / edge to BARS_IRREGULAR[name]"""
    n, L, x0 = mesh
    u, _ = unit(x0, L, n)
    cell_irr = A_irr = B_irr = W_irr = None
    if shape is not None:
        cell_irr, A_irr, B_irr, W_irr = class_masks(shape, mesh, ref)
    reg, irr = worsts(diffs(got, ref, mesh, keep), cell_irr, A_irr, B_irr, W_irr)
    reg = {q: v / u for q, v in reg.items()}
    print(f"[levelset3d {what}{name}] regular (u): " + "  ".join(f"{q} {reg[q]:.3g}/{BARS[name][q]:.3g}" for q in reg))
    bad = {q: (reg[q], BARS[name][q]) for q in reg if not reg[q] <= BARS[name][q]}
    if shape is not None:
        bars = BARS_IRREGULAR[name]
        ncut = int(np.sum(np.asarray(ref.cell_types) == -1))
        print(f"[levelset3d {what}{name}] irregular ({int(cell_irr.sum())} of {ncut} cut cells; fractions): "
              + "  ".join(f"{q} {irr[q]:.3g}/{bars[q]:.3g}" for q in irr))
        bad.update({q + " (irregular)": (irr[q], bars[q]) for q in irr if not irr[q] <= bars[q]})
    assert not bad, f"{name}: over the bar (measured, bar): {bad}"
    return reg, irr


# ---- the torus fixture ------------------------------------------------------------------------------------------------------------

class FixtureCase:
    """a sparse case: the listed entries of every field, 0 elsewhere, and `keep`, the mask of the listed entries"""

    def __init__(self, name, d):
        self.name = name
        self.n, self.L, self.x0 = tuple(d["n"]), tuple(d["L"]), tuple(d["x0"])
        self.complement = bool(d["complement"])
        M = int(np.prod([k + 1 for k in self.n]))
        self.cell_types = np.array(d["cell_types"], dtype=float)
        idx = np.array(d["index"], dtype=int)
        self.keep = np.zeros(M, dtype=bool)
        self.keep[idx] = True

        def dense(v):
            a = np.zeros(M)
            a[idx] = np.array([float(t) for t in v])
            return a
        self.V, self.G = dense(d["V"]), dense(d["G"])
        self.A, self.B, self.W = (tuple(dense(d[k][q]) for q in range(3)) for k in ("A", "B", "W"))
        self.C_w = np.stack([dense(d["C_w"][q]) for q in range(3)], axis=1)
        self.irregular = np.zeros(M, dtype=bool)
        self.irregular[np.array(d["irregular"], dtype=int)] = True


# The file holds only what cannot be derived: arrays are base64 of zlib-compressed little-endian float64 (cell types: int8).  Of the torus: V,
# Gamma, C_w, B on the cut cells, A and W on the stored cells (the cut cells and their upper neighbours).  Of the complement: C_w, B
# on the cut cells and W on the stored ones; its V = cell - V, its A = face - A, its Gamma and the flipped cell types follow from
# the torus.  A stored cell that is not cut has V = its volume or 0, C_w = its centre, B = its face or 0, by its type.
def _b64(a, dtype="<f8"):
    return base64.b64encode(zlib.compress(np.asarray(a, dtype=dtype).tobytes(), 9)).decode()


def _unb64(t, dtype="<f8"):
    return np.frombuffer(zlib.decompress(base64.b64decode(t)), dtype=dtype).astype(float)


def unpack_fixture(raw):
    """the dense case dictionaries FixtureCase reads, from the packed file"""
    n, L, x0 = raw["n"], raw["L"], raw["x0"]
    nodes = [np.asarray(a, dtype=float) for a in po.Mesh(tuple(n), tuple(L), tuple(x0)).nodes]
    ext = [k + 1 for k in n]
    ct0 = _unb64(raw["cell_types"], "i1")
    li = np.arange(len(ct0))
    real = (li % ext[0] < n[0]) & ((li // ext[0]) % ext[1] < n[1]) & (li // (ext[0] * ext[1]) < n[2])
    stored = np.array(raw["index"], dtype=int)
    pos = {int(li): q for q, li in enumerate(stored)}
    cutq = np.array([pos[int(li)] for li in np.flatnonzero(ct0 == -1)], dtype=int)
    I = [stored % ext[0], (stored // ext[0]) % ext[1], stored // (ext[0] * ext[1])]
    ext3 = [nodes[d][I[d] + 1] - nodes[d][I[d]] for d in range(3)]
    cen = [0.5 * (nodes[d][I[d]] + nodes[d][I[d] + 1]) for d in range(3)]
    full = ext3[0] * ext3[1] * ext3[2]
    face = [ext3[1] * ext3[2], ext3[0] * ext3[2], ext3[0] * ext3[1]]
    cases = {}
    for comp, name in ((False, "torus"), (True, "torus_complement")):
        r = raw[name]
        ct = np.where((ct0 == -1) | ~real, ct0, 1.0 - ct0) if comp else ct0          # (the padding layer stays 0)
        fluid = ct[stored] == 1

        def on_cut(packed, other):
            a = np.array(other, dtype=float)
            a[cutq] = _unb64(packed)
            return a
        if comp:
            t = cases["torus"]
            V, G = full - np.array(t["V"]), t["G"]
            V[~(ct[stored] == -1)] = np.where(fluid, full, 0.0)[~(ct[stored] == -1)]
            A = [face[d] - np.array(t["A"][d]) for d in range(3)]
        else:
            V, G = on_cut(r["V"], np.where(fluid, full, 0.0)), on_cut(r["G"], np.zeros(len(stored)))
            A = [_unb64(r["A"][d]) for d in range(3)]
        cases[name] = {"n": n, "L": L, "x0": x0, "complement": comp, "cell_types": ct, "index": stored, "V": V, "G": G, "A": A,
                       "B": [on_cut(r["B"][d], np.where(fluid, face[d], 0.0)) for d in range(3)],
                       "W": [_unb64(r["W"][d]) for d in range(3)],
                       "C_w": [on_cut(r["C_w"][d], cen[d]) for d in range(3)], "irregular": raw["irregular"]}
    return cases


def pack_fixture(cases, header):
    """the packed file for the dense case dictionaries the generator computes; what is left out must come back from
    unpack_fixture to 4 ulp of a cell, face or coordinate, or this raises"""
    t, c = cases["torus"], cases["torus_complement"]
    ct0 = np.array(t["cell_types"])
    cutq = np.flatnonzero(ct0[np.array(t["index"])] == -1)
    sub = lambda v: _b64(np.array(v, dtype=float)[cutq])
    raw = dict(header, n=t["n"], L=t["L"], x0=t["x0"], cell_types=_b64(ct0, "i1"), index=[int(i) for i in t["index"]],
               irregular=t["irregular"],
               torus={"V": sub(t["V"]), "G": sub(t["G"]), "C_w": [sub(v) for v in t["C_w"]], "B": [sub(v) for v in t["B"]],
                      "A": [_b64(v) for v in t["A"]], "W": [_b64(v) for v in t["W"]]},
               torus_complement={"C_w": [sub(v) for v in c["C_w"]], "B": [sub(v) for v in c["B"]], "W": [_b64(v) for v in c["W"]]})
    back = unpack_fixture(raw)
    for name, want in cases.items():
        assert np.array_equal(back[name]["cell_types"], np.array(want["cell_types"], dtype=float)), name
        for k in ("V", "G"):
            assert np.max(np.abs(back[name][k] - np.array(want[k], dtype=float))) <= 4 * 2.0 ** -52 * 0.04, (name, k)
        for k, scale in (("A", 0.12), ("B", 0.12), ("W", 0.04), ("C_w", 4.0)):
            for d in range(3):
                assert np.max(np.abs(back[name][k][d] - np.array(want[k][d], dtype=float))) <= 4 * 2.0 ** -52 * scale, (name, k, d)
    return raw


def load_fixture():
    raw = json.loads(FIXTURE.read_text())
    return {k: FixtureCase(k, v) for k, v in unpack_fixture(raw).items()}


# ---- bars -------------------------------------------------------------------------------------------------------------------------
# MEASURED: the worst of each quantity over the REGULAR entries, in units of u, of the HOST build (g++ -O2 -ffp-contract=off,
# glibc's libm) against the arbiter named (tests/test_levelset3d_host.py prints them again); the bar is 10 times that, the 10 for
# the device's libm, and the GPU is held to the same bar.
#   plane: tests/plane_oracle.py (exact clipping), 0.6 x - 0.64 y + 0.48 z - 0.37 on 9 x 8 x 7 over a shifted box, both phases, and
#     x - 1.75 (a node plane: the nodes are x0 + (j + 1/2) h) on 8^3.  phi is linear: every integrand is a piecewise polynomial between the breakpoints
#   ball, ellipsoid: oracle.geometry.Ball / Ellipsoid at 8^3, 12^3, 16^3 through .box and .section
#   torus, torus_complement: tests/golden/levelset3d_cells.json (mpmath, 30 digits)
# MEASURED_IRREGULAR: the worst over the irregular entries, as a fraction of a cell (V, W), a face (A, B, G) or h (Cw, Cg).
MEASURED = {
    "plane": {"V": 1.26, "G": 3.55, "A": 0.621, "B": 1.48, "W": 1.34, "Cw": 0.811, "Cg": 1.62},
    "ball": {"V": 1390.0, "G": 195000.0, "A": 4580.0, "B": 92300.0, "W": 1370.0, "Cw": 1470.0, "Cg": 233000.0},
    "ellipsoid": {"V": 1020.0, "G": 95600.0, "A": 1840.0, "B": 9190.0, "W": 5440000.0, "Cw": 1550.0, "Cg": 66700.0},
    "torus": {"V": 134000.0, "G": 26500000.0, "A": 811000.0, "B": 471000.0, "W": 123000.0, "Cw": 117000.0},
    "torus_complement": {"V": 134000.0, "G": 26500000.0, "A": 811000.0, "B": 1100000.0, "W": 275000.0, "Cw": 942000.0},
}
# (ball and torus: no entry of these meshes is irregular, the bars are 0 and nothing is held to them; the ellipsoid has two
# irregular cells at 8^3, next to the ends of its short axis, where a face's slice of the body is narrower than the cell)
_NONE = {"V": 0.0, "G": 0.0, "A": 0.0, "B": 0.0, "W": 0.0, "Cw": 0.0, "Cg": 0.0}
MEASURED_IRREGULAR = {
    "ball": dict(_NONE),
    "ellipsoid": {"V": 1.68e-06, "G": 0.000637, "A": 0.000608, "B": 0.00099, "W": 5.46e-06, "Cw": 3.49e-05, "Cg": 0.000563},
    # (no cell of the torus is irregular; a few staggered boxes are, and are at rounding level all the same)
    "torus": dict(_NONE, W=4.68e-17),
    "torus_complement": dict(_NONE, W=1.31e-15),
}
BARS = {name: {q: 10.0 * v for q, v in m.items()} for name, m in MEASURED.items()}
# the cap of an irregular cell: a 16-node rule across an interior (w - w*)^(3/2) singularity leaves about 16^(-5/2) ~ 1e-3 of the
# piece; 1e-2 of a cell for V and W and 4e-2 of a face for the interface, the order of the 2-D kind's KINK_ABS
IRREGULAR_CAP = {"V": 1e-2, "W": 1e-2, "G": 4e-2}
BARS_IRREGULAR = {name: {q: min(10.0 * v, IRREGULAR_CAP.get(q, math.inf)) for q, v in m.items()} for name, m in MEASURED_IRREGULAR.items()}
# the host's worst V error in regular cells stays below this fraction of a cell: more means a missed breakpoint
REGULAR_V_MAX = 1e-9
IRREGULAR_SHARE_MAX = 0.2
