"""CPU arbiter and host restatement for MOVING marker polygons (MovingPoly of penguin/jl_amd/csrc/pg_geom_polygon.h,
pg_capacity_create_spacetime_polygon) -- test infrastructure only.

  MovingPolygonArbiter   a duck-typed moving body for oracle.spacetime.make_spacetime_capacity: `.at(t)` is the exact rational
                         tests/polygon_reference.PolygonBody of the polygon's FLOAT vertices at t.  Those are computed by the
                         product's own expression in numpy -- p0 + s (p1 - p0), s = (t - t0) / (t1 - t0), and p0 / p1 themselves
                         at the two faces -- so they are the product's bits, and everything after them is exact.  It arbitrates
                         V, A, B, W, C_w, the cell types, Vn_1 and Vn.
  arbiter_front          Gamma and C_gamma (with its time component) by the per-piece rule, on exact pieces: Gamma = sum_k w_k
                         sum_pieces len_p sqrt(1 + v_n,p^2) over the pieces a cell owns at tau_k (midpoint lo <= m < hi), v_n,p =
                         u(m) . n with u(m) = u_p + lambda (u_q - u_p), u_i = (p1_i - p0_i) / (t1 - t0) and n the edge's unit
                         normal at tau_k; one square root per piece in mpmath at 30 digits.
  product_rule           make_spacetime_capacity builds its own composite rule; inside this context it gets the product's
                         (penguin.jl_amd.moving.time_rule: the same nodes, the weights scaled to add up to t1 - t0), so that the
                         arbiter integrates exactly the sum the product integrates.
  host_slab_capacity     the six k_st_* kernels of pg_capacity.hip restated on the host build's primitives
                         (tests/spacetime_polygon_host.cpp), with the kernels' order of summation: lane l of a wave adds the nodes
                         l, l + 64, ... in turn and the 64 partial sums go through the butterfly of wave_add.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from fractions import Fraction as Fr

import mpmath as mp
import numpy as np

from oracle import penguin_oracle as po
from oracle import spacetime as ost
from oracle.geometry import CUT, EMPTY, FULL
from tests.polygon_reference import PolygonBody, _mpf

P = C.POINTER(C.c_double)


def time_rule(t0, t1, panels, order):
    """penguin.jl_amd.moving.time_rule, restated"""
    x, w = np.polynomial.legendre.leggauss(order)
    edges = np.linspace(t0, t1, panels + 1)
    tau = np.concatenate([0.5 * (a + b) + 0.5 * (b - a) * x for a, b in zip(edges[:-1], edges[1:])])
    wt = np.concatenate([0.5 * (b - a) * w for a, b in zip(edges[:-1], edges[1:])])
    return tau, wt * ((t1 - t0) / wt.sum())


@contextlib.contextmanager
def product_rule():
    keep = ost.composite_gauss
    ost.composite_gauss = time_rule
    try:
        yield
    finally:
        ost.composite_gauss = keep


def normalise(p0, p1):
    """the markers the kernels see: the closing duplicate dropped where both arrays close, both reversed about the first marker
    if the signed area at t0 is negative (exact)"""
    p0, p1 = np.asarray(p0, dtype=float).reshape(-1, 2), np.asarray(p1, dtype=float).reshape(-1, 2)
    assert p0.shape == p1.shape
    if len(p0) >= 2 and np.array_equal(p0[0], p0[-1]) and np.array_equal(p1[0], p1[-1]):
        p0, p1 = p0[:-1], p1[:-1]
    ex = [(Fr(x), Fr(y)) for x, y in p0]
    area2 = sum(ex[k][0] * ex[(k + 1) % len(ex)][1] - ex[(k + 1) % len(ex)][0] * ex[k][1] for k in range(len(ex)))
    if area2 < 0:
        p0, p1 = np.concatenate([p0[:1], p0[:0:-1]]), np.concatenate([p1[:1], p1[:0:-1]])
    return np.ascontiguousarray(p0), np.ascontiguousarray(p1)


class MovingPolygonArbiter:
    def __init__(self, p0, p1, t0, t1, complement=False):
        self.p0, self.p1 = normalise(p0, p1)
        self.t0, self.t1, self.complement = float(t0), float(t1), bool(complement)
        self._at = {}

    def vertices(self, t):
        """the product's float vertices at t; the faces by identity, not by s"""
        if t == self.t0:
            return self.p0
        if t == self.t1:
            return self.p1
        s = (t - self.t0) / (self.t1 - self.t0)
        return self.p0 + s * (self.p1 - self.p0)

    def at(self, t) -> PolygonBody:
        t = float(t)
        if t not in self._at:
            body = PolygonBody([tuple(r) for r in self.vertices(t)], self.complement)
            assert np.array_equal(body.P, self.vertices(t)), "the orientation changed inside the slab"
            self._at[t] = body
        return self._at[t]

    def normal_speed(self, t, cg, h):
        return 0.0                       # (make_spacetime_capacity's Gamma is not read: arbiter_front has the per-piece rule)


def slab_reference(arb: MovingPolygonArbiter, mesh: po.Mesh, panels, order):
    with product_rule():
        return ost.make_spacetime_capacity(arb, mesh, arb.t0, arb.t1, panels=panels, order=order)


def arbiter_front(arb: MovingPolygonArbiter, mesh: po.Mesh, tau, wt):
    """(G, C_g) on the padded grid: C_g is (M, 3), the time component last; zero where a cell owns nothing"""
    n, ext, nodes = mesh.dims, mesh.ext, mesh.nodes
    M = int(np.prod(ext))
    G, Cg = np.zeros(M), np.zeros((M, 3))
    dt = Fr(arb.t1) - Fr(arb.t0)
    U = [((Fr(b[0]) - Fr(a[0])) / dt, (Fr(b[1]) - Fr(a[1])) / dt) for a, b in zip(arb.p0, arb.p1)]
    acc = {}
    for k, (t, w) in enumerate(zip(tau, wt)):
        body = arb.at(float(t))
        Pm, Q, Mk = body.P, body.Q, body.M
        for j in range(n[1]):
            for i in range(n[0]):
                lo, hi = (float(nodes[0][i]), float(nodes[1][j])), (float(nodes[0][i + 1]), float(nodes[1][j + 1]))
                near = np.flatnonzero((np.maximum(Pm[:, 0], Q[:, 0]) >= lo[0]) & (np.minimum(Pm[:, 0], Q[:, 0]) <= hi[0]) &
                                      (np.maximum(Pm[:, 1], Q[:, 1]) >= lo[1]) & (np.minimum(Pm[:, 1], Q[:, 1]) <= hi[1]))
                if not len(near):
                    continue
                Lo, Hi = (Fr(lo[0]), Fr(lo[1])), (Fr(hi[0]), Fr(hi[1]))
                for e in near:
                    p, q = body.ex[e], body.ex[(e + 1) % Mk]
                    a0, a1, ok = Fr(0), Fr(1), True
                    for ax in (0, 1):
                        dl = q[ax] - p[ax]
                        for pp, qq in ((-dl, p[ax] - Lo[ax]), (dl, Hi[ax] - p[ax])):
                            if pp == 0:
                                ok = ok and qq >= 0
                            elif pp < 0:
                                a0 = max(a0, qq / pp)
                            else:
                                a1 = min(a1, qq / pp)
                    if not (ok and a1 > a0):
                        continue
                    lam = (a0 + a1) / 2
                    dx, dy = q[0] - p[0], q[1] - p[1]
                    m = (p[0] + lam * dx, p[1] + lam * dy)
                    if not (Lo[0] <= m[0] < Hi[0] and Lo[1] <= m[1] < Hi[1]):
                        continue
                    up, uq = U[e], U[(e + 1) % Mk]
                    ux, uy = up[0] + lam * (uq[0] - up[0]), up[1] + lam * (uq[1] - up[1])
                    vn2 = (ux * dy - uy * dx) ** 2 / (dx * dx + dy * dy)
                    len2 = (a1 - a0) ** 2 * (dx * dx + dy * dy)
                    ws = mp.mpf(float(w)) * mp.sqrt(_mpf(len2 * (1 + vn2)))
                    li = j * ext[0] + i
                    s = acc.setdefault(li, [mp.mpf(0)] * 4)
                    acc[li] = [s[0] + ws, s[1] + ws * _mpf(m[0]), s[2] + ws * _mpf(m[1]), s[3] + ws * mp.mpf(float(t))]
    for li, s in acc.items():
        G[li] = float(s[0])
        Cg[li] = [float(s[1] / s[0]), float(s[2] / s[0]), float(s[3] / s[0])]
    return G, Cg


# ---- the host build, with the kernels' slab rule ---------------------------------------------------------------------------------------

def _arr(v):
    return np.ascontiguousarray(v, dtype=float)


def host_new(lib, p0, p1, mesh, t0, t1, tau, wt, complement=False):
    """(handle or None, message)"""
    a, b = _arr(np.asarray(p0, dtype=float).reshape(-1)), _arr(np.asarray(p1, dtype=float).reshape(-1))
    tw = _arr(np.column_stack([tau, wt]))
    msg = C.create_string_buffer(512)
    h = lib.stp_new(a.ctypes.data_as(P), b.ctypes.data_as(P), C.c_int64(len(a) // 2), int(bool(complement)), int(mesh.dims[0]),
                    int(mesh.dims[1]), _arr(mesh.nodes[0]).ctypes.data_as(P), _arr(mesh.nodes[1]).ctypes.data_as(P), C.c_double(t0),
                    C.c_double(t1), len(tau), tw.ctypes.data_as(P), msg, 512)
    return h, msg.value.decode()


def wave_add(terms):
    """what lane 0 holds after wave_add (pg_capacity.hip): lane l has added terms[l], terms[l + 64], ... in turn"""
    part = np.zeros(64)
    for k, v in enumerate(terms):
        part[k % 64] += v
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        part = part + part[lanes ^ off]
    return float(part[0])


class HostSlab:
    """the host build of one slab: boxes and sections at a slot (a node index k, or "t0" / "t1")"""

    def __init__(self, lib, p0, p1, mesh, L, t0, t1, tau, wt, complement=False):
        self.lib, self.mesh, self.t0, self.t1 = lib, mesh, float(t0), float(t1)
        self.tau, self.wt = np.asarray(tau, dtype=float), np.asarray(wt, dtype=float)
        h, why = host_new(lib, p0, p1, mesh, t0, t1, tau, wt, complement)
        assert h, why
        self.h = C.c_void_p(h)
        self.s = (self.tau - self.t0) / (self.t1 - self.t0)
        self.spacing = tuple(float(L[d]) / mesh.dims[d] for d in range(2))

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.stp_free(self.h)

    def _slot(self, k):
        return (1, 0.0) if k == "t0" else (2, 0.0) if k == "t1" else (0, float(self.s[k]))

    def box(self, k, lo, hi, want_surface=True):
        out = np.zeros(9)
        kind, s = self._slot(k)
        lo, hi = _arr(list(lo) + [0.0]), _arr(list(hi) + [0.0])
        self.lib.stp_box(self.h, kind, C.c_double(s), lo.ctypes.data_as(P), hi.ctypes.data_as(P), int(want_surface), out.ctypes.data_as(P))
        return out

    def section(self, k, d, x, lo, hi):
        kind, s = self._slot(k)
        lo, hi = _arr(list(lo) + [0.0]), _arr(list(hi) + [0.0])
        return self.lib.stp_section(self.h, kind, C.c_double(s), d, C.c_double(x), lo.ctypes.data_as(P), hi.ctypes.data_as(P),
                                    C.c_double(self.spacing[1 - d]))

    def far(self, i, j):
        return self.lib.stp_far(self.h, i, j)


class SlabFields:
    """the first time layer in the names tests.spacetime_program_reference.Layer gives a product capacity"""

    def __init__(self, M):
        self.V, self.G, self.cell_types = np.zeros(M), np.zeros(M), np.zeros(M)
        self.A, self.B, self.W = (tuple(np.zeros(M) for _ in range(2)) for _ in range(3))
        self.Vn_1, self.Vn = np.zeros(M), np.zeros(M)
        self.C_w_st, self.C_g_st = np.zeros((M, 3)), np.zeros((M, 3))
        self.listed = 0

    @property
    def C_w(self):
        return self.C_w_st[:, :2]

    @property
    def C_g(self):
        return self.C_g_st[:, :2]


def host_slab_capacity(hs: HostSlab, cheap_pass=True) -> SlabFields:
    """k_st_classify, k_st_cells, k_st_sections(_cut), k_st_stagger(_cut) of pg_capacity.hip for StPoly, statement by statement.
    cheap_pass=False: every cell goes through k_st_cells (the all-nodes rule)."""
    mesh = hs.mesh
    n, ext, nodes = mesh.dims, mesh.ext, [np.asarray(x, dtype=float) for x in mesh.nodes]
    M = int(np.prod(ext))
    o = SlabFields(M)
    t0, t1, tau, wt = hs.t0, hs.t1, hs.tau, hs.wt
    dt = t1 - t0
    nq = len(tau)
    hfull = hs.spacing[0] * hs.spacing[1]
    fm = (hs.spacing[1], hs.spacing[0])                      # full_measure(g, d): the spacing of the other axis

    def plain(li, lo, hi, fluid):
        o.C_w_st[li] = [0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), 0.5 * (t0 + t1)]
        if fluid:
            o.V[li], o.Vn_1[li], o.Vn[li], o.cell_types[li] = hfull * dt, hfull, hfull, FULL

    for j in range(n[1]):
        for i in range(n[0]):
            li = j * ext[0] + i
            lo, hi = (nodes[0][i], nodes[1][j]), (nodes[0][i + 1], nodes[1][j + 1])
            far = hs.far(i, j) if cheap_pass else 0
            if far != 0:
                plain(li, lo, hi, far == 1)
                continue
            o.listed += 1
            faces = [hs.box(k, lo, hi, False) for k in ("t0", "t1")]
            vend = [hfull if int(m[0]) == FULL else m[1] for m in faces]
            types = {int(m[0]) for m in faces}
            v, momt, gam, gmt = [], [], [], []
            mom, gm = ([], []), ([], [])
            for k in range(nq):
                m = hs.box(k, lo, hi, True)
                types.add(int(m[0]))
                wv = wt[k] * m[1]
                v.append(wv)
                momt.append(wv * tau[k])
                for d in range(2):
                    mom[d].append(wv * m[2 + d])
                ws = wt[k] * m[5] * np.sqrt(1.0 + 0.0 * 0.0) if m[5] > 0.0 else 0.0
                gam.append(ws)
                gmt.append(ws * tau[k])
                for d in range(2):
                    gm[d].append(ws * m[6 + d] if m[5] > 0.0 else 0.0)
            V, Gm, Mt, Gt = wave_add(v), wave_add(gam), wave_add(momt), wave_add(gmt)
            Mo, Go = [wave_add(mom[d]) for d in range(2)], [wave_add(gm[d]) for d in range(2)]
            if types == {FULL} or types == {EMPTY}:
                plain(li, lo, hi, types == {FULL})
                if Gm > 0.0:
                    o.G[li] = Gm
                    o.C_g_st[li] = [Go[0] / Gm, Go[1] / Gm, Gt / Gm]
                continue
            o.cell_types[li], o.V[li], o.G[li], o.Vn_1[li], o.Vn[li] = CUT, V, Gm, vend[0], vend[1]
            o.C_w_st[li] = [Mo[0] / V, Mo[1] / V, Mt / V] if V > 0.0 else [0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), 0.5 * (t0 + t1)]
            if Gm > 0.0:
                o.C_g_st[li] = [Go[0] / Gm, Go[1] / Gm, Gt / Gm]

    ct = o.cell_types
    stride = (1, ext[0])
    for jj in range(ext[1]):
        for ii in range(ext[0]):
            lc = jj * ext[0] + ii
            idx = (ii, jj)
            real = ii < n[0] and jj < n[1]
            for d in range(2):
                if idx[1 - d] >= n[1 - d]:
                    continue
                cl = [min(idx[k], n[k] - 1) for k in range(2)]
                lo, hi = (nodes[0][cl[0]], nodes[1][cl[1]]), (nodes[0][cl[0] + 1], nodes[1][cl[1] + 1])
                # ---- A_d, B_d
                t = float(CUT)
                if real:
                    t = ct[lc]
                elif idx[d] >= n[d] and lc - stride[d] >= 0:
                    t = ct[lc - stride[d]]
                if t == FULL:
                    o.A[d][lc] = fm[d] * dt
                    o.B[d][lc] = o.A[d][lc] if real else 0.0
                elif t != EMPTY:
                    sa = [hs.section(k, d, nodes[d][idx[d]], lo, hi) for k in range(nq)]
                    a = wave_add([wt[k] * sa[k] for k in range(nq)])
                    if all(x == fm[d] for x in sa):
                        a = fm[d] * dt
                    b = 0.0
                    if real:
                        sb = [hs.section(k, d, o.C_w_st[lc, d], lo, hi) for k in range(nq)]
                        b = wave_add([wt[k] * sb[k] for k in range(nq)])
                        if all(x == fm[d] for x in sb):
                            b = fm[d] * dt
                    o.A[d][lc], o.B[d][lc] = a, b
                # ---- W_d
                ip, inx = max(idx[d] - 1, 0), min(idx[d], n[d] - 1)
                lp, ln = lc + (ip - idx[d]) * stride[d], lc + (inx - idx[d]) * stride[d]
                if ip == inx or (ct[lp] == 0.0 and ct[ln] == 0.0):
                    continue
                if not o.C_w_st[ln, d] - o.C_w_st[lp, d] > 0.0:
                    continue
                if ct[lp] == 1.0 and ct[ln] == 1.0:
                    o.W[d][lc] = hfull * dt
                    continue
                wlo, whi = [0.0, 0.0], [0.0, 0.0]
                wlo[1 - d], whi[1 - d] = nodes[1 - d][idx[1 - d]], nodes[1 - d][idx[1 - d] + 1]
                wlo[d], whi[d] = o.C_w_st[lp, d], o.C_w_st[ln, d]
                o.W[d][lc] = wave_add([wt[k] * hs.box(k, wlo, whi, False)[1] for k in range(nq)])
    return o
