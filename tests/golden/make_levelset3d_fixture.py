"""Writes tests/golden/levelset3d_cells.json: the capacities of a torus (axis along z, centre off the nodes, R = 1.2, r = 0.5) and
of its complement on the 12^3 mesh over [0, 4]^3, with mpmath at 30 digits.  Independent of the product's geometry code:

  every horizontal section of the torus is an annulus, so the area of {z = const} /\\ box and its moments are differences of
  disc /\\ rectangle closed forms (oracle.geometry.disc_rect restated in mpmath below); V, C_w and W are one tanh-sinh integral of
  those in z, between the breakpoints where a circle of the annulus passes a corner or touches a side of the rectangle (roots of
  quadratics).  A face x = const or y = const is one integral in z of interval lengths, a face z = const is closed form.  Gamma
  is one integral of arc lengths times r / s(z), the surface element of the surface of revolution rho = R +- s(z).

Only the cut cells and their upper neighbours (whose A, B, W reach one cell down) are stored; `irregular` lists the cut cells
tests/levelset3d_cases.irregular_box flags, and the share is printed: it must stay below 20 %.

    python tests/golden/make_levelset3d_fixture.py        (a few minutes on 8 cores)"""
import json
import multiprocessing as mpc
import sys
from pathlib import Path

import mpmath as mp

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from oracle import penguin_oracle as po  # noqa: E402
from tests import levelset3d_cases as lc  # noqa: E402

mp.mp.dps = 30
N_MESH, L_MESH, X0 = lc.TORUS_MESH
C3 = [mp.mpf(c) for c in lc.TORUS_C]                            # the doubles the programs hold, exactly
R, r = mp.mpf(lc.TORUS_R), mp.mpf(lc.TORUS_r)
NODES = [[mp.mpf(float(x)) for x in a] for a in po.Mesh(N_MESH, L_MESH, X0).nodes]      # the doubles the product sees, exactly
EXT = tuple(k + 1 for k in N_MESH)
ZERO = mp.mpf(0)


def lin(i, j, k):
    return (k * EXT[1] + j) * EXT[0] + i


# ---- disc(rho) /\ rectangle, about the disc's centre (oracle.geometry._P, _Q, _q, disc_rect) ------------------------------------
def _P(rho, u):
    s2 = (rho - u) * (rho + u)
    s = mp.sqrt(s2) if s2 > 0 else ZERO
    return (u * s + rho * rho * mp.atan2(u, s)) / 2


def _Q(rho, a, b):
    a, b = min(a, rho), min(b, rho)
    if a <= 0 or b <= 0:
        return ZERO, ZERO, ZERO
    r2 = rho * rho
    if a * a + b * b <= r2:
        return a * b, a * a * b / 2, a * b * b / 2
    xb, yb = mp.sqrt(max(r2 - b * b, ZERO)), mp.sqrt(max(r2 - a * a, ZERO))
    area = b * xb + (_P(rho, a) - _P(rho, xb))
    mx = b * xb * xb / 2 + (b ** 3 - yb ** 3) / 3
    my = b * b * xb / 2 + (r2 * (a - xb) - (a ** 3 - xb ** 3) / 3) / 2
    return area, mx, my


def _q(rho, x, y):
    ar, mx, my = _Q(rho, abs(x), abs(y))
    sx, sy = (1 if x >= 0 else -1), (1 if y >= 0 else -1)
    return sx * sy * ar, sy * mx, sx * my


def disc_rect(rho, a, b, t0, t1):
    if rho <= 0 or b <= a or t1 <= t0:
        return ZERO, ZERO, ZERO
    f = [_q(rho, b, t1), _q(rho, a, t1), _q(rho, b, t0), _q(rho, a, t0)]
    return tuple(f[0][i] - f[1][i] - f[2][i] + f[3][i] for i in range(3))


def circle_angle(rho, a, b, t0, t1):
    """the total angle of the circle of radius rho (about the origin) inside [a, b] x [t0, t1]"""
    cand = []
    for xv in (a, b):
        if -rho < xv < rho:
            al = mp.acos(xv / rho)
            cand += [al, -al]
    for yv in (t0, t1):
        if -rho < yv < rho:
            al = mp.asin(yv / rho)
            cand += [al, (mp.pi - al) if al >= 0 else (-mp.pi - al)]

    def inside(t):
        return a <= rho * mp.cos(t) <= b and t0 <= rho * mp.sin(t) <= t1
    if not cand:
        return 2 * mp.pi if inside(mp.mpf("0.3")) else ZERO
    cand = sorted(set(cand))
    tot = ZERO
    for k in range(len(cand)):
        p1 = cand[k]
        p2 = cand[(k + 1) % len(cand)] + (2 * mp.pi if k == len(cand) - 1 else 0)
        if p2 > p1 and inside((p1 + p2) / 2):
            tot += p2 - p1
    return tot


def z_breaks(z0, z1, dists):
    """z0, z1 and, between them, every z at which a circle of the annulus has one of the radii `dists`, and the ends of the tube"""
    pts = {z0, z1}
    for d in list(dists) + [R]:                      # (d = R: s = 0, the top and bottom of the tube ... handled by +- r below)
        e = r * r - (d - R) ** 2
        if e >= 0:
            for sg in (-1, 1):
                z = C3[2] + sg * mp.sqrt(e)
                if z0 < z < z1:
                    pts.add(z)
    for sg in (-1, 1):
        z = C3[2] + sg * r
        if z0 < z < z1:
            pts.add(z)
    return sorted(pts)


def tube_s(z):
    e = r * r - (z - C3[2]) ** 2
    return mp.sqrt(e) if e > 0 else None


def box_moments(lo, hi, surface=False):
    """V, Mx, My, Mz about the origin (and Gamma) of torus /\\ box"""
    a, b, t0, t1 = lo[0] - C3[0], hi[0] - C3[0], lo[1] - C3[1], hi[1] - C3[1]
    dists = [mp.hypot(x, y) for x in (a, b) for y in (t0, t1)] + [abs(a), abs(b), abs(t0), abs(t1)]
    pts = z_breaks(lo[2], hi[2], dists)
    memo = {}

    def sec(z):
        if z not in memo:
            s = tube_s(z)
            if s is None:
                memo[z] = (ZERO, ZERO, ZERO)
            else:
                o, i = disc_rect(R + s, a, b, t0, t1), disc_rect(R - s, a, b, t0, t1)
                memo[z] = tuple(o[q] - i[q] for q in range(3))
        return memo[z]
    V = mp.quad(lambda z: sec(z)[0], pts)
    Mx = mp.quad(lambda z: sec(z)[1], pts) + C3[0] * V
    My = mp.quad(lambda z: sec(z)[2], pts) + C3[1] * V
    Mz = mp.quad(lambda z: z * sec(z)[0], pts)
    G = ZERO
    if surface:
        def arc(z):
            s = tube_s(z)
            if s is None:
                return ZERO
            return ((R + s) * circle_angle(R + s, a, b, t0, t1) + (R - s) * circle_angle(R - s, a, b, t0, t1)) * (r / s)
        G = mp.quad(arc, pts)
    return V, Mx, My, Mz, G


def section(d, s, lo, hi):
    """the area of torus /\\ {x_d = s} /\\ box"""
    if d == 2:
        t = tube_s(s)
        if t is None:
            return ZERO
        a, b, t0, t1 = lo[0] - C3[0], hi[0] - C3[0], lo[1] - C3[1], hi[1] - C3[1]
        return disc_rect(R + t, a, b, t0, t1)[0] - disc_rect(R - t, a, b, t0, t1)[0]
    o = 1 - d
    X, y0, y1 = s - C3[d], lo[o] - C3[o], hi[o] - C3[o]

    def chord(rho):
        e = rho * rho - X * X
        if e <= 0:
            return ZERO
        c = mp.sqrt(e)
        return max(min(y1, c) - max(y0, -c), ZERO)
    pts = z_breaks(lo[2], hi[2], [mp.hypot(X, y0), mp.hypot(X, y1), abs(X)])

    def f(z):
        t = tube_s(z)
        return ZERO if t is None else chord(R + t) - chord(R - t)
    return mp.quad(f, pts)


def cell_box(i, j, k):
    return [NODES[0][i], NODES[1][j], NODES[2][k]], [NODES[0][i + 1], NODES[1][j + 1], NODES[2][k + 1]]


def cell_type(i, j, k):
    """exact: phi = hypot(rho - R, z) - r over a box takes the values between those of the nearest and farthest (|rho - R|, |z|)"""
    lo, hi = cell_box(i, j, k)

    def rng(a, b):                                   # min and max of |t| over [a, b]
        return (ZERO if a <= 0 <= b else min(abs(a), abs(b))), max(abs(a), abs(b))
    (xm, xM), (ym, yM) = rng(lo[0] - C3[0], hi[0] - C3[0]), rng(lo[1] - C3[1], hi[1] - C3[1])
    pm, pM = mp.hypot(xm, ym), mp.hypot(xM, yM)
    tm, tM = rng(pm - R, pM - R)
    zm, zM = rng(lo[2] - C3[2], hi[2] - C3[2])
    if mp.hypot(tM, zM) <= r:
        return 1
    if mp.hypot(tm, zm) >= r:
        return 0
    return -1


def prod(lo, hi, skip=-1):
    p = mp.mpf(1)
    for d in range(3):
        if d != skip:
            p *= hi[d] - lo[d]
    return p


def stage1(I):
    lo, hi = cell_box(*I)
    return I, box_moments(lo, hi, surface=True)


def stage2(job):
    kind, I, d, comp, lo, hi, s = job
    if kind == "B":
        v = section(d, s, lo, hi)
        return kind, I, d, comp, (prod(lo, hi, d) - v if comp else v)
    v = box_moments(lo, hi)[0] if hi[d] > lo[d] else ZERO
    return kind, I, d, comp, (prod(lo, hi) - v if comp and hi[d] > lo[d] else v)


def main():
    n = N_MESH
    M = EXT[0] * EXT[1] * EXT[2]
    types = {(i, j, k): cell_type(i, j, k) for k in range(n[2]) for j in range(n[1]) for i in range(n[0])}
    cut = [I for I, t in types.items() if t == -1]
    stored = set(cut)
    for I in cut:
        for d in range(3):
            J = list(I)
            J[d] += 1
            if J[d] < n[d]:
                stored.add(tuple(J))
    stored = sorted(stored, key=lambda I: lin(*I))
    print(f"{len(cut)} cut cells, {len(stored)} stored", flush=True)
    with mpc.Pool() as pool:
        mom = dict(pool.map(stage1, cut, chunksize=4))
        cases = {}
        V, Cw, G = ({False: {}, True: {}} for _ in range(3))
        for I, t in types.items():
            lo, hi = cell_box(*I)
            full, cen = prod(lo, hi), [(lo[d] + hi[d]) / 2 for d in range(3)]
            for comp in (False, True):
                tt = t if t == -1 else (1 - t if comp else t)
                if t == -1:
                    v, mx, my, mz, g = mom[I]
                    if comp:
                        v, mx, my, mz = full - v, full * cen[0] - mx, full * cen[1] - my, full * cen[2] - mz
                    V[comp][I], Cw[comp][I], G[comp][I] = v, [mx / v, my / v, mz / v], g
                else:
                    V[comp][I], Cw[comp][I], G[comp][I] = (full if tt == 1 else ZERO), cen, ZERO
        jobs = []
        for I in stored:
            lo, hi = cell_box(*I)
            for comp in (False, True):
                for d in range(3):
                    if types[I] == -1:
                        jobs.append(("B", I, d, comp, lo, hi, Cw[comp][I][d]))
                    J = list(I)
                    J[d] -= 1
                    J = tuple(J)
                    if J[d] >= 0 and (types[I] == -1 or types[J] == -1):
                        wl, wh = list(lo), list(hi)
                        wl[d], wh[d] = Cw[comp][J][d], Cw[comp][I][d]
                        jobs.append(("W", I, d, comp, wl, wh, None))
        for I in stored:                                   # the lower faces, once (the complement is the rest of the face)
            lo, hi = cell_box(*I)
            for d in range(3):
                J = list(I)
                J[d] -= 1
                if types[I] == -1 or (J[d] >= 0 and types[tuple(J)] == -1):
                    jobs.append(("B", I, d, None, lo, hi, lo[d]))
        print(f"{len(jobs)} sections and staggered boxes", flush=True)
        done = pool.map(stage2, jobs, chunksize=8)
    res = {(kind, I, d, comp): v for kind, I, d, comp, v in done}
    shape = lc.Shape("torus", lc.TORUS_C)
    irregular = [lin(*I) for I in cut if lc.irregular_box(shape, [float(x) for x in cell_box(*I)[0]], [float(x) for x in cell_box(*I)[1]])]
    print(f"irregular: {len(irregular)} of {len(cut)} cut cells = {100.0 * len(irregular) / len(cut):.1f} % (must stay below 20 %)")

    def num(x):
        x = float(x)
        return 0 if x == 0.0 else x
    for comp in (False, True):
        ct = [0] * M
        for I, t in types.items():
            ct[lin(*I)] = t if t == -1 else (1 - t if comp else t)
        A, B, W = ([[0] * len(stored) for _ in range(3)] for _ in range(3))
        for q, I in enumerate(stored):
            lo, hi = cell_box(*I)
            for d in range(3):
                J = list(I)
                J[d] -= 1
                J = tuple(J)
                tI = ct[lin(*I)]
                tJ = ct[lin(*J)] if J[d] >= 0 else tI
                face = prod(lo, hi, d)
                if ("B", I, d, None) in res:
                    a = res[("B", I, d, None)]
                    A[d][q] = num(face - a if comp else a)
                else:
                    A[d][q] = num(face if tI == 1 else ZERO)       # (both cells at the face are trivially of one type)
                B[d][q] = num(res[("B", I, d, comp)]) if tI == -1 else num(face if tI == 1 else ZERO)
                if J[d] < 0:
                    W[d][q] = 0
                elif ("W", I, d, comp) in res:
                    W[d][q] = num(res[("W", I, d, comp)])
                else:
                    W[d][q] = num(prod(lo, hi) if tI == 1 and tJ == 1 else ZERO)
        cases["torus_complement" if comp else "torus"] = {
            "n": list(n), "L": list(L_MESH), "x0": list(X0), "complement": comp, "cell_types": ct,
            "index": [lin(*I) for I in stored],
            "V": [num(V[comp][I]) for I in stored], "G": [num(G[comp][I]) for I in stored],
            "A": A, "B": B, "W": W,
            "C_w": [[num(Cw[comp][I][d]) for I in stored] for d in range(3)],
            "irregular": irregular,
        }
    header = {"body": {"kind": "torus, axis z", "centre": list(lc.TORUS_C), "R": lc.TORUS_R, "r": lc.TORUS_r}, "digits": mp.mp.dps,
              "encoding": "arrays: base64 of zlib-compressed little-endian float64 (cell_types: int8); tests/levelset3d_cases.py unpacks them"}
    lc.FIXTURE.write_text(json.dumps(lc.pack_fixture(cases, header), separators=(",", ":")) + "\n")   # (only what cannot be derived)
    print(f"wrote {lc.FIXTURE} ({lc.FIXTURE.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
