"""CPU tests of the MOVING marker polygons (MovingFront): the host (g++ -ffp-contract=off) build of the interpolating view of
penguin/jl_amd/csrc/pg_geom_polygon.h under the kernels' slab rule (tests/spacetime_polygon_host.cpp ->
tests/_build/libspacetime_polygon_host.so; test-only, never loaded by the product) against the exact rational arbiter
(tests/spacetime_polygon_reference.py) on every case of tests/moving_polygon_cases.py, analytic sums no arbiter shares, the lookup
of the swept edges, the cheap pass, every refusal of spacetime_polygon_check, MovingFront itself, and a stand-alone sanitizer
build.  Bars and measured worsts: tests/moving_polygon_cases.py."""
import ctypes as C
import subprocess
from fractions import Fraction as Fr

import numpy as np
import pytest

import penguin.jl_amd as pj
from oracle import penguin_oracle as po
from oracle import spacetime as ost
from tests import moving_polygon_cases as mc
from tests import spacetime_polygon_reference as spr

P = C.POINTER(C.c_double)
T0, DT = mc.T0, mc.DT


@pytest.fixture(scope="module")
def lib():
    return mc.build_host_lib()


@pytest.fixture(scope="module")
def host(lib):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = mc.host_capacity(lib, name)
        return cache[name]
    return get


# ------------------------------------------------------------------------------------ against the arbiter
@pytest.mark.parametrize("name", mc.ARBITRATED)
def test_cases_avoid_every_node_and_centroid_line(name):
    mc.check_generic(name)


@pytest.mark.parametrize("name", list(mc.CASES))
def test_host_build_matches_the_arbiter(host, name):
    got, ref = host(name), mc.reference(name)
    assert np.array_equal(got.cell_types, ref.cell_types)
    assert np.count_nonzero(ref.cell_types == -1) >= 8
    assert np.array_equal(np.flatnonzero(got.G > 0), np.flatnonzero(ref.G > 0))
    mc.check(name, got, what="host ")


def test_measured_figures_are_the_host_builds(host):
    """MEASURED is what this build shows (to the 3 digits it is written with), not a looser number; and no figure is above 10
    times the largest static one (4.7 of tests/polygon_cases.py): a time average cannot be worse than its worst node"""
    for name in mc.CASES:
        r = mc.case_ratios(name, host(name))
        for q in mc.QUANTITIES:
            assert r[q] <= mc.MEASURED[name][q] * 1.006 and (mc.MEASURED[name][q] == 0.0) == (r[q] == 0.0), (name, q, r[q])
            assert mc.MEASURED[name][q] <= 47.0


def test_the_faces_are_the_given_markers_and_a_node_is_the_stated_expression(lib):
    hs = mc.host_slab(lib, "heptagon_nq3")
    arb = mc.arbiter("heptagon_nq3")
    out = np.zeros(2 * len(arb.p0))
    for which, s, want in ((0, 0.0, arb.p0), (1, 0.0, arb.p1), (2, float(hs.s[1]), arb.vertices(float(hs.tau[1])))):
        lib.stp_markers(hs.h, which, C.c_double(s), out.ctypes.data_as(P))
        assert np.array_equal(out.reshape(-1, 2), want)


def test_clockwise_fronts_and_closing_duplicates_are_normalised_together(lib):
    """reversed by the signed area at t0, the same reversal for both arrays; the duplicate dropped from both"""
    p0, p1 = mc.ends("heptagon_nq3")
    mesh = po.Mesh(*mc.HEPT_MESH)
    tau, wt = mc.rule("heptagon_nq3")
    a = spr.host_slab_capacity(spr.HostSlab(lib, p0, p1, mesh, (4.0, 4.0), T0, T0 + DT, tau, wt))
    q0, q1 = np.concatenate([p0[::-1], p0[-1:]]), np.concatenate([p1[::-1], p1[-1:]])
    b = spr.host_slab_capacity(spr.HostSlab(lib, q0, q1, mesh, (4.0, 4.0), T0, T0 + DT, tau, wt))
    assert np.array_equal(a.cell_types, b.cell_types)
    assert np.max(np.abs(a.V - b.V)) <= 64 * 2.0 ** -52 * DT * 0.16 and np.max(np.abs(a.Vn - b.Vn)) <= 64 * 2.0 ** -52 * 0.16


# ------------------------------------------------------------------------------------ the cheap pass, the lookup
@pytest.mark.parametrize("name", ["heptagon_nq3", "crystal_16", "leaving", "aligned_rect_16", "complement_heptagon"])
def test_cheap_pass_agrees_with_the_all_nodes_rule_on_every_cell(lib, host, name):
    a, b = host(name), mc.host_capacity(lib, name, cheap_pass=False)
    assert b.listed == mc.CASES[name][1][0] * mc.CASES[name][1][1] and a.listed < b.listed
    for f in ("cell_types", "V", "G", "Vn_1", "Vn", "C_w_st", "C_g_st"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def test_swept_lookup_lists_every_edge_that_reaches_a_bin_at_any_time_in_ascending_order(lib):
    """brute force: at the faces, the nodes and 7 more times, an edge whose bounding box meets a column's / row's / cell's closed
    extent is in that bin; every list ascends"""
    for name in ("heptagon_nq3", "crystal_16", "leaving"):
        _, n, L, x0, _, _ = mc.CASES[name]
        mesh = po.Mesh(n, L, x0)
        hs, arb = mc.host_slab(lib, name), mc.arbiter(name)
        nodes = [np.asarray(mesh.nodes[d], dtype=float) for d in range(2)]

        def listed(b):
            got = [lib.stp_bin_entry(hs.h, b, k) for k in range(lib.stp_bin_size(hs.h, b))]
            assert got == sorted(set(got))
            return set(got)
        bins = [listed(b) for b in range(n[0] + n[1] + n[0] * n[1])]
        for t in [T0, T0 + DT, *hs.tau, *np.linspace(T0, T0 + DT, 9)[1:-1]]:
            Pm = arb.vertices(float(t))
            Q = np.roll(Pm, -1, axis=0)
            lo, hi = np.minimum(Pm, Q), np.maximum(Pm, Q)
            for d in range(2):
                for i in range(n[d]):
                    want = set(np.flatnonzero((hi[:, d] >= nodes[d][i]) & (lo[:, d] <= nodes[d][i + 1])))
                    assert want <= bins[i if d == 0 else n[0] + i], (name, d, i, t)
            for j in range(n[1]):
                for i in range(n[0]):
                    want = set(np.flatnonzero((hi[:, 0] >= nodes[0][i]) & (lo[:, 0] <= nodes[0][i + 1]) &
                                              (hi[:, 1] >= nodes[1][j]) & (lo[:, 1] <= nodes[1][j + 1])))
                    assert want <= bins[n[0] + n[1] + j * n[0] + i], (name, i, j, t)


# ------------------------------------------------------------------------------------ analytic sums no arbiter shares
def _exact_areas(p0, p1):
    """(A0, A1, A01): the area of the polygon with vertices p0 + s (p1 - p0) is A0 (1 - s)^2 + A1 s^2 + 2 s (1 - s) A01, exactly"""
    a, b = spr.normalise(p0, p1)
    a, b = [(Fr(x), Fr(y)) for x, y in a], [(Fr(x), Fr(y)) for x, y in b]
    n = len(a)

    def form(u, v):
        return sum(u[k][0] * v[(k + 1) % n][1] - u[(k + 1) % n][0] * v[k][1] for k in range(n)) / 2
    return form(a, a), form(b, b), (form(a, b) + form(b, a)) / 2


@pytest.mark.parametrize("name", ["heptagon_nq3", "heptagon_nq80", "fine_2000_8", "crystal_16", "triangle", "aligned_rect_16"])
def test_sums_of_volumes_are_the_closed_forms(host, name):
    """inside the mesh: sum Vn_1 and sum Vn are the shoelace areas at t0 and t1, and sum V is the integral of the area, a
    quadratic in time that every rule of the suite integrates exactly -- area dt for a translation (fine_2000_8, aligned_rect_16:
    A0 = A1 = A01 up to the rounding of the markers), the closed form of a uniform scaling for the crystal.  Each within
    (cut cells + 3) 2^-52 of the summed absolute terms."""
    got = host(name)
    A0, A1, A01 = _exact_areas(*mc.ends(name))
    ncut = int(np.count_nonzero(got.cell_types == -1))
    for what, arr, want in (("Vn_1", got.Vn_1, A0), ("Vn", got.Vn, A1), ("V", got.V, Fr(DT) * (A0 + A1 + A01) / 3)):
        d, tol = abs(mc.lsum(arr) - np.longdouble(float(want))), mc.sum_tol(arr, ncut, float(want))
        print(f"[moving-polygon host {name}] sum {what} off by {float(d):.3g} (bound {float(tol):.3g})")
        assert d <= tol, (name, what, float(d), float(tol))
    if name == "crystal_16":                                     # markers c + g(t) (p - c), g linear: area(t) = g(t)^2 area(T0)
        g1 = 1.0 + 2.2 * DT
        assert float(Fr(DT) * (A0 + A1 + A01) / 3) == pytest.approx(float(A0) * DT * (1.0 + g1 + g1 * g1) / 3.0, rel=1e-14)


@pytest.mark.parametrize("name, c", [("fine_2000_8", (1.7, 0.9)), ("aligned_rect_16", (7.5, 0.0))])
def test_translation_sum_of_gamma_is_the_closed_form(host, name, c):
    """a translation at velocity c: sum Gamma = dt sum_i len_i sqrt(1 + (c . n_i)^2).  Tolerance: a cell's Gamma is a sum over at
    most M pieces (one rounding each), 8 roundings inside a piece's weight, then one per cut cell and partial sum as above"""
    got = host(name)
    p0, _ = spr.normalise(*mc.ends(name))
    e = (np.roll(p0, -1, axis=0) - p0).astype(np.longdouble)
    ln = np.sqrt(e[:, 0] ** 2 + e[:, 1] ** 2)
    vn = (c[0] * e[:, 1] - c[1] * e[:, 0]) / ln
    want = np.longdouble(DT) * np.sum(ln * np.sqrt(1 + vn * vn))
    ncut = int(np.count_nonzero(got.cell_types == -1))
    d, tol = abs(mc.lsum(got.G) - want), mc.sum_tol(got.G, ncut + 8 + len(p0), want)
    print(f"[moving-polygon host {name}] sum Gamma off by {float(d):.3g} (bound {float(tol):.3g})")
    assert d <= tol


def test_fine_circle_is_the_moving_ball_within_the_sagitta(host):
    """2000 markers on a circle of radius r against oracle.spacetime.MovingBall with the same time rule: the polygon and the disc
    differ by the lenses between chords and arcs, of height r (1 - cos(pi / M)) <= r pi^2 / (2 M^2); in a cell they cover at most
    that height times the front the cell holds (the polygon's plus the disc's), integrated over the slab"""
    name = "fine_2000_8"
    got = host(name)
    _, n, L, x0, _, pr = mc.CASES[name]
    mesh = po.Mesh(n, L, x0)
    ball = ost.MovingBall(lambda t: (2.01 + 1.7 * (t - T0), 2.01 + 0.9 * (t - T0)), lambda t: 1.0, dcenter=lambda t: (1.7, 0.9),
                          dradius=lambda t: 0.0)
    with spr.product_rule():
        ref = ost.make_spacetime_capacity(ball, mesh, T0, T0 + DT, panels=pr[0], order=pr[1])
    M = int(np.prod(mesh.ext))
    u, h = mc.unit(x0, L, n)
    sag = np.pi ** 2 / (2 * 2000.0 ** 2)
    bound = (got.G + ref.G[:M]) * sag + mc.bars(name)["V"] * u * h * h * DT
    d = np.abs(got.V - ref.V[:M])
    print(f"[moving-polygon host {name}] worst |V - V_ball| / bound = {float(np.max(d / np.maximum(bound, 1e-300))):.3g}, "
          f"worst |dV| = {float(np.max(d)):.3g}")
    assert np.all(d <= bound)
    assert np.max(d) > 0.0


# ------------------------------------------------------------------------------------ refusals
def _refusal(lib, p0, p1, N=2, t0=T0, t1=T0 + DT, tw="rule", null=()):
    a = np.ascontiguousarray(np.asarray(p0, dtype=float).reshape(-1))
    b = np.ascontiguousarray(np.asarray(p1, dtype=float).reshape(-1))
    if isinstance(tw, str):
        tw = np.column_stack(spr.time_rule(T0, T0 + DT, 2, 2))
    tw = np.ascontiguousarray(tw, dtype=float)
    msg = C.create_string_buffer(512)
    ok = lib.stp_check(N, None if "xy0" in null else a.ctypes.data_as(P), None if "xy1" in null else b.ctypes.data_as(P),
                       C.c_int64(len(a) // 2), C.c_double(t0), C.c_double(t1), len(tw), None if "tau_w" in null else tw.ctypes.data_as(P),
                       msg, 512)
    return "" if ok else msg.value.decode()


def test_spacetime_polygon_check_refuses_each_with_its_own_message(lib):
    tri0, tri1 = [(1, 1), (3, 1), (2, 3)], [(1.1, 1), (3.1, 1), (2.1, 3)]
    assert _refusal(lib, tri0, tri1) == ""
    assert "xy0 == NULL" in _refusal(lib, tri0, tri1, null=("xy0",))
    assert "xy1 == NULL" in _refusal(lib, tri0, tri1, null=("xy1",))
    assert "tau_w == NULL" in _refusal(lib, tri0, tri1, null=("tau_w",))
    assert "2-D body, the mesh is 1-D" in _refusal(lib, tri0, tri1, N=1)
    assert "2-D body, the mesh is 3-D" in _refusal(lib, tri0, tri1, N=3)
    assert "at least 3 markers (got 2)" in _refusal(lib, tri0[:2], tri1[:2])
    assert "at least 3 markers (got 2)" in _refusal(lib, tri0[:2] + tri0[:1], tri1[:2] + tri1[:1])        # the closing duplicates do not count
    assert "marker 1 has a non-finite coordinate at t0" in _refusal(lib, [(1, 1), (3, float("nan")), (2, 3)], tri1)
    assert "marker 2 has a non-finite coordinate at t1" in _refusal(lib, tri0, [(1, 1), (3, 1), (float("inf"), 3)])
    ok = np.column_stack(spr.time_rule(T0, T0 + DT, 2, 2))
    assert "1 .. 4096 time nodes" in _refusal(lib, tri0, tri1, tw=np.zeros((0, 2)))
    assert "1 .. 4096 time nodes" in _refusal(lib, tri0, tri1, tw=np.tile(ok, (1025, 1)))
    assert "empty time slab" in _refusal(lib, tri0, tri1, t1=T0)
    bad = ok.copy()
    bad[0, 0] = T0
    assert "time nodes must lie inside (t0, t1)" in _refusal(lib, tri0, tri1, tw=bad)
    bad = ok.copy()
    bad[1, 1] *= 1.0 + 1e-9
    assert "time weights must add up to t1 - t0" in _refusal(lib, tri0, tri1, tw=bad)
    assert "at t0: zero-length edge: markers 1 and 2 coincide" in _refusal(lib, [(1, 1), (3, 1), (3, 1), (2, 3)], [(1, 1), (3, 1), (3, 2), (2, 3)])
    assert "at t1: the polygon has zero signed area" in _refusal(lib, tri0, [(1, 1), (2, 2), (3, 3)])
    assert "at t1: the polygon intersects itself: edges 0 and 2" in _refusal(lib, [(0, 0), (2, 0), (2, 1), (1, 1.5), (0, 2)],
                                                                             [(0, 0), (2, 0), (2, 1), (1, -1), (0, 2)])
    # simple at both faces, degenerate half way: a square turned by half a turn on straight marker paths passes through its centre
    assert "at mid time: zero-length edge" in _refusal(lib, [(0, 0), (2, 0), (2, 2), (0, 2)], [(2, 2), (0, 2), (0, 0), (2, 0)])
    assert "orientation of the polygon differs between t0 and t1" in _refusal(lib, [(1, 1), (3, 1), (2, 3)], [(1, 1), (3, 1), (2.2, -1.5)])
    assert "at t0: zero-length edge" in _refusal(lib, tri0 + tri0[:1], tri1 + [(1.2, 1.3)])           # only one array closes: the duplicate stays


# ------------------------------------------------------------------------------------ MovingFront (host side)
def test_moving_front_generators():
    base = pj.create_circle_b(pj.FrontTracker(), 1.0, 2.0, 0.5, 12)
    mf = pj.MovingFront.rigid(base, shift=lambda t: (0.3 * t, -0.1 * t), angle=lambda t: 0.7 * t, about=(1.0, 2.0))
    assert np.array_equal(mf.markers(0.0), base.polygon())
    p = mf.markers(2.0)
    r = base.polygon() - np.array([1.0, 2.0])
    ca, sa = np.cos(1.4), np.sin(1.4)
    assert np.allclose(p, np.column_stack([1.0 + ca * r[:, 0] - sa * r[:, 1] + 0.6, 2.0 + sa * r[:, 0] + ca * r[:, 1] - 0.2]), atol=1e-15)
    assert mf(1.0 + 0.6, 2.0 - 0.2, 2.0) == pytest.approx(-0.5 * np.cos(np.pi / 12), rel=1e-12) and not mf.complement
    assert pj.MovingFront.rigid(base, complement=True)(1.0, 2.0, 0.0) > 0.0
    f0, f1, f2 = base.polygon(), base.polygon() + 1.0, base.polygon() * 2.0
    pw = pj.MovingFront.from_fronts([pj.FrontTracker([tuple(r) for r in f0]), f1, f2], [0.0, 1.0, 3.0])
    assert np.array_equal(pw.markers(0.0), f0) and np.array_equal(pw.markers(1.0), f1) and np.array_equal(pw.markers(3.0), f2)
    assert np.array_equal(pw.markers(0.25), f0 + 0.25 * (f1 - f0)) and np.array_equal(pw.markers(2.0), f1 + 0.5 * (f2 - f1))
    with pytest.raises(ValueError, match="outside"):
        pw.markers(3.5)
    with pytest.raises(ValueError, match="same number of markers"):
        pj.MovingFront.from_fronts([f0, f1[:-1]], [0.0, 1.0])
    with pytest.raises(ValueError, match="ascend"):
        pj.MovingFront.from_fronts([f0, f1], [1.0, 1.0])
    with pytest.raises(TypeError, match="callable"):
        pj.MovingFront(f0)
    grow = pj.MovingFront(lambda t: f0[: 12 - int(t)])
    grow.markers(0.0)
    with pytest.raises(ValueError, match="count and order must not change"):
        grow.markers(1.0)


def test_capacity_refuses_before_the_device():
    """a single front on a SpaceTimeMesh still has no motion; a pair needs equal counts and closed fronts; a MovingFront carries
    its own complement flag"""
    mesh = pj.Mesh((8, 8), (4.0, 4.0), (0.0, 0.0))
    st = pj.SpaceTimeMesh(mesh, [0.0, 0.1])
    a, b = pj.create_circle_b(pj.FrontTracker(), 2.0, 2.0, 1.0, 16), pj.create_circle_b(pj.FrontTracker(), 2.0, 2.0, 1.0, 17)
    with pytest.raises(pj.PenguinHipError, match="SpaceTimeMesh.*MovingFront"):
        pj.Capacity(a, st)
    with pytest.raises(pj.PenguinHipError, match="16 and 17 markers"):
        pj.Capacity((a, b), st)
    with pytest.raises(pj.PenguinHipError, match="is_closed=False"):
        pj.Capacity((a, pj.FrontTracker(a.markers, is_closed=False)), st)
    with pytest.raises(pj.PenguinHipError, match="carries its own flag"):
        pj.Capacity(pj.MovingFront.rigid(a), st, complement=True)


# ------------------------------------------------------------------------------------ sanitizers, stand-alone
def test_standalone_program_under_asan_and_ubsan():
    """a triangle that collapses towards a line at t1 with one time node and with five, a circle whose markers leave the mesh
    and a polygon that never enters it (every swept list empty), both phases: the program itself asserts ascending bins, finite
    results within [0, box measure], that pick_ball and box_measure agree on every type and that the cheap pass agrees with
    every slot."""
    out = mc.ROOT / "tests" / "_build" / "spacetime_polygon_host_asan"
    out.parent.mkdir(exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DSTP_MAIN", "-o", str(out), str(mc.ROOT / "tests" / "spacetime_polygon_host.cpp")], check=True)
    r = subprocess.run([str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "boxes checked" in r.stdout


# ------------------------------------------------------------------------------------ the motions of the GPU solves
@pytest.mark.parametrize("name, comp", [("mono_12x10", False), ("diph_16", False), ("diph_16", True)])
def test_solve_motions_have_no_sliver_cells(lib, name, comp):
    """tests/test_gpu_moving_polygon.py solves on these slabs against the oracle at 1e-10: no space-time cut cell, of either
    phase, is below 1e-4 of a full one (the host build and the arbiter agree on V to a few units of 1e-15, so either may judge)"""
    fn, n, L, x0 = mc.SOLVES[name]
    mesh = po.Mesh(n, L, x0)
    for t0, t1 in mc.SOLVE_SLABS:
        tau, wt = spr.time_rule(t0, t1, 16, 4)
        cap = spr.host_slab_capacity(spr.HostSlab(lib, fn(t0), fn(t1), mesh, L, t0, t1, tau, wt, comp))
        frac = mc.smallest_cut_fraction(cap, n, L)
        print(f"[moving-polygon host {name} complement={comp}] slab [{t0:.2f}, {t1:.2f}]: smallest cut cell {frac:.3g} of a full one")
        assert frac >= mc.SLIVER, (name, comp, t0, frac)
