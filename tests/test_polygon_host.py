"""CPU tests of the marker-polygon bodies: the host (g++ -ffp-contract=off) build of penguin/jl_amd/csrc/pg_geom_polygon.h
(tests/polygon_host.cpp -> tests/_build/libpolygon_host.so; test-only, never loaded by the product) against the exact rational
arbiter tests/polygon_reference.py on every case of tests/polygon_cases.py, the sum identities, the edge lookup, the marker
generators against their formulas, every refusal, and a stand-alone sanitizer build.  Bars and measured worsts:
tests/polygon_cases.py."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import penguin.jl_amd as pj
from oracle import penguin_oracle as po
from tests import polygon_cases as pc

P = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def lib():
    return pc.build_host_lib()


# ------------------------------------------------------------------------------------ against the arbiter
@pytest.mark.parametrize("name", pc.ARBITRATED)
def test_host_build_matches_the_arbiter(lib, name):
    got, ref = pc.host_capacity(lib, name), pc.reference(name)
    assert np.array_equal(got.cell_types, ref.cell_types)
    assert np.count_nonzero(ref.cell_types == -1) >= 8
    assert np.array_equal(np.flatnonzero(got.G > 0), np.flatnonzero(ref.G > 0))
    pc.check(name, got, ref, what="host ")


def test_measured_figures_are_the_host_builds(lib):
    """MEASURED is what this build shows (to the 3 digits it is written with), not a looser number"""
    for name in pc.ARBITRATED:
        _, n, L, x0, _ = pc.CASES[name]
        r = pc.ratios(pc.host_capacity(lib, name), pc.reference(name), x0, L, n)
        for q in pc.QUANTITIES:
            assert r[q] <= pc.MEASURED[name][q] * 1.006 + 0.0 and (pc.MEASURED[name][q] == 0.0) == (r[q] == 0.0), (name, q, r[q])


@pytest.mark.parametrize("name", pc.SQUARES)
def test_squares_on_node_and_centre_lines(lib, name):
    got, ref = pc.host_capacity(lib, name), pc.reference(name)
    assert np.array_equal(got.cell_types, ref.cell_types)
    assert np.array_equal(got.V, ref.V)
    assert float(np.sum(got.G)) == 8.0
    for a in (got.V, got.G, got.C_w, got.C_g, *got.A, *got.B, *got.W):
        assert np.all(np.isfinite(a))
    if name == "node_square_16":
        assert np.count_nonzero(got.cell_types == -1) == 0            # touching is not cutting
        assert np.count_nonzero(got.G > 0) == 31                      # the front still belongs to cells, those above / right of it (32 pieces, the lower left corner's cell has two)


def test_complement_tiles_every_cell(lib):
    a, b = pc.host_capacity(lib, "circle_16"), pc.host_capacity(lib, "complement_16")
    h = 0.25
    assert np.array_equal(a.cell_types == -1, b.cell_types == -1)
    real = np.zeros((17, 17), dtype=bool)
    real[:16, :16] = True
    real = real.ravel()
    assert np.max(np.abs(a.V + b.V - h * h)[real]) <= 4 * 2.0 ** -52 * h * h
    for d in range(2):
        face = np.ones((17, 17), dtype=bool)                      # [j, i]: A_d exists on the padding face of d itself only
        face[(16, slice(None)) if d == 0 else (slice(None), 16)] = False
        face = face.ravel()
        assert np.max(np.abs(a.A[d] + b.A[d] - h)[face]) <= 4 * 2.0 ** -52 * h


@pytest.mark.parametrize("name", list(pc.CASES))
def test_sum_identities(lib, name):
    pc.check_identities(name, pc.host_capacity(lib, name), what="host ")


# ------------------------------------------------------------------------------------ lanes, lookup
def test_one_lane_and_sixteen_lanes_agree_to_rounding(lib):
    make, n, L, x0, _ = pc.CASES["fine_circle_8"]
    mesh = po.Mesh(n, L, x0)
    a = po.make_capacity(pc.HostPolygon(lib, make(), mesh, L, lanes=1), mesh)
    b = po.make_capacity(pc.HostPolygon(lib, make(), mesh, L, lanes=16), mesh)
    assert np.array_equal(a.cell_types, b.cell_types)
    assert np.max(np.abs(a.V - b.V)) <= 64 * 2.0 ** -52 * 0.25 and np.max(np.abs(a.G - b.G)) <= 64 * 2.0 ** -52 * 0.5


def test_edge_lookup_lists_every_edge_that_reaches_a_bin_in_ascending_order(lib):
    """brute force in exact comparisons: an edge whose bounding box meets a column's / row's closed extent is in that bucket; an
    edge with a piece of positive length in a closed cell is in that cell's list; every list ascends"""
    from tests.polygon_reference import PolygonBody
    for name in ("heptagon_24", "shifted_17x13", "crystal_24"):
        make, n, L, x0, _ = pc.CASES[name]
        mesh = po.Mesh(n, L, x0)
        body = pc.HostPolygon(lib, make(), mesh, L)
        ref = PolygonBody(make().markers)
        xy = np.zeros(2 * ref.M)
        lib.poly_markers(body.h, xy.ctypes.data_as(P))
        assert np.array_equal(xy.reshape(-1, 2), ref.P)                         # the same normalisation
        Pm, Q = ref.P, ref.Q
        nodes = [np.asarray(mesh.nodes[d], dtype=float) for d in range(2)]

        def listed(b):
            got = [lib.poly_bin_entry(body.h, b, k) for k in range(lib.poly_bin_size(body.h, b))]
            assert got == sorted(set(got))
            return set(got)
        for d in range(2):
            for i in range(n[d]):
                want = set(np.flatnonzero((np.maximum(Pm[:, d], Q[:, d]) >= nodes[d][i]) & (np.minimum(Pm[:, d], Q[:, d]) <= nodes[d][i + 1])))
                assert listed(i if d == 0 else n[0] + i) == want, (name, d, i)
        for j in range(n[1]):
            for i in range(n[0]):
                lo, hi = (nodes[0][i], nodes[1][j]), (nodes[0][i + 1], nodes[1][j + 1])
                pieces, _, _ = ref._pieces(lo, hi)
                near = np.flatnonzero((np.maximum(Pm[:, 0], Q[:, 0]) >= lo[0]) & (np.minimum(Pm[:, 0], Q[:, 0]) <= hi[0]) &
                                      (np.maximum(Pm[:, 1], Q[:, 1]) >= lo[1]) & (np.minimum(Pm[:, 1], Q[:, 1]) <= hi[1]))
                got = listed(n[0] + n[1] + j * n[0] + i)
                assert got <= set(near)                                          # never outside the edge's bounding box
                if pieces:
                    assert got, (name, i, j)


def test_markers_outside_the_mesh_are_never_indexed(lib):
    """a circle twice the size of the mesh: the edges beyond it are in no cell list, the cells inside are measured"""
    front = pc.circle(2.0, 2.0, 3.5, 64)
    mesh = po.Mesh((7, 5), (4.0, 4.0), (0.0, 0.0))
    cap = po.make_capacity(pc.HostPolygon(lib, front, mesh, (4.0, 4.0)), mesh)
    real = np.zeros((6, 8), dtype=bool)
    real[:5, :7] = True
    assert np.all(cap.cell_types[real.ravel()] == 1.0)
    assert float(np.sum(cap.V)) == pytest.approx(16.0, rel=1e-14)


# ------------------------------------------------------------------------------------ marker generators
def test_marker_generators_follow_the_reference_formulas():
    f = pj.create_circle_b(pj.FrontTracker(), 0.3, -0.2, 1.5, 12)
    assert pj.get_markers(f) == [(0.3 + 1.5 * math.cos(2.0 * math.pi * (i / 12)), -0.2 + 1.5 * math.sin(2.0 * math.pi * (i / 12))) for i in range(12)]
    f = pj.create_ellipse_b(pj.FrontTracker(), 0.5, 0.5, 2.0, 1.0, 9)
    assert len(f.markers) == 9 and f.markers[0] == (2.5, 0.5)
    assert all(abs(((x - 0.5) / 2.0) ** 2 + (y - 0.5) ** 2 - 1.0) < 1e-14 for x, y in f.markers)
    f = pj.create_crystal_b(pj.FrontTracker(), 1.0, 2.0, 1.0, 6, 0.3, 96)
    assert len(f.markers) == 97 and f.markers[0] == f.markers[-1]
    for i in (0, 5, 31, 95):
        th = 2.0 * math.pi * i / 96
        r = 1.0 * (1.0 + 0.3 * math.cos(6 * th))
        assert f.markers[i] == (1.0 + r * math.cos(th), 2.0 + r * math.sin(th))
    f = pj.create_rectangle_b(pj.FrontTracker(), 0.0, 0.0, 2.0, 1.0, 16)
    m = f.markers
    assert m[0] == m[-1] and len(m) == 13                        # 12 markers on the sides (16 less the 4 corners kept free) + closing
    assert all((y in (0.0, 1.0)) != (x in (0.0, 2.0)) for x, y in m)          # on a side, never at a corner
    assert [p for p in m if p[1] == 0.0][:4] == [(2.0 * i / 5, 0.0) for i in range(1, 5)]
    assert f.is_closed and len(f.polygon()) == 12


def test_front_is_callable_as_a_signed_distance():
    f = pj.FrontTracker([(0.0, 0.0), (2.0, 0.0), (2.0, 1.0), (0.0, 1.0)])
    assert f(1.0, 0.5) == -0.5 and f(3.0, 0.5) == 1.0 and f(3.0, 2.0) == pytest.approx(math.sqrt(2.0))
    assert pj.is_point_inside(f, 1.0, 0.5) and not pj.is_point_inside(f, 2.5, 0.5)
    x = np.array([1.0, 3.0, -1.0])
    assert np.array_equal(pj.sdf(f, x, 0.5), np.array([-0.5, 1.0, 1.0]))
    pj.add_marker_b(f, -0.5, 0.5)
    assert len(pj.get_markers(f)) == 5 and f(-0.25, 0.5) < 0.0
    assert pj.FrontTracker()(0.0, 0.0) == math.inf


# ------------------------------------------------------------------------------------ refusals
def _refusal(lib, markers):
    nodes = np.linspace(0.0, 4.0, 9)
    h, why = pc.host_new(lib, markers, (8, 8), (nodes, nodes))
    assert not h
    return why


def test_polygon_body_check_refuses_each_with_its_own_message(lib):
    assert "at least 3 markers (got 2)" in _refusal(lib, [(0, 0), (1, 1)])
    assert "at least 3 markers (got 2)" in _refusal(lib, [(0, 0), (1, 1), (0, 0)])              # the closing duplicate does not count
    assert "NULL marker array" in _refusal(lib, [])
    assert "marker 1 has a non-finite coordinate" in _refusal(lib, [(0, 0), (1, float("nan")), (1, 1)])
    assert "marker 2 has a non-finite coordinate" in _refusal(lib, [(0, 0), (1, 0), (float("inf"), 1)])
    assert "zero-length edge: markers 1 and 2 coincide" in _refusal(lib, [(0, 0), (1, 0), (1, 0), (0, 1)])
    assert "zero signed area" in _refusal(lib, [(0, 0), (1, 1), (2, 2)])
    assert "zero signed area" in _refusal(lib, [(0, 0), (1, 1), (1, 0), (0, 1)])                 # a bow tie
    assert "intersects itself: edges 0 and 2" in _refusal(lib, [(0, 0), (2, 0), (2, 1), (1, -1), (0, 2)])
    assert "intersects itself" in _refusal(lib, [(0, 0), (2, 0), (1, 0), (1, 1)])                # folds back onto its own edge
    h, why = pc.host_new(lib, [(0, 0), (0, 1), (1, 1), (1, 0)], (8, 8), (np.linspace(0, 4, 9),) * 2)      # clockwise is accepted
    assert h and why == ""
    lib.poly_free(C.c_void_p(h))


def test_capacity_refuses_what_it_cannot_build():
    """before anything touches the device: an open front, too few markers, a space-time mesh"""
    mesh = pj.Mesh((8, 8), (4.0, 4.0), (0.0, 0.0))
    with pytest.raises(pj.PenguinHipError, match="is_closed=False.*convex hull"):
        pj.Capacity(pj.FrontTracker([(1, 1), (3, 1), (2, 3)], is_closed=False), mesh)
    with pytest.raises(pj.PenguinHipError, match="at least 3 markers"):
        pj.Capacity(pj.FrontTracker([(1, 1), (3, 1)]), mesh)
    with pytest.raises(pj.PenguinHipError, match="SpaceTimeMesh"):
        pj.Capacity(pj.create_circle_b(pj.FrontTracker(), 2.0, 2.0, 1.0, 16), pj.SpaceTimeMesh(mesh, [0.0, 0.1]))
    with pytest.raises(pj.PenguinHipError, match="2-D"):
        pj.Capacity(pj.create_circle_b(pj.FrontTracker(), 2.0, 2.0, 1.0, 16), pj.Mesh((8,), (4.0,), (0.0,)))


# ------------------------------------------------------------------------------------ sanitizers, stand-alone
def test_standalone_program_under_asan_and_ubsan():
    """the host binning and the three primitives on fine_circle_8's polygon, on a square whose markers and edges lie on node
    lines and on a circle larger than the mesh, both phases: the program itself asserts ascending bins, finite results within
    [0, box measure] and that pick_ball, one lane and sixteen lanes agree."""
    out = pc.ROOT / "tests" / "_build" / "polygon_host_asan"
    out.parent.mkdir(exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DPOLYGON_MAIN", "-o", str(out), str(pc.ROOT / "tests" / "polygon_host.cpp")], check=True)
    r = subprocess.run([str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "boxes checked" in r.stdout
