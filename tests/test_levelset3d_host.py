"""CPU tests of the 3-D traced-level-set bodies: the host (g++ -ffp-contract=off) build of
penguin/jl_amd/csrc/pg_geom_program3.h (tests/levelset3d_host.cpp -> tests/_build/liblevelset3d_host.so; test-only, never loaded
by the product) against the clipping oracle of a plane, oracle.geometry's Ball and Ellipsoid, the 30-digit torus fixture, every
refusal of the 3-D body check, and a stand-alone sanitizer build.  Bars, classes and measured worsts: tests/levelset3d_cases.py."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

from oracle import penguin_oracle as po
from oracle.geometry import Ball, Ellipsoid
from penguin.jl_amd.devfn import DeviceFunction, pg_program
from tests import levelset3d_cases as lc
from tests.plane_oracle import ObliqueHalfSpace

P = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def lib():
    return lc.build_host_lib()


@functools.lru_cache(maxsize=None)
def _fixture():
    return lc.load_fixture()


def _host_cap(lib, fn, mesh, comp=False):
    n, L, x0 = mesh
    return po.make_capacity(lc.HostBody3(lib, fn, comp), po.Mesh(n, L, x0))


def _cube(n):
    return ((n, n, n), (4.0, 4.0, 4.0), (0.0, 0.0, 0.0))


# ------------------------------------------------------------------------------------ the plane: exact
@pytest.mark.parametrize("comp", [False, True])
def test_oblique_plane_against_the_clipping_oracle(lib, comp):
    """phi is linear: every integrand is piecewise polynomial between the breakpoints and Gauss-Legendre is exact -- anything
    above rounding is a fault of the breakpoint streams"""
    n, L, x0 = lc.PLANE_MESH
    got = _host_cap(lib, lc.plane(), lc.PLANE_MESH, comp)
    ref = po.make_capacity(ObliqueHalfSpace(lc.PLANE_N, lc.PLANE_OFF, comp), po.Mesh(n, L, x0))
    assert np.array_equal(got.cell_types, ref.cell_types)
    reg, _ = lc.check("plane", got, ref, lc.PLANE_MESH, what=f"host comp={comp} ")
    assert max(reg.values()) <= 100.0


def test_plane_on_a_node_plane_touching_is_empty(lib):
    got = _host_cap(lib, lambda x, y, z: x - 1.75, _cube(8))
    ref = po.make_capacity(ObliqueHalfSpace((1.0, 0.0, 0.0), 1.75), po.Mesh(*_cube(8)))
    assert np.array_equal(got.cell_types, ref.cell_types)
    assert not np.any(got.cell_types == -1)                    # the cells right of x = 1.75 only touch it: EMPTY
    lc.check("plane", got, ref, _cube(8), what="host node plane ")


# ------------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("n", [8, 12, 16])
def test_ball_against_the_oracle_ball(lib, n):
    got = _host_cap(lib, lc.ball(), _cube(n))
    ref = po.make_capacity(Ball(lc.BALL_C, lc.BALL_R), po.Mesh(*_cube(n)))
    assert np.array_equal(got.cell_types, ref.cell_types)
    reg, _ = lc.check("ball", got, ref, _cube(n), lc.Shape("sphere", lc.BALL_C, (lc.BALL_R,) * 3), what=f"host n={n} ")
    assert reg["V"] * lc.unit((0.0,) * 3, (4.0,) * 3, (n,) * 3)[0] < lc.REGULAR_V_MAX


@pytest.mark.parametrize("n", [8, 12, 16])
def test_ellipsoid_against_the_oracle_ellipsoid(lib, n):
    got = _host_cap(lib, lc.ellipsoid(), _cube(n))
    ref = po.make_capacity(Ellipsoid(lc.ELL_C, lc.ELL_A), po.Mesh(*_cube(n)))
    assert np.array_equal(got.cell_types, ref.cell_types)
    reg, _ = lc.check("ellipsoid", got, ref, _cube(n), lc.Shape("sphere", lc.ELL_C, lc.ELL_A), what=f"host n={n} ")
    assert reg["V"] * lc.unit((0.0,) * 3, (4.0,) * 3, (n,) * 3)[0] < lc.REGULAR_V_MAX


# ------------------------------------------------------------------------------------ the torus fixture
@pytest.mark.parametrize("name", ["torus", "torus_complement"])
def test_host_build_matches_the_torus_fixture(lib, name):
    f = _fixture()[name]
    mesh = (f.n, f.L, f.x0)
    got = _host_cap(lib, lc.torus(), mesh, f.complement)
    assert np.array_equal(got.cell_types, f.cell_types)
    shape = lc.Shape("torus", lc.TORUS_C)
    cell_irr = lc.class_masks(shape, mesh, f)[0]
    assert np.array_equal(cell_irr, f.irregular)               # the generator's flags are this module's
    ncut = int(np.sum(f.cell_types == -1))
    assert cell_irr.sum() <= lc.IRREGULAR_SHARE_MAX * ncut, (int(cell_irr.sum()), ncut)
    reg, _ = lc.check(name, got, f, mesh, shape, what="host ", keep=f.keep)
    assert reg["V"] * lc.unit(f.x0, f.L, f.n)[0] < lc.REGULAR_V_MAX


def test_lane_shares_add_up_to_the_whole(lib):
    """the 64 shares of a cut box (outer node l & 15, inner nodes l >> 4, + 4, ...) are a partition of the host's quadrature"""
    body = lc.HostBody3(lib, lc.torus())
    lo, hi = [0.8, 1.0, 2.2], [1.1, 1.3, 2.5]
    whole = body.box(lo, hi)
    assert whole.type == -1
    # a share's `vol` is its partial volume (clamped only above, by the whole box)
    vol = sum(body.box(lo, hi, True, l, 64).vol for l in range(64))
    gam = sum(body.box(lo, hi, True, l, 64).gamma for l in range(64))
    assert vol == pytest.approx(whole.vol, rel=1e-13) and gam == pytest.approx(whole.gamma, rel=1e-13)


# ------------------------------------------------------------------------------------ refusals of the 3-D body check
def _check(lib, phi, grad, N=3, n=(8, 8, 8), L=(4.0, 4.0, 4.0), single_rank=1):
    nn = (C.c_int64 * 3)(*n)
    nodes = [np.array([j * L[d] / n[d] for j in range(n[d] + 1)]) for d in range(3)]
    msg = C.create_string_buffer(512)
    rc = lib.ls3_check(N, nn, nodes[0].ctypes.data_as(P), nodes[1].ctypes.data_as(P), nodes[2].ctypes.data_as(P),
                       C.byref(phi) if phi is not None else None, grad, single_rank, msg, 512)
    return rc, msg.value.decode()


def _progs(fn):
    df = DeviceFunction(fn)
    return df.body_program(3), (pg_program * 3)(*df.gradient_programs(3))


def test_gradient_programs_of_a_3d_body_are_three():
    grads = DeviceFunction(lc.plane()).gradient_programs(3)
    assert len(grads) == 3
    from penguin.jl_amd import devfn
    assert [devfn.program_listing(g) for g in grads] == [["CONST 0.6"], ["CONST -0.64"], ["CONST 0.48"]]


def test_entry_accepts_the_test_bodies(lib):
    for fn in (lc.plane(), lc.ball(), lc.ellipsoid(), lc.torus(), lc.rotated_ellipsoid()):
        assert _check(lib, *_progs(fn)) == (0, "")


def test_entry_refusals_each_with_its_own_message(lib):
    phi, grad = _progs(lc.ball())
    bad = pg_program.from_buffer_copy(phi)
    bad.op[0] = 200
    assert "level-set program is invalid" in _check(lib, bad, grad)[1]
    assert "gradient program 2 is invalid" in _check(lib, phi, (pg_program * 3)(grad[0], grad[1], bad))[1]
    with_t = DeviceFunction(lambda x, y, z, t: x + y + z - t).program_for(3)    # reads VAR 3
    rc, why = _check(lib, with_t, grad)
    assert rc == 1 and "reads t" in why
    assert "grad == NULL" in _check(lib, phi, None)[1]
    assert "NULL level-set program" in _check(lib, None, grad)[1]
    assert "must be 3-D" in _check(lib, phi, grad, N=2)[1]
    assert "single rank" in _check(lib, phi, grad, single_rank=0)[1]
    swapped = (pg_program * 3)(grad[0], grad[2], grad[1])
    rc, why = _check(lib, phi, swapped)
    assert rc == 1 and "central differences" in why
    sign = (pg_program * 3)(*DeviceFunction(lambda x, y, z: -lc.ball()(x, y, z)).gradient_programs(3))
    assert "central differences" in _check(lib, phi, sign)[1]


# ------------------------------------------------------------------------------------ sanitizers, stand-alone
def test_standalone_program_under_asan_and_ubsan():
    """box type, box measure and section measure on boxes of the torus and the plane, both phases: the program itself asserts
    finite results within [0, box measure]"""
    out = lc.ROOT / "tests" / "_build" / "levelset3d_sanitize"
    out.parent.mkdir(exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", str(out), str(lc.ROOT / "tests" / "levelset3d_sanitize.cpp")], check=True)
    r = subprocess.run([str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "boxes checked" in r.stdout
