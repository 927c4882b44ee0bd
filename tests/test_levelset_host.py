"""CPU tests of the traced-level-set bodies: the host (g++ -ffp-contract=off) build of penguin/jl_amd/csrc/pg_geom_program.h
(tests/levelset_host.cpp -> tests/_build/liblevelset_host.so; test-only, never loaded by the product) against the 30-digit
fixture, against oracle.geometry's closed forms and tests/plane_oracle.py through `.box` / `.section`, the tracer's derivatives
against sympy, every refusal, and a stand-alone sanitizer build.  Bars and measured worsts: tests/levelset_cases.py."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

from oracle import penguin_oracle as po
from oracle.geometry import Ball, Ellipsoid, HalfSpace
from penguin.jl_amd import PenguinHipError
from penguin.jl_amd import devfn
from penguin.jl_amd.devfn import DeviceFunction, pg_program
from tests import levelset_cases as lc
from tests.plane_oracle import ObliqueHalfSpace

P = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def lib():
    return lc.build_host_lib()


@functools.lru_cache(maxsize=None)
def _fixture():
    return lc.load_fixture()


def _host_cap(lib, fn, n, L, x0, comp=False):
    return po.make_capacity(lc.HostBody(lib, fn, len(n), comp), po.Mesh(n, L, x0))


# ------------------------------------------------------------------------------------ fixture
@pytest.mark.parametrize("name", list(lc.FIXTURE_BODIES))
def test_host_build_matches_the_fixture(lib, name):
    f = _fixture()[name]
    make, comp = lc.FIXTURE_BODIES[name]
    got = _host_cap(lib, make(), f.n, f.L, f.x0, comp)
    assert np.array_equal(got.cell_types, f.cell_types)
    lc.check(name, got, f, f.x0, f.L, f.n, what="host ")
    if name == "discs_24":
        lc.check("discs_24_smooth", lc.Masked(got, f, (f.n[0] + 1, f.n[1] + 1)), f, f.x0, f.L, f.n, what="host ")
        lc.check_kink(got, f, f.L, f.n, what="host ")


# ------------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("n", [12, 16, 24, 48])
def test_circle_against_the_oracle_ball(lib, n):
    got = _host_cap(lib, lc.circle(), (n, n), (4.0, 4.0), (0.0, 0.0))
    ref = po.make_capacity(Ball((2.01, 2.01), 1.0), po.Mesh((n, n), (4.0, 4.0), (0.0, 0.0)))
    assert np.array_equal(got.cell_types, ref.cell_types)
    lc.check("circle", got, ref, (0.0, 0.0), (4.0, 4.0), (n, n), what=f"host n={n} ")


@pytest.mark.parametrize("n", [16, 24, 48])
def test_axis_aligned_ellipse_against_the_oracle_ellipsoid(lib, n):
    got = _host_cap(lib, lc.ellipse_sqrt(2.01, 1.97, 1.3, 0.6), (n, n), (4.0, 4.0), (0.0, 0.0))
    ref = po.make_capacity(Ellipsoid((2.01, 1.97), (1.3, 0.6)), po.Mesh((n, n), (4.0, 4.0), (0.0, 0.0)))
    assert np.array_equal(got.cell_types, ref.cell_types)
    lc.check("ellipse0", got, ref, (0.0, 0.0), (4.0, 4.0), (n, n), what=f"host n={n} ")


@pytest.mark.parametrize("normal,off,n", [((0.6, -0.8), 0.31, 16), ((0.6, -0.8), 0.31, 24), ((1.0, 0.0), 1.375, 16)])
@pytest.mark.parametrize("comp", [False, True])
def test_plane_against_the_clipping_oracle(lib, normal, off, n, comp):
    """every capacity of a plane is exact: the sharpest arbiter of Γ and C_γ.  x - 1.375 lies on a node line of the 16^2 mesh: the
    cells that only touch it are EMPTY on both sides of the comparison (phi <= 0 is fluid, touching is not cutting)."""
    got = _host_cap(lib, lc.plane(normal[0], normal[1], off), (n, n), (4.0, 4.0), (0.0, 0.0), comp)
    ref = po.make_capacity(ObliqueHalfSpace(normal, off, comp), po.Mesh((n, n), (4.0, 4.0), (0.0, 0.0)))
    assert np.array_equal(got.cell_types, ref.cell_types)
    lc.check("plane", got, ref, (0.0, 0.0), (4.0, 4.0), (n, n), what=f"host n={n} comp={comp} ")


def test_half_line_in_1d_against_the_oracle_halfspace(lib):
    got = _host_cap(lib, lambda x: x - 0.37, (10,), (1.0,), (0.0,))
    ref = po.make_capacity(HalfSpace(0, 0.37, N=1), po.Mesh((10,), (1.0,), (0.0,)))
    assert np.array_equal(got.cell_types, ref.cell_types)
    lc.check("halfspace1d", got, ref, (0.0,), (1.0,), (10,), what="host ")


def test_segment_conventions(lib):
    """a sample that is exactly 0 is a root; roots in the closed segment are counted once each; pieces by their midpoint"""
    df = DeviceFunction(lambda x: (x - 0.25) * (x - 0.6))
    phi, grad = df.body_program(1), (pg_program * 1)(*df.gradient_programs(1))
    out = np.zeros(4)
    lib.ls_segment(1, C.byref(phi), grad, 0, C.c_double(0.0), C.c_double(0.0), C.c_double(1.0), out.ctypes.data_as(P))
    assert out[2] == 2.0 and out[3] == pytest.approx(0.85, abs=1e-15)      # 0.25 is sample 2 of [0, 1], 0.6 is refined
    assert out[0] == pytest.approx(0.35, abs=1e-15) and out[1] == pytest.approx(0.5 * (0.36 - 0.0625), abs=1e-15)


# ------------------------------------------------------------------------------------ derivatives
def _to_sympy(node, xs):
    import sympy as sp
    op, a = node.op, node.args
    if op == "CONST":
        return sp.Float(a[0], 30)
    if op == "VAR":
        return xs[a[0]]
    v = [_to_sympy(x, xs) for x in a]
    un = {"NEG": lambda u: -u, "ABS": sp.Abs, "SQRT": sp.sqrt, "EXP": sp.exp, "LOG": sp.log, "SIN": sp.sin, "COS": sp.cos,
          "TANH": sp.tanh, "ERF": sp.erf, "ERFC": sp.erfc}
    bi = {"ADD": lambda p, q: p + q, "SUB": lambda p, q: p - q, "MUL": lambda p, q: p * q, "DIV": lambda p, q: p / q,
          "POW": lambda p, q: p ** q, "ATAN2": sp.atan2, "MIN": sp.Min, "MAX": sp.Max}
    if op in un:
        return un[op](v[0])
    if op in bi:
        return bi[op](v[0], v[1])
    raise AssertionError(op)


GRAD_BODIES = {
    "rotated ellipse": lc.rotated_ellipse(),
    "circle": lc.circle(),
    "axis-aligned ellipse": lc.ellipse_sqrt(2.01, 1.97, 1.3, 0.6),
    "plane": lc.plane(0.6, -0.8, 0.31),
    "two discs": lc.two_discs,
    "superellipse": lambda x, y: np.abs((x - 2.0) / 1.2) ** 2.5 + np.abs((y - 2.0) / 0.7) ** 2.5 - 1.0,
    "wavy wall": lambda x, y: y - 2.0 - 0.3 * np.sin(2.0 * x) * np.exp(-0.1 * x) + np.tanh(x - 2.0) / (1.0 + x * x),
    "atan2 flower": lambda x, y: np.sqrt((x - 2.0) ** 2 + (y - 2.0) ** 2) - 1.0 - 0.2 * np.cos(5.0 * devfn.atan2(y - 2.0, x - 2.0)),
    "erf and log": lambda x, y: devfn.erf(x - 2.0) + np.log(1.0 + y * y) - devfn.erfc(y) * np.maximum(x, 0.5 * y),
}


@pytest.mark.parametrize("name", list(GRAD_BODIES))
def test_traced_gradient_matches_sympy(name):
    import sympy as sp
    fn = GRAD_BODIES[name]
    df = DeviceFunction(fn)
    xs = sp.symbols("x y", real=True)
    expr = _to_sympy(df._body_trace(2), xs)
    rng = np.random.default_rng(7)
    pts = rng.uniform(0.3, 3.7, size=(40, 2))
    grads = df.gradient_programs(2)
    for d in range(2):
        ref = sp.lambdify(xs, sp.diff(expr, xs[d]), modules=["mpmath"])
        got = devfn.interpret(grads[d], pts, 0.0)
        want = np.array([float(ref(float(p[0]), float(p[1]))) for p in pts])
        assert np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0)) <= 1e-12, (name, d)


def test_gradient_programs_fold_and_fit():
    df = DeviceFunction(lc.rotated_ellipse())
    assert df.body_program(2).n_ops >= 30
    assert all(g.n_ops <= devfn.MAX_OPS for g in df.gradient_programs(2))
    lin = DeviceFunction(lambda x, y: 0.6 * x - 0.8 * y - 0.31).gradient_programs(2)
    assert [devfn.program_listing(g) for g in lin] == [["CONST 0.6"], ["CONST -0.8"]]          # 0 * x, 1 * x, x + 0 are folded


def test_a_derivative_that_does_not_fit_names_the_body_and_the_limit():
    def body(x, y):
        u = np.sqrt(x * x + y * y + 1.0)
        for _ in range(10):                      # one more square root per level: the body grows linearly, its derivative faster
            u = np.sqrt(u + x)
        return u - 2.0
    df = DeviceFunction(body)
    assert df.body_program(2).n_ops <= devfn.MAX_OPS
    with pytest.raises(PenguinHipError, match=r"derivative along coordinate 0 of the body .*body.* more than 96 instructions"):
        df.gradient_programs(2)


def test_body_tracing_refusals():
    with pytest.raises(PenguinHipError, match="cannot trace"):
        DeviceFunction(lambda x, y, t: x + y + t).body_program(2)              # a body takes the coordinates alone
    with pytest.raises(PenguinHipError, match="Python branch"):
        DeviceFunction(lambda x, y: x if x > y else y).body_program(2)
    assert DeviceFunction(lc.circle(), complement=True)(2.01, 2.01) == 1.0 and DeviceFunction(lc.circle())(2.01, 2.01) == -1.0
    comp = DeviceFunction(lambda x, y, z, t: x + t, complement=True)                 # a complemented object is a body only
    assert "complement=True" in repr(comp)
    with pytest.raises(PenguinHipError, match="BODY"):
        comp.program_for(3)


# ------------------------------------------------------------------------------------ refusals of the C entry
def _check(lib, N, phi, grad, n=(16, 16), L=(4.0, 4.0)):
    nn = (C.c_int64 * 3)(*n, *([1] * (3 - len(n))))
    nodes = [np.array([(j + 0.5) * L[d] / n[d] for j in range(n[d] + 1)]) for d in range(min(N, len(n)))]
    while len(nodes) < 2:
        nodes.append(np.zeros(2))
    msg = C.create_string_buffer(512)
    rc = lib.ls_check(N, nn, nodes[0].ctypes.data_as(P), nodes[1].ctypes.data_as(P), C.byref(phi) if phi is not None else None,
                      grad, msg, 512)
    return rc, msg.value.decode()


def _progs(fn, N=2):
    df = DeviceFunction(fn)
    return df.body_program(N), (pg_program * N)(*df.gradient_programs(N))


def test_entry_accepts_the_test_bodies(lib):
    for fn in (lc.rotated_ellipse(), lc.two_discs, lc.circle(), lc.plane(0.6, -0.8, 0.31)):
        assert _check(lib, 2, *_progs(fn)) == (0, "")
    assert _check(lib, 1, *_progs(lambda x: x - 0.37, 1), n=(10,), L=(1.0,)) == (0, "")
    nan_half = _progs(lambda x, y: np.sqrt(x - 2.0) - 0.4)                    # NaN on half the plane decides nothing
    assert _check(lib, 2, *nan_half)[0] == 0


def test_entry_refusals_each_with_its_own_message(lib):
    phi, grad = _progs(lc.circle())
    bad = pg_program.from_buffer_copy(phi)
    bad.op[0] = 200
    assert "level-set program is invalid" in _check(lib, 2, bad, grad)[1]
    badg = (pg_program * 2)(grad[0], bad)
    assert "gradient program 1 is invalid" in _check(lib, 2, phi, badg)[1]
    with_t = DeviceFunction(lambda x, y, z, t: x + y - t).program_for(3)        # reads VAR 3
    rc, why = _check(lib, 2, with_t, grad)
    assert rc == 1 and "reads t" in why
    z = DeviceFunction(lambda x, y, z: x + y + z - 1.0).body_program(3)
    assert "reads coordinate 2" in _check(lib, 2, z, grad)[1]
    assert "reads coordinate 1" in _check(lib, 1, phi, grad, n=(10,), L=(1.0,))[1]
    assert "3-D" in _check(lib, 3, phi, grad)[1]
    assert "grad == NULL" in _check(lib, 2, phi, None)[1]
    assert "NULL level-set program" in _check(lib, 2, None, grad)[1]
    wrong = (pg_program * 2)(grad[1], grad[0])                                   # the derivatives swapped
    rc, why = _check(lib, 2, phi, wrong)
    assert rc == 1 and "central differences" in why
    sign = (pg_program * 2)(*DeviceFunction(lambda x, y: -lc.circle()(x, y)).gradient_programs(2))
    assert "central differences" in _check(lib, 2, phi, sign)[1]


# ------------------------------------------------------------------------------------ sanitizers, stand-alone
def test_standalone_program_under_asan_and_ubsan():
    """valid bodies, a body that is 0 everywhere, one that is NaN on half the plane, a disc of radius 0.6 h: the program itself
    asserts finite results within [0, box measure] for every box, section and phase."""
    out = lc.ROOT / "tests" / "_build" / "levelset_host_asan"
    out.parent.mkdir(exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DLEVELSET_MAIN", "-o", str(out), str(lc.ROOT / "tests" / "levelset_host.cpp")], check=True)
    r = subprocess.run([str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "boxes checked" in r.stdout
