"""CPU tests of moving traced level sets phi(x, t): the tracer's N + 1 derivative programs, the host (g++ -ffp-contract=off) build
of penguin/jl_amd/csrc/pg_geom_program.h with a time (tests/spacetime_program_host.cpp; test-only, never loaded by the product),
the numpy restatement of the slab rule (tests/spacetime_program_reference.py) against oracle/spacetime.py's closed-form moving
bodies, the cheap rule of k_st_classify against the all-nodes rule, every host-side refusal of
pg_capacity_create_spacetime_program, and a stand-alone sanitizer build."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from oracle import geometry as og
from oracle import penguin_oracle as po
from oracle import spacetime as ost
from penguin.jl_amd import PenguinHipError
from penguin.jl_amd import devfn
from penguin.jl_amd.devfn import DeviceFunction, pg_program
from tests import levelset_cases as lc
from tests import spacetime_program_reference as sr
from tests.test_levelset_host import _to_sympy

P = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def lib():
    return sr.build_host_lib()


# ------------------------------------------------------------------------------------ the tracer
@pytest.mark.parametrize("name", ["ellipse", "superellipse", "disc"])
def test_moving_derivative_programs_match_sympy(name):
    import sympy as sp
    df = DeviceFunction(sr.CASES[name][0])
    xs = sp.symbols("x y z t", real=True)
    expr = _to_sympy(df._moving_trace(2), xs)
    rng = np.random.default_rng(11)
    pts = rng.uniform(0.3, 3.7, size=(30, 2))
    progs = df.moving_gradient_programs(2)
    assert len(progs) == 3
    for t in (0.0, 0.37):
        for which, var in enumerate((xs[0], xs[1], xs[3])):
            ref = sp.lambdify(xs, sp.diff(expr, var), modules=["mpmath"])
            got = devfn.interpret(progs[which], pts, t)
            want = np.array([float(ref(float(p[0]), float(p[1]), 0.0, t)) for p in pts])
            assert np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0)) <= 1e-12, (name, which, t)
        # the body program is the closure
        assert np.allclose(devfn.interpret(df.moving_body_program(2), pts, t), df(pts[:, 0], pts[:, 1], t), rtol=0, atol=1e-13)


def test_a_closure_that_does_not_read_t_has_a_zero_time_derivative():
    df = DeviceFunction(lambda x, y, t: lc.circle()(x, y))
    progs = df.moving_gradient_programs(2)
    assert devfn.program_listing(progs[2]) == ["CONST 0.0"]
    static = DeviceFunction(lc.circle()).gradient_programs(2)
    assert [devfn.program_listing(p) for p in progs[:2]] == [devfn.program_listing(p) for p in static]
    assert devfn.program_listing(DeviceFunction(sr.wall_1d).moving_gradient_programs(1)[0]) == ["CONST 1.0"]


def test_moving_programs_are_compiled_once_and_the_complement_keeps_them():
    calls = []

    def body(x, y, t):
        calls.append(1)
        return sr.moving_disc(x, y, t)
    df = DeviceFunction(body)
    first = df.moving_body_program(2)
    for _ in range(3):
        assert df.moving_body_program(2) is first and len(df.moving_gradient_programs(2)) == 3
    assert len(calls) == 1                                # one trace serves every slab of a solve
    comp = DeviceFunction(sr.moving_disc, complement=True)
    assert comp.complement and comp(2.0, 2.0, 0.0) == -sr.moving_disc(2.0, 2.0, 0.0)
    assert devfn.program_listing(comp.moving_body_program(2)) == devfn.program_listing(DeviceFunction(sr.moving_disc).moving_body_program(2))
    assert 3 in [p.arg[q] for p in [comp.moving_body_program(2)] for q in range(p.n_ops) if p.op[q] == devfn.OP["VAR"]]


def test_a_time_derivative_that_does_not_fit_names_the_body_and_the_limit():
    df = DeviceFunction(sr.rotating_ellipse_naive())
    with pytest.raises(PenguinHipError, match=r"derivative along coordinate 0 of the moving body .*phi.* more than 96 instructions"):
        df.moving_gradient_programs(2)

    def wall(x, y, t):
        u = np.sqrt(t * t + 1.0)
        for _ in range(10):                      # one more square root per level: the body grows linearly, its d/dt faster
            u = np.sqrt(u + t)
        return x + 0.1 * y - u
    df = DeviceFunction(wall)
    assert df.moving_body_program(2).n_ops <= devfn.MAX_OPS
    with pytest.raises(PenguinHipError, match=r"derivative along t of the moving body .*wall.* more than 96 instructions"):
        df.moving_gradient_programs(2)
    assert all(p.n_ops <= devfn.MAX_OPS for p in DeviceFunction(sr.rotating_ellipse()).moving_gradient_programs(2))
    with pytest.raises(PenguinHipError, match="cannot trace the moving body"):
        DeviceFunction(lambda x, y: x + y).moving_body_program(2)                 # a moving body takes the coordinates and t


# ------------------------------------------------------------------------------------ the restatement against the closed forms
def _oracle_ratios(lib, fn, obody, n, L, x0, panels, order, source):
    mesh = po.Mesh(n, L, x0)
    t0, t1 = sr.T0, sr.T0 + sr.DT
    tau, wt = ost.composite_gauss(t0, t1, panels, order)
    got = sr.slab_capacity(sr.HostMovingBody(lib, fn, len(n)), mesh, t0, t1, tau, wt)
    ref = ost.make_spacetime_capacity(obody, mesh, t0, t1, panels=panels, order=order)
    M = int(np.prod(mesh.ext))
    assert np.array_equal(got.cell_types, ref.cell_types)
    assert set(got.cell_types[:M]) == {og.EMPTY, og.FULL, og.CUT}
    # B and W at the closed form's centroids: the section's sensitivity to the centroid is the closed form's, not under test
    at = sr.slab_capacity(sr.HostMovingBody(lib, fn, len(n)), mesh, t0, t1, tau, wt, C_w=ref.C_w)
    g = sr.Layer(got, len(n), M)
    g.B, g.W = tuple(b[:M] for b in at.B[:len(n)]), tuple(w[:M] for w in at.W[:len(n)])
    return sr.check("restatement vs oracle", g, sr.Layer(ref, len(n), M), x0, L, n, sr.DT, panels * order, source=source, what="host ")


def test_restatement_matches_the_oracle_half_space_1d(lib):
    """x - (0.37 + 0.2 sin 3t) on 10 cells against MovingHalfSpace with the exact rate, 4 x 4 nodes"""
    fn, _, n, L, x0 = sr.CASES["wall"]
    obody = ost.MovingHalfSpace(0, sr.WALL_POS, 1.0, N=1, dposition=sr.WALL_DPOS)
    _oracle_ratios(lib, fn, obody, n, L, x0, 4, 4, None)


@pytest.mark.parametrize("panels,order", [(4, 4), (3, 1)])
def test_restatement_matches_the_oracle_moving_ball_2d(lib, panels, order):
    """a disc with moving centre and growing radius on 12 x 10 with an offset origin, exact rates on the oracle's side"""
    fn, _, n, L, x0 = sr.CASES["disc"]
    obody = ost.MovingBall(sr.DISC_CEN, sr.DISC_RAD, False, dcenter=sr.DISC_DCEN, dradius=sr.DISC_DRAD)
    _oracle_ratios(lib, fn, obody, n, L, x0, panels, order, None)


# ------------------------------------------------------------------------------------ the cheap rule
@pytest.mark.parametrize("name", list(sr.CASES))
@pytest.mark.parametrize("nq", [3, 64])
def test_cheap_rule_never_contradicts_the_all_nodes_rule(lib, name, nq):
    """every cell k_st_classify would finish has that type under the all-nodes rule; and the rule does finish cells"""
    fn, comp, n, L, x0 = sr.CASES[name]
    mesh = po.Mesh(n, L, x0)
    tau, _ = sr.time_rule(sr.T0, sr.T0 + sr.DT, *sr.RULES[nq])
    res = sr.all_nodes_types(sr.HostMovingBody(lib, fn, len(n), comp), mesh, sr.T0, sr.T0 + sr.DT, tau)
    for li, (typ, far) in res.items():
        assert far == 0 or typ == (og.FULL if far == 1 else og.EMPTY), (name, li, typ, far)
    finished = sum(1 for typ, far in res.values() if far != 0)
    cut = sum(1 for typ, far in res.values() if typ == og.CUT)
    print(f"[cheap rule {name} nq={nq}] {len(res)} cells, {cut} cut, {len(res) - finished} left to the list")
    assert finished > 0 and len(res) - finished >= cut


# ------------------------------------------------------------------------------------ refusals, host side
def _check(lib, N, phi, grad, dphidt, t0=0.1, t1=0.15, nq=None, tau_w=None, n=None):
    n = n or ((12, 10) if N == 2 else (10,) if N == 1 else (4, 4, 4))
    mesh = po.Mesh(n[:2], (4.0,) * len(n[:2]), (0.0,) * len(n[:2]))
    nn = np.array(n, dtype=np.int64)
    nodes = [np.ascontiguousarray(a) for a in mesh.nodes] + [np.zeros(2)]
    if tau_w is None:
        tau, wt = sr.time_rule(t0, t1 if t1 > t0 else t0 + 1.0, 2, 2)
        tau_w = np.ascontiguousarray(np.column_stack([tau, wt]))
    msg = C.create_string_buffer(512)
    ref = lambda p: C.byref(p) if p is not None else None
    rc = lib.stp_check(N, nn.ctypes.data_as(C.POINTER(C.c_int64)), nodes[0].ctypes.data_as(P), nodes[1].ctypes.data_as(P), ref(phi),
                       grad, ref(dphidt), C.c_double(t0), C.c_double(t1), len(tau_w) if nq is None else nq,
                       tau_w.ctypes.data_as(P) if tau_w is not False else None, msg, 512)
    return rc, msg.value.decode()


def test_host_side_refusals_message_by_message(lib):
    df = DeviceFunction(sr.moving_disc)
    phi, d = df.moving_body_program(2), df.moving_gradient_programs(2)
    grad = (pg_program * 2)(*d[:2])
    assert _check(lib, 2, phi, grad, d[2]) == (0, "")
    assert "1-D+t and 2-D+t" in _check(lib, 3, phi, grad, d[2])[1]
    assert "NULL level-set program" in _check(lib, 2, None, grad, d[2])[1]
    assert "grad == NULL" in _check(lib, 2, phi, None, d[2])[1]
    assert "dphidt == NULL" in _check(lib, 2, phi, grad, None)[1]
    assert "tau_w == NULL" in _check(lib, 2, phi, grad, d[2], tau_w=False, nq=4)[1]
    bad = pg_program()
    bad.n_ops = 200
    assert "the level-set program is invalid: n_ops = 200" in _check(lib, 2, bad, grad, d[2])[1]
    assert "the time-derivative program is invalid" in _check(lib, 2, phi, grad, bad)[1]
    assert "gradient program 1 is invalid" in _check(lib, 2, phi, (pg_program * 2)(d[0], bad), d[2])[1]
    w1 = DeviceFunction(sr.wall_1d)
    rc, why = _check(lib, 1, phi, (pg_program * 1)(*w1.moving_gradient_programs(1)[:1]), d[2])
    assert rc == 1 and "reads coordinate 1" in why and "1-D mesh" in why
    ok = np.ascontiguousarray(np.column_stack(sr.time_rule(0.1, 0.15, 2, 2)))
    assert "1 .. 4096 time nodes" in _check(lib, 2, phi, grad, d[2], nq=0)[1]
    assert "1 .. 4096 time nodes" in _check(lib, 2, phi, grad, d[2], nq=4097)[1]
    assert "empty time slab" in _check(lib, 2, phi, grad, d[2], t0=0.15, t1=0.15, tau_w=ok)[1]
    assert "empty time slab" in _check(lib, 2, phi, grad, d[2], t0=0.15, t1=0.1, tau_w=ok)[1]
    out = ok.copy()
    out[0, 0] = 0.1
    assert "inside (t0, t1)" in _check(lib, 2, phi, grad, d[2], tau_w=out)[1]
    heavy = ok.copy()
    heavy[:, 1] *= 1.0 + 1e-9
    assert "add up to t1 - t0" in _check(lib, 2, phi, grad, d[2], tau_w=heavy)[1]
    # derivatives that are not the level set's: a spatial one, the time one (sign, and a body that does not move)
    swapped = (pg_program * 2)(d[1], d[0])
    rc, why = _check(lib, 2, phi, swapped, d[2])
    assert rc == 1 and "gradient program" in why and "central differences" in why
    neg = DeviceFunction(lambda x, y, t: -sr.moving_disc(x, y, t)).moving_gradient_programs(2)[2]
    rc, why = _check(lib, 2, phi, grad, neg)
    assert rc == 1 and "the time-derivative program gives" in why and "central differences" in why
    still = DeviceFunction(lambda x, y, t: sr.moving_disc(x, y, 0.1)).moving_gradient_programs(2)[2]
    assert "the time-derivative program gives" in _check(lib, 2, phi, grad, still)[1]


# ------------------------------------------------------------------------------------ sanitizers, stand-alone
def test_standalone_program_under_asan_and_ubsan():
    """phi = 0 everywhere, NaN on a moving half plane, a disc that appears mid-slab and has radius 0.6 h there, a 1-D wall, each with
    nq = 1, 3 and 7: the program itself asserts finite results within [0, box x dt] for every cell, face and phase, and that the
    cheap rule agrees with the all-nodes rule."""
    out = sr.ROOT / "tests" / "_build" / "spacetime_program_host_asan"
    out.parent.mkdir(exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DSPACETIME_MAIN", "-o", str(out), str(sr.ROOT / "tests" / "spacetime_program_host.cpp")], check=True)
    r = subprocess.run([str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "space-time cells checked" in r.stdout
