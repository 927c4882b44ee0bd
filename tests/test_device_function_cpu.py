"""Device functions without a GPU: the tracer (pj.DeviceFunction) against the closure it traced, its refusals, the validator and
the host interpreter of the library (pg_program_validate / pg_program_eval_host need no device) on well-formed, malformed and
random programs -- through the library and, under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program
(tests/program_host.cpp) --, the table of times against a literal replay of the loop's clock, and the presence of the new
symbols in the header, the library and the Julia twin."""
import ctypes as C
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import penguin.jl_amd as pj
from penguin.jl_amd import _lib as L
from penguin.jl_amd import api, devfn
from tests import device_function_cases as cases
from tests.device_function_cases import raw_program

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "_build"
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}

RNG = np.random.default_rng(11)
PTS = RNG.uniform(0.05, 3.95, size=(400, 3))
TIMES = (0.0, 0.3, 1.7)


def _last_error():
    buf = C.create_string_buffer(4096)
    L.lib().pg_last_error(buf, 4096)
    return buf.value.decode("utf-8", "replace")


def _closure_values(fn, pts, t, nspace=3):
    out = fn(*[pts[:, d] for d in range(nspace)], t)
    return np.broadcast_to(np.asarray(out, dtype=np.float64), (len(pts),))


# ------------------------------------------------------------------------------------ the tracer
@pytest.mark.parametrize("name", ["problem5_source", "moving_gaussian", "erfc_profile", "ramp", "constant", "time_only"])
def test_traced_program_reproduces_the_closure(name):
    """The bytecode interpreted by numpy against the original closure on random points: the same operations in the same order,
    so the two agree to the rounding of the few places where numpy itself takes another route (x ** 3 is pow there and two
    products here): 8 roundings relative, and exactly where the closure has comparisons and constants only."""
    fn = getattr(cases, name)
    f = pj.DeviceFunction(fn)
    assert 1 <= f.program.n_ops <= devfn.MAX_OPS
    for t in TIMES:
        got, want = f.evaluate_program(PTS, t), _closure_values(fn, PTS, t)
        assert got.shape == want.shape == (len(PTS),)
        assert np.all(np.abs(got - want) <= 8 * cases.EPS * np.abs(want)), (name, t, np.max(np.abs(got - want)))
        assert np.array_equal(f(PTS[:, 0], PTS[:, 1], PTS[:, 2], t), fn(PTS[:, 0], PTS[:, 1], PTS[:, 2], t))   # __call__: the original
    if name in ("ramp", "constant"):
        assert np.array_equal(f.evaluate_program(PTS, 0.3), _closure_values(fn, PTS, 0.3))


def test_arithmetic_sqrt_and_squares_agree_to_the_last_bit():
    f = pj.DeviceFunction(cases.rational)
    used = {devfn.OPCODES[f.program.op[q]] for q in range(f.program.n_ops)}
    assert used <= {"CONST", "VAR", "ADD", "SUB", "MUL", "DIV", "SQRT"}
    for t in TIMES:
        assert np.array_equal(f.evaluate_program(PTS, t), _closure_values(cases.rational, PTS, t))


def test_border_and_source_arities_are_traced_per_use_site():
    f = pj.DeviceFunction(cases.border_2d)
    p2 = f.program_for(2)
    assert [devfn.OPCODES[p2.op[q]] for q in range(p2.n_ops)].count("VAR") == 3
    assert {p2.arg[q] for q in range(p2.n_ops) if p2.op[q] == devfn.OP["VAR"]} == {0, 1, 3}      # x, y and t -- never z
    xy = PTS[:, :2]
    assert np.array_equal(f.evaluate_program(xy, 0.7, nspace=2), _closure_values(cases.border_2d, xy, 0.7, nspace=2))
    with pytest.raises(pj.PenguinHipError, match="cannot trace"):
        f.program                                      # border_2d takes (x, y, t): four arguments are one too many
    # the drivers see the closure's own signature, not __call__(*args)
    assert api._accepts(f, 3) and not api._accepts(f, 4)
    assert api._time_dependent(pj.DeviceFunction(cases.constant), 3) and not api._time_dependent(pj.DeviceFunction(lambda x, y, z: x), 3)
    # small integer powers are products, anything else is POW
    names = lambda fn: [devfn.OPCODES[o] for o in bytes(pj.DeviceFunction(fn).program.op)[:pj.DeviceFunction(fn).program.n_ops]]
    assert names(lambda x, y, z, t: x ** 3) == ["VAR", "VAR", "MUL", "VAR", "MUL"]
    assert names(lambda x, y, z, t: x ** 0) == ["CONST"]
    assert "POW" in names(lambda x, y, z, t: x ** 5) and "POW" in names(lambda x, y, z, t: x ** 0.5)
    assert "POW" in names(lambda x, y, z, t: 2.0 ** x) and "POW" in names(lambda x, y, z, t: x ** -1)
    # an exponent that is no integer at all, inf or NaN, is POW too, not a failed trace
    assert "POW" in names(lambda x, y, z, t: x ** float("inf")) and "POW" in names(lambda x, y, z, t: x ** np.float64("nan"))
    assert names(lambda x, y, z, t: np.where(x < t, y, z)) == ["VAR", "VAR", "LT", "VAR", "VAR", "SELECT"]


@pytest.mark.parametrize("fn,what", [
    (lambda x, y, z, t: math.exp(x), "float()"),
    (lambda x, y, z, t: x if x > 0 else t, "Python branch"),
    (lambda x, y, z, t: np.arcsin(x), "numpy.arcsin"),
    (lambda x, y, z, t: x % 2.0, "%"),
    (lambda x, y, z, t: x == y, "=="),
    (lambda x, y, z, t: np.array([x, y]), "ndarray"),
    (lambda x, y, z, t: "text", "str"),
])
def test_untraceable_closures_are_refused_by_name(fn, what):
    with pytest.raises(pj.PenguinHipError) as e:
        pj.DeviceFunction(fn).program
    assert what in str(e.value), str(e.value)


def test_too_many_instructions_constants_and_too_deep_a_stack_are_refused():
    def long_sum(x, y, z, t):
        s = x
        for k in range(48):
            s = s + y                                 # 1 + 2 * 48 = 97 instructions
        return s
    with pytest.raises(pj.PenguinHipError, match="more than 96 instructions"):
        pj.DeviceFunction(long_sum).program

    def one_less(x, y, z, t):
        s = -x
        for k in range(47):
            s = s + y                                 # 2 + 2 * 47 = 96
        return s
    assert pj.DeviceFunction(one_less).program.n_ops == 96

    def many_constants(x, y, z, t):
        s = x
        for k in range(33):
            s = s * (1.0 + k / 64.0)
        return s
    with pytest.raises(pj.PenguinHipError, match="more than 32 distinct constants"):
        pj.DeviceFunction(many_constants).program

    def right_deep(depth):
        def fn(x, y, z, t):
            def rec(k):
                return t if k == 1 else x + rec(k - 1)      # x + (x + (x + ... t)): depth operands on the stack
            return rec(depth)
        return fn
    assert pj.DeviceFunction(right_deep(16)).program.n_ops == 31
    with pytest.raises(pj.PenguinHipError, match="operand stack of 17"):
        pj.DeviceFunction(right_deep(17)).program


# ------------------------------------------------------------------------------------ validator and host interpreter
MALFORMED = [
    ("n_ops = 0", lambda: raw_program([], []), "n_ops = 0 is outside"),
    ("n_ops = 97", lambda: _with(raw_program([("VAR", 0)], []), n_ops=97), "n_ops = 97 is outside"),
    ("n_ops < 0", lambda: _with(raw_program([("VAR", 0)], []), n_ops=-5), "n_ops = -5 is outside"),
    ("n_const = 33", lambda: _with(raw_program([("VAR", 0)], []), n_const=33), "n_const = 33 is outside"),
    ("n_const < 0", lambda: _with(raw_program([("VAR", 0)], []), n_const=-1), "n_const = -1 is outside"),
    ("unknown opcode", lambda: raw_program([("VAR", 0), (25, 0)], []), "instruction 1: unknown opcode 25"),
    ("opcode 255", lambda: raw_program([(255, 0)], []), "instruction 0: unknown opcode 255"),
    ("constant index", lambda: raw_program([("CONST", 2)], [1.0, 2.0]), "instruction 0: constant index 2 with 2 constants"),
    ("constant without pool", lambda: raw_program([("CONST", 0)], []), "constant index 0 with 0 constants"),
    ("variable index", lambda: raw_program([("VAR", 4)], []), "instruction 0: variable index 4"),
    ("unary underflow", lambda: raw_program([("NEG", 0)], []), "instruction 0: stack underflow (1 operands needed, 0 there)"),
    ("binary underflow", lambda: raw_program([("VAR", 0), ("ADD", 0)], []), "instruction 1: stack underflow (2 operands needed, 1 there)"),
    ("select underflow", lambda: raw_program([("VAR", 0), ("VAR", 1), ("SELECT", 0)], []), "instruction 2: stack underflow (3 operands needed, 2 there)"),
    ("too deep", lambda: raw_program([("VAR", 0)] * 17 + [("ADD", 0)] * 16, []), "instruction 16: stack deeper than 16"),
    ("two left", lambda: raw_program([("VAR", 0), ("VAR", 1)], []), "ends with 2 values"),
    ("three left", lambda: raw_program([("VAR", 0), ("VAR", 1), ("VAR", 3)], []), "ends with 3 values"),
]


def _with(p, **kw):
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("label,make,message", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_validator_refuses_each_malformed_program_with_its_own_message(label, make, message):
    """... and the interpreter runs none of them: the output array keeps what it held."""
    lib, p = L.lib(), make()
    assert lib.pg_program_validate(C.byref(p)) != 0
    assert message in _last_error(), _last_error()
    pts, out = np.ones((4, 3)), np.full(4, -7.0)
    assert lib.pg_program_eval_host(C.byref(p), C.c_int64(4), L.dptr(pts), C.c_double(0.0), L.dptr(out)) != 0
    assert message in _last_error() and np.all(out == -7.0)


def test_validator_accepts_the_limits_and_null_is_refused():
    lib = L.lib()
    for p in (cases.full_length_program(), cases.depth16_program(), cases.all_opcodes_program(), raw_program([("VAR", 3)], [])):
        assert lib.pg_program_validate(C.byref(p)) == 0, _last_error()
    assert lib.pg_program_validate(None) != 0 and "NULL program" in _last_error()
    p = raw_program([("VAR", 0)], [])
    assert lib.pg_program_eval_host(C.byref(p), C.c_int64(3), None, C.c_double(0.0), None) != 0
    assert lib.pg_program_eval_host(C.byref(p), C.c_int64(0), None, C.c_double(0.0), None) == 0


@pytest.mark.parametrize("name", ["problem5_source", "moving_gaussian", "erfc_profile", "ramp", "constant", "time_only", "rational"])
def test_host_interpreter_against_the_numpy_interpretation(name):
    """The same bytecode through the library's host interpreter and through numpy: identical where every operation is
    correctly rounded, and within 4 roundings per libm call chained (numpy's vector exp / sin and glibc's differ by an ulp)."""
    p = pj.DeviceFunction(getattr(cases, name)).program
    out = np.empty(len(PTS))
    for t in TIMES:
        L.check(L.lib().pg_program_eval_host(C.byref(p), C.c_int64(len(PTS)), L.dptr(np.ascontiguousarray(PTS)), C.c_double(t), L.dptr(out)))
        want = devfn.interpret(p, PTS, t)
        if name in ("ramp", "constant", "rational"):
            assert np.array_equal(out, want)
        else:
            assert np.all(np.abs(out - want) <= 16 * cases.EPS * np.abs(want)), (name, t, np.max(np.abs(out - want) / np.abs(want)))


def test_every_opcode_program_host_against_long_double():
    p = cases.all_opcodes_program()
    pts = RNG.uniform(0.5, 1.5, size=(300, 3))
    out = np.empty(len(pts))
    L.check(L.lib().pg_program_eval_host(C.byref(p), C.c_int64(len(pts)), L.dptr(pts), C.c_double(0.375), L.dptr(out)))
    ref = devfn.interpret(p, pts, 0.375, dtype=np.longdouble, erf_fn=cases.erf_ld, erfc_fn=cases.erfc_ld)
    assert cases.worst_rel_error(out, ref) <= 16 * cases.EPS      # 23 chained terms, each within an ulp


# ------------------------------------------------------------------------------------ the table of times
@pytest.mark.parametrize("dt,Te,max_steps", [(0.1, 1.0, None), (0.1, 0.95, None), (1.0 / 3.0, 2.0, None), (0.05, 10.0, 7), (0.3, 0.0, None)])
def test_table_of_times_is_a_literal_replay_of_the_loops_clock(dt, Te, max_steps):
    want = []
    t, steps = 0.0, 0
    while t < Te:
        if max_steps is not None and steps >= max_steps:
            break
        t += dt
        want.append((t, t + dt))                      # the two times the host-driven loop evaluates its closures at
        steps += 1
    got = api._program_times(dt, Te, max_steps)
    assert got.shape == (len(want), 2) and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got, np.array(want).reshape(len(want), 2))
    # ... and row for row the clock of the separable tables
    tab = api._separable_table([lambda t: t], dt, Te, max_steps)
    assert np.array_equal(tab.reshape(-1, 2), got)


# ------------------------------------------------------------------------------------ the symbols
NEW_SYMBOLS = ["pg_program_validate", "pg_program_eval_host", "pg_solver_set_program", "pg_solver_set_border_program",
               "pg_solver_program_info", "pg_debug_program_eval", "pg_debug_td_eval_ms"]


def test_new_symbols_in_the_header_the_library_and_the_julia_twin():
    hdr = (ROOT / "include" / "penguin_hip.h").read_text(encoding="utf-8")
    jl = (ROOT / "julia" / "PenguinHIP.jl").read_text(encoding="utf-8")
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, hdr), name
        assert getattr(lib, name) is not None
    for name in ("pg_solver_set_program", "pg_solver_set_border_program", "pg_program_validate", "pg_program_eval_host"):
        assert f"(:{name}, libpg)" in jl, name
    assert "struct DeviceFunction" in jl and "struct Sym" in jl
    # the Python mirror of the struct and of the opcodes is the header's
    assert C.sizeof(devfn.pg_program) == 8 + 2 * 96 + 8 * 32
    for k, name in enumerate(devfn.OPCODES):
        assert re.search(r"\bPG_OP_%s = %d\b" % (name, k), hdr), name
    assert re.search(r"PG_OP_COUNT = %d\b" % len(devfn.OPCODES), hdr)
    m = re.search(r"PG_PROG_MAX_OPS = (\d+), PG_PROG_MAX_CONST = (\d+), PG_PROG_MAX_STACK = (\d+)", hdr)
    assert tuple(int(v) for v in m.groups()) == (devfn.MAX_OPS, devfn.MAX_CONST, devfn.MAX_STACK)
    # the Julia twin numbers its opcodes the same way
    for k, name in enumerate(devfn.OPCODES):
        assert re.search(r"\bPG_OP_%s = UInt8\(%d\)" % (name, k), jl), name


# ------------------------------------------------------------------------------------ under ASan + UBSan, stand-alone
def _py_validate(rec: bytes) -> bool:
    p = devfn.pg_program.from_buffer_copy(rec)
    if not (1 <= p.n_ops <= 96 and 0 <= p.n_const <= 32):
        return False
    depth = 0
    for q in range(p.n_ops):
        op, arg = p.op[q], p.arg[q]
        if op >= len(devfn.OPCODES) or (op == 0 and arg >= p.n_const) or (op == 1 and arg > 3):
            return False
        need = devfn._ARITY[devfn.OPCODES[op]]
        if depth < need:
            return False
        depth += 1 - need
        if depth > 16:
            return False
    return depth == 1


def _random_records(n):
    rng = np.random.default_rng(2024)
    size = C.sizeof(devfn.pg_program)
    out = []
    for k in range(n):
        rec = bytearray(rng.integers(0, 256, size=size, dtype=np.uint8).tobytes())
        if k % 2:                                     # half of them with counts in range, opcodes and operands likely valid:
            p = devfn.pg_program.from_buffer(rec)     # these reach the walk over the instructions, some the interpreter
            p.n_ops, p.n_const = int(rng.integers(1, 12)), int(rng.integers(0, 33))
            for q in range(p.n_ops):
                p.op[q], p.arg[q] = int(rng.integers(0, 26)), int(rng.integers(0, 5))
            if k % 4 == 1:                            # ... and a quarter built to be valid: operands first, then operations
                nv = int(rng.integers(1, 9))
                ops = [(int(rng.integers(0, 2)), 0) for _ in range(nv)] + [(int(rng.choice([2, 3, 4, 5, 14, 15, 18, 19, 20, 23])), 0)] * (nv - 1)
                ops += [(int(rng.integers(6, 14)), 0)] * int(rng.integers(0, 3))
                p.n_ops, p.n_const = len(ops), 4
                for q, (o, _) in enumerate(ops):
                    p.op[q], p.arg[q] = o, int(rng.integers(0, 4))
            del p
        out.append(bytes(rec))
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_validator_and_interpreter_stand_alone_under_asan_ubsan():
    """Valid, malformed and random byte strings through program_validate and the host interpreter in a program of their own,
    built from pg_program.h with -fsanitize=address,undefined: every verdict as the restatement above gives it, the valid
    programs' values as numpy interprets them, and not a word from either sanitizer."""
    BUILD.mkdir(exist_ok=True)
    exe = BUILD / "program_host_asan"
    subprocess.run(["g++", "-std=c++17", *FLAGS, str(ROOT / "tests" / "program_host.cpp"), "-o", str(exe)], check=True, cwd=ROOT)
    valid = [pj.DeviceFunction(getattr(cases, n)).program for n in ("problem5_source", "ramp", "erfc_profile", "rational")]
    valid += [cases.full_length_program(), cases.depth16_program(), cases.all_opcodes_program()]
    records = [bytes(p) for p in valid] + [bytes(make()) for _, make, _ in MALFORMED] + _random_records(3000)
    feed = BUILD / "program_records.bin"
    feed.write_bytes(b"".join(records))
    npts = 16
    r = subprocess.run([str(exe), str(feed), str(npts)], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == f"all records done {len(records)}" and len(lines) == len(records) + 1
    i = np.arange(npts)
    pts = np.stack([0.5 + ((i * 37) % 101) / 101.0, 0.5 + ((i * 53) % 103) / 103.0, 0.5 + ((i * 71) % 107) / 107.0], axis=1)
    accepted = 0
    for k, (rec, line) in enumerate(zip(records, lines)):
        ok = line.startswith("ok")
        assert ok == _py_validate(rec), (k, line[:120])
        if k < len(valid):
            assert ok
            got = np.array([int(w, 16) for w in line.split()[1:]], dtype=np.uint64).view(np.float64)
            want = devfn.interpret(valid[k], pts, 0.375)
            assert np.all(np.abs(got - want) <= 16 * cases.EPS * np.abs(want)), k
        elif k < len(valid) + len(MALFORMED):
            assert line.startswith("bad ") and MALFORMED[k - len(valid)][2] in line, line
        accepted += ok
    assert accepted >= len(valid) + 300, accepted          # the random records did reach the interpreter
