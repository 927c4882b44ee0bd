"""Programs, closures and the long-double reference shared by tests/test_device_function_cpu.py and
tests/test_gpu_device_function.py."""
import numpy as np

from penguin.jl_amd import devfn

EPS = 2.0 ** -53          # one rounding of float64
LD = np.longdouble


def raw_program(ops, consts):
    """pg_program from [(opcode name or number, arg), ...] and the constants -- nothing is checked (malformed ones on purpose)."""
    p = devfn.pg_program()
    p.n_ops, p.n_const = len(ops), len(consts)
    for q, (o, a) in enumerate(ops[:devfn.MAX_OPS]):
        p.op[q], p.arg[q] = (devfn.OP[o] if isinstance(o, str) else o), a
    for k, v in enumerate(consts[:devfn.MAX_CONST]):
        p.konst[k] = v
    return p


def full_length_program():
    """All 96 instructions: x, then 47 times (operand, operation) alternating  acc * 0.75 + y  style steps on positive values,
    then ABS."""
    ops = [("VAR", 0)]
    for k in range(47):
        if k % 2 == 0:
            ops += [("CONST", k % 3), ("MUL", 0)]
        else:
            ops += [("VAR", 1 + k % 3), ("ADD", 0)]          # y, z, t in turn
    ops.append(("ABS", 0))
    assert len(ops) == 96
    return raw_program(ops, [0.75, 1.25, 0.9])


def depth16_program():
    """Sixteen operands on the stack -- the deepest a program may go -- folded from the top: x + (y + (z + (t + (c0 + ...))))."""
    ops = [("VAR", k) if k < 4 else ("CONST", k - 4) for k in range(16)]
    ops += [("ADD", 0) if k % 2 == 0 else ("MUL", 0) for k in range(15)]
    return raw_program(ops, [0.5 + 0.0625 * k for k in range(12)])


def all_opcodes_closure(x, y, z, t):
    d = devfn
    s = np.sqrt(x) + np.exp(-y) + np.log(z + 1.0) + np.sin(x) + np.cos(y) + np.tanh(z) + x ** y + d.atan2(y, x)
    s = s + d.erf(x) + d.erfc(y - 1.0) + np.minimum(x, y) + np.maximum(y, z) + np.abs(x - 2.0) + x / y
    s = s + d.select(x < y, x, y) + d.select(x <= z, 1.0, 2.0) * d.select(y > z, z, 0.5) + d.select(z >= x, y * t, 0.25)
    return s


def all_opcodes_program():
    """Every opcode at least once, on x, y, z in [0.5, 1.5]: every term is positive, nothing cancels."""
    p = devfn.DeviceFunction(all_opcodes_closure).program
    used = {devfn.OPCODES[p.op[q]] for q in range(p.n_ops)}
    assert used == set(devfn.OPCODES), sorted(set(devfn.OPCODES) - used)
    return p


# ---- erf / erfc in long double (numpy has neither): erf by the series of positive terms
#      erf(x) = 2/sqrt(pi) exp(-x^2) sum_n 2^n x^(2n+1) / (1 * 3 * ... * (2n+1)),
#      erfc = 1 - erf, good to a relative 1e-18 where erfc is not small: the tests keep |x| of erfc below 1.6 (erfc > 0.02)
def erf_ld(x):
    x = np.asarray(x, dtype=LD)
    a = np.abs(x)
    term = a.copy()
    total = a.copy()
    for n in range(1, 400):
        term = term * (2 * a * a) / LD(2 * n + 1)
        total = total + term
        if np.all(term <= total * LD(1e-22)):
            break
    pi = LD(4) * np.arctan(LD(1))
    return np.sign(x) * LD(2) / np.sqrt(pi) * np.exp(-a * a) * total


def erfc_ld(x):
    x = np.asarray(x, dtype=LD)
    assert np.all(x < 1.6), "erfc_ld is 1 - erf: keep erfc away from 0"
    return LD(1) - erf_ld(x)


def worst_rel_error(got, ref):
    """max |got - ref| / |ref| in long double (|ref| = 0: the absolute error, which must then be 0)."""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    den = np.where(ref == 0, LD(1), np.abs(ref))
    return float(np.max(np.abs(got - ref) / den))


# ---- the closures of the CPU tests
def problem5_source(x, y, z, t):
    """The source of the reference's Schwartz-Colella heat problem in 3-D (not separable for any K)."""
    r2 = (x - 2.0) ** 2 + (y - 2.0) ** 2 + (z - 2.0) ** 2
    return 4.0 * (r2 + 5.0 * (t + 1.0)) / (125.0 * np.pi * (t + 1.0) ** 3) * np.exp(-r2 / (5.0 * (t + 1.0)))


def moving_gaussian(x, y, z, t):
    return np.exp(-((x - 1.0 - 2.0 * t) ** 2 + (y - 2.0 + 0.5 * t) ** 2) / 0.3)


def erfc_profile(x, y, z, t):
    return devfn.erfc(x / (2.0 * np.sqrt(t + 1.0)))


def ramp(x, y, z, t):
    s = t - 0.25 * x
    return devfn.select(s < 0.0, 0.0, devfn.select(s >= 1.0, 1.0, s)) + devfn.select(y > 2.0, 0.5, 0.0) * (z <= 1.0)


def constant(x, y, z, t):
    return 0.375


def time_only(x, y, z, t):
    return np.sin(3.0 * t) / (t + 1.0)


def border_2d(x, y, t):
    return 0.5 + 0.25 * x + np.sqrt(y + 1.0) * (t + 0.5)


def rational(x, y, z, t):
    """+ - * /, sqrt and squares only: every operation is correctly rounded on every side."""
    return (x * x + np.sqrt(y * y + 1.0)) / (t + 2.0) - (z - 0.5) ** 2 * x + np.sqrt(x) / (y + 3.0)
