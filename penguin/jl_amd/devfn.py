"""Device functions: a scalar closure of (coordinates..., t) traced ONCE into the postfix program the library evaluates on the
device every step (include/penguin_hip.h pg_program; DESIGN.md "Device functions").

    f = pj.DeviceFunction(lambda x, y, z, t: np.exp(-(x * x + y * y) / (t + 1.0)) / (t + 1.0))

The closure is called with symbolic operands (Sym) which overload the arithmetic operators, the comparisons and numpy's
ufuncs; `pj.dev.select / erf / erfc / atan2` cover what numpy lacks.  What cannot be traced -- math.exp, a Python `if` on a
symbol, a ufunc without an opcode, more than 96 instructions -- raises PenguinHipError naming the operation: nothing falls back
silently.  The object stays an ordinary callable that forwards to the ORIGINAL closure, so constructors, a CPU reference and the
host-driven loop use it as a plain closure and a wrong trace shows up as a difference."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Tuple

import numpy as np

from ._lib import PenguinHipError

MAX_OPS, MAX_CONST, MAX_STACK = 96, 32, 16      # PG_PROG_MAX_*

OPCODES = ["CONST", "VAR", "ADD", "SUB", "MUL", "DIV", "NEG", "ABS", "SQRT", "EXP", "LOG", "SIN", "COS", "TANH", "POW", "ATAN2",
           "ERF", "ERFC", "MIN", "MAX", "LT", "LE", "GT", "GE", "SELECT"]
OP = {name: k for k, name in enumerate(OPCODES)}     # PG_OP_*
_UNARY = {"NEG", "ABS", "SQRT", "EXP", "LOG", "SIN", "COS", "TANH", "ERF", "ERFC"}
_ARITY = {name: (0 if name in ("CONST", "VAR") else 1 if name in _UNARY else 3 if name == "SELECT" else 2) for name in OPCODES}
MAX_INT_POW = 4        # x ** k, k = 0 .. 4 an integer: multiplications; anything else: POW


class pg_program(C.Structure):
    _fields_ = [("n_ops", C.c_int32), ("n_const", C.c_int32), ("op", C.c_uint8 * MAX_OPS), ("arg", C.c_uint8 * MAX_OPS),
                ("konst", C.c_double * MAX_CONST)]


def _is_number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) or (isinstance(v, np.ndarray) and v.ndim == 0)


class Sym:
    """A node of the traced expression: ("CONST", value) / ("VAR", i) / (opcode name, operands...)."""

    __slots__ = ("op", "args")
    __array_priority__ = 1000.0

    def __init__(self, op, *args):
        self.op, self.args = op, args

    # ---- construction
    @staticmethod
    def wrap(v, what="an operand") -> "Sym":
        if isinstance(v, Sym):
            return v
        if _is_number(v):
            return Sym("CONST", float(v))
        raise PenguinHipError(f"DeviceFunction: cannot trace {what} of type {type(v).__name__} (scalars and traced values only)")

    @staticmethod
    def make(op, *args) -> "Sym":
        return Sym(op, *[Sym.wrap(a, f"an operand of {op}") for a in args])

    # ---- arithmetic
    def __add__(self, o): return Sym.make("ADD", self, o)
    def __radd__(self, o): return Sym.make("ADD", o, self)
    def __sub__(self, o): return Sym.make("SUB", self, o)
    def __rsub__(self, o): return Sym.make("SUB", o, self)
    def __mul__(self, o): return Sym.make("MUL", self, o)
    def __rmul__(self, o): return Sym.make("MUL", o, self)
    def __truediv__(self, o): return Sym.make("DIV", self, o)
    def __rtruediv__(self, o): return Sym.make("DIV", o, self)
    def __neg__(self): return Sym.make("NEG", self)
    def __pos__(self): return self
    def __abs__(self): return Sym.make("ABS", self)

    def __pow__(self, e, mod=None):
        if mod is not None:
            raise PenguinHipError("DeviceFunction: cannot trace pow with a modulus")
        if _is_number(e) and math.isfinite(e) and float(e) == int(e) and 0 <= int(e) <= MAX_INT_POW:
            k = int(e)
            if k == 0:
                return Sym("CONST", 1.0)
            out = self
            for _ in range(k - 1):
                out = Sym("MUL", out, self)
            return out
        return Sym.make("POW", self, e)

    def __rpow__(self, b): return Sym.make("POW", b, self)

    # ---- comparisons (1.0 / 0.0)
    def __lt__(self, o): return Sym.make("LT", self, o)
    def __le__(self, o): return Sym.make("LE", self, o)
    def __gt__(self, o): return Sym.make("GT", self, o)
    def __ge__(self, o): return Sym.make("GE", self, o)

    def __eq__(self, o):
        raise PenguinHipError("DeviceFunction: cannot trace == on a traced value (the program format has <, <=, >, >= and select)")

    def __ne__(self, o):
        raise PenguinHipError("DeviceFunction: cannot trace != on a traced value (the program format has <, <=, >, >= and select)")

    __hash__ = None

    # ---- what cannot be traced
    def __bool__(self):
        raise PenguinHipError("DeviceFunction: cannot trace a Python branch (`if`, `and`, `or`, `not`, min / max builtins) on a "
                              "traced value; use pj.dev.select(cond, a, b), np.minimum or np.maximum")

    def __float__(self):
        raise PenguinHipError("DeviceFunction: cannot trace float() of a traced value (math.exp, math.sin, ... take floats: use "
                              "numpy's functions or pj.dev.*)")

    __int__ = __index__ = __complex__ = __float__

    def __floordiv__(self, o):
        raise PenguinHipError("DeviceFunction: cannot trace // (no opcode)")

    def __mod__(self, o):
        raise PenguinHipError("DeviceFunction: cannot trace % (no opcode)")

    __rfloordiv__, __rmod__ = __floordiv__, __mod__

    def __iter__(self):
        raise PenguinHipError("DeviceFunction: cannot trace iteration over a traced value (it is a scalar)")

    # ---- numpy
    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        name = ufunc.__name__
        if method != "__call__" or kwargs:
            raise PenguinHipError(f"DeviceFunction: cannot trace numpy.{name}.{method} with these arguments")
        if name in _UFUNC_1 and len(inputs) == 1:
            return Sym.make(_UFUNC_1[name], *inputs)
        if name in _UFUNC_2 and len(inputs) == 2:
            return Sym.make(_UFUNC_2[name], *inputs)
        if name == "square":
            return Sym.wrap(inputs[0]) ** 2
        if name == "positive":
            return Sym.wrap(inputs[0])
        if name == "reciprocal":
            return Sym.make("DIV", 1.0, inputs[0])
        if name in ("power", "float_power"):
            return Sym.wrap(inputs[0]) ** inputs[1] if not isinstance(inputs[1], Sym) else Sym.make("POW", *inputs)
        raise PenguinHipError(f"DeviceFunction: cannot trace numpy.{name} (no opcode)")

    def __array_function__(self, func, types, args, kwargs):
        if func is np.where and len(args) == 3 and not kwargs:
            return select(*args)
        raise PenguinHipError(f"DeviceFunction: cannot trace numpy.{func.__name__} on a traced value")


_UFUNC_1 = {"negative": "NEG", "absolute": "ABS", "fabs": "ABS", "sqrt": "SQRT", "exp": "EXP", "log": "LOG", "sin": "SIN",
            "cos": "COS", "tanh": "TANH"}
_UFUNC_2 = {"add": "ADD", "subtract": "SUB", "multiply": "MUL", "divide": "DIV", "true_divide": "DIV", "arctan2": "ATAN2",
            "minimum": "MIN", "fmin": "MIN", "maximum": "MAX", "fmax": "MAX", "less": "LT", "less_equal": "LE", "greater": "GT",
            "greater_equal": "GE"}


# ---- pj.dev: what numpy lacks, on traced values and on numbers / arrays alike ---------------------------------------------------

try:                                            # (vectorised erf / erfc for the closure's calls with arrays)
    from scipy.special import erf as _np_erf, erfc as _np_erfc
except Exception:                               # pragma: no cover
    _np_erf, _np_erfc = np.vectorize(math.erf, otypes=[np.float64]), np.vectorize(math.erfc, otypes=[np.float64])


def _traced(*vs) -> bool:
    return any(isinstance(v, Sym) for v in vs)


def erf(x):
    return Sym.make("ERF", x) if _traced(x) else _np_erf(x)


def erfc(x):
    return Sym.make("ERFC", x) if _traced(x) else _np_erfc(x)


def atan2(y, x):
    return Sym.make("ATAN2", y, x) if _traced(y, x) else np.arctan2(y, x)


def select(cond, a, b):
    """a where cond is not zero, b elsewhere (cond: a comparison of traced values, or a boolean / array)."""
    if _traced(cond, a, b):
        return Sym.make("SELECT", cond, a, b)
    return np.where(np.asarray(cond) != 0, a, b)


# ---- trace -> bytecode --------------------------------------------------------------------------------------------------------

def _compile(root: Sym, what: str) -> pg_program:
    ops: List[Tuple[int, int]] = []
    consts: List[float] = []
    where: Dict[bytes, int] = {}
    depth = deepest = 0
    stack = [(root, False)]                      # explicit post-order walk: operands left to right, then the operation
    while stack:
        node, done = stack.pop()
        if not done and node.op not in ("CONST", "VAR"):
            stack.append((node, True))
            for a in reversed(node.args):
                stack.append((a, False))
            continue
        if node.op == "CONST":
            key = np.float64(node.args[0]).tobytes()         # (by bits: -0.0 and 0.0, every NaN, stay what they are)
            if key not in where:
                if len(consts) == MAX_CONST:
                    raise PenguinHipError(f"DeviceFunction: {what} needs more than {MAX_CONST} distinct constants")
                where[key] = len(consts)
                consts.append(float(node.args[0]))
            ops.append((OP["CONST"], where[key]))
        elif node.op == "VAR":
            ops.append((OP["VAR"], node.args[0]))
        else:
            ops.append((OP[node.op], 0))
        depth += 1 - _ARITY[node.op]
        deepest = max(deepest, depth)
        if len(ops) > MAX_OPS:
            raise PenguinHipError(f"DeviceFunction: {what} needs more than {MAX_OPS} instructions (x ** k and repeated "
                                  "subexpressions are emitted every time they occur)")
    if deepest > MAX_STACK:
        raise PenguinHipError(f"DeviceFunction: {what} needs an operand stack of {deepest} values, more than {MAX_STACK} "
                              "(regroup the expression: a + (b + (c + ...)) nests, ((a + b) + c) + ... does not)")
    p = pg_program()
    p.n_ops, p.n_const = len(ops), len(consts)
    for q, (o, a) in enumerate(ops):
        p.op[q], p.arg[q] = o, a
    for k, v in enumerate(consts):
        p.konst[k] = v
    return p


# ---- derivatives of a trace (the level-set bodies: Capacity(DeviceFunction(...), mesh)) ----------------------------------------

def _const(s: Sym) -> Optional[float]:
    return s.args[0] if s.op == "CONST" else None


def _k(v: float) -> Sym:
    return Sym("CONST", float(v))


# the four operations with the folds that keep a derivative short: 0 * x, 1 * x, x + 0, x - 0, 0 / x, x / 1, and constants
def _add(a: Sym, b: Sym) -> Sym:
    ca, cb = _const(a), _const(b)
    if ca is not None and cb is not None:
        return _k(ca + cb)
    if ca == 0.0:
        return b
    if cb == 0.0:
        return a
    return Sym("ADD", a, b)


def _neg(a: Sym) -> Sym:
    if _const(a) is not None:
        return _k(-_const(a))
    if a.op == "NEG":
        return a.args[0]
    return Sym("NEG", a)


def _sub(a: Sym, b: Sym) -> Sym:
    ca, cb = _const(a), _const(b)
    if ca is not None and cb is not None:
        return _k(ca - cb)
    if cb == 0.0:
        return a
    if ca == 0.0:
        return _neg(b)
    return Sym("SUB", a, b)


def _mul(a: Sym, b: Sym) -> Sym:
    ca, cb = _const(a), _const(b)
    if ca is not None and cb is not None:
        return _k(ca * cb)
    if ca == 0.0 or cb == 0.0:
        return _k(0.0)
    if ca == 1.0:
        return b
    if cb == 1.0:
        return a
    if ca == -1.0:
        return _neg(b)
    if cb == -1.0:
        return _neg(a)
    return Sym("MUL", a, b)


def _div(a: Sym, b: Sym) -> Sym:
    ca, cb = _const(a), _const(b)
    if ca == 0.0:
        return _k(0.0)
    if cb == 1.0:
        return a
    if ca is not None and cb is not None and cb != 0.0:
        return _k(ca / cb)
    return Sym("DIV", a, b)


def _select(c: Sym, a: Sym, b: Sym) -> Sym:
    if _const(a) is not None and _const(a) == _const(b):
        return a
    return Sym("SELECT", c, a, b)


def differentiate(node: Sym, var: int) -> Sym:
    """d node / d x_var as a trace: one rule per opcode.  ABS, MIN, MAX and SELECT are piecewise through SELECT (the derivative of
    the branch the value comes from), comparisons have derivative 0, POW with a constant exponent has its own rule."""
    op, a = node.op, node.args
    if op == "CONST":
        return _k(0.0)
    if op == "VAR":
        return _k(1.0 if a[0] == var else 0.0)
    if op in ("LT", "LE", "GT", "GE"):
        return _k(0.0)
    d = [differentiate(x, var) for x in a]
    if op == "SELECT":
        return _select(a[0], d[1], d[2])
    if op == "ADD":
        return _add(d[0], d[1])
    if op == "SUB":
        return _sub(d[0], d[1])
    if op == "NEG":
        return _neg(d[0])
    if op == "MUL":
        return _add(_mul(d[0], a[1]), _mul(a[0], d[1]))
    if op == "DIV":
        if _const(d[1]) == 0.0:
            return _div(d[0], a[1])
        return _div(_sub(_mul(d[0], a[1]), _mul(a[0], d[1])), _mul(a[1], a[1]))
    if op == "MIN":
        return _select(Sym("LE", a[0], a[1]), d[0], d[1])
    if op == "MAX":
        return _select(Sym("GE", a[0], a[1]), d[0], d[1])
    if op == "POW":
        e = _const(a[1])
        if e is not None:                        # u ** e: e u ** (e - 1) u'
            return _mul(_mul(_k(e), Sym("POW", a[0], _k(e - 1.0))), d[0])
        out = _mul(_mul(node, Sym("LOG", a[0])), d[1])          # u ** v: u ** v (v' log u + v u' / u)
        if _const(d[0]) != 0.0:
            out = _add(out, _mul(node, _div(_mul(a[1], d[0]), a[0])))
        return out
    if op == "ATAN2":                            # atan2(y, x): (x y' - y x') / (x x + y y)
        return _div(_sub(_mul(a[1], d[0]), _mul(a[0], d[1])), _add(_mul(a[0], a[0]), _mul(a[1], a[1])))
    u, du = a[0], d[0]
    if _const(du) == 0.0:
        return _k(0.0)
    if op == "ABS":
        return _select(Sym("GE", u, _k(0.0)), du, _neg(du))
    if op == "SQRT":
        return _div(du, _mul(_k(2.0), node))
    if op == "EXP":
        return _mul(node, du)
    if op == "LOG":
        return _div(du, u)
    if op == "SIN":
        return _mul(Sym("COS", u), du)
    if op == "COS":
        return _neg(_mul(Sym("SIN", u), du))
    if op == "TANH":
        return _mul(_sub(_k(1.0), _mul(node, node)), du)
    if op in ("ERF", "ERFC"):
        g = _mul(_k((2.0 if op == "ERF" else -2.0) / math.sqrt(math.pi)), Sym("EXP", _neg(_mul(u, u))))
        return _mul(g, du)
    raise PenguinHipError(f"DeviceFunction: no derivative rule for {op}")


def program_listing(p: pg_program) -> List[str]:
    out = []
    for q in range(p.n_ops):
        name = OPCODES[p.op[q]] if p.op[q] < len(OPCODES) else f"?{p.op[q]}"
        out.append(f"{name} {p.konst[p.arg[q]]!r}" if name == "CONST" else f"VAR {'xyzt'[p.arg[q]]}" if name == "VAR" else name)
    return out


def interpret(p: pg_program, coords, t, dtype=np.float64, erf_fn=None, erfc_fn=None) -> np.ndarray:
    """The bytecode interpreted with numpy at the rows of coords (npts x up to 3 columns, missing ones 0) and the time t: what the
    device computes, operation for operation.  dtype=np.longdouble gives a reference of higher precision (erf_fn / erfc_fn:
    functions of that precision; numpy has none)."""
    coords = np.asarray(coords, dtype=dtype)
    if coords.ndim == 1:
        coords = coords[:, None]
    n = coords.shape[0]
    var = [coords[:, d] if d < coords.shape[1] else np.zeros(n, dtype=dtype) for d in range(3)] + [np.full(n, t, dtype=dtype)]
    one, zero = dtype(1.0), dtype(0.0)
    f_erf = erf_fn or (lambda x: _np_erf(x).astype(dtype))
    f_erfc = erfc_fn or (lambda x: _np_erfc(x).astype(dtype))
    un = {"NEG": np.negative, "ABS": np.abs, "SQRT": np.sqrt, "EXP": np.exp, "LOG": np.log, "SIN": np.sin, "COS": np.cos,
          "TANH": np.tanh, "ERF": f_erf, "ERFC": f_erfc}
    bi = {"ADD": np.add, "SUB": np.subtract, "MUL": np.multiply, "DIV": np.divide, "POW": np.power, "ATAN2": np.arctan2,
          "MIN": np.fmin, "MAX": np.fmax, "LT": np.less, "LE": np.less_equal, "GT": np.greater, "GE": np.greater_equal}
    st: List[np.ndarray] = []
    with np.errstate(all="ignore"):
        for q in range(p.n_ops):
            name = OPCODES[p.op[q]]
            if name == "CONST":
                st.append(np.full(n, p.konst[p.arg[q]], dtype=dtype))
            elif name == "VAR":
                st.append(var[p.arg[q]])
            elif name in un:
                st.append(np.asarray(un[name](st.pop()), dtype=dtype))
            elif name == "SELECT":
                b, a, c = st.pop(), st.pop(), st.pop()
                st.append(np.where(c != zero, a, b))
            else:
                b, a = st.pop(), st.pop()
                r = bi[name](a, b)
                st.append(np.where(r, one, zero) if r.dtype == np.bool_ else np.asarray(r, dtype=dtype))
    assert len(st) == 1
    return np.ascontiguousarray(st[0], dtype=dtype)


class DeviceFunction:
    """DeviceFunction(fn): fn(x, y, z, t) for sources and interface values (three coordinates, the missing ones of a 1-D / 2-D
    problem 0.0, as the constructors call every closure), fn(x_1 .. x_N, t) for the value of a border condition.  Traced per
    use site: `.program` is the three-coordinate trace, `program_for(nspace)` the one of another arity.

    As the body of a Capacity, fn(x_1 .. x_N) is a level set with the fluid where it is <= 0: `body_program(N)` is its trace
    and `gradient_programs(N)` the N traces of its partial derivatives, differentiated rule by rule from that trace.
    `complement=True` is the body -fn (the other phase of a two-phase problem; `Capacity(body, mesh, complement=True)` sets it):
    calls return -fn, the body programs stay fn's and the capacity kernels negate.  Such an object is a body only: `program_for`
    (time-dependent data) refuses it.

    As the body of a space-time Capacity (the prescribed-motion solvers), fn(x_1 .. x_N, t) is a moving level set:
    `moving_body_program(N)` and `moving_gradient_programs(N)` (the N spatial derivatives, then d/dt)."""

    def __init__(self, fn, complement: bool = False):
        if isinstance(fn, DeviceFunction):
            complement = complement != fn.complement
            fn = fn.fn
        self.complement = bool(complement)       # as a BODY: -fn (the traces stay those of fn, the kernels negate)
        if not callable(fn):
            raise TypeError(f"DeviceFunction takes a callable, not {fn!r}")
        self.fn = fn
        self._programs: Dict[int, pg_program] = {}
        self._bodies: Dict[int, Sym] = {}
        self.__signature__ = None
        try:
            import inspect
            self.__signature__ = inspect.signature(fn)       # the drivers ask a closure how many arguments it takes
        except (TypeError, ValueError):
            pass

    def __call__(self, *args):
        return -self.fn(*args) if self.complement else self.fn(*args)

    def __repr__(self):
        return f"DeviceFunction({self.fn!r}, complement=True)" if self.complement else f"DeviceFunction({self.fn!r})"

    def program_for(self, nspace: int) -> pg_program:
        """The program of fn(x_1 .. x_nspace, t), traced on first use."""
        if self.complement:
            raise PenguinHipError(f"{self!r}: complement=True makes a BODY (the other phase of a Capacity); as a source, an interface "
                                  "value or a border value the program would be fn's while calls give -fn: write the sign into the closure")
        if nspace not in self._programs:
            what = f"{self.fn!r} with {nspace} coordinates and t"
            args = [Sym("VAR", d) for d in range(nspace)] + [Sym("VAR", 3)]
            try:
                out = self.fn(*args)
            except PenguinHipError:
                raise
            except Exception as e:
                raise PenguinHipError(f"DeviceFunction: cannot trace {what}: {type(e).__name__}: {e}") from e
            if isinstance(out, (list, tuple)) or (isinstance(out, np.ndarray) and out.ndim > 0):
                raise PenguinHipError(f"DeviceFunction: {what} returned {type(out).__name__}, not a scalar")
            if isinstance(out, np.ndarray) and out.dtype == object:
                out = out.item()
            self._programs[nspace] = _compile(Sym.wrap(out, "the returned value"), what)
        return self._programs[nspace]

    @property
    def program(self) -> pg_program:
        return self.program_for(3)

    # ---- a level-set body: fn(x_1 .. x_N), no t
    def _body_trace(self, N: int) -> Sym:
        if N not in self._bodies:
            what = f"the body {self.fn!r} with {N} coordinates"
            try:
                out = self.fn(*[Sym("VAR", d) for d in range(N)])
            except PenguinHipError:
                raise
            except Exception as e:
                raise PenguinHipError(f"DeviceFunction: cannot trace {what}: {type(e).__name__}: {e}") from e
            if isinstance(out, (list, tuple)) or (isinstance(out, np.ndarray) and out.ndim > 0):
                raise PenguinHipError(f"DeviceFunction: {what} returned {type(out).__name__}, not a scalar")
            if isinstance(out, np.ndarray) and out.dtype == object:
                out = out.item()
            self._bodies[N] = Sym.wrap(out, "the returned value")
        return self._bodies[N]

    def body_program(self, N: int) -> pg_program:
        """The program of the level set fn(x_1 .. x_N)."""
        return _compile(self._body_trace(N), f"the body {self.fn!r} with {N} coordinates")

    def gradient_programs(self, N: int) -> List[pg_program]:
        """The N programs of the partial derivatives of fn(x_1 .. x_N), differentiated from its trace."""
        root = self._body_trace(N)
        return [_compile(differentiate(root, d), f"the derivative along coordinate {d} of the body {self.fn!r}") for d in range(N)]

    # ---- a moving level-set body: fn(x_1 .. x_N, t)
    def _moving_trace(self, N: int) -> Sym:
        key = -N                                 # (the static traces of the same object sit under N)
        if key not in self._bodies:
            what = f"the moving body {self.fn!r} with {N} coordinates and t"
            try:
                out = self.fn(*([Sym("VAR", d) for d in range(N)] + [Sym("VAR", 3)]))
            except PenguinHipError:
                raise
            except Exception as e:
                raise PenguinHipError(f"DeviceFunction: cannot trace {what}: {type(e).__name__}: {e}") from e
            if isinstance(out, (list, tuple)) or (isinstance(out, np.ndarray) and out.ndim > 0):
                raise PenguinHipError(f"DeviceFunction: {what} returned {type(out).__name__}, not a scalar")
            if isinstance(out, np.ndarray) and out.dtype == object:
                out = out.item()
            self._bodies[key] = Sym.wrap(out, "the returned value")
        return self._bodies[key]

    def moving_body_program(self, N: int) -> pg_program:
        """The program of the moving level set fn(x_1 .. x_N, t): coordinates VAR 0 .. N-1, t VAR 3.  Compiled once per object
        and N (a solve asks for it on every slab)."""
        key = ("moving body", N)
        if key not in self._programs:
            self._programs[key] = _compile(self._moving_trace(N), f"the moving body {self.fn!r} with {N} coordinates and t")
        return self._programs[key]

    def moving_gradient_programs(self, N: int) -> List[pg_program]:
        """N + 1 programs: the N spatial partial derivatives of fn(x_1 .. x_N, t), then d/dt, differentiated from its trace and
        folded like the static ones (a closure that does not read t gives the constant 0).  Compiled once per object and N."""
        key = ("moving derivatives", N)
        if key not in self._programs:
            root = self._moving_trace(N)
            body = f"the moving body {self.fn!r}"
            progs = [_compile(differentiate(root, d), f"the derivative along coordinate {d} of {body}") for d in range(N)]
            progs.append(_compile(differentiate(root, 3), f"the derivative along t of {body}"))
            self._programs[key] = tuple(progs)
        return list(self._programs[key])

    def evaluate_program(self, coords, t, nspace: Optional[int] = None, dtype=np.float64, **kw) -> np.ndarray:
        """The bytecode interpreted with numpy at the rows of coords; nspace (default: 3, the arity of sources and interface
        values) chooses the trace."""
        return interpret(self.program_for(3 if nspace is None else nspace), coords, t, dtype=dtype, **kw)
