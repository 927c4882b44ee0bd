"""Time-separable data on the host side (no GPU): TimeSeparable evaluates Σ φ_k(x) a_k(t) as numpy does, _separable_table
replays the clock of the host-driven loop float for float, and the three C-ABI symbols are declared, exported and ccall'ed with
matching arity."""
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HDR = (ROOT / "include" / "penguin_hip.h").read_text()
JL = (ROOT / "julia" / "PenguinHIP.jl").read_text()
SYMBOLS = ("pg_solver_set_separable", "pg_solver_clear_separable", "pg_solver_time_data_info")


@pytest.fixture(scope="module")
def pj():
    import penguin.jl_amd as pj

    return pj


def test_call_matches_numpy_for_one_two_and_three_coordinates(pj):
    rng = np.random.default_rng(7)
    x, y, z = rng.standard_normal((3, 11))
    a1, a2 = (lambda t: 1.0 + t), (lambda t: math.sin(40.0 * t))
    t = 0.37
    ts1 = pj.TimeSeparable([(2.5, a1), (lambda x: np.cos(x), a2)])
    assert np.array_equal(ts1(x, t), 2.5 * a1(t) + np.cos(x) * a2(t))
    ts2 = pj.TimeSeparable([(lambda x, y: x * y, a1), (-1.0, a2)])
    assert np.array_equal(ts2(x, y, t), x * y * a1(t) + -1.0 * a2(t))
    ts3 = pj.TimeSeparable([(lambda x, y, z: x + 2 * y - z, a1), (lambda x, y, z: np.exp(z), a2), (0.25, lambda t: t * t)])
    assert np.array_equal(ts3(x, y, z, t), (x + 2 * y - z) * a1(t) + np.exp(z) * a2(t) + 0.25 * (t * t))
    # scalars in, scalar out; a φ(x, y) handed the zero-padded z of a 2-D problem takes the leading coordinates
    assert ts3(0.5, -1.0, 2.0, t) == (0.5 - 2.0 - 2.0) * a1(t) + math.exp(2.0) * a2(t) + 0.25 * (t * t)
    assert np.array_equal(ts2(x, y, np.zeros_like(x), t), ts2(x, y, t))
    # a scalar φ alone gives a scalar (constant data, as the drivers understand it)
    assert pj.TimeSeparable([(3.0, a1)])(x, y, z, t) == 3.0 * a1(t)


def test_constructor_refuses_what_the_library_would(pj):
    a = lambda t: t
    with pytest.raises(ValueError):
        pj.TimeSeparable([])
    with pytest.raises(ValueError):
        pj.TimeSeparable([(1.0, a)] * 9)
    with pytest.raises(TypeError):
        pj.TimeSeparable([(1.0, 2.0)])
    assert len(pj.TimeSeparable([(1.0, a)] * 8).terms) == 8


def _replay(dt, Tend, max_steps):
    """The host-driven loop's clock, literally (api.solve_DiffusionUnsteadyMono_b): the t of every step, already advanced."""
    ts, t, steps = [], 0.0, 0
    while t < Tend:
        if max_steps is not None and steps >= max_steps:
            break
        t += dt
        ts.append(t)
        steps += 1
    return ts


@pytest.mark.parametrize("dt,Tend,max_steps", [
    (0.1, 0.3, None),             # the replay decides the row count, not arithmetic on paper
    (0.1, 1.0, None),
    (0.011111111111111112, 6 * 0.011111111111111112, None),
    (0.07, 0.5, None),            # Tend is no multiple of dt
    (0.07, 0.5, 3),               # max_steps cuts the loop short
    (0.07, 0.5, 0),
    (0.25, 0.0, None),            # no step at all
])
def test_table_replays_the_host_loop_clock(pj, dt, Tend, max_steps):
    from penguin.jl_amd.api import _separable_table

    coefs = [lambda t: 1.0 + t, lambda t: math.sin(40.0 * t), lambda t: 1.0 if t > 3.5 * dt else 0.0]
    tab = _separable_table(coefs, dt, Tend, max_steps)
    ts = _replay(dt, Tend, max_steps)
    assert tab.shape == (len(ts), 2, 3) and tab.dtype == np.float64 and tab.flags["C_CONTIGUOUS"]
    for q, t in enumerate(ts):
        for k, a in enumerate(coefs):
            assert tab[q, 0, k] == a(t)            # the very floats: a_k at the loop's t, already advanced ...
            assert tab[q, 1, k] == a(t + dt)       # ... and at t + Δt
    # a TimeSeparable stands for its own time parts
    same = _separable_table(pj.TimeSeparable([(1.0, a) for a in coefs]), dt, Tend, max_steps)
    assert np.array_equal(same, tab)


def test_row_count_is_the_loop_count_where_rounding_decides(pj):
    from penguin.jl_amd.api import _separable_table

    # 3 * 0.1 accumulates to 0.30000000000000004 >= 0.3: three steps; eight of them to 0.7999999999999999 < 0.8: nine steps
    assert len(_separable_table([lambda t: t], 0.1, 0.3)) == len(_replay(0.1, 0.3, None)) == 3
    assert len(_separable_table([lambda t: t], 0.1, 0.8)) == len(_replay(0.1, 0.8, None)) == 9


def _balanced(txt, start):
    depth = 0
    for k in range(start, len(txt)):
        depth += txt[k] == "("
        depth -= txt[k] == ")"
        if depth == 0:
            return k + 1
    raise AssertionError("unbalanced")


def _split(args):
    out, depth, cur = [], 0, ""
    for ch in args:
        depth += ch in "({["
        depth -= ch in ")}]"
        if ch == "," and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    return [a for a in out + [cur] if a.strip()]


def test_symbols_are_declared_exported_and_ccalled_with_matching_arity():
    from penguin.jl_amd import _lib as L
    from penguin.jl_amd.build import build_library

    if not L.LIB_PATH.exists():
        build_library()
    hdr = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    declared = L.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for sym in SYMBOLS:
        assert sym in declared and sym in exported, sym
        m = re.search(r"\bint32_t\s+%s\s*\(" % sym, hdr)
        c_args = _split(hdr[m.end():_balanced(hdr, m.end() - 1) - 1])
        j = re.search(r"ccall\(\(:%s,\s*libpg\),\s*Int32,\s*\(" % sym, JL)
        assert j, f"{sym} is not ccall'ed in julia/PenguinHIP.jl"
        tend = _balanced(JL, j.end() - 1)
        types = _split(JL[j.end():tend - 1])
        values = _split(JL[tend:_balanced(JL, j.start() + len("ccall")) - 1].lstrip()[1:])
        assert len(c_args) == len(types) == len(values), (sym, len(c_args), len(types), len(values))
    assert re.search(r"enum\s*\{\s*PG_TD_SOURCE\s*=\s*0,\s*PG_TD_INTERFACE\s*=\s*1,\s*PG_TD_BORDER\s*=\s*2\s*\}", HDR)
    assert re.search(r"enum\s*\{\s*PG_TD_MAX_TERMS\s*=\s*8\s*\}", HDR)
    from penguin.jl_amd import api

    assert (api._TD_SOURCE, api._TD_INTERFACE, api._TD_BORDER, api.TimeSeparable.MAX_TERMS) == (0, 1, 2, 8)
