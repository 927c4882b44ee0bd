"""What one solve is told (KrylovCall: the start, the compact system's scatter, the multigrid hierarchy, the deferred
extrapolated state, the speculative product) is an argument of that solve and nothing of it outlives it: one handle goes
through every kind of time step in turn -- compact and quiet steps, a multigrid step, an IDR(s) step from the previous state,
a GMRES step, a change of matrix -- and every step is the oracle's; a twin handle that is asked for something the library
refuses before EVERY step takes bitwise the same steps.

P32 of test_gpu_recovery.py (3-D, n = 32, sphere at (2.01, 2.01, 2.01)) is the smallest problem of the suite whose loop system
is compact.

pg_step_info carries a solve's iterations, its verdict and its two norms; the products and host polls of a single step are not
part of the C interface (pg_run_info sums the products of a run), so the twin is held to equal iterations, equal norms to the
bit and equal states to the bit for the single steps, and to equal iterations and products for the run at the end."""
import ctypes as C

import numpy as np
import pytest

from penguin.jl_amd import _lib as L
from penguin.jl_amd import api as _api
from tests.test_gpu_recovery import RELTOL, _first, _held, _p32, _step

pytestmark = pytest.mark.gpu

# (scheme, options of the step, what the step is)
SEQUENCE = ([("BE", {}, "default")] * 4 + [("BE", {"precond": "mg-step"}, "mg-step"), ("BE", {"method": "idrs", "nshadow": 4}, "idrs"),
                                          ("BE", {"method": "gmres"}, "gmres")] + [("BE", {}, "default")] * 3 + [("CN", {}, "default")] * 3)
# refused by do_step in its first lines, before the step consumes anything: a steady system's multigrid on this unsteady solver,
# and the time loop's multigrid with a method it does not serve
REFUSED = [{"precond": "mg"}, {"precond": "mg-step", "method": "gmres"}]
RUN_STEPS = 4

_cache = {}


def _refused(s, scheme, k):
    with pytest.raises(L.PenguinHipError, match="refused"):
        _step(s, scheme, **REFUSED[k % 2])


def _run(s, scheme, steps):
    """`steps` steps of pg_solver_run: the entry that knows another step follows, hence the one that queues the next step's
    product behind a quiet step's first batch"""
    opts = _api._krylov_opts("bicgstab", {"reltol": RELTOL})
    run = L.pg_run_info()
    L.check(L.lib().pg_solver_run(s._h, C.c_double(1e300), C.c_int32(L.PG_SCHEME[scheme]), C.byref(opts), C.c_int32(0), C.c_int64(steps),
                                  C.c_int32(0), C.byref(run)))
    return run


def _sequence(pj, refuse):
    """-> per solve (iters, converged, resnorm, bnorm), the states, guess_info() after every step, the run's counts"""
    s = _p32(pj).solver()
    info, x = _first(s)
    counts, states, guesses = [(info.iters, info.converged, info.resnorm, info.bnorm)], [x], [None]
    for k, (scheme, kw, _) in enumerate(SEQUENCE):
        if refuse:
            _refused(s, scheme, k)
        info, x = _step(s, scheme, **kw)
        counts.append((info.iters, info.converged, info.resnorm, info.bnorm))
        states.append(x)
        guesses.append(s.guess_info())
    assert s.system_info(1).loop_is_compact == 1
    if refuse:
        _refused(s, "BE", 0)
    run = _run(s, "BE", RUN_STEPS)
    states.append(s._fetch_state())
    assert s.unconverged == 0
    return counts, states, guesses, (run.steps, run.total_iters, run.products, run.half_exits, run.unconverged_steps)


def _plain(pj):
    if "plain" not in _cache:
        _cache["plain"] = _sequence(pj, False)
    return _cache["plain"]


def test_every_kind_of_step_in_turn_on_one_handle_is_the_oracles_step(pj):
    P = _p32(pj)
    counts, states, guesses, run = _plain(pj)
    missed = []
    for k, (scheme, _, what) in enumerate(SEQUENCE):
        iters, converged = counts[k + 1][:2]
        assert converged == 1, (k, what)
        _held(f"step {k} ({scheme}, {what}, {iters} iterations)", states[k + 1], P.oracle_next(states[k], scheme), missed)
    assert not missed, missed
    # the extrapolated start keeps states again by the end of each run of default steps
    ends = [k for k, (_, _, what) in enumerate(SEQUENCE) if what == "default" and (k + 1 == len(SEQUENCE) or SEQUENCE[k + 1][2] != "default"
                                                                                    or SEQUENCE[k + 1][0] != SEQUENCE[k][0])]
    assert ends == [3, 9, 12]
    for k in ends:
        print(f"after step {k}: {guesses[k + 1]}")
        assert guesses[k + 1]["kept"] >= 1, (k, guesses[k + 1])
    assert run[0] == RUN_STEPS and run[4] == 0, run
    ref = states[len(SEQUENCE)]
    for _ in range(RUN_STEPS):
        ref = P.oracle_next(ref, "BE")
    _held(f"the run of {RUN_STEPS} BE steps at the end", states[-1], ref, missed)
    assert not missed, missed


def test_a_refused_call_before_every_step_changes_nothing(pj):
    counts, states, guesses, run = _plain(pj)
    tcounts, tstates, tguesses, trun = _sequence(pj, True)
    for k, (a, b) in enumerate(zip(counts, tcounts)):
        assert a == b, (k, a, b)                      # iterations, verdict, ||r||_W and ||b||_W to the bit
    for k, (a, b) in enumerate(zip(states, tstates)):
        assert np.array_equal(a, b), (k, float(np.max(np.abs(a - b))))
    assert guesses == tguesses
    assert run == trun, (run, trun)
