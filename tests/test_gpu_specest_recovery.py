"""precond="poly-est" on systems Gershgorin admits is the precond = 0 solve -- also when the polynomial is declared stagnated:
the plain finish of a first solve (krylov_solve's own fallback) and the re-solve on the full system after the compact system
stagnated (do_step) must go exactly as they go with precond = 0, and no spectral estimate may run on a matrix that has its
stagnation verdict.  The two cases are those of tests/test_gpu_recovery.py (give-up point at one iteration, check_every = 1,
degree 2).  The degree cannot be asked for together with the option (both are values of `precond`), so it comes from
PG_POLY_DEGREE=2, which the library reads once at start-up: each case runs in a child process of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import penguin_oracle as po
from tests.common import rel_l2
from tests.test_gpu_parity import TOL_T
from tests.test_gpu_recovery import ROOT, _first, _p32, _robin_disc, _set_give_up, _step

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def first_solve_case(pj):
    """(runs in the child) the unsteady Dirichlet first solve on the 64^2 disc, stagnation verdict at the first poll"""
    n, ph, oph, bcb, obcb, _, _ = _robin_disc(pj)
    M, dt = (n + 1) ** 2, 0.75 * (4.0 / n) ** 2
    so = po.DiffusionUnsteadyMono(oph, obcb, po.Dirichlet(1.0), dt, np.zeros(2 * M), "BE")
    po.solve_system(so, method="\\")
    got = {}
    for precond in (0, "poly-est"):
        s = pj.DiffusionUnsteadyMono(ph, bcb, pj.Dirichlet(1.0), dt, np.zeros(2 * M), "BE")
        assert s.system_info(0).neumann_ok == 1
        _set_give_up(1)
        try:
            info, x = _first(s, check_every=1, precond=precond)
        finally:
            _set_give_up(0)
        assert info.converged == 1 and s.unconverged == 0
        assert s.system_info(0).neumann_ok == 0                               # the verdict fell, the plain iteration finished
        assert s.spectral_estimate(0, run=False)["steps"] == 0                # ... and nothing was estimated
        got[precond] = (info.iters, x)
    print(f"first solve: {got[0][0]} / {got['poly-est'][0]} iterations, rel-L2 {rel_l2(got['poly-est'][1], so.x):.2e}")
    assert rel_l2(got["poly-est"][1], so.x) <= TOL_T
    assert got[0][0] == got["poly-est"][0] and _bits_equal(got[0][1], got["poly-est"][1])


def compact_step_case(pj):
    """(runs in the child) P32: four Crank-Nicolson steps on the compact system, a step with the stagnation verdict, two more"""
    P = _p32(pj)
    got = {}
    for precond in (0, "poly-est"):
        s = P.solver()
        _first(s, precond=precond)
        for _ in range(4):
            info, x = _step(s, "CN", precond=precond)
        assert s.system_info(1).loop_is_compact == 1 and s.system_info(1).neumann_ok == 1
        seq = []
        _set_give_up(1)
        try:
            info, x1 = _step(s, "CN", precond=precond, check_every=1)
        finally:
            _set_give_up(0)
        assert info.converged == 1
        assert s.system_info(1).loop_is_compact == 0 and s.system_info(1).neumann_ok == 0
        if precond == "poly-est":
            assert rel_l2(x1, P.oracle_next(x, "CN")) <= TOL_T
        seq.append((info.iters, x1))
        for _ in range(2):
            info, x1 = _step(s, "CN", precond=precond)
            assert info.converged == 1
            seq.append((info.iters, x1))
        assert s.unconverged == 0
        assert s.spectral_estimate(1, run=False)["steps"] == 0                # no estimate on the matrix with the verdict
        got[precond] = seq
    print("iterations of the verdict step and the two after it:", [i for i, _ in got[0]], [i for i, _ in got["poly-est"]])
    for (ia, xa), (ib, xb) in zip(got[0], got["poly-est"]):
        assert ia == ib and _bits_equal(xa, xb)


@pytest.mark.parametrize("case", ["first_solve_case", "compact_step_case"])
def test_stagnation_under_the_option_goes_as_with_precond_0(case):
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, '.'); import penguin.jl_amd as pj; pj.init(0); "
                        f"import tests.test_gpu_specest_recovery as t; t.{case}(pj); print('recovery ok')"], cwd=ROOT,
                       env={**os.environ, "PG_POLY_DEGREE": "2"}, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "recovery ok" in r.stdout, (r.stdout[-3000:], r.stderr[-4000:])
