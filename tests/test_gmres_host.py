"""The scalars of restarted GMRES (pg_host_algos.h: pghost::GmLayout, gm_begin, gm_hess, gm_solve_y -- the code the device's one-thread
kernels run) compiled with AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program (tests/gmres_host.cpp) that works
on a heap block of exactly GmLayout::size() doubles: replayed on the Arnoldi coefficients of the numpy restatement
(tests/gmres_reference.py) and on drawn Hessenberg matrices for every restart length at a boundary of the groups of 8 -- full cycles
and cycles the estimate cuts -- and on the edges: ||w||^2 slightly negative, d = 0, rr = 0, the lowering branch, NaN / Inf.  CPU only."""
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.gmres_reference import (DONE_CONVERGED, DONE_CYCLE, DONE_NO, DONE_STOPPED, GmScalars, gmres_dev_ref, heat_system,
                                   peclet_system, small_box_system, symmetric_scaling)

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "_build"
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}
RESTARTS = (1, 2, 7, 8, 9, 16, 17, 20, 200)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def exe():
    BUILD.mkdir(exist_ok=True)
    out = BUILD / "gmres_host"
    subprocess.run(["g++", "-std=c++17", *FLAGS, str(ROOT / "tests" / "gmres_host.cpp"), "-o", str(out)], check=True, cwd=ROOT)
    return out


def _num(v):
    return repr(float(v))


class Replay:
    """Commands for tests/gmres_host.cpp and, per command, the line the restatement expects (None: a number that is not compared
    -- an entry the step leaves as it found it after it has stopped)."""

    def __init__(self):
        self.lines, self.expect, self.sc = [], [], None

    def case(self, m, reltol, abstol=0.0):
        self.sc = GmScalars(m, reltol, abstol)
        self.lines.append(f"case {m} {_num(reltol * reltol)} {_num(abstol * abstol)}")
        self.expect.append(("C", [(m + 1) * m + 6 * m + 7]))
        return self.sc

    def begin(self, rr, rrw, first):
        sc = self.sc
        with np.errstate(all="ignore"):
            sc.begin(rr, rrw, first)
        self.lines.append(f"begin {int(first)} {_num(rr)} {_num(rrw)}")
        self.expect.append(("B", [sc.done, float(sc.notfinite), sc.iters, sc.tol2, sc.tolw2, sc.bb, sc.rrw, sc.J, sc.invn, *sc.g]))

    def hess(self, j, h1, h2, nn):
        sc = self.sc
        ran = sc.done == DONE_NO
        with np.errstate(all="ignore"):
            sc.hess(j, h1, h2, nn)
        self.lines.append(f"hess {j} " + " ".join(_num(v) for v in [*h1[: j + 1], *h2[: j + 1], nn]))
        rotated = ran and sc.done != DONE_STOPPED
        self.expect.append(("H", [sc.done, float(sc.notfinite), sc.iters, sc.J, sc.invn,
                                  *([sc.cs[j], sc.sn[j], sc.g[j], sc.g[j + 1], *sc.H[: j + 2, j]] if rotated else [None] * (j + 6))]))

    def solve(self):
        self.sc.solve_y()
        self.lines.append("solve")
        self.expect.append(("Y", [self.sc.J, *self.sc.y[: self.sc.J]]))

    def trace(self, items):
        for item in items:
            if item[0] == "begin":
                self.begin(item[1], item[2], item[3])
            elif item[0] == "hess":
                self.hess(*item[1:])
            else:
                self.solve()


def _run(exe, replay, name):
    """Every line of the program against the restatement: the same operations in the same order -- rtol 1e-12 (the compiler's
    contractions), flags and counts exactly, NaN where the restatement has NaN."""
    feed = BUILD / f"gmres_{name}.txt"
    feed.write_text("\n".join(replay.lines) + "\n")
    r = subprocess.run([str(exe), str(feed)], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and r.stderr.strip() == ""
    out = r.stdout.splitlines()
    assert out[-1] == f"all commands done {len(replay.lines)}" and len(out) == len(replay.lines) + 1
    for k, (line, (tag, want)) in enumerate(zip(out, replay.expect)):
        words = line.split()
        assert words[0] == tag, (k, line)
        got = [float(v) for v in words[1:]]
        assert len(got) == len(want), (k, replay.lines[k][:80], line[:200])
        nflags = {"C": 1, "B": 3, "H": 4, "Y": 1}[tag]
        for i, (g, w) in enumerate(zip(got, want)):
            if w is None:
                continue
            w = float(w)
            if i < nflags:
                assert g == w, (k, i, replay.lines[k][:80], g, w)
            elif math.isnan(w):
                assert math.isnan(g), (k, i, g)
            elif math.isinf(w):
                assert g == w, (k, i, g, w)
            else:
                assert abs(g - w) <= 1e-12 * abs(w), (k, i, replay.lines[k][:80], g, w)
    return out


# ------------------------------------------------------------------------------------ the restatement's own Arnoldi coefficients
def test_replay_of_real_solves_under_asan_ubsan(exe):
    """Heat 16^2 with every restart length (reltol 1e-13: full cycles, and the last one cut by the estimate), the small box (the
    lowering branch between cycles), the Peclet system with restart 200 (one long cycle cut by the estimate)."""
    rep = Replay()
    A, b, S = symmetric_scaling(*heat_system(16))
    kinds = set()
    for m in RESTARTS:
        trace = []
        _, info = gmres_dev_ref(A, b, restart=m, reltol=1e-13, weights=S, maxiter=60, trace=trace)
        rep.case(min(m, len(b)), 1e-13)
        rep.trace(trace)
        assert info["converged"] and info["cycles"] >= 1
        kinds.add("full cycles, then a cut one" if info["cycles"] >= 2 else "one cut cycle")
    assert len(kinds) == 2
    Ab, bb, Sb = small_box_system(0.04)
    for m in (20, 5):
        trace = []
        _, info = gmres_dev_ref(Ab, bb, restart=m, reltol=1e-10, weights=Sb, trace=trace)
        assert info["lowered"] >= 1 and info["converged"]
        sc = rep.case(m, 1e-10)
        tol2 = []
        for item in trace:
            rep.trace([item])
            tol2.append(sc.tol2)
        assert min(tol2) < tol2[0]                       # the lowering happened in the replay too
    Ap, bp = peclet_system(32, "uniform")
    trace = []
    _, info = gmres_dev_ref(Ap, bp, restart=200, reltol=1e-10, trace=trace)
    assert info["converged"] and info["cycles"] == 1 and 100 < info["iters"] < 200
    rep.case(200, 1e-10)
    rep.trace(trace)
    _run(exe, rep, "real")


# ------------------------------------------------------------------------------------ drawn Hessenberg matrices
def _draw(rng, m):
    """A well-conditioned (m+1) x m upper Hessenberg matrix (diagonal 4, entries of size <= 1 / sqrt(m), subdiagonal in [0.5, 1]) as
    the two passes of CGS2 would deliver it: h1 carries the matrix, h2 a correction eleven digits down."""
    Hm = np.triu(rng.uniform(-1.0, 1.0, size=(m + 1, m)) / math.sqrt(m), 0)
    Hm[np.arange(m), np.arange(m)] += 4.0
    sub = rng.uniform(0.5, 1.0, size=m)
    h1 = [Hm[: j + 1, j].copy() for j in range(m)]
    h2 = [1e-11 * rng.uniform(-1.0, 1.0, size=j + 1) for j in range(m)]
    raw = np.zeros((m + 1, m))
    for j in range(m):
        raw[: j + 1, j] = h1[j] + h2[j]
        raw[j + 1, j] = math.sqrt(sub[j] * sub[j])
    return h1, h2, sub * sub, raw


@pytest.mark.parametrize("m", RESTARTS)
def test_drawn_cycles_full_and_cut_against_the_restatement_and_lstsq(exe, m):
    rng = np.random.default_rng(100 + m)
    rep = Replay()
    checks = []
    for cut in (False, True):
        h1, h2, nn, raw = _draw(rng, m)
        beta2 = 7.0
        # full: no tolerance -- all m columns; cut: the estimate falls by hn / d <= 1 / hypot(3, 1) = 0.32 per column, the cycle
        # ends within the first half of them
        reltol = 0.0 if not cut else 0.4 ** max(1, m // 2)
        sc = rep.case(m, reltol)
        rep.begin(beta2, 3.0 * beta2, True)
        for j in range(m):
            rep.hess(j, h1[j], h2[j], nn[j])
        rep.solve()
        J = sc.J
        assert (J == m and sc.done in (DONE_NO, DONE_CYCLE)) if not cut else (sc.done == DONE_CYCLE and 1 <= J <= m)
        if cut and m >= 2:
            assert J <= m // 2
        rhs = np.zeros(J + 1)
        rhs[0] = math.sqrt(beta2)
        y = np.linalg.lstsq(raw[: J + 1, :J], rhs, rcond=None)[0]
        checks.append((len(rep.lines) - 1, y))
        # the verdict of the restart that follows: a residual below / above the weighted tolerance
        rep.begin(1e-3 * sc.tol2 if cut else 0.5, 0.5 * sc.tolw2 if cut else 0.5, False)
        assert sc.done == (DONE_CONVERGED if cut else DONE_NO)
    out = _run(exe, rep, f"drawn_{m}")
    for k, y in checks:
        got = np.array([float(v) for v in out[k].split()[2:]])
        assert np.linalg.norm(got - y) <= 1e-10 * np.linalg.norm(y), (m, k)


# ------------------------------------------------------------------------------------ the edges
def test_edges_under_asan_ubsan(exe):
    rep = Replay()
    for m in RESTARTS:
        rng = np.random.default_rng(m)
        h1, h2, nn, _ = _draw(rng, m)
        jmid = m // 2
        # ||w||^2 slightly negative at the last step of a cycle: hn = 0, the Krylov space is exhausted -- the cycle ends, no verdict
        sc = rep.case(m, 0.0)
        rep.begin(2.0, 2.0, True)
        for j in range(m):
            rep.hess(j, h1[j], h2[j], nn[j] if j < m - 1 else -1e-18)
        assert sc.done == DONE_CYCLE and sc.exhausted and sc.J == m and sc.invn == 0.0
        rep.solve()
        # d = 0 at j = 0: singular, no column;  the flag survives the begin that follows, whatever its residual
        sc = rep.case(m, 1e-12)
        rep.begin(2.0, 2.0, True)
        rep.hess(0, [0.0], [0.0], 0.0)
        assert sc.done == DONE_STOPPED and sc.J == 0 and not sc.notfinite and sc.iters == 1
        rep.hess(min(1, m - 1), np.ones(2), np.ones(2), 1.0)       # (a step after the stop does nothing)
        rep.solve()
        rep.begin(0.0, 0.0, False)
        assert sc.done == DONE_STOPPED
        # d = 0 at j > 0: H[j, j] rotates to 0 when the column is a multiple of the one before;  J = j columns are kept
        if m >= 2:
            sc = rep.case(m, 0.0)
            rep.begin(1.0, 1.0, True)
            rep.hess(0, [0.0], [0.0], 1.0)                         # c = 0, s = 1
            rep.hess(1, [0.0, 0.0], [0.0, 0.0], 0.0)               # column 1 = 0 -> d = 0
            assert sc.done == DONE_STOPPED and sc.J == 1 and sc.iters == 2
            rep.solve()
            rep.begin(1.0, 1.0, False)
            assert sc.done == DONE_STOPPED
        # the first call with rr = 0: done, invn = 0, and nothing runs after it
        sc = rep.case(m, 1e-12)
        rep.begin(0.0, 0.0, True)
        assert sc.done == DONE_CONVERGED and sc.invn == 0.0
        rep.hess(0, h1[0], h2[0], nn[0])
        assert sc.iters == 0
        rep.solve()
        # the lowering branch: estimate met (cycle ended), weighted test open by a factor 100 -> tol2 = 0.25 rr / 100
        sc = rep.case(m, 1e-3)
        rep.begin(4.0, 400.0, True)
        t0 = sc.tol2
        for j in range(jmid + 1):
            rep.hess(j, h1[j], h2[j], nn[j])
        rep.solve()
        rep.begin(0.9 * t0, 100.0 * sc.tolw2, False)
        assert sc.done == DONE_NO and sc.tol2 == 0.25 * (0.9 * t0) * (sc.tolw2 / (100.0 * sc.tolw2)) < t0 and sc.just_lowered
        rep.begin(0.9 * t0, 1.0001 * sc.tolw2, False)              # aim above the tolerance in force: not raised
        assert not sc.just_lowered
        # abstol alone
        sc = rep.case(m, 0.0, 1e-3)
        rep.begin(1.0, 1.0, True)
        assert sc.tol2 == sc.tolw2 == 1e-6 and sc.done == DONE_NO
        rep.begin(1.0, 1e-6, False)
        assert sc.done == DONE_CONVERGED
        # not finite: rr, rrw at the start and at a restart; h1, h2 and ||w||^2 at the first, a middle and the last step
        for bad in (math.nan, math.inf, -math.inf):
            for rr, rrw in ((bad, 1.0), (1.0, bad), (bad, bad)):
                sc = rep.case(m, 1e-12)
                rep.begin(rr, rrw, True)
                assert sc.done == DONE_STOPPED and sc.notfinite and sc.invn == 0.0
                rep.hess(0, h1[0], h2[0], nn[0])
                rep.solve()
                sc = rep.case(m, 1e-12)
                rep.begin(2.0, 2.0, True)
                rep.hess(0, h1[0], h2[0], nn[0])
                rep.solve()
                rep.begin(rr, rrw, False)
                assert sc.done == DONE_STOPPED and sc.notfinite
                rep.begin(1e-40, 1e-40, False)                     # a clean residual afterwards does not revive it
                assert sc.done == DONE_STOPPED
            for jbad in sorted({0, jmid, m - 1}):
                for where in ("h1", "h2", "nn"):
                    sc = rep.case(m, 0.0)
                    rep.begin(2.0, 2.0, True)
                    for j in range(jbad + 1):
                        a, c, v = h1[j].copy(), h2[j].copy(), nn[j]
                        if j == jbad:
                            if where == "h1":
                                a[j // 2] = bad
                            elif where == "h2":
                                c[j] = bad
                            else:
                                v = bad
                        rep.hess(j, a, c, v)
                    assert sc.done == DONE_STOPPED and sc.notfinite and sc.J == jbad and sc.iters == jbad + 1, (m, bad, jbad, where)
                    rep.solve()
                    assert np.all(np.isfinite(sc.y[: sc.J]))
                    rep.begin(math.nan, math.nan, False)
                    assert sc.done == DONE_STOPPED
    out = _run(exe, rep, "edges")
    # the verdict is never 1 once a norm was not finite (column 2 of a B / H line is the mark, column 1 the flag)
    marked = [line.split() for line in out if line[0] in "BH" and float(line.split()[2]) == 1.0]
    assert len(marked) > 20 * len(RESTARTS) and all(float(w[1]) == DONE_STOPPED for w in marked)
