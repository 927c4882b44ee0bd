"""The scalars of IDR(s) (pg_host_algos.h: pghost::idr_lower_solve and pghost::idr_shadow -- the code the device runs) compiled with
AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program (tests/idrs_host.cpp): triangular systems of every size
s = 1 .. 8 -- well conditioned, singular, zero, not finite, and an s the method refuses -- compared with the numpy restatement
(tests/idrs_reference.py lower_solve), and the shadow values bit for bit against numpy's.  CPU only."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.idrs_reference import MAX_S, lower_solve, shadow

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "_build"
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def exe():
    BUILD.mkdir(exist_ok=True)
    out = BUILD / "idrs_host"
    subprocess.run(["g++", "-std=c++17", *FLAGS, str(ROOT / "tests" / "idrs_host.cpp"), "-o", str(out)], check=True, cwd=ROOT)
    return out


def _cases():
    rng = np.random.default_rng(9)
    out = []
    for s in range(1, MAX_S + 1):
        M = np.tril(rng.normal(size=(s, s))) + 3.0 * np.eye(s)
        M += np.triu(rng.normal(size=(s, s)), 1)                  # the upper triangle is never read
        rhs = rng.normal(size=s)
        for lo in range(s + 1):                                   # c: (k, s);  alpha: (0, k), the empty range included
            out.append((s, lo, s, M, rhs))
            out.append((s, 0, lo, M, rhs))
        Z = M.copy()
        Z[s - 1, s - 1] = 0.0                                     # singular: the last pivot vanishes
        out.append((s, 0, s, Z, rhs))
        out.append((s, 0, s, np.zeros((s, s)), rhs))              # zero
        out.append((s, 0, s, np.zeros((s, s)), np.zeros(s)))      # 0 / 0
        N = M.copy()
        N[s // 2, s // 2] = np.nan
        out.append((s, 0, s, N, rhs))
        I = M.copy()
        I[0, 0] = np.inf
        out.append((s, 0, s, I, rhs))
        bad = rhs.copy()
        bad[s - 1] = np.inf
        out.append((s, 0, s, M, bad))
    out.append((9, 0, 9, np.eye(9), np.ones(9)))                  # refused: nothing is touched beyond the arrays
    out.append((4, 3, 2, np.eye(4), np.ones(4)))                  # a range that is none
    out.append((4, 0, 5, np.eye(4), np.ones(4)))
    return out


def test_lower_solve_under_asan_ubsan_against_the_restatement(exe):
    cases = _cases()
    feed = BUILD / "idrs_systems.txt"
    with open(feed, "w") as f:
        for s, lo, hi, M, rhs in cases:
            f.write(f"{s} {lo} {hi}\n" + " ".join(repr(float(v)) for v in np.asarray(M).ravel()) + "\n"
                    + " ".join(repr(float(v)) for v in rhs) + "\n")
    r = subprocess.run([str(exe), "solve", str(feed)], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert f"all systems done {len(cases)}" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    refused = solved = 0
    for (s, lo, hi, M, rhs), line in zip(cases, r.stdout.splitlines()):
        got = [float(v) for v in line.split()]
        ok, out = bool(int(got[0])), np.array(got[1:])
        assert len(out) == MAX_S
        if s > MAX_S or lo > hi or hi > s:
            assert not ok and np.all(out == 0.0)
            continue
        want, ok_want = lower_solve(np.asarray(M, dtype=np.float64), lo, hi, rhs)
        assert ok == ok_want, (s, lo, hi)
        refused += not ok
        solved += ok
        assert np.all(out[s:] == 0.0)
        if not ok:
            assert np.all(out == 0.0)
        else:
            # the same operations in the same order: agreement to the rounding of the compiler's contractions
            assert np.allclose(out[:s], want, rtol=1e-12, atol=1e-12 * max(np.abs(want).max(), 1e-300)), (s, lo, hi, out, want)
    assert refused >= 5 * MAX_S and solved >= 2 * MAX_S      # (an infinite pivot gives a finite 0: solved)


def test_shadow_values_are_bit_equal_to_numpy(exe):
    rows = 4096
    r = subprocess.run([str(exe), "shadow", str(rows)], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert f"all rows done {rows}" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    lines = r.stdout.splitlines()[:rows]
    got = np.array([[int(w, 16) for w in line.split()] for line in lines], dtype=np.uint64)
    assert got.shape == (rows, MAX_S)
    want = np.stack([shadow(np.arange(rows), k) for k in range(MAX_S)], axis=1).view(np.uint64)
    assert np.array_equal(got, want)
