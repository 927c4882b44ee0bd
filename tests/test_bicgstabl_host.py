"""The small solve of BiCGStab(l)'s minimal-residual step (pg_host_algos.h: pghost::bicgstabl_small_solve -- the code the device
runs on one thread) compiled with AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program (tests/bicgstabl_host.cpp),
fed Gram matrices of every size l = 1 .. 8 -- well conditioned, rank deficient, zero, not finite, and an l the method refuses --
and compared with the numpy restatement (tests/bicgstabl_reference.py small_solve).  CPU only."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.bicgstabl_reference import MAX_L, small_solve

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "_build"
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _cases():
    rng = np.random.default_rng(7)
    out = []
    for l in range(1, MAX_L + 1):
        R = rng.normal(size=(l + 1, 50))
        out.append((l, R @ R.T))                                  # full rank
        # a power basis r, Ar, .., A^l r of a matrix close to the identity: the ill-conditioned Gram matrices the method meets
        A = np.eye(50) + 0.3 * rng.normal(size=(50, 50)) / np.sqrt(50)
        P = [rng.normal(size=50)]
        for _ in range(l):
            P.append(A @ P[-1])
        P = np.array(P)
        out.append((l, P @ P.T))
        if l >= 2:
            R2 = R.copy()
            R2[l] = R2[1] - 3.0 * R2[l - 1] if l >= 3 else 2.0 * R2[1]      # the last vector depends on earlier ones
            out.append((l, R2 @ R2.T))
        out.append((l, np.zeros((l + 1, l + 1))))
    bad = np.eye(3)
    bad[1, 1] = np.nan
    out.append((2, bad))
    bad = np.eye(3)
    bad[2, 2] = np.inf
    out.append((2, bad))
    out.append((9, np.eye(10)))                                   # refused: k = 0 and nothing is touched beyond the arrays
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_small_solve_under_asan_ubsan_against_the_restatement():
    BUILD.mkdir(exist_ok=True)
    exe = BUILD / "bicgstabl_host"
    subprocess.run(["g++", "-std=c++17", *FLAGS, str(ROOT / "tests" / "bicgstabl_host.cpp"), "-o", str(exe)], check=True, cwd=ROOT)
    cases = _cases()
    feed = BUILD / "bicgstabl_gram.txt"
    with open(feed, "w") as f:
        for l, G in cases:
            f.write(f"{l}\n" + " ".join(repr(float(v)) for v in np.asarray(G).ravel()) + "\n")
    r = subprocess.run([str(exe), str(feed)], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert f"all matrices done {len(cases)}" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    lines = r.stdout.splitlines()
    shrunk = 0
    for (l, G), line in zip(cases, lines):
        got = [float(v) for v in line.split()]
        k, gamma = int(got[0]), np.array(got[1:])
        if l > MAX_L:
            assert k == 0 and np.all(gamma == 0.0)
            continue
        want, kw = small_solve(G, l)
        assert k == kw, (l, k, kw)
        shrunk += 0 < k < l
        assert np.all(gamma[l + 1:] == 0.0) and gamma[0] == 0.0
        # the same operations in the same order: agreement to rounding of the compiler's contractions
        assert np.allclose(gamma[: l + 1], want, rtol=1e-9, atol=1e-9 * max(np.abs(want).max(), 1e-300)), (l, gamma, want)
    assert shrunk >= 1
