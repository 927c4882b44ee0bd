"""The host side of the spectral estimate (pg_host_algos.h: pghost::hessenberg_eigenvalues, the shifted QR iteration on the
Arnoldi recursion's Hessenberg matrix) compiled with AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program
(tests/specest_host.cpp), fed the Hessenberg matrices the numpy restatement produces on four of the oracle's systems plus three
hand-made ones, and compared with numpy.linalg.eigvals.  CPU only."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import specest_reference as sr
from tests import specest_systems as ss

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "_build"
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
FED = [("diph-be", 32), ("diph-cn-d10", 32), ("robin-cn", 32), ("neumann-be", 32)]


def _sorted(ev):
    ev = np.asarray(ev, dtype=complex)
    return ev[np.lexsort((np.round(ev.imag, 9), np.round(ev.real, 9)))]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_hessenberg_eigenvalues_under_asan_ubsan_against_numpy():
    BUILD.mkdir(exist_ok=True)
    exe = BUILD / "specest_host"
    subprocess.run(["g++", "-std=c++17", *FLAGS, str(ROOT / "tests" / "specest_host.cpp"), "-o", str(exe)], check=True, cwd=ROOT)
    feed = BUILD / "specest_hessenberg.txt"
    with open(feed, "w") as f:
        for name, n in FED:
            H, k = sr.arnoldi(ss.system(name, n)["Ahat"])
            assert k == sr.STEPS
            f.write(f"{k} {k + 1}\n")
            f.write(" ".join(repr(float(v)) for v in np.asarray(H[: k + 1, :k]).ravel(order="F")) + "\n")
    r = subprocess.run([str(exe), str(feed)], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "all matrices done" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    lines = r.stdout.splitlines()
    seen, i = [], 0
    while i < len(lines):
        if not lines[i].startswith("matrix"):
            i += 1
            continue
        n = int(lines[i].split()[1])
        M = np.array([[float(v) for v in lines[i + 1 + q].split()] for q in range(n)])
        ev = np.array([complex(float(l.split()[1]), float(l.split()[2])) for l in lines[i + 1 + n: i + 1 + 2 * n]])
        i += 1 + 2 * n
        want = np.linalg.eigvals(M)
        scale = np.max(np.abs(want))
        worst = np.max(np.abs(_sorted(ev) - _sorted(want)))
        print(f"n = {n}: largest modulus {scale:.4f}, worst difference {worst:.2e}, complex: {int(np.sum(ev.imag != 0))}")
        assert worst <= 1e-12 * scale, (n, worst)
        seen.append((n, int(np.sum(ev.imag != 0))))
    assert [n for n, _ in seen] == [sr.STEPS] * len(FED) + [2, 4, 1]
    assert seen[-3][1] == 2 and seen[-2][1] == 2 and seen[-1][1] == 0      # the rotation block and the split matrix have a complex pair
