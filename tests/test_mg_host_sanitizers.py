"""The host side of the multigrid set-up (pg_host_algos.h: the dense inverse of the last level, the choice of the fused tail)
compiled with AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program (tests/mg_host_asan.cpp) and run on seeded
random inputs with functional checks.  CPU only."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "_build"
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_multigrid_host_set_up_under_asan_ubsan():
    BUILD.mkdir(exist_ok=True)
    exe = BUILD / "mg_host_asan"
    subprocess.run(["g++", "-std=c++17", *FLAGS, str(ROOT / "tests" / "mg_host_asan.cpp"), "-o", str(exe)], check=True, cwd=ROOT)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "all checks passed" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
