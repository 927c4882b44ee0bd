"""The marching-unit planner's edge rows on the host (pg_host_algos.h, tests/march_host.cpp): synthetic run lists -- a 3-D ball
of chords on 24^3 (as it is, with a row that carries an eighth entry, with a cell taken out of a chord) and a 2-D disc on
48^2 -- are planned, the records executed the way the kernel executes them and compared with the rows applied one by one.
The program checks: every row is covered exactly once (marched, edge or fallback), every edge row's operands are the
elements its plane's lines hold (y equals the row-by-row product exactly), at most 8 edge rows at an end of a plane and 64
in a unit, the row with the extra entry and the row behind it stay outside the units, no unit carries a row across a gap in
a line, and no edge row has a slot that points behind the vector (NaN there).  Built plain and, once, with
AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone executable."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "_build"
SRC = ROOT / "tests" / "march_host.cpp"
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build_and_run(name, flags, env=None):
    BUILD.mkdir(exist_ok=True)
    exe = BUILD / name
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags, str(SRC), "-o", str(exe)], check=True, cwd=ROOT)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r


def _counts(out):
    res = {}
    for line in out.splitlines():
        m = re.match(r"(.+?) rows (\d+) marched (\d+) edge (\d+) fallback (\d+) units (\d+)$", line)
        if m:
            res[m.group(1)] = tuple(int(v) for v in m.groups()[1:])
    return res


def test_edge_rows_are_planned_and_cover_every_row_once():
    c = _counts(_build_and_run("march_host", ["-O2"]).stdout)
    assert set(c) == {"ball24", "ball24+entry", "ball24+gap", "strip130", "disc48", "ball24 kmax 1"}, c
    for name, (rows, marched, edge, fallback, units) in c.items():
        assert marched + edge + fallback == rows and edge > 0 and units > 0, (name, c[name])
    # the row with an eighth entry and the row behind it left the units, nothing else moved
    assert c["ball24+entry"][2] == c["ball24"][2] - 2 and c["ball24+entry"][1] == c["ball24"][1]
    # the 2-D disc: 5-point units take edge rows too
    assert c["disc48"][2] > 0


def test_edge_row_planner_under_asan_ubsan():
    r = _build_and_run("march_host_asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                           "-fno-omit-frame-pointer"],
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    assert len(_counts(r.stdout)) == 6
