"""The schedule of the mixed-precision Horner chain (pg_host_algos.h: pghost::mixed_chain_schedule, mixed_chain_tail,
mixed_tail_max), compiled with AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program
(tests/mixed_chain_host.cpp) and checked for m = 4 .. 40, g in {0.3, 0.72, 0.95} and every j = 0 .. m.  CPU only.

Notation.  λ_0 > ... > λ_(m-1): the Chebyshev nodes of [1 - g, 1 + g]; f_k(λ) = 1 - λ / λ_k.  The chain applies the roots in
the order r_1 .. r_m with m - 1 launches (launch i = 0 .. m-2 applies r_(i+2); r_1 rides in the first launch's coefficients),
so the intermediate a launch stores after s = 2 .. m-1 applied roots splits the polynomial into a LEADING product
Π_(k<=s) f_(r_k) -- what the intermediate holds -- and a TRAILING product Π_(k>s) f_(r_k) -- what multiplies its rounding on
the way to the result.  "Partial products" below are both, at the intermediates that matter: those stored in fp32 for the
mixed order (s = 2 .. n32 + 1), all of them for the all-fp64 order (largest and smallest remaining root in turn, applied from
its far end: pg_krylov.hip).

Checked:
  * order is a permutation of 0 .. m-1, the launch kinds read first, middle x (n32 - 1), hand-over, fp64 x (j - 1) with
    n32 = m - 1 - j >= 2; j = 0 is served as j = 1; "all fp64" exactly when fewer than two fp32 launches would remain;
  * the largest partial product of the mixed order over a grid of 8001 points is no larger than that of the all-fp64 order
    for the same m (1e-9 relative slack for the two evaluation orders);
    This is NARROWER than "the largest partial product is no larger than that of today's order": at the splits inside the
    tail (s = n32 + 2 .. m-1, intermediates stored in fp64) the mixed order does exceed the all-fp64 order's largest -- in 61
    (g = 0.3), 202 (g = 0.72) and 9 (g = 0.95) of the 703 admissible (m, j), by up to 4.1 x (g = 0.72, m = 6, j = 3: 5.18
    against 1.25; 1.4 - 1.9 x at m = 19 - 20, j = 4 - 5) -- because the head's product is large exactly where the damping tail
    is small.  Those products multiply fp64 roundings only, so what is asserted there is an absolute bound instead:
    no larger than the all-fp64 order's largest for the same m, or than TAIL_SPLIT_BOUND = 64, whichever is greater --
    64 x 2^-53 = 7e-15 is a fourteenth of the tightest relative tolerance anything here solves to (1e-13), and 2^23 times
    less than what an fp32 intermediate with a partial product of 1 contributes;
  * the tail's product on the grid is at most damp^j C with C = C(m, g, j) = mixed_tail_max / damp^j, mixed_tail_max being
    the maximum over the interval computed from the tail's roots in long double (end points and the critical point between
    neighbouring roots), damp = max(MIXED_DAMP, ρ(g)), ρ(g) = g / (1 + sqrt(1 - g²)) -- and that maximum is itself no smaller
    than the minimax value 1 / T_j(1/g) no polynomial of degree j with value 1 at 0 can beat (a check of the routine).  The
    largest C the run found is printed per g; at this writing 0.85 (g = 0.3), 5.3 (g = 0.72, at m = 10, j = 5) and 19.2
    (g = 0.95, at m = 38, j = 19): a true Chebyshev polynomial would give 2 (ρ / damp)^j <= 2, the roots snapped to the m
    nodes cost the rest;
  * the j rule returns the smallest j >= 1 with floor32 damp^j <= safety needed, is monotone in the needed reduction (a smaller
    one never shortens the tail), and returns -1 ("all fp64") once fewer than two fp32 launches would remain, for needed = 0
    and for needed = 1."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "_build"
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
GS = (0.3, 0.72, 0.95)
FIRST, MIDDLE, HANDOVER, F64 = 1, 2, 3, 0
NGRID = 8001
TAIL_SPLIT_BOUND = 64.0     # partial products at the fp64-stored splits inside the tail (module docstring)

_OUT = {}


def _run():
    if "lines" not in _OUT:
        BUILD.mkdir(exist_ok=True)
        exe = BUILD / "mixed_chain_host"
        subprocess.run(["g++", "-std=c++17", *FLAGS, str(ROOT / "tests" / "mixed_chain_host.cpp"), "-o", str(exe)], check=True, cwd=ROOT)
        r = subprocess.run([str(exe), *[repr(g) for g in GS]], capture_output=True, text=True, timeout=300,
                           env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        sched, tail, const = {}, {}, None
        for line in r.stdout.splitlines():
            t = line.split()
            if t[0] == "sched":
                m, g, j, ok = int(t[1]), float(t[2]), int(t[3]), int(t[4])
                if ok:
                    parts = line.split("|")
                    js, n32 = (int(v) for v in parts[1].split())
                    sched[(m, g, j)] = dict(j=js, n32=n32, order=[int(v) for v in parts[2].split()],
                                            kind=[int(v) for v in parts[3].split()], tail_max=np.longdouble(parts[4].strip()))
                else:
                    sched[(m, g, j)] = None
            elif t[0] == "tail":
                tail.setdefault((int(t[1]), float(t[2])), []).append((float(t[3]), int(t[4])))
            elif t[0] == "const":
                const = tuple(float(v) for v in t[1:])
        _OUT.update(lines=True, sched=sched, tail=tail, const=const)
    return _OUT


def _roots(m, g):
    return 1.0 + g * np.cos(np.pi * (2.0 * np.arange(m) + 1.0) / (2.0 * m))      # descending


def _today(m):
    """application order of the all-fp64 chain: tau[m-1] .. tau[0] of pg_krylov.hip, tau = largest, smallest, ... in turn"""
    idx, lo, hi = [], 0, m - 1
    for k in range(m):
        if k & 1:
            idx.append(hi)
            hi -= 1
        else:
            idx.append(lo)
            lo += 1
    return idx[::-1]


def _partials(order, lam, x, splits):
    """largest |leading| and |trailing| product over the grid at the splits s (s roots applied)"""
    F = 1.0 - np.outer(1.0 / lam[order], x)
    lead = np.abs(np.cumprod(F, axis=0)).max(axis=1)                     # lead[s - 1]: the first s factors
    trail = np.abs(np.cumprod(F[::-1], axis=0)[::-1]).max(axis=1)        # trail[s]: the factors after the first s
    return max(max(lead[s - 1], trail[s]) for s in splits)


pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.mark.parametrize("g", GS)
def test_order_and_launch_kinds(g):
    sched = _run()["sched"]
    for m in range(4, 41):
        for j in range(0, m + 1):
            c = sched[(m, g, j)]
            js = max(j, 1)
            if m - 1 - js < 2:
                assert c is None, (m, g, j)
                continue
            assert c is not None and c["j"] == js and c["n32"] == m - 1 - js, (m, g, j, c)
            assert sorted(c["order"]) == list(range(m)), (m, g, j)
            assert c["kind"] == [FIRST] + [MIDDLE] * (c["n32"] - 1) + [HANDOVER] + [F64] * (js - 1), (m, g, j, c["kind"])
        assert sched[(m, g, 0)] == sched[(m, g, 1)], (m, g)


@pytest.mark.parametrize("g", GS)
def test_no_partial_product_larger_than_the_all_fp64_orders(g):
    sched = _run()["sched"]
    x = np.linspace(1.0 - g, 1.0 + g, NGRID)
    worst = 0.0
    for m in range(4, 41):
        lam = _roots(m, g)
        ref = _partials(_today(m), lam, x, range(2, m))
        for j in range(0, m + 1):
            c = sched[(m, g, j)]
            if c is None:
                continue
            new = _partials(c["order"], lam, x, range(2, c["n32"] + 2))
            worst = max(worst, new / ref)
            assert new <= ref * (1.0 + 1e-9), (m, g, j, new, ref)
    print(f"g = {g}: largest partial product, mixed order / all-fp64 order: at most {worst:.4f}")


@pytest.mark.parametrize("g", GS)
def test_partial_products_at_the_tails_own_splits_are_bounded(g):
    sched = _run()["sched"]
    x = np.linspace(1.0 - g, 1.0 + g, NGRID)
    above, worst = 0, (0.0, None)
    for m in range(4, 41):
        lam = _roots(m, g)
        ref = _partials(_today(m), lam, x, range(2, m))
        for j in range(1, m + 1):
            c = sched[(m, g, j)]
            if c is None or c["n32"] + 2 > m - 1:
                continue
            new = _partials(c["order"], lam, x, range(c["n32"] + 2, m))
            if new > ref * (1.0 + 1e-9):
                above += 1
                worst = max(worst, (new / ref, (m, j, new, ref)))
            assert new <= max(ref, TAIL_SPLIT_BOUND) * (1.0 + 1e-9), (m, g, j, new, ref)
    print(f"g = {g}: (m, j) whose tail splits exceed the all-fp64 order's largest partial product: {above}; worst ratio {worst}")


@pytest.mark.parametrize("g", GS)
def test_tail_is_a_damping_set(g):
    out = _run()
    sched, (floor32, damp0, safety) = out["sched"], out["const"]
    rho = g / (1.0 + np.sqrt(1.0 - g * g))
    damp = max(damp0, rho)
    x = np.linspace(1.0 - g, 1.0 + g, NGRID)
    worst_c, worst_at, worst_half = 0.0, None, 0.0
    for m in range(4, 41):
        lam = _roots(m, g)
        for j in range(1, m + 1):
            c = sched[(m, g, j)]
            if c is None:
                continue
            tail = c["order"][m - j:]
            on_grid = np.abs(np.prod(1.0 - np.outer(1.0 / lam[tail], x), axis=0)).max()
            tmax = float(c["tail_max"])
            const = tmax / damp ** j                              # the constant C(m, g, j) of the docstring
            assert on_grid <= damp ** j * const * (1.0 + 1e-12), (m, g, j, on_grid, tmax)
            minimax = 1.0 / np.cosh(j * np.arccosh(1.0 / g))
            assert tmax >= minimax * (1.0 - 1e-12), (m, g, j, tmax, minimax)
            assert on_grid >= tmax * (1.0 - 1e-3), (m, g, j, on_grid, tmax)   # (the routine does not overstate it either)
            if const > worst_c:
                worst_c, worst_at = const, (m, j)
            if 2 * j <= m:
                worst_half = max(worst_half, const)
    print(f"g = {g}: damp {damp:.4f} (rho {rho:.4f}); largest C = tail_max / damp^j: {worst_c:.3f} at (m, j) = {worst_at}; "
          f"for j <= m / 2: {worst_half:.3f}")


@pytest.mark.parametrize("g", GS)
def test_tail_rule(g):
    out = _run()
    tail, (floor32, damp0, safety) = out["tail"], out["const"]
    assert (floor32, damp0, safety) == (1e-7, 0.45, 0.5)
    damp = max(damp0, g / (1.0 + np.sqrt(max(0.0, 1.0 - g * g))))
    for m in range(4, 41):
        rows = tail[(m, g)]
        ladder = [(nd, j) for nd, j in rows if 0.0 < nd < 1.0]
        assert len(ladder) == 60 and all(a[0] > b[0] for a, b in zip(ladder, ladder[1:]))
        prev = 1
        for nd, j in ladder:
            want, left = 1, floor32 * damp
            while left > safety * nd and want < m:
                left *= damp
                want += 1
            want = want if m - 1 - want >= 2 else -1
            assert j == want, (m, g, nd, j, want)
            if prev == -1:
                assert j == -1, (m, g, nd)              # once the tail has eaten the chain it stays all fp64
            else:
                assert j == -1 or j >= prev, (m, g, nd, j, prev)
            prev = j
        assert [j for nd, j in rows if nd == 0.0 or nd == 1.0] == [-1, -1], (m, g)
