"""CPU unit test of the oblique half-space DEVICE functions (BODY_PLANE of penguin/jl_amd/csrc/pg_geom.h) compiled for the
host with g++ (tests/plane_host.cpp -> tests/_build/libplane_host.so; test-only build, never loaded by the product) against
the independent clipping / convex-hull formulation of tests/plane_oracle.py.

Bars: the project's bars for its other exact body (tests/test_gpu_parity.py, half-space capacities): classification
identical, volumes to 1e-12 of a full cell, Γ and sections to 1e-12 max(h^(N-1), 1), centroids to 1e-12 (|x0| + L) where the
fluid part is more than 1e-3 of the cell."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.plane_oracle import ObliqueHalfSpace, classify

ROOT = Path(__file__).resolve().parent.parent
P = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def lib():
    out = ROOT / "tests" / "_build" / "libplane_host.so"
    out.parent.mkdir(exist_ok=True)
    src = ROOT / "tests" / "plane_host.cpp"
    hdr = ROOT / "penguin" / "jl_amd" / "csrc" / "pg_geom.h"
    if not out.exists() or out.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out), str(src)], check=True)
    l = C.CDLL(str(out))
    l.plane_section.restype = C.c_double
    l.halfspace_section.restype = C.c_double
    return l


def _arr(v):
    return np.ascontiguousarray(v, dtype=float)


def pbox(lib, N, normal, offset, lo, hi, comp=0, surf=1):
    out = np.zeros(9)
    n, lo, hi = _arr(normal), _arr(lo), _arr(hi)
    lib.plane_box(N, comp, n.ctypes.data_as(P), C.c_double(offset), lo.ctypes.data_as(P), hi.ctypes.data_as(P), surf,
                  out.ctypes.data_as(P))
    return out


def psec(lib, N, normal, offset, d, s, lo, hi, comp=0, full_measure=-1.0):
    n, lo, hi = _arr(normal), _arr(lo), _arr(hi)
    return lib.plane_section(N, comp, n.ctypes.data_as(P), C.c_double(offset), d, C.c_double(s), lo.ctypes.data_as(P),
                             hi.ctypes.data_as(P), C.c_double(full_measure))


def _normal(rng, N, trial):
    """about half generic; the rest with one component exactly 0, or 1e-9 of the largest, or axis aligned"""
    n = rng.normal(size=N)
    n[np.abs(n) < 0.05] = 0.05
    kind = trial % 6
    if N > 1 and kind == 3:
        n[rng.integers(N)] = 0.0
    elif N > 1 and kind == 4:
        k = int(np.argmax(np.abs(n)))
        j = (k + 1 + rng.integers(N - 1)) % N
        n[j] = 1e-9 * abs(n[k]) * rng.choice([-1.0, 1.0])
    elif kind == 5:
        k = rng.integers(N)
        n = np.where(np.arange(N) == k, rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 2.0), 0.0)
    return n


@pytest.mark.parametrize("N,trials", [(1, 300), (2, 900), (3, 240)])
def test_box_and_section_measures_match_the_clipping_oracle(lib, N, trials):
    rng = np.random.default_rng(40 + N)
    ncut = 0
    for trial in range(trials):
        n = _normal(rng, N, trial)
        h = rng.choice([0.05, 0.2, 0.01]) * rng.uniform(0.5, 1.0, N)
        x0 = rng.uniform(-1.0, 1.0, N)
        lo, hi = x0, x0 + h
        vals = [float(np.dot(n, np.where(np.array(b), hi, lo))) for b in np.ndindex(*(2,) * N)]
        span = max(vals) - min(vals)
        offset = rng.uniform(min(vals) - 0.15 * span, max(vals) + 0.15 * span)       # through the box, mostly
        L = float(np.max(np.abs(x0)) + np.max(h))
        full = float(np.prod(h))
        face = max(float(np.max(h)) ** (N - 1), 1.0)
        for comp in (0, 1):
            body = ObliqueHalfSpace(n, offset, bool(comp))
            m = body.box(list(lo), list(hi))
            o = pbox(lib, N, n, offset, lo, hi, comp)
            assert int(o[0]) == m.type                                  # bit-exact classification
            t0 = lib.plane_pick_type(N, _arr(n).ctypes.data_as(P), C.c_double(offset), _arr(lo).ctypes.data_as(P), _arr(hi).ctypes.data_as(P))
            assert (t0 if (not comp or t0 == -1) else 1 - t0) == m.type  # what k_classify makes of pick_ball's answer
            if m.type == -1:
                ncut += 1
                assert o[5] > 0.0 and m.gamma > 0.0                     # Γ > 0 <=> CUT
                assert abs(o[1] - m.vol) <= 1e-12 * full
                assert abs(o[5] - m.gamma) <= 1e-12 * face
                if m.vol > 1e-3 * full:
                    assert np.max(np.abs(o[2:2 + N] - np.array(m.centroid))) <= 1e-12 * L
                    assert np.max(np.abs(o[6:6 + N] - np.array(m.cgamma))) <= 1e-12 * L
            else:
                assert o[1] == m.vol and o[5] == 0.0                    # full / empty: identical expression
                assert np.array_equal(o[2:2 + N], np.array(m.centroid))
            for d in range(N):
                for s in (lo[d], hi[d], rng.uniform(lo[d], hi[d])):
                    ref = body.section(d, float(s), list(lo), list(hi))
                    assert abs(psec(lib, N, n, offset, d, s, lo, hi, comp) - ref) <= 1e-12 * face
    assert ncut > trials // 4


@pytest.mark.parametrize("N", [1, 2, 3])
def test_full_and_empty_sections_pass_the_callers_measure_through_bit_for_bit(lib, N):
    """A_d - B_d must be an exact zero between full neighbours: a section that classifies FULL returns the caller's
    full_measure (or, without one, the product of the extents) bitwise, an EMPTY one exactly 0."""
    rng = np.random.default_rng(7 + N)
    seen = {1: 0, 0: 0}
    for trial in range(300):
        n = _normal(rng, N, trial)
        h = rng.uniform(0.05, 0.2, N)
        lo = rng.uniform(-1.0, 1.0, N)
        hi = lo + h
        offset = float(np.dot(n, 0.5 * (lo + hi))) + rng.choice([-1.0, 1.0]) * rng.uniform(0.3, 3.0) * float(np.dot(np.abs(n), h))
        fm = 0.1234567 * rng.uniform(0.5, 1.5)
        for comp in (0, 1):
            s_n, s_off = (-n, -offset) if comp else (n, offset)
            for d in range(N):
                for s in (lo[d], hi[d], 0.5 * (lo[d] + hi[d])):
                    plo, phi = lo.copy(), hi.copy()
                    plo[d] = phi[d] = s
                    t, _, _ = classify(list(s_n), s_off, list(plo), list(phi))
                    if t == -1:
                        continue
                    seen[t] += 1
                    own = 1.0
                    first = True
                    for k in range(N):
                        if k != d:
                            own = (hi[k] - lo[k]) if first else own * (hi[k] - lo[k])
                            first = False
                    want_given = (1.0 if N == 1 else fm) if t == 1 else 0.0
                    want_own = own if t == 1 else 0.0
                    assert psec(lib, N, n, offset, d, s, lo, hi, comp, fm) == want_given
                    assert psec(lib, N, n, offset, d, s, lo, hi, comp) == want_own
    assert seen[1] > 50 and seen[0] > 50


@pytest.mark.parametrize("N", [1, 2, 3])
def test_axis_aligned_plane_is_the_half_space(lib, N):
    """n = ±e_axis: the same type as BODY_HALFSPACE of the same host build, and values within the bars."""
    rng = np.random.default_rng(70 + N)
    ncut = 0
    for _ in range(200):
        axis = int(rng.integers(N))
        sgn = float(rng.choice([-1.0, 1.0]))
        h = rng.uniform(0.05, 0.2, N)
        lo = rng.uniform(-1.0, 1.0, N)
        hi = lo + h
        pos = rng.uniform(lo[axis] - 0.3 * h[axis], hi[axis] + 0.3 * h[axis])
        n = np.zeros(N)
        n[axis] = sgn
        L = float(np.max(np.abs(lo)) + np.max(h))
        full = float(np.prod(h))
        face = max(float(np.max(h)) ** (N - 1), 1.0)
        for comp in (0, 1):
            o = pbox(lib, N, n, sgn * pos, lo, hi, comp)
            ref = np.zeros(9)
            lib.halfspace_box(N, comp, axis, C.c_double(pos), C.c_double(sgn), _arr(lo).ctypes.data_as(P), _arr(hi).ctypes.data_as(P), 1,
                              ref.ctypes.data_as(P))
            assert int(o[0]) == int(ref[0])
            assert abs(o[1] - ref[1]) <= 1e-12 * full
            assert abs(o[5] - ref[5]) <= 1e-12 * face
            if int(ref[0]) == -1:
                ncut += 1
                if ref[1] > 1e-3 * full:
                    assert np.max(np.abs(o[2:2 + N] - ref[2:2 + N])) <= 1e-12 * L
                    assert np.max(np.abs(o[6:6 + N] - ref[6:6 + N])) <= 1e-12 * L
            for d in range(N):
                s = rng.uniform(lo[d], hi[d])
                r = lib.halfspace_section(N, comp, axis, C.c_double(pos), C.c_double(sgn), d, C.c_double(s), _arr(lo).ctypes.data_as(P),
                                          _arr(hi).ctypes.data_as(P))
                assert abs(psec(lib, N, n, sgn * pos, d, s, lo, hi, comp) - r) <= 1e-12 * face
    assert ncut > 100


def test_plane_through_a_corner_up_to_rounding_keeps_a_positive_interface(lib):
    """A plane through a mesh node cuts 1e-16 of a cell off, or nothing, as rounding has it: whenever the rule says CUT,
    Γ > 0 and 0 < V < full on both sides."""
    n = (0.36, 0.48, 0.8)
    h = 0.2
    for i, j, k in ((5, 0, 8), (1, 3, 8), (5, 5, 5), (9, 2, 5)):                 # 9 i + 12 j + 20 k = 205: nodes on the plane
        node = np.array([0.1 + i * h, 0.1 + j * h, 0.1 + k * h])
        for shift in np.ndindex(2, 2, 2):
            lo = node - np.array(shift) * h
            hi = lo + h
            for comp in (0, 1):
                body = ObliqueHalfSpace(n, 1.804, bool(comp))
                m = body.box(list(lo), list(hi))
                o = pbox(lib, 3, n, 1.804, lo, hi, comp)
                assert int(o[0]) == m.type
                assert (o[5] > 0.0) == (m.type == -1) == (m.gamma > 0.0)
                assert abs(o[1] - m.vol) <= 1e-12 * h ** 3
                assert abs(o[5] - m.gamma) <= 1e-12
