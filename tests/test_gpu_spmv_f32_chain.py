"""The Horner launches with an element type per vector stream (launch_spmv_typed of pg_spmv.h: the mixed-precision chain of
pg_krylov.hip) against the fp64 launch mode 8, bit for bit.

The typed kernels convert at the load and at the store (round to nearest) and run the fp64 kernel's arithmetic in between, in
the same entry order.  So on inputs that are converted exactly -- fp32 vectors widened to fp64 -- the fp64 launch mode 8
(pg_debug_spmv_apply, itself held against an extended-precision host product by tests/test_gpu_spmv_host_reference.py) returns
a y64 of which the typed launch must return float32(y64) (first and middle launch) or y64 itself (hand-over launch); the first
launch also writes p32 = float32(σ x) for every row.  No tolerance anywhere.

Cases: the six images of tests/test_gpu_spmv_host_reference.py (four with marching units and edge rows; the Robin disc and the
diphasic system for the slices and chunks on their own -- the diphasic image has no unit at all), their run and loop matrices
(the diphasic solver has its constructor matrix only), that file's three coefficient triples and three vector families.  σ =
2^-30 matches the 2^±30 family: σ x stays a normal fp32 number."""
import zlib

import numpy as np
import pytest

from tests import spmv_reference as R
from tests.test_gpu_spmv_host_reference import MARCHING, PCS, _system

pytestmark = pytest.mark.gpu

WHICH = {**{c: (3, 7) for c in MARCHING}, "mono2d_robin": (3, 7), "diph2d": (2,)}
PAIRS = [(c, w) for c, ws in WHICH.items() for w in ws]
SIGMA = 2.0 ** -30
GUARD = R.GUARD
SENTINEL_F32 = 0x7FC5EED0        # PG_DEBUG_SPMV_SENTINEL_F32 of include/penguin_hip.h
FIRST, MIDDLE, HANDOVER = 1, 2, 3

_VEC = {}


def _vectors(pj, case, which, family):
    """x (n_vec) and base (n) of the family, fixed seed; read-only"""
    key = (case, which, family)
    if key not in _VEC:
        n, nv = _system(pj, case, which)[4:6]
        rng = np.random.default_rng(zlib.crc32(repr(("f32", key)).encode()))
        v = {"x": R.vector(family, nv, rng), "base": R.vector(family, n, rng)}
        v["x32"] = (SIGMA * v["x"]).astype(np.float32)
        v["base32"] = (SIGMA * v["base"]).astype(np.float32)
        for a in v.values():
            a.setflags(write=False)
        assert np.all(np.isfinite(v["x32"])) and np.all((v["x32"] != 0) == (v["x"] != 0))     # σ x stays in fp32's normal range
        _VEC[key] = v
    return _VEC[key]


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _guards32(a, n, label):
    g = _bits32(a)[n:]
    assert g.size == GUARD and np.all(g == np.uint32(SENTINEL_F32)), (label, np.nonzero(g != np.uint32(SENTINEL_F32))[0][:8])


def _same32(got, want64, n, label):
    """got[:n] is float32(want64[:n]) bit for bit, every row written, guards untouched"""
    _guards32(got, n, label)
    with np.errstate(over="ignore"):
        want = np.asarray(want64[:n], dtype=np.float64).astype(np.float32)
    bad = np.nonzero(_bits32(got[:n]) != _bits32(want))[0]
    assert bad.size == 0, (label, bad.size, bad[:8].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case,which", PAIRS)
def test_typed_launches_equal_the_fp64_launch_on_converted_inputs(pj, case, which, family):
    from penguin.jl_amd import _lib as L
    s = _system(pj, case, which)[0]
    n = _system(pj, case, which)[4]
    v = _vectors(pj, case, which, family)
    x32w, base32w = v["x32"].astype(np.float64), v["base32"].astype(np.float64)
    for pc in PCS:
        label = f"{case} which {which} {family} pc {pc}"
        # (a) first launch: x = base fp64, σ folded into the coefficients (a power of two: exact); y fp32, p32 = float32(σ x)
        pca = tuple(SIGMA * c for c in pc)
        y64 = L.debug_spmv_apply(s._h, which, 70, 8, v["x"], pc=pca)["y"]
        out = L.debug_spmv_apply_typed(s._h, which, FIRST, v["x"], pc=pca, sigma=SIGMA)
        _same32(out["y"], y64, n, label + " first: y")
        _same32(out["p32"], SIGMA * v["x"], n, label + " first: p32")
        # (b) middle launch: x, base, y fp32
        y64 = L.debug_spmv_apply(s._h, which, 70, 8, x32w, base=base32w, pc=pc)["y"]
        out = L.debug_spmv_apply_typed(s._h, which, MIDDLE, v["x32"], base=v["base32"], pc=pc)
        _same32(out["y"], y64, n, label + " middle: y")
        assert out["p32"] is None
        # (c) hand-over launch: x fp32, base fp64, 1 / σ folded into pc0 and pc1; y fp64
        pcc = (pc[0] / SIGMA, pc[1] / SIGMA, pc[2])
        y64 = L.debug_spmv_apply(s._h, which, 70, 8, x32w, base=v["base"], pc=pcc)["y"]
        out = L.debug_spmv_apply_typed(s._h, which, HANDOVER, v["x32"], base=v["base"], pc=pcc)
        assert out["y"].size == n + GUARD
        assert np.all(_bits64(out["y"])[n:] == np.uint64(R.SENTINEL_BITS)), label + " hand-over: guard words"
        bad = np.nonzero(_bits64(out["y"][:n]) != _bits64(y64[:n]))[0]
        assert bad.size == 0, (label + " hand-over: y", bad.size, bad[:8].tolist())
        assert not np.any(_bits64(y64[:n]) == np.uint64(R.SENTINEL_BITS))        # (every row of the reference was written)


@pytest.mark.parametrize("case,which", [("sphere80_be", 7), ("diph2d", 2)])
def test_typed_launch_behind_the_done_flag_writes_nothing(pj, case, which):
    from penguin.jl_amd import _lib as L
    s = _system(pj, case, which)[0]
    v = _vectors(pj, case, which, "uniform")
    pc = PCS[1]
    out = L.debug_spmv_apply_typed(s._h, which, FIRST, v["x"], pc=pc, sigma=SIGMA, done=1)
    assert np.all(_bits32(out["y"]) == np.uint32(SENTINEL_F32)) and np.all(_bits32(out["p32"]) == np.uint32(SENTINEL_F32))
    out = L.debug_spmv_apply_typed(s._h, which, MIDDLE, v["x32"], base=v["base32"], pc=pc, done=1)
    assert np.all(_bits32(out["y"]) == np.uint32(SENTINEL_F32))
    out = L.debug_spmv_apply_typed(s._h, which, HANDOVER, v["x32"], base=v["base"], pc=pc, done=1)
    assert np.all(_bits64(out["y"]) == np.uint64(R.SENTINEL_BITS))
