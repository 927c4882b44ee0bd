"""The host reference of the SpMV launch modes and its checker (tests/spmv_reference.py), on a synthetic matrix, without the
library: the reference agrees with exact rational arithmetic to 2^-60; the checker accepts the plain fp64 product in three
summation orders and rejects every defect the GPU tests (tests/test_gpu_spmv_host_reference.py) are there to catch.  What is
rejected here is what those tests can see."""
from fractions import Fraction

import numpy as np
import pytest

from tests import spmv_reference as R

PC = (0.75, -0.4375, 1.25)


def _matrix():
    """7-point stencil on 12^3 cells with random values (border rows: fewer entries), then five long irregular rows."""
    rng = np.random.default_rng(20240607)
    m = 12
    idx = np.arange(m ** 3).reshape(m, m, m)
    rows, cols = [idx.ravel()], [idx.ravel()]
    for ax in range(3):
        for sh in (-1, 1):
            src = np.take(idx, range(max(0, -sh), m - max(0, sh)), axis=ax).ravel()
            rows.append(src)
            cols.append(src + sh * m ** (2 - ax))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    n0 = m ** 3
    long_rows = [9, 17, 40, 133, 300]
    n = n0 + len(long_rows)
    for q, ln in enumerate(long_rows):
        rows = np.concatenate([rows, np.full(ln, n0 + q)])
        cols = np.concatenate([cols, np.sort(rng.choice(n, ln, replace=False))])
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    val = (rng.random(rows.size) - 0.5) * np.ldexp(1.0, rng.integers(-3, 10, rows.size).astype(np.int32))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    return rowptr, cols.astype(np.int64), val, n


ROWPTR, COL, VAL, N = _matrix()
NV = N + 7                                       # a few ghost entries behind the own rows, never referenced by a column
SAMPLE = np.concatenate([np.random.default_rng(5).choice(N - 5, 195, replace=False), np.arange(N - 5, N)])


def _vectors(family):
    rng = np.random.default_rng(11)
    return {k: R.vector(family, NV if k == "x" else N, rng) for k in ("x", "aux", "dotx", "base")}


def _fr(pair, i=None):
    return Fraction(float(pair[0])) + Fraction(float(pair[1])) if i is None else Fraction(float(pair[0][i])) + Fraction(float(pair[1][i]))


ARITH = [None, "dd"] + (["longdouble"] if R.HAVE_LONGDOUBLE else [])


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("arith", ARITH)
def test_reference_agrees_with_rational_arithmetic(arith, family):
    """Row sums, Σ|a x| and the mode-8 value on 200 rows (the long ones among them), and a dot over every row: to 2^-60 of the
    row's Σ|a x| (of its mode-8 magnitude; of Σ|w y|)."""
    v = _vectors(family)
    if arith == "longdouble":       # (the reference takes it only for rows of <= 16 entries: 2^-60 holds there)
        sample = SAMPLE[np.diff(ROWPTR)[SAMPLE] <= R.LONGDOUBLE_MAX_ROW]
    else:
        sample = SAMPLE
    p = R.Product(ROWPTR, COL, VAL, v["x"], arith=arith)
    assert p.arith == ("dd" if arith is None else arith)          # five rows are longer than 16 entries
    m8, mag = p.mode8(v["base"], *PC)
    tol = Fraction(1, 2 ** 60)
    for i in sample:
        a, b = ROWPTR[i], ROWPTR[i + 1]
        terms = [Fraction(float(VAL[k])) * Fraction(float(v["x"][COL[k]])) for k in range(a, b)]
        s, sabs = sum(terms, Fraction(0)), sum((abs(t) for t in terms), Fraction(0))
        assert abs(_fr(p.s, i) - s) <= tol * sabs, (i, b - a)
        assert abs(_fr(p.abs, i) - sabs) <= tol * sabs, (i, b - a)
        m = Fraction(PC[2]) * Fraction(float(v["base"][i])) + Fraction(PC[0]) * Fraction(float(v["x"][i])) + Fraction(PC[1]) * s
        mmag = abs(Fraction(PC[2]) * Fraction(float(v["base"][i]))) + abs(Fraction(PC[0]) * Fraction(float(v["x"][i]))) + abs(Fraction(PC[1])) * sabs
        assert abs(_fr(m8, i) - m) <= tol * mmag, i
        assert Fraction(float(mag[i])) >= mmag and Fraction(float(mag[i])) <= mmag * (1 + Fraction(1, 2 ** 40)), i
    y = p.s[0]
    d, dabs = R.dd_dot(v["aux"], y)
    ex = [Fraction(float(a)) * Fraction(float(b)) for a, b in zip(v["aux"], y)]
    assert abs(_fr(d) - sum(ex, Fraction(0))) <= tol * sum((abs(t) for t in ex), Fraction(0))
    assert abs(_fr(dabs) - sum((abs(t) for t in ex), Fraction(0))) <= tol * sum((abs(t) for t in ex), Fraction(0))


def test_row_sums_of_both_arithmetics_agree_on_short_rows():
    if not R.HAVE_LONGDOUBLE:
        return       # (one arithmetic only: nothing to compare; the double-double path is checked against Fraction above)
    short = np.nonzero(np.diff(ROWPTR) <= R.LONGDOUBLE_MAX_ROW)[0]
    v = _vectors("scales")
    a, b = R.Product(ROWPTR, COL, VAL, v["x"], arith="longdouble"), R.Product(ROWPTR, COL, VAL, v["x"], arith="dd")
    diff = np.abs((a.s[0] - b.s[0]) + (a.s[1] - b.s[1]))[short]
    assert np.all(diff <= 2.0 ** -60 * b.abs[0][short])


# ---- plain fp64 products in three orders -----------------------------------------------------------------------------------
def _padded(x):
    k = np.diff(ROWPTR)
    w = 1
    while w < k.max():
        w *= 2
    P = np.zeros((N, w))
    j = np.arange(COL.size) - np.repeat(ROWPTR[:-1], k)
    P[np.repeat(np.arange(N), k), j] = VAL * x[COL]
    return P, k


def _fp64_product(x, order):
    P, k = _padded(x)
    if order == "pairwise":
        while P.shape[1] > 1:
            P = P[:, 0::2] + P[:, 1::2]
        return P[:, 0]
    s = np.zeros(N)
    cols = range(P.shape[1]) if order == "forwards" else range(P.shape[1] - 1, -1, -1)
    for j in cols:
        s = s + P[:, j]
    return s


def _dot64(w, y, order):
    p = w * y
    if order == "pairwise":
        return float(np.sum(p))                     # numpy sums pairwise
    s = 0.0
    for t in (p if order == "forwards" else p[::-1]):
        s += t
    return s


def _launch(v, mode, order="forwards", dotx=True, base=True, pc=PC):
    """What a correct fp64 kernel hands back for one launch: (y with guard words, 5 slot sums, checker keywords)."""
    s = _fp64_product(v["x"], order)
    kw = {"aux": v["aux"] if mode in (1, 3) else None, "dotx": v["dotx"] if (dotx and mode in (2, 3)) else None,
          "base": v["base"] if (base and mode == 8) else None, "pc": pc}
    if mode == 8:
        b = v["base"] if base else v["x"][:N]
        y = pc[2] * b + (pc[0] * v["x"][:N] + pc[1] * s)
    else:
        y = s
    sentinel = np.array([R.SENTINEL_BITS], dtype=np.uint64).view(np.float64)[0]
    yf = np.full(N + R.GUARD, sentinel)
    yf[:N] = y
    sums = np.full(5, sentinel)
    ops = {"aux": v["aux"], "d": v["dotx"] if kw["dotx"] is not None else v["x"][:N], "y": y}
    for slot, name in R.DOT_SLOTS[mode].items():
        sums[slot] = _dot64(ops[name], y, order)
    return yf, sums, kw


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("order", ["forwards", "backwards", "pairwise"])
def test_checker_accepts_the_fp64_product_in_any_order(order, family):
    v = _vectors(family)
    prod = R.Product(ROWPTR, COL, VAL, v["x"])
    worst = {"row": 0.0, "dot": 0.0}
    for mode in (0, 1, 2, 3, 8):
        for dotx in ((False, True) if mode in (2, 3) else (False,)):
            for base in ((False, True) if mode == 8 else (False,)):
                yf, sums, kw = _launch(v, mode, order, dotx, base)
                r = R.check_launch(prod, mode, yf, sums, label=f"{order} mode {mode}", **kw)
                worst = {k: max(worst[k], r[k]) for k in worst}
    print(order, family, "largest error / bound:", worst)
    assert worst["row"] <= 1.0 and worst["dot"] <= 1.0
    if family == "integers":
        pass      # (the values are not dyadic here: the products round)
    else:
        assert worst["row"] > 0.0      # the bounds are not vacuous: an fp64 product does err


def _row_bound(prod, mode, kw, i):
    if mode == 8:
        _, mag = prod.mode8(kw["base"] if kw["base"] is not None else prod.x[:N], *kw["pc"])
        return (float(R.gamma(prod.k[i] + 3)) + R.PAD) * mag[i]
    return (float(R.gamma(prod.k[i])) + R.PAD) * prod.abs[0][i]


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 8])
def test_checker_rejects_a_row_moved_by_twice_its_bound(mode):
    v = _vectors("uniform")
    prod = R.Product(ROWPTR, COL, VAL, v["x"])
    for i in (0, 777, N - 1):                      # a corner row, a bulk row, the longest row
        for sign in (1.0, -1.0):
            yf, sums, kw = _launch(v, mode)
            ref = prod.mode8(kw["base"] if kw["base"] is not None else prod.x[:N], *PC)[0] if mode == 8 else prod.s
            yf[i] = ref[0][i] + sign * 2.0 * _row_bound(prod, mode, kw, i) * (1 + 2.0 ** -20)
            with pytest.raises(R.SpmvMismatch, match="outside their bound"):
                R.check_launch(prod, mode, yf, None, **kw)


@pytest.mark.parametrize("mode,slot", [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 4)])
def test_checker_rejects_a_dot_with_one_row_left_out(mode, slot):
    """The row left out is one of median weight in the dot, not the heaviest."""
    v = _vectors("uniform")
    prod = R.Product(ROWPTR, COL, VAL, v["x"])
    yf, sums, kw = _launch(v, mode)
    y = yf[:N]
    w = {"aux": v["aux"], "d": v["dotx"], "y": y}[R.DOT_SLOTS[mode][slot]]
    i = int(np.argsort(np.abs(w * y))[N // 2])
    sums[slot] -= w[i] * y[i]
    with pytest.raises(R.SpmvMismatch, match=f"dot slot {slot}"):
        R.check_launch(prod, mode, yf, sums, **kw)
    # ... and the same defect in the folded sum alone
    yf, sums, kw = _launch(v, mode)
    folded = sums.copy()
    folded[slot] -= w[i] * y[i]
    partials = np.zeros((5, 8))
    partials[:, 0] = np.where(np.isfinite(sums), sums, 0.0)
    partials[:, 0][slot] = folded[slot]
    with pytest.raises(R.SpmvMismatch, match=f"dot slot {slot} .* folded sum"):
        R.check_launch(prod, mode, yf, sums, folded=folded, partials=partials, ticket=0, **kw)


@pytest.mark.parametrize("mode", [2, 3])
def test_checker_rejects_the_dot_taken_with_x_instead_of_dotx(mode):
    v = _vectors("uniform")
    prod = R.Product(ROWPTR, COL, VAL, v["x"])
    yf, sums, kw = _launch(v, mode, dotx=False)            # the kernel ignored dotx ...
    kw["dotx"] = v["dotx"]                                 # ... which the launch was given
    with pytest.raises(R.SpmvMismatch, match="dot slot 0"):
        R.check_launch(prod, mode, yf, sums, **kw)


@pytest.mark.parametrize("base", [True, False])
def test_checker_rejects_mode_8_with_pc0_and_pc2_swapped(base):
    v = _vectors("uniform")
    prod = R.Product(ROWPTR, COL, VAL, v["x"])
    for pc in (PC, (1.0, -0.8, 0.8)):
        yf, sums, kw = _launch(v, 8, base=base, pc=(pc[2], pc[1], pc[0]))
        kw["pc"] = pc
        if base:
            with pytest.raises(R.SpmvMismatch, match="outside their bound"):
                R.check_launch(prod, 8, yf, None, **kw)
        else:
            # base aliased to x: pc2 x + pc0 x is symmetric in the two -- the swap is the same polynomial and must pass
            R.check_launch(prod, 8, yf, None, **kw)


@pytest.mark.parametrize("mode", [0, 3, 8])
def test_checker_rejects_an_unwritten_row_and_an_overwritten_guard_word(mode):
    v = _vectors("uniform")
    prod = R.Product(ROWPTR, COL, VAL, v["x"])
    sentinel = np.array([R.SENTINEL_BITS], dtype=np.uint64).view(np.float64)[0]
    for i in (0, 1000, N - 1):
        yf, sums, kw = _launch(v, mode)
        yf[i] = sentinel
        with pytest.raises(R.SpmvMismatch, match="not written"):
            R.check_launch(prod, mode, yf, sums, **kw)
    for g in (0, 1, R.GUARD - 1):
        yf, sums, kw = _launch(v, mode)
        yf[N + g] = 0.0
        with pytest.raises(R.SpmvMismatch, match="guard words"):
            R.check_launch(prod, mode, yf, sums, **kw)
    yf, sums, kw = _launch(v, mode)
    yf[N] = np.nan                                          # another NaN than the sentinel is an overwrite too
    with pytest.raises(R.SpmvMismatch, match="guard words"):
        R.check_launch(prod, mode, yf, sums, **kw)


def test_checker_of_the_folded_phase_and_of_the_done_flag():
    v = _vectors("uniform")
    prod = R.Product(ROWPTR, COL, VAL, v["x"])
    yf, sums, kw = _launch(v, 3)
    rng = np.random.default_rng(3)
    g = 37
    partials = np.zeros((5, g))
    for slot in (0, 1, 4):                                  # g partials that sum to the slot's dot (up to rounding)
        w = rng.random(g)
        partials[slot] = sums[slot] * w / w.sum()
    folded = np.array([float(np.sum(partials[s][::-1])) for s in range(5)])
    sums = partials.sum(axis=1)
    r = R.check_launch(prod, 3, yf, sums, folded=folded, partials=partials, ticket=0, **kw)
    assert r["fold"] <= 1.0
    with pytest.raises(R.SpmvMismatch, match="ticket"):
        R.check_launch(prod, 3, yf, sums, folded=folded, partials=partials, ticket=5, **kw)
    bad = folded.copy()
    bad[4] -= partials[4][g // 2]                           # the last block missed one block's partial
    with pytest.raises(R.SpmvMismatch, match="slot 4"):
        R.check_launch(prod, 3, yf, sums, folded=bad, partials=partials, ticket=0, **kw)
    sentinel = np.array([R.SENTINEL_BITS], dtype=np.uint64).view(np.float64)[0]
    untouched = np.full(N + R.GUARD, sentinel)
    R.check_untouched(untouched, N, ticket=0)
    untouched[5] = 1.0
    with pytest.raises(R.SpmvMismatch, match="done flag"):
        R.check_untouched(untouched, N, ticket=0)
    with pytest.raises(R.SpmvMismatch, match="done flag"):
        R.check_untouched(np.full(N + R.GUARD, sentinel), N, ticket=1)
