"""Extended-precision host reference of one SpMV launch (pg_spmv.h: launch modes 0, 1, 2, 3, 8) and the checker that holds a
launch's output against it.  Nothing here knows the library: the inputs are a CSR matrix and host vectors, the outputs of a
launch are plain arrays (what pg_debug_spmv_apply hands back, or what a test computes itself).

Reference.  Every value is carried as an unevaluated sum hi + lo of two doubles.  Row sums s = A x and Σ_j |a_ij x_j| are
formed in np.longdouble where it has a 64-bit significand and no row is longer than 16 entries (k 2^-64 <= 2^-60 relative to
Σ_j |a_ij x_j|), and in double-double arithmetic (two-sum / two-product, ~2^-100) otherwise; dots are always summed in
double-double, pairwise.

Bounds (standard forward bounds, any order of evaluation, with or without FMA; u = 2^-53, γ_k = k u / (1 - k u); the 2^-58
pays for the reference's own error):
    row of y, modes 0-3    |y_i - s_i|  <= (γ_k + 2^-58) Σ_j |a_ij x_j|,                     k = entries of row i
    row of y, mode 8       |y_i - m_i|  <= (γ_{k+3} + 2^-58) (|pc2 base_i| + |pc0 x_i| + |pc1| Σ_j |a_ij x_j|),
                           m_i = pc2 base_i + pc0 x_i + pc1 s_i
    dot (w, y)             |d - Σ w_i y_i| <= (γ_{n+1} + 2^-58) Σ |w_i y_i|   over the y the launch RETURNED
    folded sum             |f - Σ partials| <= γ_g Σ |partial|,   g partial sums per slot (the exact sum of the same partials)
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -53
PAD = 2.0 ** -58
SENTINEL_BITS = 0x7FF8C0DE5EED0BAD      # PG_DEBUG_SPMV_SENTINEL of include/penguin_hip.h
GUARD = 64                              # guard words behind row n of the y a launch hands back
HAVE_LONGDOUBLE = np.finfo(np.longdouble).nmant >= 63
LONGDOUBLE_MAX_ROW = 16

# dot slots of the launch modes (pg_spmv.h): slot -> (left operand, right operand); "d" = dotx, or x when there is none
DOT_SLOTS = {0: {}, 1: {0: "aux"}, 2: {0: "d", 1: "y"}, 3: {0: "d", 1: "y", 4: "aux"}, 8: {}}
FOLD_SLOTS = {1: 1, 2: 2, 3: 5}         # slots [0, nslots) a folded launch sums (mode 3: slots 2 and 3 belong to another kernel)


class SpmvMismatch(AssertionError):
    pass


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


# ---- double-double ------------------------------------------------------------------------------------------------------
def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _fast_two_sum(a, b):
    s = a + b
    return s, b - (s - a)


def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def dd_add(a, b):
    s, e = two_sum(a[0], b[0])
    t, f = two_sum(a[1], b[1])
    s, e = _fast_two_sum(s, e + t)
    return _fast_two_sum(s, e + f)


def dd_mul_f64(a, c):
    """(hi, lo) * double"""
    p, e = two_prod(a[0], c)
    return _fast_two_sum(p, e + a[1] * c)


def dd_total(a):
    """Σ of the pairs, pairwise"""
    hi, lo = np.array(a[0], dtype=np.float64).ravel(), np.array(a[1], dtype=np.float64).ravel()
    if hi.size == 0:
        return 0.0, 0.0
    while hi.size > 1:
        if hi.size & 1:
            hi, lo = np.append(hi, 0.0), np.append(lo, 0.0)
        h = hi.size // 2
        hi, lo = dd_add((hi[:h], lo[:h]), (hi[h:], lo[h:]))
    return float(hi[0]), float(lo[0])


def dd_dot(w, y):
    """(Σ w_i y_i, Σ |w_i y_i|) with exact products, each sum a pair"""
    p = two_prod(np.asarray(w, dtype=np.float64), np.asarray(y, dtype=np.float64))
    neg = p[0] < 0.0
    return dd_total(p), dd_total((np.where(neg, -p[0], p[0]), np.where(neg, -p[1], p[1])))


def _dd_rowsums(rowptr, prod):
    """Σ over the entries of each row of the pairs `prod`, entry by entry (a vector operation per entry slot)"""
    n = rowptr.size - 1
    ln = np.diff(rowptr)
    hi, lo = np.zeros(n), np.zeros(n)
    order = np.argsort(-ln, kind="stable")          # rows by falling length: slot j is held by a prefix of them
    sl = ln[order]
    for j in range(int(ln.max()) if n else 0):
        rows = order[: int(np.searchsorted(-sl, -j, side="left"))]      # rows with more than j entries
        k = rowptr[rows] + j
        hi[rows], lo[rows] = dd_add((hi[rows], lo[rows]), (prod[0][k], prod[1][k]))
    return hi, lo


def _ld_rowsums(rowptr, prod_ld):
    n = rowptr.size - 1
    out = np.zeros(n, dtype=np.longdouble)
    rows = np.nonzero(np.diff(rowptr) > 0)[0]
    if rows.size:
        out[rows] = np.add.reduceat(prod_ld, rowptr[rows])
    return out


def _ld_pair(v):
    hi = v.astype(np.float64)
    return hi, (v - hi.astype(np.longdouble)).astype(np.float64)


class Product:
    """s = A x and Σ_j |a_ij x_j| per row, as pairs; `arith`: None = longdouble where it suffices, "dd", "longdouble"."""

    def __init__(self, rowptr, col, val, x, arith=None):
        self.rowptr = np.asarray(rowptr, dtype=np.int64)
        col = np.asarray(col, dtype=np.int64)
        val = np.asarray(val, dtype=np.float64)
        self.x = np.asarray(x, dtype=np.float64)
        self.n = self.rowptr.size - 1
        self.k = np.diff(self.rowptr)
        assert self.rowptr[0] == 0 and self.rowptr[-1] == col.size == val.size and np.all(self.k >= 0)
        assert col.size == 0 or (col.min() >= 0 and col.max() < self.x.size)
        kmax = int(self.k.max()) if self.n else 0
        if arith is None:
            arith = "longdouble" if HAVE_LONGDOUBLE and kmax <= LONGDOUBLE_MAX_ROW else "dd"
        self.arith = arith
        xg = self.x[col]
        if arith == "longdouble":
            assert HAVE_LONGDOUBLE
            p = val.astype(np.longdouble) * xg.astype(np.longdouble)
            self._s_ld = _ld_rowsums(self.rowptr, p)
            self.s = _ld_pair(self._s_ld)
            self.abs = _ld_pair(_ld_rowsums(self.rowptr, np.abs(p)))
        else:
            p = two_prod(val, xg)
            neg = p[0] < 0.0
            self.s = _dd_rowsums(self.rowptr, p)
            self.abs = _dd_rowsums(self.rowptr, (np.where(neg, -p[0], p[0]), np.where(neg, -p[1], p[1])))

    def mode8(self, base, pc0, pc1, pc2):
        """m = pc2 base + pc0 x + pc1 s (pair) and the magnitude |pc2 base| + |pc0 x| + |pc1| Σ|a x| (double, rounded up a little)"""
        base = np.asarray(base, dtype=np.float64)
        xo = self.x[: self.n]
        if self.arith == "longdouble":
            L = np.longdouble
            m = L(pc2) * base.astype(L) + L(pc0) * xo.astype(L) + L(pc1) * self._s_ld
            m = _ld_pair(m)
        else:
            m = dd_add(dd_add(two_prod(base, pc2), two_prod(xo, pc0)), dd_mul_f64(self.s, pc1))
        mag = (np.abs(pc2 * base) + np.abs(pc0 * xo) + abs(pc1) * (self.abs[0] + np.abs(self.abs[1]))) * (1.0 + 8 * U)
        return m, mag


def _err(y, ref):
    """|y - (hi + lo)|: y - hi is exact where the two are close, and where they are not the rounding does not matter"""
    return np.abs((y - ref[0]) - ref[1])


def check_launch(prod, mode, y_full, slot_sums=None, *, aux=None, dotx=None, base=None, pc=(0.0, 0.0, 0.0), folded=None,
                 partials=None, ticket=None, label=""):
    """Hold what one launch of mode `mode` returned against the reference product `prod`.  y_full: n + GUARD doubles.
    slot_sums: 5 sums of the launch's partials (None: the dots are not checked); folded / partials (5 x g) / ticket: the
    folded scalar phase.  Returns the largest error / bound ratios {"row": .., "dot": .., "fold": ..}; raises SpmvMismatch."""
    n = prod.n
    y_full = np.ascontiguousarray(y_full, dtype=np.float64)
    if y_full.size != n + GUARD:
        raise SpmvMismatch(f"{label}: y has {y_full.size} entries, expected {n} + {GUARD}")
    bits = y_full.view(np.uint64)
    touched = np.nonzero(bits[n:] != np.uint64(SENTINEL_BITS))[0]
    if touched.size:
        raise SpmvMismatch(f"{label}: guard words behind row n overwritten: offsets {touched[:8].tolist()}")
    y = y_full[:n]
    unwritten = np.nonzero(bits[:n] == np.uint64(SENTINEL_BITS))[0]
    if unwritten.size:
        raise SpmvMismatch(f"{label}: {unwritten.size} rows of y not written, first {unwritten[:8].tolist()}")
    if not np.all(np.isfinite(y)):
        raise SpmvMismatch(f"{label}: y has non-finite rows, first {np.nonzero(~np.isfinite(y))[0][:8].tolist()}")
    ratios = {"row": 0.0, "dot": 0.0, "fold": 0.0}
    if mode == 8:
        b = prod.x[:n] if base is None else np.asarray(base, dtype=np.float64)
        ref, mag = prod.mode8(b, *pc)
        bound = (gamma(prod.k + 3) + PAD) * mag
    else:
        ref = prod.s
        bound = (gamma(prod.k) + PAD) * (prod.abs[0] + np.abs(prod.abs[1])) * (1.0 + 4 * U)
    err = _err(y, ref)
    bad = np.nonzero(err > bound)[0]
    if bad.size:
        i = bad[np.argmax(err[bad] / np.maximum(bound[bad], 1e-300))]
        raise SpmvMismatch(f"{label}: {bad.size} rows of y outside their bound, first {bad[:8].tolist()}; worst row {i}: y {y[i]!r} "
                           f"reference {ref[0][i]!r} error {err[i]:.3e} bound {bound[i]:.3e} entries {prod.k[i]}")
    nz = bound > 0.0
    if np.any(nz):
        ratios["row"] = float(np.max(err[nz] / bound[nz]))
    # ---- dots: over the y the launch returned
    if slot_sums is not None:
        ops = {"aux": aux, "d": prod.x[:n] if dotx is None else dotx, "y": y}
        for slot, name in DOT_SLOTS[mode].items():
            w = np.asarray(ops[name], dtype=np.float64)
            d_ref, d_abs = dd_dot(w, y)
            dbound = (float(gamma(n + 1)) + PAD) * (d_abs[0] + abs(d_abs[1])) * (1.0 + 4 * U)
            for what, got in (("partial sums", slot_sums), ("folded sum", folded)):
                if got is None:
                    continue
                e = abs((float(got[slot]) - d_ref[0]) - d_ref[1])
                if not e <= dbound:
                    raise SpmvMismatch(f"{label}: dot slot {slot} ({name}, y) from the {what}: {float(got[slot])!r} reference {d_ref[0]!r} "
                                       f"error {e:.3e} bound {dbound:.3e}")
                if dbound > 0.0:
                    ratios["dot"] = max(ratios["dot"], e / dbound)
    # ---- the folded scalar phase: the last block's sums of the very partials the launch stored
    if folded is not None:
        partials = np.asarray(partials, dtype=np.float64).reshape(5, -1)
        g = partials.shape[1]
        for slot in range(FOLD_SLOTS[mode]):
            p = partials[slot]
            if not np.all(np.isfinite(p)):
                raise SpmvMismatch(f"{label}: partials of slot {slot} not all written")
            t = dd_total((p, np.zeros(g)))
            fbound = float(gamma(g)) * float(np.sum(np.abs(p))) * (1.0 + 4 * U)
            e = abs((float(folded[slot]) - t[0]) - t[1])
            if not e <= fbound:
                raise SpmvMismatch(f"{label}: folded sum of slot {slot}: {float(folded[slot])!r}, its partials sum to {t[0]!r}: error {e:.3e} "
                                   f"bound {fbound:.3e}")
            if fbound > 0.0:
                ratios["fold"] = max(ratios["fold"], e / fbound)
        if ticket is not None and ticket != 0:
            raise SpmvMismatch(f"{label}: the ticket word reads {ticket} after the launch, not 0")
    return ratios


def check_untouched(y_full, n, ticket=None, label=""):
    """A launch that found the done flag set: every word of y still holds the sentinel and no ticket was drawn."""
    bits = np.ascontiguousarray(y_full, dtype=np.float64).view(np.uint64)
    if bits.size != n + GUARD or np.any(bits != np.uint64(SENTINEL_BITS)):
        raise SpmvMismatch(f"{label}: a launch behind the done flag wrote {int(np.sum(bits != np.uint64(SENTINEL_BITS)))} words of y")
    if ticket is not None and ticket != 0:
        raise SpmvMismatch(f"{label}: a launch behind the done flag left the ticket at {ticket}")


# ---- vectors of the tests ------------------------------------------------------------------------------------------------
FAMILIES = ("uniform", "scales", "integers")


def vector(family, n, rng):
    """uniform in [-0.5, 0.5] / random sign x 2^e, e uniform in [-30, 30], x a random mantissa in [1, 2) / the integers
    (j mod 97) - 48 from a random start (exact products with dyadic values)"""
    if family == "uniform":
        return rng.random(n) - 0.5
    if family == "scales":
        return rng.choice([-1.0, 1.0], n) * np.ldexp(1.0 + rng.random(n), rng.integers(-30, 31, n).astype(np.int32))
    assert family == "integers"
    return ((np.arange(n, dtype=np.int64) + int(rng.integers(0, 97))) % 97 - 48).astype(np.float64)
