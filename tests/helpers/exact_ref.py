"""Exact references for the fp64 routes, and the bounds that hold a kernel to them (host only, no GPU).

set_sums():          S[j, c] = sum_{i in G_j} w_ij * x_ic to ~2^-106 of sum |w_ij * x_ic|, then rounded once to fp64
                     (error-free TwoSum accumulation, TwoProduct by Veltkamp splitting for weighted terms)
assert_fp64_bound(): |got - ref| <= (k + c) * 2^-53 * mag per element, NaN and +-Inf patterns equal
col_medians():       R's median.default per column (na.rm = TRUE) with normalize_medians' ignore.zero rule

Why (k + c) u mag.  A sum of k terms in ANY order and association (atomics, trees, gene slices, partial sums) makes
k - 1 roundings, each of relative size <= u = 2^-53 of a partial sum, and no partial sum exceeds mag = sum |term|:
|err| <= (k - 1) u mag (to first order; the spare u mag of the bound covers the second-order terms).  `c` counts the
roundings that follow the sum -- on the device AND in the test's own fp64 restatement of the epilogue -- each of them
<= u |value| <= u mag.  A subnormal result adds at most 2^-1075 absolute per rounding: the floor (k + c) 2^-1074.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -53
_SPLIT = 134217729.0            # 2^27 + 1 (Veltkamp)


def two_sum(a, b):
    """s + e == a + b exactly, s = fl(a + b) (Knuth; any magnitudes, finite inputs)"""
    s = a + b
    bb = s - a
    e = (a - (s - bb)) + (b - bb)
    return s, e


def _split(a):
    t = _SPLIT * a
    hi = t - (t - a)
    return hi, a - hi


def two_prod(a, b):
    """p + e == a * b exactly, p = fl(a * b) (Dekker / Veltkamp; finite inputs, no overflow or underflow of e)"""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


class _Acc:
    """an unevaluated sum hi + lo + lo2 that absorbs terms without error (up to ~2^-159 of the absolute terms)"""

    def __init__(self, shape):
        self.hi = np.zeros(shape)
        self.lo = np.zeros(shape)
        self.lo2 = np.zeros(shape)

    def add(self, sl, x):
        hi, e = two_sum(self.hi[sl], x)
        self.hi[sl] = hi
        lo, e2 = two_sum(self.lo[sl], e)
        self.lo[sl] = lo
        self.lo2[sl] += e2

    def value(self):
        s, t = two_sum(self.hi, self.lo)
        # (hi, lo) -> (s, t) with |t| <= ulp(s) / 2: adding the small remainder rounds once
        return s + (t + self.lo2)


def dense_of_csc(Xp, Xi, Xx, g):
    """a dgCMatrix's slots as a dense g x n array (stored zeros and stored NaN kept)"""
    Xp = np.asarray(Xp, dtype=np.int64)
    n = len(Xp) - 1
    X = np.zeros((g, n))
    cols = np.repeat(np.arange(n), np.diff(Xp))
    X[np.asarray(Xi, dtype=np.int64), cols] = np.asarray(Xx, dtype=np.float64)
    return X


def fraction_sum(terms):
    """the exact sum of finite fp64 terms rounded once to fp64 (slow; the yardstick of the self-tests)"""
    from fractions import Fraction
    return float(sum((Fraction(float(t)) for t in terms), Fraction(0)))


def set_sums(Gp, Gi, X, weights=None, set_scale=None):
    """Exact set sums.  X: g x n (dense; dense_of_csc() for a dgCMatrix).  Set j holds the genes Gi[Gp[j]:Gp[j+1]];
    `weights` (one per entry of Gi) or `set_scale` (one per set) weight its terms, else they are 0/1.

    Returns (ref, mag, k), each m x n: the exact sum rounded once, sum |w x| (fp64), and the number of nonzero terms.
    NaN / Inf terms give what the IEEE sum gives in any order: NaN if a term is NaN or +Inf meets -Inf, else +-Inf.
    Finite terms must keep their partial sums below DBL_MAX (the error-free transformations need finite values)."""
    Gp = np.asarray(Gp, dtype=np.int64)
    Gi = np.asarray(Gi, dtype=np.int64)
    X = np.asarray(X, dtype=np.float64)
    m, n = len(Gp) - 1, X.shape[1]
    sizes = np.diff(Gp)
    order = np.argsort(-sizes, kind="stable")          # the sets still active at step t are a prefix of `order`
    start = Gp[:-1][order]
    ssz = sizes[order]
    acc = _Acc((m, n))
    mag = np.zeros((m, n))
    k = np.zeros((m, n), dtype=np.int64)
    nan = np.zeros((m, n), dtype=bool)
    pinf = np.zeros((m, n), dtype=bool)
    ninf = np.zeros((m, n), dtype=bool)
    w_all = None if weights is None else np.asarray(weights, dtype=np.float64)
    sc = None if set_scale is None else np.asarray(set_scale, dtype=np.float64)[order]
    with np.errstate(all="ignore"):
        for t in range(int(sizes.max()) if m else 0):
            a = int(np.searchsorted(-ssz, -t, side="left"))   # sets with size > t
            if a == 0:
                break
            sl = slice(0, a)
            pos = start[:a] + t
            x = X[Gi[pos], :]
            if w_all is not None:
                w = np.broadcast_to(w_all[pos][:, None], x.shape)
            elif sc is not None:
                w = np.broadcast_to(sc[:a][:, None], x.shape)
            else:
                w = None
            p = x if w is None else w * x
            fin = np.isfinite(p)
            nan[sl] |= np.isnan(p)
            pinf[sl] |= p == np.inf
            ninf[sl] |= p == -np.inf
            pf = np.where(fin, p, 0.0)
            mag[sl] += np.abs(pf)
            k[sl] += pf != 0.0
            if w is None:
                acc.add(sl, pf)
            else:
                hi, e = two_prod(np.where(fin, w, 0.0), np.where(fin, x, 0.0))
                acc.add(sl, hi)
                acc.add(sl, np.where(np.isfinite(e), e, 0.0))
    ref = acc.value()
    ref = np.where(pinf, np.inf, ref)
    ref = np.where(ninf, -np.inf, ref)
    ref = np.where(nan | (pinf & ninf), np.nan, ref)
    inv = np.empty(m, dtype=np.int64)
    inv[order] = np.arange(m)
    return ref[inv], mag[inv], k[inv]


def fp64_bound(mag, k, c):
    """(k + c) 2^-53 mag plus the subnormal floor (k + c) 2^-1074"""
    kc = np.asarray(k, dtype=np.float64) + float(c)
    return kc * U * np.asarray(mag, dtype=np.float64) + kc * 2.0 ** -1074


def bound_violations(got, ref, bound):
    """number of elements with |got - ref| > bound, or whose NaN / +Inf / -Inf pattern differs"""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    with np.errstate(all="ignore"):
        special = ~np.isfinite(got) | ~np.isfinite(ref)
        same_special = (np.isnan(got) & np.isnan(ref)) | (np.isinf(got) & (got == ref))
        err = np.abs(got - ref)
        bad = np.where(special, ~same_special, ~(err <= bound))
    return int(np.count_nonzero(bad))


def fp64_bound_violations(got, ref, mag, k, c):
    """number of elements outside (k + c) 2^-53 mag, or whose NaN / +Inf / -Inf pattern differs"""
    return bound_violations(got, ref, fp64_bound(mag, k, c))


def assert_within(got, ref, bound, what=""):
    """every element of `got` within `bound` (elementwise) of `ref`, and the same NaN / +Inf / -Inf elements"""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), got.shape)
    nbad = bound_violations(got, ref, bound)
    if nbad:
        with np.errstate(all="ignore"):
            fin = np.isfinite(got) & np.isfinite(ref)
            ratio = np.where(fin, np.abs(got - ref) / bound, 0.0)
            i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError(f"{what}: {nbad} of {got.size} elements outside the bound or with another NaN/Inf pattern; "
                             f"worst at {i}: got {got[i]!r} ref {ref[i]!r} bound {bound[i]!r} ({ratio[i]:.3g} x the bound)")


def assert_fp64_bound(got, ref, mag, k, c, what=""):
    """every element of `got` within (k + c) 2^-53 mag of `ref`, and the same NaN / +Inf / -Inf elements"""
    assert_within(got, ref, fp64_bound(mag, k, c), f"{what} [(k + {c}) 2^-53 mag]")


# ------------------------------------------------------------------ medians
def midpoint(a, b):
    """(a + b) / 2 rounded once: 0.5 * (a + b) unless the sum of two finite values overflows (then the exact halves)"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        s = a + b
        over = np.isinf(s) & np.isfinite(a) & np.isfinite(b)
        return np.where(over, 0.5 * a + 0.5 * b, 0.5 * s)


def resolve_ignore_zero(S, ignore_zero=None):
    """normalize_medians' ignore.zero (R/plaid.R:556-557): NULL -> min(x, na.rm = TRUE) == 0 (-0.0 == 0 too)"""
    if ignore_zero is not None:
        return bool(ignore_zero)
    S = np.asarray(S, dtype=np.float64)
    ok = ~np.isnan(S)
    return bool(ok.any() and S[ok].min() == 0.0)


def col_medians(S, ignore_zero=None):
    """per column: median.default(x[!is.na(x)]), with exact zeros dropped first under ignore.zero and 0 for a column
    with nothing left (R/plaid.R:561-570); NA (NaN) for an empty column otherwise.  Selection on sorted values; an even
    count returns midpoint() of the two middle values.  The order of -0.0 and +0.0 is not defined by R's sort: a zero
    median is returned as +0.0, as the kernels' order-preserving keys (which identify the two zeros) return it."""
    S = np.asarray(S, dtype=np.float64)
    iz = resolve_ignore_zero(S, ignore_zero)
    v = S + 0.0                                        # -0.0 -> +0.0
    if iz:
        v = np.where(v == 0.0, np.nan, v)
    m, n = v.shape
    srt = np.sort(v, axis=0)                           # NaN last
    cnt = np.count_nonzero(~np.isnan(v), axis=0)
    cols = np.arange(n)
    ia = np.maximum(cnt - 1, 0) // 2
    ib = np.minimum(cnt // 2, max(m - 1, 0))
    if m == 0:
        return np.full(n, 0.0 if iz else np.nan)
    a, b = srt[ia, cols], srt[ib, cols]
    with np.errstate(all="ignore"):
        med = np.where(a == b, a, midpoint(a, b))
    return np.where(cnt == 0, 0.0 if iz else np.nan, med)


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def assert_same_bits(got, exp, what=""):
    """bit for bit, every NaN counted equal to every NaN"""
    got = np.asarray(got, dtype=np.float64)
    exp = np.asarray(exp, dtype=np.float64)
    both_nan = np.isnan(got) & np.isnan(exp)
    bad = ~both_nan & (bits(got) != bits(exp))
    if bad.any():
        i = np.flatnonzero(bad.ravel())[:5]
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} differ; first at {i.tolist()}: "
                             f"got {got.ravel()[i].tolist()} expected {exp.ravel()[i].tolist()}")
