"""The dense-G matrix-core backend of the crossprod (plaid_amd/csrc/kernels_mfma.hip) restated on the host, and the bound
that holds it to exact sums (numpy only, no GPU).

split3():        the hi / mid / lo bf16 planes of split3_bf16_kernel for fp64 input, and what they leave over
splittable():    whether a value enters the bf16 operand at all (else the kernels carry it in fp64)
mfma_bound():    the per-score allowance |device - exact|, derived below
emulate():       the planes summed in fp32 in one fixed order -- for the self-tests of the bound (tests/test_mfma_ref.py),
                 NOT a bit-level model of the device: the matrix instruction documents neither its order nor its rounding

The reference to hold the kernel against is exact_ref.set_sums, which also supplies mag and k.
"""
from __future__ import annotations

import numpy as np

from tests.helpers import exact_ref as er

U24 = 2.0 ** -24                # the split's relative residual: 24 significant bits
ULP32 = 2.0 ** -23              # one fp32 ulp, relative: covers truncation as well as round-to-nearest
TINY32 = 2.0 ** -126            # the smallest normal fp32 / bf16 magnitude
HALF_INT_EXACT = 20448.0        # half-integer ranks up to here (the largest the LDS-resident kernels take) split exactly


def to_bf16(x32):
    """fp32 -> bf16 (returned as the fp32 value it stands for), round to nearest even; NaN stays NaN, what rounds past
    the largest bf16 becomes +-Inf"""
    x32 = np.asarray(x32, dtype=np.float32)
    u = np.ascontiguousarray(x32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    out = r.view(np.float32).reshape(x32.shape)
    return np.where(np.isnan(x32), np.float32(np.nan), out)


def _head(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return to_bf16(np.asarray(x, dtype=np.float64).astype(np.float32))


def splittable(x):
    """True where the bf16 head of x is finite.  NaN, +-Inf and a finite |x| >= (2 - 2^-8) 2^127 (3.39e38: the head
    rounds to Inf, and mid = x - Inf would be garbage) are not: the kernels stage them as 0 and add them in fp64"""
    return np.isfinite(_head(x))


def split3(x):
    """(hi, mid, lo, residual) of fp64 x, each fp64: hi = bf16(fp32(x)), mid = bf16(fp32(x - hi)), lo =
    bf16(fp32(x - hi - mid)), the differences taken in fp64 (they are exact there: a bf16 head agrees with x in its
    leading bits), residual = x - hi - mid - lo.  Values that are not splittable() give four zeros"""
    x = np.asarray(x, dtype=np.float64)
    x = np.where(splittable(x), x, 0.0)
    hi = _head(x).astype(np.float64)
    r = x - hi
    mid = _head(r).astype(np.float64)
    r = r - mid
    lo = _head(r).astype(np.float64)
    return hi, mid, lo, r - lo


def mfma_bound(mag, k, c):
    """|device - exact| per score for the bf16 x 3 / fp32-accumulate backend; mag = sum |x| over the set's finite terms,
    k the number of nonzero terms, c the fp64 roundings that follow the sum (all three as exact_ref counts them).

        bound = 3 k 2^-23 mag  +  (k + c) 2^-53 mag + (k + c) 2^-1074  +  3 k 2^-126

    Derivation (nothing here is measured on the device).
      * The split.  Each plane is bf16(fp32(r)) of what is left, r: 8 significant bits, round to nearest, behind a cast
        that loses at most 2^-24 |r|; the difference r - plane is exact in fp64.  So a plane leaves at most
        (2^-9 + 2^-24) |r|, and three of them (2^-9 + 2^-24)^3 |x| < 2^-26 |x| -- as long as every plane is a normal
        number.  The bound uses what the kernel file states, "24 significant bits": residual <= 2^-24 |x| per value,
        <= 2^-24 mag per score.
      * The fp32 accumulation.  G is 0/1, so the products are the plane values themselves, exact.  The set's score is a sum
        of 3 k nonzero fp32 terms in an order, a grouping and with an internal rounding that the instruction does not
        document: at most 3 k - 1 additions of two nonzero operands, each off by at most one fp32 ulp (2^-23 relative,
        which covers truncation as well as round-to-nearest) of a partial sum, and no partial sum exceeds
        sum |plane| <= mag to first order: (3 k - 1) 2^-23 mag.
      * Together (3 k - 1) 2^-23 mag + 2^-24 mag < 3 k 2^-23 mag: the first term of the bound.  (To first order, as in
        exact_ref: the half ulp left over covers the second-order terms.)
      * The epilogue converts the fp32 sum to fp64 (exact) and rounds c times in fp64: exact_ref.fp64_bound's c (its k u mag
        is kept too: the test's own restatement of the reference is allowed what every fp64 route is allowed).
      * Below the normal range.  A plane value or a partial sum under 2^-126 may be rounded to a subnormal (absolute error
        <= 2^-134, half the spacing of bf16 subnormals) or flushed to zero by the cast, the matrix core's inputs or its
        accumulator (absolute error < 2^-126); which of these the hardware does is not assumed: one 2^-126 for each of
        the 3 k terms.
    Half-integers of magnitude <= 20,448 (ranks) need 16 bits: hi and mid hold them, lo = residual = 0; and fp32 adds them
    exactly while the sums stay below 2^23.  The bound does not use that; tests/test_mfma_ref.py checks the split part.
    Range: the fp32 accumulator overflows where a partial sum passes 3.4e38, so mag has to stay below 2^127."""
    mag = np.asarray(mag, dtype=np.float64)
    kf = np.asarray(k, dtype=np.float64)
    return 3.0 * kf * ULP32 * mag + er.fp64_bound(mag, k, c) + 3.0 * kf * TINY32


def emulate(x, drop_lo=False, skip=None):
    """The planes of the terms x of ONE set (fp64, in gene order) summed in fp32 one after the other: every hi, then every
    mid, then every lo.  drop_lo leaves the third plane out; skip (a boolean mask over x) leaves terms out altogether --
    the two mistakes the bound must see.  Returns a float"""
    x = np.asarray(x, dtype=np.float64).ravel()
    if skip is not None:
        x = x[~np.asarray(skip, dtype=bool)]
    hi, mid, lo, _ = split3(x)
    planes = [hi, mid] if drop_lo else [hi, mid, lo]
    terms = np.concatenate(planes).astype(np.float32) if len(x) else np.zeros(1, dtype=np.float32)
    assert np.array_equal(terms.astype(np.float64), np.concatenate(planes)) if len(x) else True
    return float(np.cumsum(terms, dtype=np.float32)[-1])


def emulate_sets(Gp, Gi, X, drop_lo=False, skip_genes=None):
    """emulate() for every (set, sample): m x n.  skip_genes: a boolean mask over the genes"""
    Gp = np.asarray(Gp, dtype=np.int64)
    Gi = np.asarray(Gi, dtype=np.int64)
    X = np.asarray(X, dtype=np.float64)
    m, n = len(Gp) - 1, X.shape[1]
    out = np.zeros((m, n))
    for j in range(m):
        idx = np.sort(Gi[Gp[j]:Gp[j + 1]])
        sk = None if skip_genes is None else np.asarray(skip_genes, dtype=bool)[idx]
        for c in range(n):
            out[j, c] = emulate(X[idx, c], drop_lo, sk)
    return out


# ---------------------------------------------------------------- the inputs the tests share
KINDS = ("well", "cancel", "normal", "tiny_mix", "half_ranks")


def data(kind, g, n, seed):
    """well: gamma(2, 1) + 0.25 (positive); cancel: +-1e6 + N(0, 1) (mag >> |sum|); normal: N(0, 1); tiny_mix: O(1)
    values next to values in [1e-45, 1e-30] of either sign (below and around the fp32 normal range); half_ranks: average
    ranks of tied data, multiples of 1/2 in [1, g] -- where the split is exact.  Every column is its own draw"""
    rng = np.random.default_rng(seed)
    if kind == "well":
        return rng.gamma(2.0, 1.0, size=(g, n)) + 0.25
    if kind == "cancel":
        return np.where(rng.random((g, n)) < 0.5, 1e6, -1e6) + rng.normal(size=(g, n))
    if kind == "normal":
        return rng.normal(size=(g, n))
    if kind == "tiny_mix":
        tiny = 10.0 ** rng.uniform(-45.0, -30.0, size=(g, n)) * np.where(rng.random((g, n)) < 0.5, 1.0, -1.0)
        return np.where(rng.random((g, n)) < 0.5, rng.normal(size=(g, n)), tiny)
    if kind == "half_ranks":
        v = rng.integers(0, max(2, g // 3), size=(g, n))
        R = np.empty((g, n))
        for c in range(n):                                   # average ranks: (number below) + (number equal + 1) / 2
            s = np.sort(v[:, c])
            R[:, c] = (np.searchsorted(s, v[:, c], "left") + np.searchsorted(s, v[:, c], "right") + 1) / 2.0
        return R
    raise ValueError(kind)


SIZES = (0, 1, 2, 8, 31, 32, 33, 64, 65, 400)


def sets(g, m, seed):
    """m sets over g genes in UNSORTED gene order: first the sizes of SIZES that fit (size <= g; 0 is the empty set), then
    {g - 1}, then {0, g - 1} (the first and the last gene; {0} again if g = 1), then random sizes in 1 ... min(g, 400).
    When m is smaller than that list its head is kept, but {g - 1} and {0, g - 1} are always in (they replace the tail).
    Returns (Gp, Gi, names) with names["last"], names["ends"] and names["empty"] (or None) set indices"""
    rng = np.random.default_rng(seed)
    lists = [rng.choice(g, size=s, replace=False) for s in SIZES if s <= g]
    ends = np.array([0, g - 1]) if g > 1 else np.array([0])
    if m == 1:
        lists = [np.array([g - 1])]
    else:
        lists = lists[:m - 2] + [np.array([g - 1]), ends]
        lists += [rng.choice(g, size=int(rng.integers(1, min(g, 400) + 1)), replace=False) for _ in range(m - len(lists))]
    assert len(lists) == m
    names = {"empty": None, "last": None, "ends": None}
    for j, s in enumerate(lists):
        if len(s) == 0:
            names["empty"] = j
        elif len(s) == 1 and s[0] == g - 1 and names["last"] is None:
            names["last"] = j
        elif np.array_equal(s, ends):
            names["ends"] = j
    Gp = np.concatenate([[0], np.cumsum([len(s) for s in lists])]).astype(np.int32)
    Gi = (np.concatenate(lists) if len(lists) else np.zeros(0)).astype(np.int32)
    return Gp, Gi, names
