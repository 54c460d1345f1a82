"""References for the two compact stagings of the dense crossprod (host only, no GPU).

rank_sums():      the set sums of a matrix of half-integers, in integers -- what the u16 quad kernel (2 * rank as u16, 32-bit
                  integer sums) and the fp32 pair kernel on rank inputs must return bit for bit
expected_bits():  the device entry's score for alpha = 1, beta = 0 from those sums
mixed_bound():    the error bound of the fp32 pair kernel on arbitrary doubles (PLAIDHIP_PRECISION_MIXED)
emulate_mixed():  that kernel's arithmetic on the terms of one set, in numpy -- and the mistake the bound must see
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from tests.helpers import exact_ref as er

U32 = 2.0 ** -24


def rank_sums(Gp, Gi, R):
    """Exact set sums of half-integers.  R: g x n, every value a multiple of 1/2 with |value| <= 32,767.5 (2 * value fits
    16 bits and a sign).  2 R as int64 times the 0/1 membership matrix (scipy CSC, int64) is an integer product: no device
    kernel and no floating-point summation.  Every sum is a multiple of 1/2 below 2^31, so float64(sum2) / 2 is exact.
    Returns (sums m x n float64, k: the m set sizes)."""
    Gp = np.asarray(Gp, dtype=np.int64)
    Gi = np.asarray(Gi, dtype=np.int64)
    R = np.asarray(R, dtype=np.float64)
    g = R.shape[0]
    m = len(Gp) - 1
    twice = R * 2.0
    assert np.all(np.isfinite(twice)) and np.all(twice == np.rint(twice)) and np.all(np.abs(twice) <= 65535.0), \
        "rank_sums: half-integers of magnitude <= 32,767.5 only"
    T = twice.astype(np.int64)
    M = sp.csc_matrix((np.ones(len(Gi), dtype=np.int64), Gi, Gp), shape=(g, m))
    sum2 = np.asarray(M.T.dot(T), dtype=np.int64)
    assert np.all(np.abs(sum2) < 2 ** 32)
    return sum2.astype(np.float64) / 2.0, np.diff(Gp)


def set_weight(k):
    """the mean statistic's set weight, the device's fp64 value fl(1 / (1e-8 + k)) (gsva_ref._w)"""
    return 1.0 / (1e-8 + np.asarray(k, dtype=np.float64))


def expected_bits(sums, k, stat):
    """The device entry's score for alpha = 1, beta = 0 from exact sums: "sum" the sum itself, "mean" fl(sum * w) with
    w = set_weight(k).  The kernels' epilogue alpha * (sum * w) + beta * (k * w) has ONE rounding then (1 * p is exact,
    0 * q is an exact zero, p + 0 is exact), whether or not the compiler contracts it into an fma; an empty set gives
    0 * w + 0 = 0.0"""
    if stat == "sum":
        return np.asarray(sums, dtype=np.float64)
    return np.asarray(sums, dtype=np.float64) * set_weight(k)[:, None]


def mixed_bound(mag, k, c):
    """|device - exact| for the fp32-staged pair kernel on arbitrary doubles, per score; mag = sum |x| over the set, k its
    nonzero terms, c the fp64 roundings after the sum (exact_ref.fp64_bound).  With u = 2^-24:

      * casting each value to fp32 costs <= u |x| (round to nearest), <= u mag over the set;
      * the kernel adds the eight values a lane gathers per chunk as two four-term fp32 sums (v0 + v1) + (v2 + v3): two
        roundings on the way of every term, whatever the grouping or the gene order inside the chunk, so each partial is
        off by <= ((1 + u)^2 - 1) = (2 u + u^2) of the sum of its |staged values|;
      * the staged values sum to <= (1 + u) mag in magnitude;
      * the partials are accumulated in fp64, in some order, and the epilogue rounds c times: exact_ref.fp64_bound(mag, k, c)
        (at most k - 1 of the additions have two nonzero operands).

    u mag + (2 u + u^2)(1 + u) mag = u mag (3 + 3 u + u^2) <= 3 u (1 + 2^-22) mag, so

        bound = 3 * 2^-24 * (1 + 2^-22) * mag  +  (k + c) * 2^-53 * mag  +  k * 2^-149

    the last term for values below the fp32 normal range (2^-126), where the cast is off by up to half a subnormal
    spacing, 2^-150, and an fp32 sum by as much again.  This restates the precision the kernel's own comment gives; it is
    not measured on the device.  The reference to hold it against is exact_ref.set_sums."""
    mag = np.asarray(mag, dtype=np.float64)
    kf = np.asarray(k, dtype=np.float64)
    return 3.0 * U32 * (1.0 + 2.0 ** -22) * mag + er.fp64_bound(mag, k, c) + kf * 2.0 ** -149


def emulate_mixed(x, acc32=False):
    """The fp32 pair kernel's arithmetic on the terms x of ONE set, taken in the given order: cast to fp32, pad to a
    multiple of 8 with zeros, per chunk of eight the two four-term fp32 sums (v0 + v1) + (v2 + v3) and (v4 + v5) + (v6 + v7),
    each added to its own fp64 accumulator chunk after chunk, then the two accumulators added.  acc32 = True keeps the two
    accumulators in fp32 instead -- the mistake (chunk partials summed in fp32 across the whole set) that mixed_bound() must
    see.  Returns a float (fp64)."""
    x = np.asarray(x, dtype=np.float64).ravel()
    with np.errstate(over="ignore"):
        v = x.astype(np.float32)
    pad = (-len(v)) % 8
    if pad or len(v) == 0:
        v = np.concatenate([v, np.zeros(pad if len(v) else 8, dtype=np.float32)])
    v = v.reshape(-1, 8)
    s0 = (v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])
    s1 = (v[:, 4] + v[:, 5]) + (v[:, 6] + v[:, 7])
    assert s0.dtype == np.float32 and s1.dtype == np.float32
    acc = np.float32 if acc32 else np.float64
    # (np.cumsum adds strictly one after the other: the accumulator's running value after every chunk)
    a0 = np.cumsum(s0.astype(acc), dtype=acc)[-1]
    a1 = np.cumsum(s1.astype(acc), dtype=acc)[-1]
    return float(acc(a0 + a1))


# ---------------------------------------------------------------- the inputs the tests share
def data(kind, g, n, seed):
    """the two kinds of tests/test_gpu_exact_sums.py::_data: "well" (positive, gamma(2, 1) + 0.25) and "cancel"
    (+-1e6 + N(0, 1): mag >> |sum|, where a relative tolerance says nothing)"""
    rng = np.random.default_rng(seed)
    if kind == "well":
        return rng.gamma(2.0, 1.0, size=(g, n)) + 0.25
    return np.where(rng.random((g, n)) < 0.5, 1e6, -1e6) + rng.normal(size=(g, n))


def sets(g, seed, m_random=130, kmax=400):
    """`m_random` sets of 1 ... kmax genes in UNSORTED gene order, then: an empty set, {g - 1}, {g - 2}, every gene (in
    a shuffled order).  Returns (Gp, Gi, names) with names["empty" | "last" | "before_last" | "all"] the set indices"""
    rng = np.random.default_rng(seed)
    kmax = min(kmax, g)
    sizes = rng.integers(1, kmax + 1, size=m_random)
    sizes[0] = 1
    sizes[1] = kmax
    lists = [rng.choice(g, size=int(s), replace=False) for s in sizes]
    names = {"empty": m_random, "last": m_random + 1, "before_last": m_random + 2, "all": m_random + 3}
    lists += [np.zeros(0, dtype=np.int64), np.array([g - 1]), np.array([g - 2]), rng.permutation(g)]
    Gp = np.concatenate([[0], np.cumsum([len(s) for s in lists])]).astype(np.int32)
    Gi = np.concatenate(lists).astype(np.int32)
    return Gp, Gi, names
