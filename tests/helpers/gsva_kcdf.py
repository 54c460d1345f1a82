"""GSVA's Gaussian kernel CDF estimate (kcdf = "Gaussian"), the row transform "gauss" of replaid.gsva.exact, written twice
from the form pinned in include/plaidhip.h (plaidhip_gsva_kcdf), for the tests (host only, no GPU).

Per gene row x (n >= 2 samples), all in fp64, every sum sequential in sample order k = 0 .. n - 1 from 0.0:

    mean = (x_0 + ... + x_{n-1}) / n;  ss = sum_k d_k * d_k, d_k = x_k - mean;  h = sqrt(ss / (n - 1)) / 4.0
    c(d): v = d / h;  v < -10 -> 0.0;  v > 10 -> 1.0;  else t = T[(int)(fabs(v) / 10.0 * 10000.0)];  v < 0 ? 1.0 - t : t
    V_j  = sum_k c(x_j - x_k)

A NaN index (h == 0: v = 0 / 0) reads T[0]; a NaN h (a NaN or an infinity in the row) gives a NaN row.

literal() is GSVA's double loop in plain Python floats; pinned() the same operations in numpy, whose np.add.accumulate
adds in order (np.sum is pairwise and would not).  T is a parameter: the GPU tests pass the library's own table.
"""
from __future__ import annotations

import math

import numpy as np

TABLE = 10001


def table_erfc():
    """T[i] = Phi(10.0 * i / 10000.0) with the C library's erfc, as the library builds it"""
    T = np.array([0.5 * math.erfc(-(10.0 * float(i) / 10000.0) / math.sqrt(2.0)) for i in range(TABLE)])
    return np.maximum.accumulate(T)


def literal(X, T):
    """the double loop, one Python float operation per pinned operation"""
    X = np.asarray(X, dtype=np.float64)
    g, n = X.shape
    T = [float(t) for t in T]
    V = np.empty((g, n))
    inf = float("inf")
    for i in range(g):
        x = [float(v) for v in X[i]]
        s = 0.0
        for k in range(n):
            s = s + x[k]
        mean = s / float(n)
        ss = 0.0
        for k in range(n):
            d = x[k] - mean
            ss = ss + d * d
        q = ss / float(n - 1)
        h = (math.sqrt(q) if q >= 0.0 and q != inf else q) / 4.0       # (sqrt(inf) = inf, sqrt(NaN) = NaN)
        if h != h:
            V[i] = np.nan
            continue
        for j in range(n):
            acc = 0.0
            for k in range(n):
                d = x[j] - x[k]
                if h == 0.0:
                    v = float("nan") if d == 0.0 or d != d else math.copysign(inf, d)
                else:
                    v = d / h
                if v < -10.0:
                    c = 0.0
                elif v > 10.0:
                    c = 1.0
                else:
                    u = math.fabs(v) / 10.0 * 10000.0
                    t = T[int(u) if u == u else 0]
                    c = 1.0 - t if v < 0.0 else t
                acc = acc + c
            V[i, j] = acc
    return V


def bandwidths(X):
    """h per row, the sums by np.add.accumulate"""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[1]
    with np.errstate(all="ignore"):
        mean = np.add.accumulate(X, axis=1)[:, -1] / float(n)
        d = X - mean[:, None]
        ss = np.add.accumulate(d * d, axis=1)[:, -1]
        return np.sqrt(ss / float(n - 1)) / 4.0


def pinned(X, T, cols=None, block_elems=1 << 24):
    """the pinned form in numpy: V (g x n), or its columns `cols` (the sums still run over all n samples)"""
    X = np.asarray(X, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    g, n = X.shape
    cols = np.arange(n) if cols is None else np.asarray(cols)
    h = bandwidths(X)
    V = np.empty((g, len(cols)))
    step = max(1, block_elems // max(1, n * len(cols)))
    with np.errstate(all="ignore"):
        for a in range(0, g, step):
            x = X[a:a + step]
            hh = h[a:a + step, None, None]
            v = (x[:, cols, None] - x[:, None, :]) / hh                 # [row, j, k]
            u = np.abs(v) / 10.0 * 10000.0
            idx = np.where(u <= 10000.0, u, 0.0).astype(np.int64)      # (NaN and the out-of-range terms read T[0])
            t = T[idx]
            c = np.where(v < -10.0, 0.0, np.where(v > 10.0, 1.0, np.where(v < 0.0, 1.0 - t, t)))
            V[a:a + step] = np.add.accumulate(c, axis=2)[:, :, -1]
    V[np.isnan(h)] = np.nan
    return V


def seam_row(n, m, p, rng):
    """Integer multiples of 2^p (p >= 0) with mean 0 and sd = 4 m 2^p exactly (n >= 16), so that h = m 2^p and every
    difference d is a multiple of 2^p.  m = 1: d / h is exact and fabs(v) / 10 * 10000 lands ON integers (1000 v is an
    integer for every dyadic v it can be one for).  m = 5: v = d / 5 is rounded and the expression lands BESIDE the integer
    200 d for some d (d = 7: 1399.9999999999998, d = 11: 2200.0000000000005).  The values +-5 m 2^p are in the row, so
    v = +-10 exactly occurs, and so does |v| > 10."""
    assert p >= 0 and m in (1, 5) and n >= 16
    pairs = n // 2
    target = 16 * m * m * (n - 1)                                       # sum of squares in units of 4^p
    for _ in range(1000):
        a = [5 * m] + [int(v) for v in rng.integers(0, 6 * m + 1, size=pairs - 3)]
        rem = target // 2 - sum(v * v for v in a)
        if rem < 0:
            continue
        hit = next(((q, r) for q in range(math.isqrt(rem), -1, -1) for r in [math.isqrt(rem - q * q)]
                    if q * q + r * r == rem), None)
        if hit is None:
            continue
        a += list(hit)
        x = np.array([v for w in a for v in (w, -w)] + ([0] if n % 2 else []), dtype=np.float64) * 2.0 ** p
        rng.shuffle(x)
        return x
    raise AssertionError("no seam row found")
