"""Host restatements of plaid.fisher (include/plaidhip.h: plaidhip_fisher).

tail_exact is the definition in exact rational arithmetic; tail_form is the pinned form, operation for operation, in
Python floats (IEEE fp64, no contraction); fisher_ref is the whole entry in numpy integers and tail_form."""
from fractions import Fraction
from math import comb

import numpy as np

from .gsea_perm_ref import bh, make_sets  # noqa: F401  (make_sets: re-exported for the tests)

COLUMNS = ("size", "ovUp", "ovDn", "pUp", "pDn", "pAny", "padjUp", "padjDn", "padjAny", "orUp", "orDn", "orAny")
P_FLOOR = Fraction(1, 2**900)      # below this exact p the pinned form promises only [0, 2^-890]
P_SMALL = 2.0**-890


def bounds(N, K, k):
    return max(0, k + K - N), min(k, K)


def tail_exact(N, K, k, x):
    """P(X >= x), X ~ Hypergeometric(N, K, k), as a Fraction.  The terms are integers w_t = C(K, t) C(N - K, k - t), formed
    by an integer recurrence from t = lo (each step's division is exact)."""
    lo, hi = bounds(N, K, k)
    if x <= lo:
        return Fraction(1)
    if x > hi:
        return Fraction(0)
    w = comb(K, lo) * comb(N - K, k - lo)
    total, upper = 0, 0
    for t in range(lo, hi + 1):
        total += w
        if t >= x:
            upper += w
        if t < hi:
            num = w * (K - t) * (k - t)
            den = (t + 1) * (N - K - k + t + 1)
            assert num % den == 0
            w = num // den
    assert total == comb(N, k)
    return Fraction(upper, total)


def tail_form(N, K, k, x):
    """the pinned form of include/plaidhip.h, operation for operation"""
    lo, hi = bounds(N, K, k)
    if x <= lo:
        return 1.0
    if x > hi:
        return 0.0
    t0 = min(max(((k + 1) * (K + 1)) // (N + 2), lo), hi)
    u, total, upper = 1.0, 1.0, (1.0 if t0 >= x else 0.0)
    for t in range(t0, hi):
        u = (u * (float(K - t) * float(k - t))) / (float(t + 1) * float(N - K - k + t + 1))
        total += u
        if t + 1 >= x:
            upper += u
    u = 1.0
    for t in range(t0, lo, -1):
        u = (u * (float(t) * float(N - K - k + t))) / (float(K - t + 1) * float(k - t + 1))
        total += u
        if t - 1 >= x:
            upper += u
    return upper / total


def tail_bound(N, K, k):
    """the relative bound of tail_form against tail_exact wherever the exact p >= 2^-900: (4 n + 2) 2^-53, n = hi - lo + 1"""
    lo, hi = bounds(N, K, k)
    return Fraction(4 * (hi - lo + 1) + 2, 2**53)


def odds(N, K, k, x):
    """((double)a (double)d) / ((double)b (double)c') with IEEE division"""
    num, den = float(x) * float(N - k - K + x), float(k - x) * float(K - x)
    if den == 0.0:
        return float("nan") if num == 0.0 else float("inf")
    return num / den


def fisher_ref(sig, Gp, Gi, tail=tail_form):
    """(out m x 12 x c, tot 2 x c, ov_len m x c int32, ov_idx Gp[m] x c int32) of plaidhip_fisher"""
    sig = np.asarray(sig).reshape(len(sig), -1).astype(np.int64)
    N, c = sig.shape
    m, nnz = len(Gp) - 1, int(Gp[-1])
    out = np.full((m, 12, c), np.nan, order="F")
    tot = np.zeros((2, c), order="F")
    ov_len = np.zeros((m, c), dtype=np.int32, order="F")
    ov_idx = np.full((nnz, c), -1, dtype=np.int32, order="F")
    for l in range(c):
        s = sig[:, l]
        nU, nD = int(np.sum(s == 1)), int(np.sum(s == -1))
        tot[:, l] = nU, nD
        for j in range(m):
            mem = np.asarray(Gi[Gp[j]:Gp[j + 1]], dtype=np.int64)
            k = len(mem)
            oU, oD = int(np.sum(s[mem] == 1)), int(np.sum(s[mem] == -1))
            out[j, 0:3, l] = k, oU, oD
            hit = mem[s[mem] != 0]
            ov_len[j, l] = len(hit)
            ov_idx[Gp[j]:Gp[j] + len(hit), l] = hit
            if k == 0 or k == N:
                continue
            for d, (K, x) in enumerate(((nU, oU), (nD, oD), (nU + nD, oU + oD))):
                out[j, 3 + d, l] = tail(N, K, k, x)
                out[j, 9 + d, l] = odds(N, K, k, x)
        for d in range(3):
            out[:, 6 + d, l] = bh(out[:, 3 + d, l])
    return out, tot, ov_len, ov_idx


FIXED_TABLES = [(64, 10, 5, 3), (20000, 1500, 140, 30), (20000, 1500, 500, 80), (131072, 6000, 2000, 200),
                (4097, 4000, 4000, 3950), (4097, 100, 4096, 100), (20000, 10000, 10000, 5600), (1000, 500, 500, 330)]


def random_tables(count=300, seed=7, nmax=5000):
    """`count` seeded tables (N, K, k, x) with N < nmax and lo <= x <= hi + 1: x is uniform over that range in every second
    table (mostly far tails) and a draw of the distribution itself, moved by -2 .. 5, in the others (the bulk)"""
    rng = np.random.default_rng(seed)
    tabs = []
    for q in range(count):
        N = int(rng.integers(1, nmax))
        K, k = int(rng.integers(0, N + 1)), int(rng.integers(0, N + 1))
        lo, hi = bounds(N, K, k)
        if q % 2 == 0 or k == 0:
            x = int(rng.integers(lo, hi + 2))
        else:
            x = int(rng.hypergeometric(K, N - K, k)) + int(rng.integers(-2, 6))
        tabs.append((N, K, k, min(max(x, lo), hi + 1)))
    return tabs
