"""The original single-sample GSEA statistic (gao.ssgsea with single = TRUE), written from its definition for the tests of
replaid.ssgsea.exact (host only, no GPU).

For one sample column with N genes: r = average ranks, the walk visits the genes in order(r, decreasing = TRUE) with tied
genes in row order (a stable order); a set S with k members present adds w_j / sum_S(w) at a member (w = r^alpha) and
subtracts 1 / (N - k) at a non-member; ES is the SUM of the running sum over the N steps, / N with scale.  Summed in closed
form with q = N - pos + 1 = rank(x, ties = "last"):
    ES = A / B - (T - C) / (N - k),   A = sum_S w q,  B = sum_S w,  C = sum_S q,  T = N (N + 1) / 2
walk_scores() is the literal running sum, closed_form() the pinned fp64 epilogue of include/plaidhip.h, fraction_scores()
the closed form in exact rational arithmetic.  norm divides by diff(range(es)) over the whole result (one NaN -> all NaN).
A column holding a NaN scores NaN for every set (the project's documented choice).
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np
from scipy.stats import rankdata


def last_ranks(X):
    """rank(x, ties.method = "last") per column: among equal values the later row gets the smaller rank (NaN-free X)"""
    X = np.asarray(X, dtype=np.float64)
    g = X.shape[0]
    rows = np.broadcast_to(-np.arange(g)[:, None], X.shape)
    order = np.lexsort((rows, X + 0.0), axis=0)          # ascending value, later rows first inside a tie
    Q = np.empty(X.shape, dtype=np.float64)
    np.put_along_axis(Q, order, np.arange(1, g + 1, dtype=np.float64)[:, None].repeat(X.shape[1], 1), axis=0)
    return Q


def average_ranks(X):
    return rankdata(np.asarray(X, dtype=np.float64) + 0.0, method="average", axis=0)


def members(Gp, Gi, j):
    return np.asarray(Gi[Gp[j]:Gp[j + 1]], dtype=np.int64)


def walk_scores(X, Gp, Gi, alpha, scale=True, norm=False):
    """the literal walk: sets x samples"""
    X = np.asarray(X, dtype=np.float64)
    g, n = X.shape
    m = len(Gp) - 1
    S = np.empty((m, n))
    for c in range(n):
        x = X[:, c]
        if np.isnan(x).any():
            S[:, c] = np.nan
            continue
        r = average_ranks(x[:, None])[:, 0]
        w = r ** alpha
        order = np.argsort(-r, kind="stable")
        for j in range(m):
            inset = np.zeros(g, dtype=bool)
            inset[members(Gp, Gi, j)] = True
            k = int(inset.sum())
            with np.errstate(all="ignore"):
                hit = np.where(inset[order], w[order], 0.0) / w[inset].sum()
                miss = np.where(inset[order], 0.0, 1.0) / (g - k)
                es = np.sum(np.cumsum(hit) - np.cumsum(miss))
            S[j, c] = es / g if scale else es
    return _norm(S) if norm else S


def _norm(S):
    with np.errstate(all="ignore"):
        if np.isnan(S).any():
            return S / np.nan
        return S / (S.max() - S.min())


def operands(X, alpha):
    """(Q, W): last ranks and average ranks ^ alpha in fp64 (np.power), NaN where X is NaN"""
    X = np.asarray(X, dtype=np.float64)
    Q = np.full(X.shape, np.nan)
    W = np.full(X.shape, np.nan)
    ok = ~np.isnan(X).any(axis=0)
    if ok.any():
        Q[:, ok] = last_ranks(X[:, ok])
        W[:, ok] = average_ranks(X[:, ok]) ** alpha
    return Q, W


def set_sums_exact(Gp, Gi, V):
    """sum over each set's members of V's rows, for V whose set sums are exact in fp64 (integers, half-integers)"""
    m = len(Gp) - 1
    out = np.empty((m, V.shape[1]))
    for j in range(m):
        out[j] = V[members(Gp, Gi, j)].sum(axis=0)
    return out


def pinned_epilogue(A, B, C, k, N, colnan, scale=True, norm=False):
    """the epilogue of include/plaidhip.h, operation for operation in fp64"""
    k = np.asarray(k, dtype=np.int64)[:, None]
    T = float(N * (N + 1) // 2)
    with np.errstate(all="ignore"):
        d1 = A / B
        d2 = (T - C) / (N - k).astype(np.float64)
        es = d1 - d2
        if scale:
            es = es / float(N)
    es[:, np.asarray(colnan, dtype=bool)] = np.nan
    return _norm(es) if norm else es


def closed_form(X, Gp, Gi, alpha, scale=True, norm=False):
    """the closed form in fp64 with exact set sums of the operands (exact at alpha = 0 and 1)"""
    X = np.asarray(X, dtype=np.float64)
    g = X.shape[0]
    Q, W = operands(X, alpha)
    colnan = np.isnan(X).any(axis=0)
    Qz, Wz = np.nan_to_num(Q), np.nan_to_num(W)
    C = set_sums_exact(Gp, Gi, Qz)
    if alpha == 0:
        A, B = C, np.diff(Gp).astype(np.float64)[:, None] * np.ones_like(C)
    else:
        A, B = set_sums_exact(Gp, Gi, Wz * Qz), set_sums_exact(Gp, Gi, Wz)
    return pinned_epilogue(A, B, C, np.diff(Gp), g, colnan, scale, norm)


def fraction_scores(X, Gp, Gi, alpha, scale=True):
    """the closed form in rationals (w rounded to fp64 once, as the device has it); None for 0 / 0"""
    X = np.asarray(X, dtype=np.float64)
    g, n = X.shape
    m = len(Gp) - 1
    Q, W = operands(X, alpha)
    T = Fraction(g * (g + 1), 2)
    out = [[None] * n for _ in range(m)]
    for c in range(n):
        for j in range(m):
            idx = members(Gp, Gi, j)
            k = len(idx)
            if k == 0 or k == g:
                continue
            A = sum((Fraction(float(W[i, c])) * Fraction(float(Q[i, c])) for i in idx), Fraction(0))
            B = sum((Fraction(float(W[i, c])) for i in idx), Fraction(0))
            C = sum((Fraction(float(Q[i, c])) for i in idx), Fraction(0))
            es = A / B - (T - C) / (g - k)
            out[j][c] = es / g if scale else es
    return out
