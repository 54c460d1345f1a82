"""GSVA's random-walk statistic (Haenzelmann et al. 2013), written from its definition for the tests of replaid.gsva.exact
(host only, no GPU).

For one sample column of the row-transformed matrix v with N genes: q = rank(v, ties = "last"), the walk visits the genes
at pos = N + 1 - q (1 first; order(v, decreasing = TRUE) with tied genes in row order).  The gene at pos weighs
w = |q - N / 2| ^ tau (0 ^ 0 = 1): a table over the positions, the same for every column and set.  A set with k members
adds w / B at a member (B = the members' w summed) and subtracts 1 / (N - k) at a non-member; mx_pos / mx_neg are the
running sum's largest positive / negative excursion (0 when there is none).  max_diff: mx_pos + mx_neg; otherwise
mx_pos if mx_pos > |mx_neg| else mx_neg.

literal_walk() is GSVA's C loop over all N positions; pinned() the form of include/plaidhip.h in numpy fp64 (the running
sum rises only at a hit, so max(after_t) and min(before_t) hold its extremes); fraction_pinned() the same operations in
exact rationals rounded to fp64 once each.  k = 0, k = N and B == 0 give NaN, a column holding a NaN scores NaN for every
set.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from tests.helpers.ssgsea_walk import last_ranks, members


def weight_table(N, tau):
    """w by position: T[pos - 1] = |q - N / 2| ^ tau with q = N + 1 - pos"""
    if tau == 0:
        return np.ones(N)
    q = np.arange(N, 0, -1, dtype=np.float64)
    return np.power(np.abs(q - N / 2.0), float(tau))


def row_transform(X, rowtf):
    """replaid.gsva's row transforms as the oracle writes them (R/plaid.R:343, 346); "none": X itself"""
    X = np.asarray(X, dtype=np.float64)
    if rowtf == "none":
        return X
    if rowtf == "z":
        with np.errstate(all="ignore"):
            return (X - X.mean(axis=1, keepdims=True)) / (1e-8 + X.std(axis=1, ddof=1, keepdims=True))
    if rowtf == "ecdf":
        return np.stack([np.sum(r[None, :] <= r[:, None], axis=1) / len(r) for r in X])
    raise ValueError("Error: unknown row transform" + str(rowtf))


def positions(V):
    """(pos, ok): walk positions (int64) of the NaN-free columns `ok` of V"""
    V = np.asarray(V, dtype=np.float64)
    ok = ~np.isnan(V).any(axis=0)
    pos = np.zeros(V.shape, dtype=np.int64)
    if ok.any():
        pos[:, ok] = V.shape[0] + 1 - last_ranks(V[:, ok]).astype(np.int64)
    return pos, ok


def combine(mx_pos, mx_neg, max_diff):
    if max_diff:
        return mx_pos + mx_neg
    return np.where(mx_pos > np.abs(mx_neg), mx_pos, mx_neg)


def literal_walk(V, Gp, Gi, tau, max_diff=True):
    """GSVA's loop: cum += w / B at a member, cum -= 1 / (N - k) otherwise, the extremes tracked at each of the N steps"""
    V = np.asarray(V, dtype=np.float64)
    g, n = V.shape
    m = len(Gp) - 1
    pos, ok = positions(V)
    T = weight_table(g, tau)
    S = np.full((m, n), np.nan)
    for c in range(n):
        if not ok[c]:
            continue
        order = np.argsort(pos[:, c])                      # the gene at position 1, 2, ...
        for j in range(m):
            inset = np.zeros(g, dtype=bool)
            inset[members(Gp, Gi, j)] = True
            k = int(inset.sum())
            if k == 0 or k == g:
                continue
            hit = inset[order]
            B = 0.0
            for wv in T[hit]:
                B += wv
            if B == 0.0:
                continue
            dec = 1.0 / float(g - k)
            cum = np.cumsum(np.where(hit, T / B, -dec))    # (a sequential sum: one rounding per step)
            S[j, c] = combine(max(cum.max(), 0.0), min(cum.min(), 0.0), max_diff)
    return S


def pinned(V, Gp, Gi, tau, max_diff=True, with_extremes=False):
    """the pinned form in numpy fp64 (cw_t by a sequential cumsum); with_extremes: also mx_pos and mx_neg"""
    V = np.asarray(V, dtype=np.float64)
    g, n = V.shape
    m = len(Gp) - 1
    pos, ok = positions(V)
    T = weight_table(g, tau)
    S = np.full((m, n), np.nan)
    mxp = np.full((m, n), np.nan)
    mxn = np.full((m, n), np.nan)
    cols = np.flatnonzero(ok)
    for j in range(m):
        idx = members(Gp, Gi, j)
        k = len(idx)
        if k == 0 or k == g or cols.size == 0:
            continue
        ps = np.sort(pos[np.ix_(idx, cols)], axis=0)
        ws = T[ps - 1]
        t = np.arange(1, k + 1, dtype=np.int64)[:, None]
        cw = np.cumsum(ws, axis=0)
        cwprev = np.vstack([np.zeros((1, cols.size)), cw[:-1]])
        B = cw[-1]
        miss = (ps - t).astype(np.float64) / float(g - k)
        with np.errstate(all="ignore"):
            after = cw / B - miss
            before = cwprev / B - miss
        before[ps < 2] = 0.0
        p = np.maximum(after.max(axis=0), 0.0)
        q = np.minimum(before.min(axis=0), 0.0)
        bad = B == 0.0
        p[bad] = np.nan
        q[bad] = np.nan
        mxp[j, cols], mxn[j, cols] = p, q
        S[j, cols] = np.where(bad, np.nan, combine(p, q, max_diff))
    return (S, mxp, mxn) if with_extremes else S


def _fl(x: Fraction) -> Fraction:
    """an exact value rounded to fp64 (float(Fraction) rounds correctly), as a rational again"""
    return Fraction(float(x))


def fraction_pinned(V, Gp, Gi, tau, max_diff=True):
    """the pinned operations with every intermediate computed exactly and rounded once: cw_t / B, miss_t, their
    difference, the final sum.  Exact sums of w (tau 0 and 1: they are fp64 numbers anyway)."""
    V = np.asarray(V, dtype=np.float64)
    g, n = V.shape
    m = len(Gp) - 1
    pos, ok = positions(V)
    T = [Fraction(float(x)) for x in weight_table(g, tau)]
    S = np.full((m, n), np.nan)
    for c in range(n):
        if not ok[c]:
            continue
        for j in range(m):
            idx = members(Gp, Gi, j)
            k = len(idx)
            if k == 0 or k == g:
                continue
            ps = sorted(int(pos[i, c]) for i in idx)
            B = sum((T[p - 1] for p in ps), Fraction(0))
            if B == 0:
                continue
            mxp, mxn, cw = Fraction(0), Fraction(0), Fraction(0)
            for t, p in enumerate(ps, start=1):
                miss = _fl(Fraction(p - t, g - k))
                prev, cw = cw, cw + T[p - 1]
                if p >= 2:
                    mxn = min(mxn, _fl(_fl(prev / B) - miss))
                mxp = max(mxp, _fl(_fl(cw / B) - miss))
            if max_diff:
                S[j, c] = float(_fl(mxp + mxn))
            else:
                S[j, c] = float(mxp if mxp > abs(mxn) else mxn)
    return S
