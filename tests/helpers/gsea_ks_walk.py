"""The max-deviation GSEA score (gao.ssgsea with single = FALSE), written from its definition for the tests of
replaid.ssgsea.exact(single = FALSE) (host only, no GPU).

For one sample column with N genes: r = average ranks, q = rank(x, ties = "last"), w = r^alpha; the walk visits the genes
at pos = N + 1 - q (1 first).  A set with k members adds w / B at a member (B = the members' w summed) and subtracts
1 / (N - k) at a non-member; the score is the running sum's value of largest magnitude, the first one among equals, / N
with scale.  The running sum falls linearly between two hits, so with the members sorted by pos (t = 1..k)
    cw_t = w_1 + ... + w_t,  miss_t = (pos_t - t) / (N - k)
    after_t = cw_t / B - miss_t,  before_t = cw_{t-1} / B - miss_t  (pos_t >= 2)
hold its extremes; they are visited in position order, the best starts at 0 and is replaced by a strictly larger |.| only.

walk_max_dev() is the literal walk over all N positions, candidates_max_dev() the pinned form of include/plaidhip.h in
numpy fp64, fraction_max_dev() the same operations evaluated in exact rationals and rounded to fp64 once each (what IEEE
arithmetic must give).  k = 0 and k = N give NaN, a column holding a NaN scores NaN for every set, norm divides by
diff(range()) of the whole result (one NaN -> all NaN).
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from tests.helpers.ssgsea_walk import _norm, average_ranks, last_ranks, members


def _ranks(X, alpha):
    """(pos, w) of the NaN-free columns `ok` of X: walk positions (int64) and r^alpha (np.power)"""
    X = np.asarray(X, dtype=np.float64)
    ok = ~np.isnan(X).any(axis=0)
    g = X.shape[0]
    pos = np.zeros(X.shape, dtype=np.int64)
    w = np.ones(X.shape)
    if ok.any():
        pos[:, ok] = g + 1 - last_ranks(X[:, ok]).astype(np.int64)
        w[:, ok] = average_ranks(X[:, ok]) ** alpha
    return pos, w, ok


def walk_max_dev(X, Gp, Gi, alpha, scale=True, norm=False):
    """the literal walk: the running sum at every one of the N positions, then the first argmax(abs())"""
    X = np.asarray(X, dtype=np.float64)
    g, n = X.shape
    m = len(Gp) - 1
    pos, w, ok = _ranks(X, alpha)
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
            hit = np.cumsum(np.where(inset[order], w[order, c], 0.0))
            miss = np.cumsum(np.where(inset[order], 0, 1)).astype(np.float64)
            d = hit / hit[-1] - miss / float(g - k)
            if scale:
                d = d / float(g)
            best = d[np.argmax(np.abs(d))]
            S[j, c] = best if abs(best) > 0.0 else 0.0
    return _norm(S) if norm else S


def candidates(pos_sorted, w_sorted, N, scale):
    """the 2k candidates (before_1, after_1, before_2, ...) of one set for every column: pos_sorted / w_sorted are k x n,
    sorted by position down each column.  An absent before_t (pos_t = 1) is 0, which never replaces the best."""
    k = pos_sorted.shape[0]
    t = np.arange(1, k + 1, dtype=np.int64)[:, None]
    cw = np.cumsum(w_sorted, axis=0)
    cwprev = np.vstack([np.zeros((1, cw.shape[1])), cw[:-1]])
    B = cw[-1]
    miss = (pos_sorted - t).astype(np.float64) / float(N - k)
    after = cw / B - miss
    before = cwprev / B - miss
    before[pos_sorted < 2] = 0.0
    if scale:
        after = after / float(N)
        before = before / float(N)
    cand = np.empty((2 * k, pos_sorted.shape[1]))
    cand[0::2] = before
    cand[1::2] = after
    return cand


def candidates_max_dev(X, Gp, Gi, alpha, scale=True, norm=False, with_extremes=False):
    """the pinned form in numpy fp64 (cw_t by a sequential cumsum); with_extremes: also max(d, 0) and min(d, 0) of the
    candidates of every pair (NaN where the score is)"""
    X = np.asarray(X, dtype=np.float64)
    g, n = X.shape
    m = len(Gp) - 1
    pos, w, ok = _ranks(X, alpha)
    S = np.full((m, n), np.nan)
    dmax = np.full((m, n), np.nan)
    dmin = np.full((m, n), np.nan)
    cols = np.flatnonzero(ok)
    for j in range(m):
        idx = members(Gp, Gi, j)
        k = len(idx)
        if k == 0 or k == g or cols.size == 0:
            continue
        p = pos[np.ix_(idx, cols)]
        order = np.argsort(p, axis=0)
        ps = np.take_along_axis(p, order, axis=0)
        ws = np.take_along_axis(w[np.ix_(idx, cols)], order, axis=0)
        cand = candidates(ps, ws, g, scale)
        first = np.argmax(np.abs(cand), axis=0)            # the first maximum
        best = cand[first, np.arange(cols.size)]
        S[j, cols] = np.where(np.abs(best) > 0.0, best, 0.0)
        dmax[j, cols] = np.maximum(cand.max(axis=0), 0.0)
        dmin[j, cols] = np.minimum(cand.min(axis=0), 0.0)
    if norm:
        S = _norm(S)
    return (S, dmax, dmin) if with_extremes else S


def _fl(x: Fraction) -> Fraction:
    """an exact value rounded to fp64 (float(Fraction) rounds correctly), as a rational again"""
    return Fraction(float(x))


def fraction_max_dev(X, Gp, Gi, alpha, scale=True):
    """the pinned operations with every intermediate computed exactly and rounded once: cw_t / B, miss_t, their
    difference, the division by N.  Exact sums of w (alpha 0 and 1: they are fp64 numbers anyway).  sets x samples."""
    X = np.asarray(X, dtype=np.float64)
    g, n = X.shape
    m = len(Gp) - 1
    pos, w, ok = _ranks(X, alpha)
    S = np.full((m, n), np.nan)
    for c in range(n):
        if not ok[c]:
            continue
        for j in range(m):
            idx = members(Gp, Gi, j)
            k = len(idx)
            if k == 0 or k == g:
                continue
            mem = sorted((int(pos[i, c]), Fraction(float(w[i, c]))) for i in idx)
            B = sum((wi for _, wi in mem), Fraction(0))
            best, cw = Fraction(0), Fraction(0)
            for t, (p, wi) in enumerate(mem, start=1):
                miss = _fl(Fraction(p - t, g - k))
                prev, cw = cw, cw + wi
                for cwv, present in ((prev, p >= 2), (cw, True)):
                    if not present:
                        continue
                    v = _fl(_fl(cwv / B) - miss)
                    if scale:
                        v = _fl(v / g)
                    if abs(v) > abs(best):
                        best = v
            S[j, c] = float(best)
    return S
