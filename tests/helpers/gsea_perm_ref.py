"""Host restatements of plaid.gsea as include/plaidhip.h pins it (plaidhip_gsea).

Three forms of the enrichment score of one set under one placement -- a vectorised numpy form (the reference of the GPU
tests), the literal walk over all N positions, and the same operations in fractions.Fraction -- the null statistics in
the pinned summation order, Philox4x32-10, the placement rule, and Benjamini-Hochberg."""
from fractions import Fraction

import numpy as np

BLOCK = 64           # PLAIDHIP_GSEA_PERM_BLOCK
COLUMNS = ("ES", "NES", "pval", "padj", "nMoreExtreme", "size", "nGeEs", "nLeEs", "nGeZero", "nLeZero", "sumPos", "sumNeg")
M32 = 0xFFFFFFFF


# ---- Philox4x32-10 and the placements -----------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """the four output words for a counter (4 words) and a key (2 words), in Python integers"""
    c0, c1, c2, c3 = (int(x) & M32 for x in counter)
    k0, k1 = (int(x) & M32 for x in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def _philox_o0_o1(i, b, seed):
    """words o0, o1 for the counters (i, b, 0, 0), i a uint64 array (values < 2^32), vectorised"""
    c0 = i.astype(np.uint64)
    c1 = np.full_like(c0, np.uint64(b))
    c2 = np.zeros_like(c0)
    c3 = np.zeros_like(c0)
    k0, k1 = int(seed) & M32, (int(seed) >> 32) & M32
    m = np.uint64(M32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2     # (32 x 32 bits: no overflow of 64)
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1


def placement_keys(g, b, seed):
    """y of every gene for permutation b: r 2^17 + i, r = (o0 << 4) | (o1 >> 28)"""
    i = np.arange(g, dtype=np.uint64)
    o0, o1 = _philox_o0_o1(i, b, seed)
    r = (o0 << np.uint64(4)) | (o1 >> np.uint64(28))
    y = (r << np.uint64(17)) + i
    yd = y.astype(np.float64)
    assert np.array_equal(yd.astype(np.uint64), y)       # exact: below 2^53
    return yd


def placements(g, B, seed, b0=0):
    """P (g x B int32, Fortran order): column b = (ascending min rank of y) - 1"""
    P = np.empty((g, B), dtype=np.int32, order="F")
    for b in range(B):
        y = placement_keys(g, b0 + b, seed)
        o = np.argsort(y, kind="stable")
        assert np.all(np.diff(y[o]) > 0)                 # free of ties
        P[o, b] = np.arange(g, dtype=np.int32)
    return P


def observed_placement(stat):
    """pos_obs: gene i's place in order(-stat), stable"""
    o = np.argsort(-np.asarray(stat, dtype=np.float64), kind="stable")
    pos = np.empty(len(o), dtype=np.int32)
    pos[o] = np.arange(len(o), dtype=np.int32)
    return pos


def walk_weights(pos, weight):
    Wpos = np.empty(len(pos), dtype=np.float64)
    Wpos[pos] = weight
    return Wpos


# ---- the enrichment score, three ways ---------------------------------------------------------------------------------------------
def _choose(maxP, minP, zero=0.0):
    return maxP if maxP > -minP else (minP if maxP < -minP else zero)


def es_numpy(pos, members, Wpos):
    """vectorised: cumsum is sequential, every other operation is element-wise IEEE"""
    N, k = len(pos), len(members)
    if k == 0 or k == N:
        return np.nan
    p = np.sort(pos[members].astype(np.int64)) + 1
    cw = np.cumsum(Wpos[p - 1])
    B = cw[-1]
    if B == 0.0:
        cw = np.arange(1, k + 1, dtype=np.float64)
        B = float(k)
    t = np.arange(1, k + 1, dtype=np.int64)
    miss = (p - t).astype(np.float64) / float(N - k)
    after = cw / B - miss
    before = np.concatenate([[0.0], cw[:-1]]) / B - miss
    return float(_choose(after.max(), before.min()))


def es_literal(pos, members, Wpos):
    """the walk over all N positions, one at a time"""
    N, k = len(pos), len(members)
    if k == 0 or k == N:
        return float("nan")
    hit = np.zeros(N, dtype=bool)
    hit[pos[members]] = True
    B = 0.0
    for q in range(N):
        if hit[q]:
            B = B + float(Wpos[q])
    unweighted = B == 0.0
    if unweighted:
        B = float(k)
    t, cw, maxP, minP = 0, 0.0, -np.inf, np.inf
    for q in range(N):
        if not hit[q]:
            continue
        p = q + 1
        prev = cw
        t += 1
        cw = float(t) if unweighted else cw + float(Wpos[q])
        miss = float(p - t) / float(N - k)
        after, before = cw / B - miss, prev / B - miss
        maxP, minP = max(maxP, after), min(minP, before)
    return float(_choose(maxP, minP))


def es_fraction(pos, members, Wpos, parts=False):
    """the same operations in rationals: a Fraction (None for k = 0 or k = N); parts: (maxP, minP) instead.  Where the two
    are equal in magnitude the rational score is 0 while a rounding may decide the fp64 forms either way.
    Every candidate cw / B - (p - t) / (N - k) is written over the one denominator B (N - k), so the extremes are found
    among integer numerators and reduced once."""
    N, k = len(pos), len(members)
    if k == 0 or k == N:
        return None
    p = [int(x) + 1 for x in np.sort(pos[members].astype(np.int64))]
    w = [Fraction(float(x)) for x in Wpos[np.asarray(p) - 1]]
    scale = max(f.denominator for f in w)                       # a power of two: every weight is an integer over it
    wi = [f.numerator * (scale // f.denominator) for f in w]
    B = sum(wi)
    if B == 0:
        wi, B = [1] * k, k
    D = N - k
    cw, mx, mn = 0, None, None
    for t in range(1, k + 1):
        miss = (p[t - 1] - t) * B
        before = cw * D - miss
        cw += wi[t - 1]
        after = cw * D - miss
        mx = after if mx is None or after > mx else mx
        mn = before if mn is None or before < mn else mn
    maxP, minP = Fraction(mx, B * D), Fraction(mn, B * D)
    return (maxP, minP) if parts else _choose(maxP, minP, Fraction(0))


# ---- the null statistics ---------------------------------------------------------------------------------------------------------
def null_stats(es, null):
    """the 12 columns (padj NaN, size left to the caller) of one (set, list) pair from its ES and its B null scores; the two
    sums in blocks of 64, sequential inside a block and over the blocks, from 0.0"""
    out = np.full(12, np.nan)
    if es != es:
        return out
    nb = np.asarray(null, dtype=np.float64)
    n_ge, n_le = float(np.sum(nb >= es)), float(np.sum(nb <= es))
    n_ge0, n_le0 = float(np.sum(nb >= 0.0)), float(np.sum(nb <= 0.0))
    sum_pos = sum_neg = 0.0
    for b0 in range(0, len(nb), BLOCK):
        sp = sn = 0.0
        for e in nb[b0:b0 + BLOCK]:
            sp = sp + (float(e) if e > 0.0 else 0.0)
            sn = sn + (float(e) if e < 0.0 else 0.0)
        sum_pos, sum_neg = sum_pos + sp, sum_neg + sn
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.float64
        nes = d(es) / (d(sum_pos) / d(n_ge0)) if es > 0.0 else d(es) / np.abs(d(sum_neg) / d(n_le0))
        pval = min((1.0 + n_le) / (1.0 + n_le0), (1.0 + n_ge) / (1.0 + n_ge0))
    out[[0, 1, 2, 4]] = es, nes, pval, n_ge if es > 0.0 else n_le
    out[6:] = n_ge, n_le, n_ge0, n_le0, sum_pos, sum_neg
    return out


def bh(p):
    """Benjamini-Hochberg (p.adjust(p, "BH")) over the non-NaN entries; NaN stays NaN"""
    p = np.asarray(p, dtype=np.float64)
    q = np.full(p.shape, np.nan)
    ok = np.flatnonzero(~np.isnan(p))
    if len(ok) == 0:
        return q
    n = len(ok)
    o = ok[np.argsort(-p[ok], kind="stable")]                 # decreasing p
    adj = p[o] * float(n) / np.arange(n, 0, -1, dtype=np.float64)   # (p n) / rank, as the library's host routine
    q[o] = np.minimum(1.0, np.minimum.accumulate(adj))
    return q


def gsea_ref(stat, weight, Gp, Gi, P, es=es_numpy):
    """(out m x 12 x c, null m x B x c) of plaidhip_gsea for placements P (g x B), by the form `es`"""
    stat = np.asarray(stat, dtype=np.float64).reshape(len(stat), -1)
    weight = np.asarray(weight, dtype=np.float64).reshape(stat.shape)
    g, c = stat.shape
    m, B = len(Gp) - 1, P.shape[1]
    out = np.full((m, 12, c), np.nan, order="F")
    null = np.full((m, B, c), np.nan, order="F")
    for j in range(m):
        out[j, 5, :] = Gp[j + 1] - Gp[j]
    for l in range(c):
        if not np.all(np.isfinite(stat[:, l])):
            continue
        pos = observed_placement(stat[:, l])
        Wpos = walk_weights(pos, weight[:, l])
        for j in range(m):
            mem = np.asarray(Gi[Gp[j]:Gp[j + 1]], dtype=np.int64)
            e = es(pos, mem, Wpos)
            if e != e:
                continue
            for b in range(B):
                null[j, b, l] = es(P[:, b], mem, Wpos)
            size = out[j, 5, l]
            out[j, :, l] = null_stats(e, null[j, :, l])
            out[j, 5, l] = size
        out[:, 3, l] = bh(out[:, 2, l])
    return out, null


def make_sets(N, sizes, seed):
    """one set of every size in `sizes` (those that fit 0..N), members drawn without replacement, as a CSC pattern"""
    rng = np.random.default_rng(seed)
    Gp, Gi = [0], []
    for k in sizes:
        if k < 0 or k > N:
            continue
        Gi.extend(np.sort(rng.choice(N, size=k, replace=False)).tolist())
        Gp.append(len(Gi))
    return np.asarray(Gp, dtype=np.int32), np.asarray(Gi, dtype=np.int32)
