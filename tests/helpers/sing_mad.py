"""replaid.sing.exact on the host (include/plaidhip.h: plaidhip_sing_exact): singscore's normalised score and the MAD of a
set's ranks, per set and sample column.  Three forms of the same statistic:

    pinned    the operations of the header in numpy: integer sums and medians, two divisions, one product
    literal   scipy.stats.rankdata(method = "min"), np.mean-free sums, np.median and the constant 1.4826, as an R user
              would write singscore's simpleScore
    rational  the same operations in exact rationals, every fp64 operation rounded once (float(Fraction) rounds correctly)

and the two ways the device finds the j-th smallest deviation without a sort (kernels_sing.hip): the window identity and
the crossing search over the windows.  X: g x n; Gp / Gi (and Dp / Di): the aligned 0-based pattern.  A column holding a
NaN gives NaN everywhere.  Results: dict of m x n matrices named as plaid_amd.engine.SING_EXACT_OUTPUTS.
"""
from fractions import Fraction

import numpy as np

MAD_CONSTANT = 1.4826   # R's literal in mad()
NAMES = ("TotalScore", "UpScore", "DownScore", "TotalDispersion", "UpDispersion", "DownDispersion")


def min_ranks(x):
    """rank(x, ties = "min") as int64, 1..N (-0.0 ties with 0.0)"""
    x = np.asarray(x, dtype=np.float64)
    return np.searchsorted(np.sort(x), x, side="left").astype(np.int64) + 1


def _members(Gp, Gi, j, N):
    rows = np.asarray(Gi[Gp[j]:Gp[j + 1]], dtype=np.int64)
    return rows[(rows >= 0) & (rows < N)]


# ------------------------------------------------------------------------------------------------------------- pinned
def score_pinned(total, k, N, center):
    """total: the exact integer sum of the k ranks"""
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.float64(total) / np.float64(k)
        low = np.float64(k + 1) / np.float64(2.0)
        s = (mean - low) / np.float64(N - k)
        if k == N:                                        # high == low; with ties the quotient would be -Inf: NaN by rule
            s = np.float64(np.nan)
        return s - np.float64(0.5) if center else s


def mad4(s):
    """4 * median |s - median(s)| of the integer ranks s, in integers"""
    s = np.sort(np.asarray(s, dtype=np.int64))
    k = len(s)
    M2 = 2 * s[k // 2] if k % 2 else s[k // 2 - 1] + s[k // 2]
    d2 = np.sort(np.abs(2 * s - M2))                      # 2 |s - med|
    return int(2 * d2[k // 2] if k % 2 else d2[k // 2 - 1] + d2[k // 2])


def disp_pinned(s):
    if len(s) == 0:
        return np.float64(np.nan)
    return np.float64(MAD_CONSTANT) * (np.float64(mad4(s)) * np.float64(0.25))


def _run(X, Gp, Gi, Dp, Di, center, score_fn, disp_fn, rank_fn):
    X = np.asarray(X, dtype=np.float64)
    N, n = X.shape
    m = len(Gp) - 1
    down = Dp is not None
    out = {name: np.full((m, n), np.nan) for name in NAMES}
    for c in range(n):
        x = X[:, c]
        if np.isnan(x).any():
            continue
        r = rank_fn(x)
        for j in range(m):
            su = r[_members(Gp, Gi, j, N)]
            out["UpScore"][j, c] = score_fn(su, N, center)
            out["UpDispersion"][j, c] = disp_fn(su)
            if down:
                sd = (N + 1) - r[_members(Dp, Di, j, N)]
                out["DownScore"][j, c] = score_fn(sd, N, center)
                out["DownDispersion"][j, c] = disp_fn(sd)
    if down:
        out["TotalScore"] = out["UpScore"] + out["DownScore"]
        out["TotalDispersion"] = out["UpDispersion"] + out["DownDispersion"]
    else:
        for name in ("TotalScore", "DownScore", "TotalDispersion", "DownDispersion"):
            del out[name]
    return out


def pinned(X, Gp, Gi, Dp=None, Di=None, center=True):
    return _run(X, Gp, Gi, Dp, Di, center, lambda s, N, ce: score_pinned(int(s.sum()), len(s), N, ce), disp_pinned, min_ranks)


# ------------------------------------------------------------------------------------------------------------ literal
def literal(X, Gp, Gi, Dp=None, Di=None, center=True):
    from scipy.stats import rankdata

    def score(s, N, ce):
        k = len(s)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.float64(np.sum(s.astype(np.float64))) / np.float64(k)
            low, high = (k + 1) / 2.0, (2 * N - k + 1) / 2.0
            v = (mean - low) / np.float64(high - low)
            if high == low:                                   # k = N: not defined (-Inf in a tied column): NaN by rule
                v = np.nan
            return v - 0.5 if ce else v

    def disp(s):
        if len(s) == 0:
            return np.nan
        s = s.astype(np.float64)
        return 1.4826 * np.median(np.abs(s - np.median(s)))

    return _run(X, Gp, Gi, Dp, Di, center, score, disp, lambda x: rankdata(x, method="min").astype(np.int64))


# ----------------------------------------------------------------------------------------------------------- rational
def _rn(q):
    return float(q)   # a Fraction rounds to nearest even


def rational(X, Gp, Gi, Dp=None, Di=None, center=True):
    def ranks(x):
        xs = [float(v) for v in x]
        return np.array([1 + sum(1 for u in xs if u < v) for v in xs], dtype=np.int64)

    def score(s, N, ce):
        k = len(s)
        if k == 0 or k == N:
            return np.nan
        mean = _rn(Fraction(int(s.sum()), k))
        num = _rn(Fraction(mean) - Fraction(k + 1, 2))
        v = _rn(Fraction(num) / (N - k))
        return _rn(Fraction(v) - Fraction(1, 2)) if ce else v

    def disp(s):
        k = len(s)
        if k == 0:
            return np.nan
        t = sorted(int(v) for v in s)
        med = Fraction(t[k // 2]) if k % 2 else Fraction(t[k // 2 - 1] + t[k // 2], 2)
        d = sorted(abs(Fraction(v) - med) for v in t)
        md = d[k // 2] if k % 2 else (d[k // 2 - 1] + d[k // 2]) / 2
        return _rn(Fraction(MAD_CONSTANT) * md)

    return _run(X, Gp, Gi, Dp, Di, center, score, disp, ranks)


# --------------------------------------------------------------------------------- the j-th smallest deviation, no sort
def kth_dev2_windows(s, M2, j):
    """2 * the j-th smallest |s_t - M2 / 2| of the SORTED integers s: min over the windows of j consecutive members of the
    larger deviation of the window's two ends"""
    s = np.asarray(s, dtype=np.int64)
    k = len(s)
    lo, hi = s[:k - j + 1], s[j - 1:]
    return int(np.min(np.maximum(np.abs(2 * lo - M2), np.abs(2 * hi - M2))))


def kth_dev2_crossing(s, M2, j, lo=0, hi=None):
    """the same by the device's search: the first window l in [lo, hi] with s_l + s_{l+j-1} >= M2 (hi: none before it),
    then the smaller of that window's upper deviation and its predecessor's lower one.  Returns (value, l)."""
    k = len(s)
    W = k - j + 1
    hi = W if hi is None else hi
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if int(s[mid]) + int(s[mid + j - 1]) >= M2:
            hi = mid
        else:
            lo = mid + 1
    best = None
    if lo < W:
        best = 2 * int(s[lo + j - 1]) - M2
    if lo > 0:
        a = M2 - 2 * int(s[lo - 1])
        best = a if best is None or a < best else best
    return best, lo


def mad4_device(s):
    """4 * median |s - median(s)| as sing_mad_kernel computes it from the sorted ranks"""
    s = np.sort(np.asarray(s, dtype=np.int64))
    k = len(s)
    if k % 2:
        M2 = 2 * int(s[k // 2])
        return 2 * kth_dev2_crossing(s, M2, (k + 1) // 2)[0]
    M2 = int(s[k // 2 - 1]) + int(s[k // 2])
    j1, j2 = k // 2, k // 2 + 1
    d1, l1 = kth_dev2_crossing(s, M2, j1)
    W2 = k - j2 + 1
    d2, _ = kth_dev2_crossing(s, M2, j2, max(l1 - 1, 0), min(l1, W2))
    return d1 + d2
