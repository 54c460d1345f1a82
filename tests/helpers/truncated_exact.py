"""Host forms of replaid.ucell.exact and replaid.aucell.exact (include/plaidhip.h: plaidhip_ucell_exact,
plaidhip_aucell_exact), the compressed columns of the truncated-rank stage, and the cases the tests share.

Three forms of each statistic: the numpy form with the device's operations (integers, then one fp64 division), the closed
form in exact rationals, and a literal form (sort, walk the tie groups; AUCell's sum(diff(c(x, A)) * seq_along(x)))."""
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

NAN = float("nan")


# ------------------------------------------------------------------------------------------------ ranks of one column
def desc_average_ranks2(x):
    """2 * rank(-x, ties = "average") as integers"""
    x = np.asarray(x, dtype=np.float64) + 0.0
    order = np.argsort(-x, kind="stable")
    xs = x[order]
    d2 = np.empty(len(x), dtype=np.int64)
    i = 0
    while i < len(x):
        j = i
        while j + 1 < len(x) and xs[j + 1] == xs[i]:
            j += 1
        d2[order[i:j + 1]] = (i + 1) + (j + 1)   # twice the mean of the positions i + 1 .. j + 1
        i = j + 1
    return d2


def positions(x):
    """N + 1 - rank(x, ties = "last"): distinct integers, the earlier row of a tie first"""
    x = np.asarray(x, dtype=np.float64) + 0.0
    pos = np.empty(len(x), dtype=np.int64)
    pos[np.argsort(-x, kind="stable")] = np.arange(1, len(x) + 1)
    return pos


def ucell_weights2(x, T, rule="ucell"):
    """2 u per row.  rule "pmin": the negative control, c = pmin(d, T + 1)"""
    d2 = desc_average_ranks2(x)
    if rule == "pmin":
        return 2 * (T + 1) - np.minimum(d2, 2 * (T + 1))
    return np.where(d2 <= 2 * T, 2 * (T + 1) - d2, 0)


def aucell_weights(x, A):
    pos = positions(x)
    return np.where(pos < A, A - pos, 0)


# ------------------------------------------------------------------------------------------------------- numpy forms
def _members(Gp, Gi, j):
    return np.asarray(Gi[Gp[j]:Gp[j + 1]], dtype=np.int64)


def ucell_from_s2(S2, k, K, T):
    """the pinned integer work and its one division"""
    if K == 0:
        return NAN
    U2 = 2 * K * (T + 1) - int(S2) - K * (K + 1)
    auc = np.float64(1.0) - np.float64(U2) / np.float64(2 * K * T)
    return 0.0 if auc < 0.0 else float(auc)


def ucell_exact(X, Gp, Gi, T, k_full=None, rule="ucell"):
    X = np.asarray(X, dtype=np.float64)
    m, n = len(Gp) - 1, X.shape[1]
    S = np.full((m, n), NAN)
    for c in range(n):
        if np.isnan(X[:, c]).any():
            continue
        u2 = ucell_weights2(X[:, c], T, rule)
        for j in range(m):
            mem = _members(Gp, Gi, j)
            K = len(mem) if k_full is None else int(k_full[j])
            S[j, c] = ucell_from_s2(u2[mem].sum(), len(mem), K, T)
    return S


def ucell_total(up, down, w_neg):
    """total = up - w_neg * down: one product, one subtraction; < 0 gives 0; NaN stays"""
    t = up - np.float64(w_neg) * down
    return np.where(t < 0.0, 0.0, t)


def aucell_from_area(area, k, A):
    kk = min(k, A - 1)
    max_auc = kk * A - kk * (kk + 1) // 2
    if max_auc == 0:
        return NAN
    return float(np.float64(int(area)) / np.float64(max_auc))


def aucell_exact(X, Gp, Gi, A):
    X = np.asarray(X, dtype=np.float64)
    m, n = len(Gp) - 1, X.shape[1]
    S = np.full((m, n), NAN)
    for c in range(n):
        if np.isnan(X[:, c]).any():
            continue
        w = aucell_weights(X[:, c], A)
        for j in range(m):
            mem = _members(Gp, Gi, j)
            S[j, c] = aucell_from_area(w[mem].sum(), len(mem), A)
    return S


# ------------------------------------------------------------------------------------------ rationals: closed and literal
def ucell_closed_fraction(x, mem, T, K=None, rule="ucell"):
    k = len(mem)
    K = k if K is None else K
    if K == 0:
        return None
    S2 = int(ucell_weights2(x, T, rule)[mem].sum())
    return max(Fraction(0), 1 - Fraction(2 * K * (T + 1) - S2 - K * (K + 1), 2 * K * T))


def ucell_literal_fraction(x, mem, T, K=None):
    """sort, walk the tie groups, truncate, rank sum, Mann-Whitney U"""
    x = [float(v) + 0.0 for v in x]
    N, k = len(x), len(mem)
    K = k if K is None else K
    if K == 0:
        return None
    order = sorted(range(N), key=lambda i: -x[i])
    d = [None] * N
    i = 0
    while i < N:
        j = i
        while j + 1 < N and x[order[j + 1]] == x[order[i]]:
            j += 1
        for q in range(i, j + 1):
            d[order[q]] = Fraction((i + 1) + (j + 1), 2)
        i = j + 1
    c = [dd if dd <= T else Fraction(T + 1) for dd in d]
    rank_sum = sum(c[i] for i in mem) + (K - k) * (T + 1)
    U = rank_sum - Fraction(K * (K + 1), 2)
    return max(Fraction(0), 1 - U / (K * T))


def aucell_closed_fraction(x, mem, A):
    k = len(mem)
    kk = min(k, A - 1)
    den = kk * A - kk * (kk + 1) // 2
    if den == 0:
        return None
    return Fraction(int(aucell_weights(x, A)[mem].sum()), den)


def _diff_area(xs, A):
    """AUCell's sum(diff(c(x, A)) * seq_along(x))"""
    ext = list(xs) + [A]
    return sum((ext[i + 1] - ext[i]) * (i + 1) for i in range(len(xs)))


def aucell_literal_fraction(x, mem, A):
    pos = positions(x)
    xs = sorted(int(pos[i]) for i in mem if pos[i] < A)
    kk = min(len(mem), A - 1)
    den = _diff_area(range(1, kk + 1), A)
    if den == 0:
        return None
    return Fraction(_diff_area(xs, A), den)


# --------------------------------------------------------------------------------- the compressed columns of the stage
def dense_lists(X, mode, T):
    """per column (rows ascending, weights) of the non-zero weights; a NaN column has none"""
    out = []
    for c in range(X.shape[1]):
        x = X[:, c]
        if np.isnan(x).any():
            out.append((np.zeros(0, np.int64), np.zeros(0)))
            continue
        w = ucell_weights2(x, T) / 2.0 if mode == "ucell" else aucell_weights(x, T).astype(np.float64)
        rows = np.nonzero(w)[0]
        out.append((rows, w[rows]))
    return out


def csc_lists(Xs, mode, T):
    """what plaidhip_dev_truncated_ranks_csc_f64 leaves for the slots of Xs (explicit zeros kept): (lists, u0).  UCell: the
    stored values ranked among themselves, the zeros' group from the counts, weights shifted by u0."""
    g, n = Xs.shape
    lists, u0 = [], np.zeros(n)
    for c in range(n):
        rows = Xs.indices[Xs.indptr[c]:Xs.indptr[c + 1]].astype(np.int64)
        vals = Xs.data[Xs.indptr[c]:Xs.indptr[c + 1]] + 0.0
        if np.isnan(vals).any():
            lists.append((np.zeros(0, np.int64), np.zeros(0)))
            continue
        if mode == "aucell":
            x = np.zeros(g)
            x[rows] = vals
            w = aucell_weights(x, T).astype(np.float64)
            r = np.nonzero(w)[0]
            lists.append((r, w[r]))
            continue
        npos, nneg, ln = int((vals > 0).sum()), int((vals < 0).sum()), len(vals)
        Z = g - npos - nneg
        d0_2 = 2 * npos + Z + 1
        z2 = 2 * (T + 1) - d0_2 if (Z > 0 and d0_2 <= 2 * T) else 0
        u0[c] = z2 / 2.0
        r2 = 2 * (ln + 1) - desc_average_ranks2(vals) if ln else np.zeros(0, np.int64)   # 2 * ascending rank among the stored
        d2 = np.where(vals > 0, 2 * (ln + 1) - r2, 2 * (g + 1) - r2)
        w2 = np.where(vals != 0, np.where(d2 <= 2 * T, 2 * (T + 1) - d2, 0) - z2, 0)
        keep = w2 != 0
        lists.append((rows[keep], w2[keep] / 2.0))
    return lists, u0


# --------------------------------------------------------------------------------------------------------------- cases
def to_csc(X, rng=None, explicit=0.0):
    """the CSC form of X with sorted rows; `explicit`: the share of its zeros that are stored all the same"""
    X = np.asarray(X, dtype=np.float64)
    keep = (X != 0) | np.isnan(X)
    if explicit > 0.0:
        keep |= (rng.random(X.shape) < explicit)
    indptr, indices, data = [0], [], []
    for c in range(X.shape[1]):
        r = np.nonzero(keep[:, c])[0]
        indices.append(r)
        data.append(X[r, c])
        indptr.append(indptr[-1] + len(r))
    M = sp.csc_matrix((X.shape[0], X.shape[1]))
    M.indptr = np.asarray(indptr, dtype=np.int32)
    M.indices = np.concatenate(indices).astype(np.int32) if indices else np.zeros(0, np.int32)
    M.data = np.concatenate(data).astype(np.float64) if data else np.zeros(0)
    return M


def make_sets(N, rng, sizes):
    Gp, Gi = [0], []
    for k in sizes:
        k = min(k, N)
        Gi.extend(sorted(rng.choice(N, size=k, replace=False).tolist()))
        Gp.append(len(Gi))
    return np.asarray(Gp, dtype=np.int32), np.asarray(Gi, dtype=np.int32)


K_SET = 10   # the set size the ranks T = k - 1, k, k + 1 go round


def rank_values(N):
    """T and A: 1, 2, k - 1, k, k + 1, N - 1, N"""
    return sorted({t for t in (1, 2, K_SET - 1, K_SET, K_SET + 1, N - 1, N) if 1 <= t <= N})


def set_sizes(N):
    """0, 1, k, 63, 64, 65, a set larger than most T, and k = N"""
    return [0, 1, K_SET, 63, 64, 65, min(N, 200), N]


def columns(N, seed):
    """the columns of one case matrix, by name"""
    rng = np.random.default_rng(seed)
    T = K_SET
    cols = {}
    cols["normal"] = rng.normal(size=N)
    cols["tied"] = rng.integers(0, 5, size=N).astype(np.float64)
    counts = np.where(rng.random(N) < 0.1, rng.integers(1, 6, size=N), 0).astype(np.float64)
    cols["counts"] = counts
    cols["signed"] = np.where(rng.random(N) < 0.3, rng.integers(-3, 4, size=N), 0).astype(np.float64)
    cols["constant"] = np.full(N, 7.0)
    cols["zero"] = np.zeros(N)
    x = rng.normal(size=N)
    x[N // 2] = np.nan
    cols["nan"] = x
    # boundary tie groups in UCell mode at T = K_SET: `a` larger values, a group of c: average a + (c + 1) / 2
    for name, a, c in (("tie_at_T", T - 2, 3), ("tie_half_above_T", T - 2, 4), ("tie_above_T", T - 1, 5)):
        if a + c <= N:
            x = np.zeros(N)
            idx = rng.permutation(N)
            x[idx[:a]] = 100.0 + np.arange(a)
            x[idx[a:a + c]] = 50.0
            if name == "tie_above_T":
                x[idx[a + c:]] = -rng.random(N - a - c)   # everything else below, distinct
            cols[name] = x
    # stored values: 0 (the zero column), 1, below T, T, above T, all positive
    for name, z in (("nnz_1", 1), ("nnz_below_T", T - 3), ("nnz_T", T), ("nnz_above_T", T + 5)):
        if z <= N:
            x = np.zeros(N)
            x[rng.choice(N, size=z, replace=False)] = 1.0 + rng.integers(0, 3, size=z)
            cols[name] = x
    # AUCell's zero filling: stored rows with implicit rows before, between and after them, across the 64-row boundary
    x = np.zeros(N)
    for r, v in ((3, 5.0), (N - 2, 1.0), (61, 2.0), (63, -1.0), (64, 2.0), (66, 9.0), (130, -4.0)):
        if r < N:
            x[r] = v
    cols["zero_fill"] = x
    return cols


def case(N, seed=0):
    """(names, X dense N x n, Gp, Gi) of the case matrix with N rows"""
    cols = columns(N, 1000 + seed + N)
    names = list(cols)
    X = np.asfortranarray(np.stack([cols[k] for k in names], axis=1))
    Gp, Gi = make_sets(N, np.random.default_rng(77 + N), set_sizes(N))
    return names, X, Gp, Gi


SIZES = (63, 64, 65, 257, 4097)
BIG = 20353   # a column longer than the bucket ranker takes in one pass (20,352 keys)


def assert_same_bits(a, b, what=""):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    same = (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b)) | ((a == 0) & (b == 0))
    if not same.all():
        w = np.argwhere(~same)[:5]
        raise AssertionError(f"{what}: {(~same).sum()} of {same.size} differ, first at {w.tolist()}: "
                             f"{[(a[tuple(i)], b[tuple(i)]) for i in w]}")
