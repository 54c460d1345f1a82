"""Exact restatements of replaid.gsva, replaid.aucell and replaid.scse, and the bounds that hold a device to them
(host only, no GPU).

The three scorers are rank sums or plain sums followed by a short epilogue.  Every reference below evaluates the
statistic in np.longdouble (x87 extended, eps = 2^-63, asserted) on exact set sums (exact_ref.set_sums on the fp64 head
and tail of every long-double term), rounds once to fp64, and returns an ELEMENTWISE bound on |device - reference| built
like exact_ref's (k + c) 2^-53 mag: k terms summed in any order, c the roundings that follow, counted from the device's
own expressions.  u = 2^-53 throughout.

replaid.gsva adds one thing the other routes do not have: a real-valued row transform IN FRONT of the ranks.  A rank
is a step function of z, so no error bound on z carries over to the score -- unless the ranks cannot change.  z_delta()
bounds the device's error on every z, separated() states when that error cannot reorder two |z| of a column or flip a
sign, and under that precondition (asserted for every input of the GPU tests, never skipped) the z stage adds NOTHING to
the score's bound: the device's signed ranks are the reference's, exactly.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.stats as st

from tests.helpers import exact_ref as er
from tests.helpers.pow_ref import pow_allowance_u

ld = np.longdouble
assert np.finfo(ld).eps == 2.0 ** -63, "the references need x87 extended precision (long double with a 64-bit significand)"
U = er.U
# (one device weight r^p, p != 1: pow_ref.pow_allowance_u(p) u -- counted from pow_quarters' code or pow()'s 3 u, and held
# on the device over every rank by tests/test_gpu_rank_weights.py)
EXP2_ULPS = 3.0         # the allowance for one device 2^x (map_kernel ops 2, 3): 3 u


# ------------------------------------------------------------------ shared with test_gpu_exact_sums.py
def _w(Gp):
    """the mean statistic's set weight, the device's fp64 value: fl(1 / (1e-8 + k))"""
    return 1.0 / (1e-8 + np.diff(Gp).astype(np.float64))


def _long_sums(Gp, Gi, W):
    """exact set sums of long-double terms: the fp64 head and tail of each term summed apart"""
    hi = W.astype(np.float64)
    lo = (W - hi.astype(np.longdouble)).astype(np.float64)
    s_hi, mag, k = er.set_sums(Gp, Gi, hi)
    s_lo, _, _ = er.set_sums(Gp, Gi, lo)
    return s_hi.astype(np.longdouble) + s_lo.astype(np.longdouble), mag, k


def _normalized_ref(T, E, ignore_zero=False):
    """normalize_medians(T) in long double, and a bound on |device - reference| for a device whose raw scores S lie
    within E of T elementwise.  A column median is 1-Lipschitz in the max norm, so |med(S) - med(T)| <= max_col E; the
    midpoints round once on either side (2 u |med|); mean(med) adds its own sum and division roundings
    ((n + 2) u mean|med|); then fl(fl(S - med) + add) rounds twice and the reference once.

    `ignore_zero` is normalize_medians' ignore.zero, already resolved: TRUE drops the exact zeros of a column before its
    median (0 for a column with nothing left).  The Lipschitz argument then runs over the nonzero scores, so it needs the
    device's zero pattern to be T's -- which holds where a zero score is a sum of exact zero weights (replaid.aucell)"""
    u = er.U
    n = T.shape[1]
    med = er.col_medians(T, ignore_zero)
    Mc = E.max(axis=0) + 2.0 * u * np.abs(med)
    add = np.mean(med.astype(ld))
    N = ((T.astype(ld) - med.astype(ld)[None, :]) + add).astype(np.float64)
    A = Mc.mean() + (n + 2) * u * np.abs(med).mean()
    B = E + Mc[None, :] + A + u * (np.abs(T) + np.abs(med)[None, :]) + 2.0 * u * np.abs(N) + u * abs(float(add))
    return N, B


def ratio(got, ref, bound):
    """the largest |got - ref| / bound over the finite elements (0 / 0 counts as 0)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), got.shape)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(np.nanmax(r)) if r.size else 0.0


def _pattern_matrix(Gp, Gi, g):
    return sp.csc_matrix((np.ones(len(Gi)), np.asarray(Gi), np.asarray(Gp)), shape=(g, len(Gp) - 1))


# ------------------------------------------------------------------ the z row transform
def z_exact(X):
    """z = (x - rowMeans(X)) / (1e-8 + rowSds(X)) (R/plaid.R:343), sd with n - 1, in long double; mean = sum / n.
    Identical rows give identical z; a constant row whose sum is exact in long double (1.25 n is) gives exactly 0."""
    X = np.asarray(X, dtype=np.float64).astype(ld)
    n = X.shape[1]
    mean = X.sum(axis=1, keepdims=True) / ld(n)
    d = X - mean
    sd = np.sqrt((d * d).sum(axis=1, keepdims=True) / ld(n - 1))
    return d / (ld(1e-8) + sd)


def z_delta(X):
    """Elementwise first-order bound delta >= |device z - z_exact| (fp64, the shape of X), for every device route:
    dense (kernels_stats.hip: block partials chained in column order), a dgCMatrix's row view (kernels_csr.hip: lanes,
    then a tree; several shards: the host adds the shards' sums), one shard or several.  The roundings of the device's
    expressions, row by row, with A = mean |x_i|, mu and sd the exact mean and sd, Q = sum (x_i - mu)^2:

      mean    s = sum of n terms, any order: |s_d - s| <= (n - 1) u n A.  mu_d = fl(s_d / n), or fl(s_d * fl(1 / n)):
              at most 2 more roundings of a value <= A:                       e_mu = |mu_d - mu| <= (n + 1) u A
      d_i     fl(x_i - mu_d):                       |d_i,d - (x_i - mu)| <= e_mu + u |x_i - mu|
      Q_d     squares (1 rounding each, or none under FMA contraction) and an n-term sum in any order; a dgCMatrix adds
              fl(q + fl(z fl(mu^2))) for its implicit zeros, 3 more.  The shift of every d_i by e_mu moves Q by at most
              2 e_mu sum |x_i - mu| <= 2 e_mu sqrt(n Q):
                                                     |Q_d - Q| / Q <= 2 e_mu sqrt(n / (n - 1)) / sd + (n + 5) u
      sd_d    fl(sqrt(fl(Q_d / (n - 1)))): the division, then the root halves what came before and rounds once:
                                                     rho = |sd_d - sd| / sd <= e_mu sqrt(n / (n - 1)) / sd + ((n + 5) / 2 + 1.5) u
      den_d   fl(1e-8 + sd_d), sd / den <= 1:          |den_d - den| / den <= rho + u
      z_d     fl(fl(x - mu_d) / den_d): the numerator carries e_mu + u |x - mu|, the division rounds once:

                  delta = e_mu / den + |z| (rho + 3 u),        times (1 + 2^-4) for the second-order terms and the long-
                                                               double reference's own n 2^-64

    delta grows with A / sd (through e_mu / den and rho): a gene with a large mean and a small spread loses its z to
    cancellation, and the bound says so; it is no fixed constant.  For a constant row (Q = 0, z = 0) the |z| term
    vanishes and delta = e_mu / (1e-8): the bound ALLOWS a device z of ~1e-6 there, so a constant row is never
    'separated' by this bound -- it is a declared tie (separated()), whose exact 0 the device has to produce."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[1]
    Xl = X.astype(ld)
    mean = Xl.sum(axis=1, keepdims=True) / ld(n)
    d = Xl - mean
    sd = np.sqrt((d * d).sum(axis=1, keepdims=True) / ld(n - 1)).astype(np.float64)
    A = np.abs(X).mean(axis=1, keepdims=True)
    den = 1e-8 + sd
    z = np.abs((d / (ld(1e-8) + sd.astype(ld))).astype(np.float64))
    e_mu = (n + 1) * U * A
    with np.errstate(all="ignore"):
        rho = np.where(sd > 0.0, e_mu * np.sqrt(n / (n - 1.0)) / sd, 0.0) + ((n + 5) / 2.0 + 1.5) * U
    return (e_mu / den + z * (rho + 3.0 * U)) * (1.0 + 2.0 ** -4)


def separated(Z, delta, tie_groups=()):
    """The precondition that makes the device's signed ranks the reference's.  Z: z_exact (long double), delta: z_delta,
    tie_groups: lists of row indices that tie BY CONSTRUCTION -- bit-identical rows (equal z in every column, on any
    route that treats equal rows alike), a constant row and an all-zero dgCMatrix row (z exactly 0; a group of one).

      1. in every column, neighbours a, b in the sorted |z| are more than 2 (delta_a + delta_b) apart,
      2. every |z| exceeds 2 delta (the sign is the reference's),
    except: two rows of one declared group whose z are equal, two declared rows whose z are both exactly 0 (1.), and a
    declared row's exact 0 (2.).  A declared exact 0 is a value the device has to produce exactly (the bound delta of a
    constant row is far too wide to promise it; the GPU test fails if it is missed), so its delta counts as 0 towards
    its neighbours.  An undeclared exact tie or exact zero is ambiguous.

    Returns (ambiguous, margin): the number of pairs / values that break 1. or 2., and the smallest gap / (2 (delta_a +
    delta_b)) or |z| / (2 delta) met outside the exceptions.  The GPU tests' inputs must give ambiguous == 0."""
    Z = np.asarray(Z)
    g, n = Z.shape
    delta = np.broadcast_to(np.asarray(delta, dtype=np.float64), Z.shape)
    label = np.full(g, -1, dtype=np.int64)
    for q, rows in enumerate(tie_groups):
        label[np.asarray(rows, dtype=np.int64)] = q
    declared = (label >= 0)[:, None]
    absz = np.abs(Z)
    zero = absz == 0
    delta = np.where(zero & declared, 0.0, delta)
    # 2. signs
    need2 = 2.0 * delta
    ok2 = (absz.astype(np.float64) > need2) | (zero & declared)
    amb = int(np.count_nonzero(~ok2))
    with np.errstate(all="ignore"):
        m2 = np.where(zero & declared, np.inf, absz.astype(np.float64) / need2)
    margin = float(m2.min()) if m2.size else np.inf
    # 1. neighbours in the sorted |z| of every column
    order = np.argsort(absz, axis=0, kind="stable")
    cols = np.arange(n)[None, :]
    a, b = order[:-1, :], order[1:, :]
    gap = (absz[b, cols] - absz[a, cols]).astype(np.float64)
    need1 = 2.0 * (delta[a, cols] + delta[b, cols])
    same_group = (label[a] == label[b]) & (label[a] >= 0) & (gap == 0.0)
    both_zero = zero[a, cols] & zero[b, cols] & (label[a] >= 0) & (label[b] >= 0)
    exempt = same_group | both_zero
    amb += int(np.count_nonzero(~(gap > need1) & ~exempt))
    with np.errstate(all="ignore"):
        m1 = np.where(exempt, np.inf, gap / need1)
    if m1.size:
        margin = min(margin, float(m1.min()))
    return amb, margin


def ecdf_counts(X):
    """n * ecdf(x)(x_i) = #{x <= x_i} per gene over its samples (R/plaid.R:346 without the factor 1 / n): integers"""
    return st.rankdata(np.asarray(X, dtype=np.float64), method="max", axis=1).astype(np.float64)


# ------------------------------------------------------------------ replaid.gsva
def gsva_signed_ranks(X, rowtf):
    """(sign, R): the sign of zX and the average ranks of |zX| per column (R/plaid.R:352), from z_exact or ecdf_counts"""
    from oracle import plaid_oracle as po
    if rowtf == "z":
        Z = z_exact(X)
    elif rowtf == "ecdf":
        Z = ecdf_counts(X).astype(ld)
    else:
        raise ValueError(rowtf)
    absz = np.abs(Z)
    R = np.stack([po._rank_vec(absz[:, j], "average") for j in range(Z.shape[1])], axis=1)
    return np.sign(Z).astype(np.float64), R


def gsva_raw_ref(X, Gp, Gi, tau, rowtf):
    """(T, E, wmax): replaid.gsva before normalize_medians, T = w (P / max) with P the exact set sums of the weights
    sign r^(1 + tau) (long double) and max the largest |weight| of the whole matrix, and the bound E = (k + c) u mag on
    the device's raw score, mag = w sum |weight| / max.  The device (shard_scorer.cpp, scorer_worker) sums its own weights
    (k - 1 roundings) and applies fl(1 / max) * (sum * w): 3 roundings; the reference rounds T once; one spare: c = 5 for
    tau = 0, where weights and max are half-integers, exact on both sides.  tau > 0: every device weight is within
    a = pow_allowance_u(1 + tau) u of r^(1 + tau) (3 u for 1.5 and 1.3 on whichever route a column takes, 4.5 u for
    pow_quarters' 1.75), which carries to the sum and to the max: c = 5 + 2 a.  The row transform adds nothing: under
    separated() it changes no rank."""
    sign, R = gsva_signed_ranks(X, rowtf)
    power = ld(np.float64(1.0) + np.float64(tau)) if tau > 0 else ld(1.0)     # the device's fp64 exponent
    W = sign.astype(ld) * np.power(R.astype(ld), power)
    wmax = np.abs(W).max()
    P, mag, k = _long_sums(Gp, Gi, W)
    w = _w(Gp)[:, None]
    T = (w.astype(ld) * (P / wmax)).astype(np.float64)
    c = 5.0 + (2.0 * pow_allowance_u(np.float64(1.0) + np.float64(tau)) if tau > 0 else 0.0)
    E = (k + c) * U * (w * mag / float(wmax))
    return T, E, float(wmax)


def gsva_ref(X, Gp, Gi, tau=0.0, rowtf="z", raw=None):
    """(N, B): replaid.gsva(X, G, tau, rowtf) (R/plaid.R:338-363) and the elementwise bound on |device - N|.  X dense
    g x n (a dgCMatrix: its toarray()).  ignore.zero (min(S) == 0) resolves FALSE on both sides: asserted from a smallest
    raw score that no error within E can bring to 0 (negative for "z"; "ecdf" scores are all positive)"""
    T, E = raw if raw is not None else gsva_raw_ref(X, Gp, Gi, tau, rowtf)[:2]     # (raw: gsva_raw_ref's, computed before)
    assert abs(T.min()) > 10.0 * E.max(), "min(S) must be clearly nonzero for ignore.zero = FALSE on every route"
    return _normalized_ref(T, E, False)


def gsva_min_move(Gp, tau, wmax):
    """per set, a floor on what a rank off by 1/2 (or a sign 0 -> +-1) moves a raw score by:
    1/2 w_j (1 - 0.5^(1 + tau)) / max"""
    return 0.5 * _w(Gp) * (1.0 - 0.5 ** (1.0 + tau)) / wmax


def gsva_fp64(X, Gp, Gi, tau=0.0, rowtf="z", bump=None):
    """A plain fp64 restatement of the route (numpy's z, the oracle's ranks, a sparse product, the oracle's
    normalize_medians), for the sensitivity tests.  bump = (gene, sample, "rank"): that rank + 1/2;
    (gene, sample, "sign"): a sign 0 becomes -1 (what a z of -2e-8 in place of 0 does)"""
    from oracle import plaid_oracle as po
    X = np.asarray(X, dtype=np.float64)
    if rowtf == "z":
        with np.errstate(all="ignore"):
            Z = (X - X.mean(axis=1, keepdims=True)) / (1e-8 + X.std(axis=1, ddof=1, keepdims=True))
    else:
        Z = ecdf_counts(X)
    R = np.stack([po._rank_vec(np.abs(Z[:, j]), "average") for j in range(Z.shape[1])], axis=1)
    sign = np.sign(Z)
    if bump is not None:
        i, c, what = bump
        if what == "rank":
            R[i, c] += 0.5
        else:
            assert sign[i, c] == 0.0
            sign[i, c] = -1.0
    W = sign * R ** (1.0 + tau) if tau > 0 else sign * R
    wmax = np.abs(W).max()
    S = (1.0 / wmax) * ((_pattern_matrix(Gp, Gi, X.shape[0]).T @ W) * _w(Gp)[:, None])
    return po.normalize_medians(np.asarray(S), False)[0]


# ------------------------------------------------------------------ replaid.aucell
def aucell_ref(X, Gp, Gi, K):
    """(N, B, T, ignore_zero): replaid.aucell (R/plaid.R:304-309).  Weights 1.08 pmax((r - (max(r) - K)) / K, 0) of the
    dense average ranks r (a dgCMatrix: its zeros tie) in long double, exact set sums, plaid's mean and medians.  The
    device's map_kernel (op 1) rounds a subtraction, a division and a product per weight (3 u on each weight, so on the
    sum), the crossprod k - 1 times, sum * w once, the reference once, one spare: E = (k + 6) u mag.  A weight is exactly
    0 on both sides or positive on both (fmax of the same exact difference of half-integers; K an integer), so the zero
    pattern of the raw scores is exact: a set with no member in the top K scores 0, min(S) == 0 and ignore.zero
    resolves TRUE; with no such set (K >= g) it resolves FALSE.  The reference applies that rule."""
    from oracle import plaid_oracle as po
    X = np.asarray(X, dtype=np.float64)
    R = po._dense(po.colranks(X, ties_method="average"))
    rmax = R.max()
    Rl = R.astype(ld)
    W = ld(1.08) * np.maximum((Rl - (ld(rmax) - ld(K))) / ld(K), ld(0.0))
    P, mag, k = _long_sums(Gp, Gi, W)
    w = _w(Gp)[:, None]
    T = (P * w.astype(ld)).astype(np.float64)
    E = (k + 6.0) * U * mag * w
    iz = bool(T.min() == 0.0)
    assert T.min() >= 0.0
    N, B = _normalized_ref(T, E, iz)
    return N, B, T, iz


def aucell_fp64(X, Gp, Gi, K, bump=None):
    """fp64 restatement of replaid.aucell; bump = (gene, sample): that rank + 1/2"""
    from oracle import plaid_oracle as po
    X = np.asarray(X, dtype=np.float64)
    R = po._dense(po.colranks(X, ties_method="average"))
    rmax = R.max()
    if bump is not None:
        R[bump[0], bump[1]] += 0.5
    W = 1.08 * np.maximum((R - (rmax - K)) / K, 0.0)
    S = np.asarray((_pattern_matrix(Gp, Gi, X.shape[0]).T @ W) * _w(Gp)[:, None])
    return po.normalize_medians(S)[0]


# ------------------------------------------------------------------ replaid.scse
def scse_resolve_log2(X, remove_log2):
    """removeLog2 = NULL (R/plaid.R:160-161): min(X) == 0 and max(X) < 20 over ALL entries (implicit zeros included)"""
    if remove_log2 is not None:
        return bool(remove_log2)
    D = X.toarray() if sp.issparse(X) else np.asarray(X, dtype=np.float64)
    return bool(D.min() == 0.0 and D.max() < 20.0)


def scse_terms(X, removed):
    """(V, terms): the matrix the sums are taken of, in long double, and the number of terms of every column's sum |V|
    (dense: g; a dgCMatrix: its stored entries).  removeLog2: a dense X takes 2^x where x > 0 (:168-169), a dgCMatrix on
    every STORED value, zeros and negatives included (:166)"""
    if sp.issparse(X):
        Xs = sp.csc_matrix(X)
        g, n = Xs.shape
        cols = np.repeat(np.arange(n), np.diff(Xs.indptr))
        vals = Xs.data.astype(ld)
        V = np.zeros((g, n), dtype=ld)
        V[Xs.indices, cols] = np.exp2(vals) if removed else vals
        return V, np.diff(Xs.indptr).astype(np.float64)
    D = np.asarray(X, dtype=np.float64).astype(ld)
    if removed:
        D = np.where(D > 0, np.exp2(D), D)
    return D, np.full(D.shape[1], float(D.shape[0]))


def scse_ref(X, Gp, Gi, remove_log2=None, score_mean=False, exp2_ulps=EXP2_ULPS):
    """(ref, B, removed): replaid.scse (R/plaid.R:155-190).  X dense or scipy CSC.  Exact set sums P of V (X, or 2^x in
    long double), exact column sums D = sum |V| (set_sums with one all-genes set), then in long double
        mean: (P w) / (D / g + 1e-8)          sum: P / (D + 1e-8) * 100
    with w the device's fp64 set weight.  The device (scorer_worker; affine_kernel) computes
        S f,  f = fl(mul / fl(fl(D_d * div_scale) + 1e-8)),  div_scale = fl(1 / g) or 1,  mul = 1 or 100.
    Roundings relative to |ref|: D_d's sum of t terms (t - 1), div_scale and its product (2), + 1e-8 (1), the division
    (1), S f (1), the reference (1), one spare: t + 6.  Relative to mag = sum |terms| scaled like ref: the crossprod's
    k - 1, sum * w (1), one spare: k + 1.  So
        B = u ((k + 1 + a) mag + (t + 6 + a) |ref|),
    a = 0 without removeLog2 (fully derived), else the allowance `exp2_ulps` for one device 2^x: a relative error a u on
    every term moves the numerator by a u mag and the denominator by a u."""
    removed = scse_resolve_log2(X, remove_log2)
    V, terms = scse_terms(X, removed)
    g = V.shape[0]
    P, magS, k = _long_sums(Gp, Gi, V)
    allp = np.array([0, g], dtype=np.int64)
    D, _, _ = _long_sums(allp, np.arange(g, dtype=np.int64), np.abs(V))          # 1 x n
    w = _w(Gp)[:, None]
    if score_mean:
        den = D / ld(g) + ld(1e-8)
        T = (P * w.astype(ld)) / den
        scale = w / den.astype(np.float64)
    else:
        den = D + ld(1e-8)
        T = P / den * ld(100.0)
        scale = 100.0 / den.astype(np.float64)
    ref = T.astype(np.float64)
    a = float(exp2_ulps) if removed else 0.0
    B = U * ((k + 1.0 + a) * (magS * scale) + (terms[None, :] + 6.0 + a) * np.abs(ref))
    return ref, B, removed
