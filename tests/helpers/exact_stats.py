"""Exact references for plaid.test (R/plaid.R:392-537), and the bounds that hold the device moments and the host tail
to them (host only, no GPU, no fixtures).  Written from the R formulas, not from the kernels.

group_moments():   per row of a rows x n matrix and per group of 0/1 labels: the mean and the sum of squared deviations,
                   exact in rational arithmetic and rounded once, with mag = sum |x| and the term count n_k
mean_bound() / ssd_bound():  the fp64 error bounds of the device's block-partial means and two-pass ssd (derivations in
                   the docstrings, in the style of tests/test_gpu_exact_sums.py's `c`)
two_pt() ...:      the distribution functions of the tail at 50 digits (mpmath)
onesample / twosample / welch:  the three statistics at 50 digits from exact sufficient statistics, in the reference's own
                   formula (the 1e-8 guards, max(df, 1))
*_interval():     the interval a correctly rounded pipeline's p-value must lie in, given the error box of its sufficient
                   statistics; a box that reaches var <= 0 or df < 1 is "not separable" (None), which callers COUNT
"""
from __future__ import annotations

import itertools
from fractions import Fraction

import numpy as np

from tests.helpers import exact_ref as er

U = er.U
P_LO, P_HI = 1e-99, 1.0 - 1e-99          # R/plaid.R:444 (1 - 1e-99 == 1.0 in fp64, as in R)

# Worst relative distance of stats.cpp's distribution functions from the 50-digit value, MEASURED on the grid of
# tests/test_plaid_test_tail_exact.py (glibc x86-64), and what that test asserts: four times the measured value (the
# factor covers libm differences between hosts).  The *_interval() functions widen by ASSERTED_ACC.
MEASURED_ACC = {"pt": 2.9e-13, "chisq": 2.3e-16, "qnorm": 3.3e-16, "pnorm": 6.0e-14}
ASSERTED_ACC = {k: 4.0 * v for k, v in MEASURED_ACC.items()}


# ------------------------------------------------------------------------------------------------ group moments
def _frac3(hi, lo, lo2):
    return Fraction(float(hi)) + Fraction(float(lo)) + Fraction(float(lo2))


def group_moments(A, y):
    """A: rows x n (finite or not), y: n labels in {0, 1}.  Returns a dict of (2, rows) arrays, group 0 first:
      sum   the exact group sum rounded once            mag   sum |x| over the group's finite values (fp64)
      mean  the exact sum / n_k rounded once (NaN for an empty group: 0 / 0, as rowMeans of no columns)
      ssd   the exact sum (x - mean_exact)^2 rounded once, = sum x^2 - (sum x)^2 / n_k in rationals (0 for an empty group)
      n     (2,) the group sizes
    A group with a NaN, or with +Inf and -Inf: sum / mean / ssd NaN.  With Inf of one sign: sum / mean that Inf, ssd NaN
    (Inf - Inf).  Sums of x and x^2 are accumulated error-free (TwoSum / TwoProduct), then combined as Fractions."""
    A = np.asarray(A, dtype=np.float64)
    y = np.asarray(y)
    rows, n = A.shape
    out = {k: np.zeros((2, rows)) for k in ("sum", "mean", "ssd", "mag")}
    out["n"] = np.array([int(np.sum(y == 0)), int(np.sum(y == 1))])
    for grp in (0, 1):
        cols = np.flatnonzero(y == grp)
        nk = len(cols)
        s, q = er._Acc((rows,)), er._Acc((rows,))
        mag = np.zeros(rows)
        nan = np.zeros(rows, dtype=bool)
        pinf = np.zeros(rows, dtype=bool)
        ninf = np.zeros(rows, dtype=bool)
        with np.errstate(all="ignore"):
            for c in cols:
                x = A[:, c]
                fin = np.isfinite(x)
                nan |= np.isnan(x)
                pinf |= x == np.inf
                ninf |= x == -np.inf
                xf = np.where(fin, x, 0.0)
                mag += np.abs(xf)
                s.add(slice(None), xf)
                p, e = er.two_prod(xf, xf)
                q.add(slice(None), p)
                q.add(slice(None), e)
        sm, mean, ssd = np.zeros(rows), np.full(rows, np.nan), np.zeros(rows)
        for r in range(rows):
            sx = _frac3(s.hi[r], s.lo[r], s.lo2[r])
            sm[r] = float(sx)
            if nk:
                mean[r] = float(sx / nk)
                ssd[r] = float(_frac3(q.hi[r], q.lo[r], q.lo2[r]) - sx * sx / nk)
        bad = nan | (pinf & ninf)
        for arr in (sm, mean):
            arr[pinf] = np.inf
            arr[ninf] = -np.inf
            arr[bad] = np.nan
        if nk:
            ssd[nan | pinf | ninf] = np.nan
        else:
            mean[:] = np.nan
        out["sum"][grp], out["mean"][grp], out["ssd"][grp], out["mag"][grp] = sm, mean, ssd, mag
    return out


MEAN_C_DENSE = 3    # after the sum: fl(1 / n_k), the product with it (reduce_blocks_kernel), the reference's rounding
MEAN_C_CSR = 2      # after the sum: the division s / n_k (csr_row_moments_kernel), the reference's rounding


def sum_bound(mag, nk):
    """|device sum - exact sum| <= (n_k + 1) u mag: the n_k terms of a group are added in some order (128-column block
    partials, then the blocks; the other group's columns add exact zeros) -- n_k - 1 roundings of partial sums that
    never exceed mag -- and c = 1 for the reference's own rounding."""
    return er.fp64_bound(mag, nk, 1)


def mean_bound(mag, nk, c=MEAN_C_DENSE):
    """|device mean - exact mean| <= (n_k + c) u mag / n_k.  The sum as in sum_bound(); then c roundings of relative size
    u, each of a value <= mag / n_k: c = 3 for reduce_blocks_kernel (fl(1 / n_k), sum * fl(1 / n_k), the reference's
    rounding), c = 2 where the kernel divides (s / n_k, the reference's rounding).  An empty group has no bound (NaN)."""
    nk = np.asarray(nk, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(nk > 0, er.fp64_bound(np.asarray(mag) / np.maximum(nk, 1.0), nk, c), 0.0)


def ssd_bound(ssd, nk, mean_err, implicit_zeros=False):
    """|device ssd - exact ssd| for the two-pass form taken about the device's ROUNDED mean mh, |mh - m| <= mean_err.

    Exactly, sum (x - mh)^2 = sum (x - m)^2 + n_k (mh - m)^2: the first-order term 2 (m - mh) sum (x - m) VANISHES because
    m is the exact mean.  So the rounded mean costs only n_k mean_err^2, and with Q = ssd + n_k mean_err^2:
      fl(x - mh) and its square: (1 + d)^2 (1 + d) -> 3 u per term; the sum of n_k non-negative terms: (n_k - 1) u;
      the reference's rounding: u.         |err| <= (n_k + 4) u Q + n_k mean_err^2     (one spare u for second order)
    implicit_zeros (the CSR form, csr_row_moments_kernel): the stored values as above, plus z * fl(mh * mh) added once --
    the square, the product with z and the addition are 3 more roundings of values <= Q: (n_k + 7) u Q + n_k mean_err^2.
    The one-pass form sum x^2 - n mean^2 errs by ~u sum x^2 instead, which this bound does not cover when |m| >> sd."""
    nk = np.asarray(nk, dtype=np.float64)
    e2 = nk * np.asarray(mean_err, dtype=np.float64) ** 2
    Q = np.asarray(ssd, dtype=np.float64) + e2
    return er.fp64_bound(Q, nk, 7 if implicit_zeros else 4) + e2


# ------------------------------------------------------------------------------------------------ 50-digit functions
def _mp():
    import mpmath
    return mpmath


DPS = 50


def two_pt(t, df):
    """2 * pt(|t|, df, lower.tail = FALSE) = I_{df / (df + t^2)}(df / 2, 1 / 2) at 50 digits (evaluated on the side whose
    argument is <= 1/2, at a working precision that leaves 50 digits after the 1 - ...)"""
    mp = _mp()
    with mp.workdps(DPS + 20):
        t, df = mp.mpf(t), mp.mpf(df)
        if mp.isnan(t) or mp.isnan(df) or not df > 0:
            return mp.nan
        if mp.isinf(t):
            return mp.mpf(0)
        t2 = t * t
        x, yy = df / (df + t2), t2 / (df + t2)
        if df > 2000:
            return _two_pt_quad(df / 2, x)
        try:
            if x <= 0.5:
                return +mp.betainc(df / 2, mp.mpf(1) / 2, 0, x, regularized=True)
            return 1 - mp.betainc(mp.mpf(1) / 2, df / 2, 0, yy, regularized=True)
        except mp.libmp.libhyper.NoConvergence:
            return _two_pt_quad(df / 2, x)


def _two_pt_quad(a, x):
    """I_x(a, 1/2) for large a, where the hypergeometric series of betainc needs ~a terms: with u = x exp(-s / a),
    I_x(a, 1/2) = x^a / (a B(a, 1/2)) * int_0^inf exp(-s) (1 - x exp(-s / a))^(-1/2) ds, a smooth integrand with at most an
    integrable square-root singularity at s = 0 (x -> 1), which tanh-sinh quadrature resolves.  Call inside workdps."""
    mp = _mp()
    if x == 1:
        return mp.mpf(1)
    integral = mp.quad(lambda s: mp.exp(-s) / mp.sqrt(1 - x * mp.exp(-s / a)), [0, 0.01, 1, 8, 30, 100, 200, mp.inf])
    lognorm = mp.loggamma(a + mp.mpf(1) / 2) - mp.loggamma(a) - mp.log(mp.pi) / 2
    return mp.exp(lognorm + a * mp.log(x)) * integral / a


def chisq_upper_even(x, k):
    """pchisq(x, 2k, lower.tail = FALSE) = Q(k, x / 2)"""
    mp = _mp()
    with mp.workdps(DPS + 10):
        x = mp.mpf(x)
        if not x > 0:
            return mp.mpf(1)
        return +mp.gammainc(k, x / 2, mp.inf, regularized=True)


def pnorm_upper(z):
    mp = _mp()
    with mp.workdps(DPS + 10):
        return mp.erfc(mp.mpf(z) / mp.sqrt(2)) / 2


def qnorm(p):
    """qnorm(p): the root of the tail probability on the side of p that keeps its digits, by Newton at 50 digits"""
    mp = _mp()
    with mp.workdps(DPS + 10):
        p = mp.mpf(p)
        if p == 0.5:
            return mp.mpf(0)
        if p == 0 or p == 1:
            return mp.inf if p == 1 else -mp.inf
        upper = p > 0.5
        tail = 1 - p if upper else p              # exact: p is a double, the working precision holds 1 - p
        z = mp.sqrt(-2 * mp.log(tail)) if tail < 0.1 else mp.mpf(0.5)      # P(Z > z) = tail, z > 0
        for _ in range(200):
            f = mp.erfc(z / mp.sqrt(2)) / 2 - tail
            dz = f / (mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi))
            z += dz
            if abs(dz) <= mp.mpf(10) ** (-DPS - 5) * max(abs(z), 1):
                break
        else:
            raise ArithmeticError("qnorm: Newton did not converge")
        return z if upper else -z


def clamp_p(p):
    """P1[is.na(P1)] <- 1; pmin(pmax(P1, 1e-99), 1 - 1e-99) in fp64"""
    p = float(p)
    if p != p:
        p = 1.0
    return min(max(p, P_LO), P_HI)


# ------------------------------------------------------------------------------------------------ the three statistics
GUARD = 1e-8        # the reference's 1e-8, the double


def onesample_t_df(k, s1, s2):
    """matrix_onesample_ttest, R/plaid.R:476-486: (meanx, t, df) at 50 digits; var <= 0 -> t is None"""
    mp = _mp()
    k, s1, s2 = mp.mpf(k), mp.mpf(s1), mp.mpf(s2)
    meanx = s1 / (mp.mpf(GUARD) + k)
    var = (s2 - meanx * meanx * k) / (k - 1)
    if not var > 0:
        return meanx, None, None
    t = meanx / (mp.mpf(GUARD) + mp.sqrt(var)) * mp.sqrt(k)
    return meanx, t, max(k - 1, mp.mpf(1))


def twosample_t_df(g, k, s1, s2, tot1, tot2):
    """matrix_twosample_ttest, R/plaid.R:488-520: (diff, t, dof before max(dof, 1)); a variance <= 0 -> t is None"""
    mp = _mp()
    g, k, s1, s2, tot1, tot2 = (mp.mpf(v) for v in (g, k, s1, s2, tot1, tot2))
    sum1, sum0 = k, g - k
    ssq1, ssq0 = s2, tot2 - s2
    mean1, mean0 = s1 / (mp.mpf(GUARD) + sum1), (tot1 - s1) / (mp.mpf(GUARD) + sum0)
    var0 = (ssq0 - mean0 * mean0 * sum0) / (sum0 - 1)
    var1 = (ssq1 - mean1 * mean1 * sum1) / (sum1 - 1)
    f = mean1 - mean0
    if not (var0 > 0 and var1 > 0):
        return f, None, None
    varsum = var0 / sum0 + var1 / sum1
    dof = varsum ** 2 / (var0 / sum0 * (sum0 - 1) + var1 / sum1 * (sum1 - 1))
    return f, f / mp.sqrt(varsum), dof


def welch_t_df(m0, m1, ssd0, ssd1, n0, n1):
    """Rfast::ttests(x, ina), R/plaid.R:429: the Welch t and its Satterthwaite degrees of freedom"""
    mp = _mp()
    m0, m1, ssd0, ssd1, n0, n1 = (mp.mpf(v) for v in (m0, m1, ssd0, ssd1, n0, n1))
    a, b = ssd0 / (n0 - 1) / n0, ssd1 / (n1 - 1) / n1
    if not (a > 0 and b > 0):
        return None, None
    t = (m0 - m1) / mp.sqrt(a + b)
    return t, (a + b) ** 2 / (a * a / (n0 - 1) + b * b / (n1 - 1))


# ------------------------------------------------------------------------------------------------ the interval check
# Roundings of the host formulas (stats.cpp) after the sufficient statistics, counted generously:
#   var = (s2 - meanx^2 k) / (k - 1): meanx (denominator, division: 2 u), its square (-> 5 u), times k (6 u), the
#   subtraction (u of the result): <= 7 u s2 absolute on the numerator since meanx^2 k <= s2 -- taken as 8 u on s2 (and on
#   tot2 - s2), i.e. the BOX of s2 / tot2 is widened by 8 u |s2| before the corners are taken.
#   t from (mean, var): division by k - 1, sqrt, the guard's addition, division, sqrt(k), the product: <= 8 u relative.
#   dof: ~2 x the roundings of varsum, squared: <= 16 u relative.
HOST_S2_U, HOST_T_U, HOST_DF_U = 8, 8, 16


def _corners(boxes):
    return itertools.product(*[(lo, hi) if lo != hi else (lo,) for lo, hi in boxes])


def _box(v, err):
    mp = _mp()
    v, err = mp.mpf(float(v)) if not isinstance(v, mp.mpf) else v, mp.mpf(float(err))
    return (v - err, v + err)


def _p_range(ts, dfs, df_floor):
    """[min, max] of clamp(2 pt(|t|, max(df, floor))) over the corners' t and df, the host's own roundings of t and df and
    the accuracy of the distribution function included.  Without a floor (Welch: dof >= min(n0, n1) - 1 >= 1 in exact
    arithmetic) a df below 1 is not separable: None."""
    mp = _mp()
    at = [abs(t) for t in ts]
    t_lo, t_hi = min(at) * (1 - HOST_T_U * U), max(at) * (1 + HOST_T_U * U)
    if min(ts) < 0 < max(ts):
        t_lo = mp.mpf(0)
    d_lo, d_hi = min(dfs) * (1 - HOST_DF_U * U), max(dfs) * (1 + HOST_DF_U * U)
    if df_floor:                                   # max(dof, 1) is continuous and p monotone in it: the floor moves both ends
        d_lo, d_hi = max(d_lo, mp.mpf(df_floor)), max(d_hi, mp.mpf(df_floor))
    elif d_lo < 1:
        return None
    ps = [two_pt(t, d) for t in (t_lo, t_hi) for d in (d_lo, d_hi)]
    acc = ASSERTED_ACC["pt"]
    return clamp_p(min(ps) * (1 - acc)), clamp_p(max(ps) * (1 + acc))


def onesample_interval(k, s1, e1, s2, e2):
    """(p_lo, p_hi, mean_lo, mean_hi) of p.one for exact per-set sums s1 = sum fc, s2 = sum fc^2 known to +- e1, e2; None
    if the box reaches var <= 0 (not separable).  k >= 2."""
    mp = _mp()
    with mp.workdps(DPS):
        e2 = float(e2) + HOST_S2_U * U * abs(float(s2))
        ts, dfs, ms = [], [], []
        for a, b in _corners([_box(s1, e1), _box(s2, e2)]):
            mean, t, df = onesample_t_df(k, a, b)
            if t is None:
                return None
            ts.append(t), dfs.append(df), ms.append(mean)
        # df = max(k - 1, 1) is an integer: no rounding, no box
        at = [abs(t) for t in ts]
        t_lo, t_hi = min(at) * (1 - HOST_T_U * U), max(at) * (1 + HOST_T_U * U)
        if min(ts) < 0 < max(ts):
            t_lo = mp.mpf(0)
        ps = [two_pt(t_lo, dfs[0]), two_pt(t_hi, dfs[0])]
        acc = ASSERTED_ACC["pt"]
        return clamp_p(min(ps) * (1 - acc)), clamp_p(max(ps) * (1 + acc)), float(min(ms)), float(max(ms))


def twosample_interval(g, k, s1, e1, s2, e2, tot1, et1, tot2, et2):
    """(p_lo, p_hi, diff_lo, diff_hi) of p.two; None if the box reaches a variance <= 0 (not separable).  The reference's
    dof (":513 NEED CHECKING") is usually far below 1, where pmax(dof, 1) holds it at 1: the floor is applied, not excluded."""
    mp = _mp()
    with mp.workdps(DPS):
        e2 = float(e2) + HOST_S2_U * U * abs(float(s2))
        et2 = float(et2) + HOST_S2_U * U * abs(float(tot2))
        ts, dfs, fs = [], [], []
        for a, b, c, d in _corners([_box(s1, e1), _box(s2, e2), _box(tot1, et1), _box(tot2, et2)]):
            f, t, dof = twosample_t_df(g, k, a, b, c, d)
            if t is None:
                return None
            ts.append(t), dfs.append(dof), fs.append(f)
        r = _p_range(ts, dfs, 1)
        return None if r is None else (r[0], r[1], float(min(fs)), float(max(fs)))


def welch_interval(m0, e0, m1, e1, ssd0, q0, ssd1, q1, n0, n1):
    """(p_lo, p_hi) of p.lm for exact group means / ssd known to +- e0, e1, q0, q1; None if the box reaches a variance
    <= 0 or dof < 1 (not separable).  n0, n1 >= 2."""
    mp = _mp()
    with mp.workdps(DPS):
        ts, dfs = [], []
        for a, b, c, d in _corners([_box(m0, e0), _box(m1, e1), _box(ssd0, q0), _box(ssd1, q1)]):
            t, dof = welch_t_df(a, b, c, d, n0, n1)
            if t is None:
                return None
            ts.append(t), dfs.append(dof)
        return _p_range(ts, dfs, 0)


def in_interval(p, iv):
    return iv[0] <= p <= iv[1]


# ------------------------------------------------------------------------------------------------ meta-p and FDR
def combine_interval(ps, method):
    """the interval of matrix_combine_p (R/plaid.R:522-537) over fp64 p-values `ps` (already clamped): fisher (0):
    x = -2 sum log p, each log and each addition one rounding -> x (1 +- (np + 2) u); stouffer (1): each -qnorm(p) within
    ASSERTED_ACC['qnorm'], the sum and the division by sqrt(np) (np + 2) u.  Widened by the accuracy of the last function."""
    mp = _mp()
    with mp.workdps(DPS):
        npv = len(ps)
        if method == 0:
            x = -2 * sum(mp.log(mp.mpf(float(p))) for p in ps)
            mag = 2 * sum(abs(mp.log(mp.mpf(float(p)))) for p in ps)
            ex = (npv + 2) * U * mag
            vals = [chisq_upper_even(max(x - ex, 0), npv), chisq_upper_even(x + ex, npv)]
            acc = ASSERTED_ACC["chisq"]
        else:
            zs = [-qnorm(p) for p in ps]
            if any(mp.isinf(z) for z in zs):                       # qnorm(1 - 1e-99) = qnorm(1.0) = Inf in fp64, as in R
                v = float(pnorm_upper(sum(zs))) if len({z for z in zs if mp.isinf(z)}) == 1 else float("nan")
                return v, v
            mag = sum(abs(z) for z in zs)
            zz = sum(zs) / mp.sqrt(npv)
            ez = (ASSERTED_ACC["qnorm"] + (npv + 2) * U) * mag / mp.sqrt(npv)
            vals = [pnorm_upper(zz - ez), pnorm_upper(zz + ez)]
            acc = ASSERTED_ACC["pnorm"]
        return float(min(vals) * (1 - acc)), float(max(vals) * (1 + acc))


def p_adjust_fdr(p):
    """stats::p.adjust(p, 'fdr'): pmin(1, cummin(n / i * p[o]))[ro] over the non-NA entries, o = decreasing order;
    NA stay NA and do not count in n"""
    p = np.asarray(p, dtype=np.float64)
    q = np.full(p.shape, np.nan)
    ok = np.flatnonzero(~np.isnan(p))
    n = len(ok)
    if n == 0:
        return q
    o = ok[np.argsort(-p[ok], kind="stable")]
    i = np.arange(n, 0, -1, dtype=np.float64)
    q[o] = np.minimum(1.0, np.minimum.accumulate(p[o] * float(n) / i))
    return q


# ------------------------------------------------------------------------------------------------ gene fold changes
FC_C = 8   # roundings after the two means: m1 - m0, the crossprod's one-term sum, fl(1e-8 + 1), the division -- on the
           # device and host (4) -- and the same four in the test's own fp64 restatement of the exact value


def fold_changes(X, y, c=MEAN_C_DENSE):
    """(fc, err): fc = fl(mean1 - mean0) of the exactly rounded group means of every row of X, and a bound on
    |device fc - fc|: the two means' bounds (mean_bound with `c`) plus 4 u |fc| (the device's subtraction, this one, and the
    two reference roundings of the means, each <= u |mean| <= the means' own bounds, taken once more as u |fc| each)."""
    r = group_moments(X, y)
    nk = r["n"][:, None].astype(np.float64)
    mb = mean_bound(r["mag"], nk, c)
    with np.errstate(all="ignore"):
        fc = r["mean"][1] - r["mean"][0]
        return fc, mb[0] + mb[1] + 4 * U * np.abs(fc)


def singleton_fc_bound(fc, err):
    """gsetFC of a one-gene set under tests = "one": fc / (1 + 1e-8).  "That of the mean, times two, plus the division":
    (err + FC_C u |fc|) / (1 + 1e-8) -- err from fold_changes() already holds the two means' bounds."""
    return (err + FC_C * U * np.abs(fc)) / (1.0 + GUARD) + 2.0 ** -1074


# ------------------------------------------------------------------------------------------------ p.one / p.two cases
# The inputs of tests/test_gpu_plaid_test_exact.py::test_one_and_two_sample_p_values_from_the_device_crossprod, built here so
# that tests/test_exact_stats_ref.py can count the sets that are not separable from the reference alone: (g, n, m, seed)
CROSSPROD_CASES = [(2000, 60, 40, 11), (4097, 129, 60, 12), (257, 1000, 24, 13)]


def crossprod_case(g, n, m, seed):
    """X (g x n) with a real group effect, + N(0, 0.3) per gene on the y == 1 columns; m sets of 2 ... 200 genes, the last
    one of g - 2 genes"""
    rng = np.random.default_rng(seed)
    y = (rng.random(n) < 0.4).astype(np.int32)
    y[:4] = [0, 1, 0, 1]
    X = rng.gamma(2.0, 1.0, size=(g, n))
    X[:, y == 1] += rng.normal(0.0, 0.3, size=(g, 1))
    sizes = rng.integers(2, min(200, g - 2) + 1, size=m)
    sizes[0], sizes[-1] = 2, g - 2
    sets = [np.sort(rng.choice(g, size=int(k), replace=False)) for k in sizes]
    Gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return X, y, Gp, np.concatenate(sets).astype(np.int32)


def crossprod_intervals(X, y, Gp, Gi):
    """Per set: (onesample_interval, twosample_interval) of p.one / p.two (None where not separable).

    Sufficient statistics: fc and err from fold_changes(); s1 = sum fc and s2 = sum fc^2 over the set by
    exact_ref.set_sums.  Error boxes: a device fc within err of fc makes fc^2 within 2 |fc| err + err^2 + u fc^2 (the
    device's rounding of the square) + u fc^2 (this file's); the set sums add (k + 1) u mag each (k terms in any order, the
    reference's rounding) and the per-gene errors; the totals over all g genes, summed on the host in gene order,
    (g + 1) u sum |.| and the per-gene errors."""
    fc, err = fold_changes(X, y)
    g = len(fc)
    f2 = fc * fc
    e2 = 2 * np.abs(fc) * err + err * err + 2 * U * f2
    ref, mag, k = er.set_sums(Gp, Gi, np.stack([fc, f2, err, e2], axis=1))
    sizes = np.diff(Gp).astype(np.float64)
    s1, s2 = ref[:, 0], ref[:, 1]
    b1 = er.fp64_bound(mag[:, 0], sizes, 1) + ref[:, 2] * (1 + 4 * U)
    b2 = er.fp64_bound(mag[:, 1], sizes, 1) + ref[:, 3] * (1 + 4 * U)
    tot1, tot2 = er.fraction_sum(fc), er.fraction_sum(f2)
    bt1 = float(er.fp64_bound(np.abs(fc).sum(), g, 1)) + float(err.sum()) * (1 + 4 * U)
    bt2 = float(er.fp64_bound(f2.sum(), g, 1)) + float(e2.sum()) * (1 + 4 * U)
    out = []
    for j in range(len(sizes)):
        kj = int(sizes[j])
        out.append((onesample_interval(kj, s1[j], b1[j], s2[j], b2[j]),
                    twosample_interval(g, kj, s1[j], b1[j], s2[j], b2[j], tot1, bt1, tot2, bt2)))
    return out
