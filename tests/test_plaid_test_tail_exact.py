"""The host tail of plaid.test (stats.cpp, plaidhip_plaid_test_finish) against 50-digit references (mpmath) -- no GPU.

Measured on the grid below (glibc x86-64), worst relative distance from the 50-digit value, and what is asserted (four
times the measured value: libm differs a little between hosts); tests/helpers/exact_stats.py holds the same numbers:

    function                                      measured    asserted
    2 pt(|t|, df)   df 1 ... 1e7, p >= 1e-99       2.9e-13     1.2e-12
    pchisq(x, 2k, lower = FALSE), k = 1, 2, 3      2.3e-16     9.2e-16
    qnorm(p)        1e-99 ... 1 - 1e-16            3.3e-16     1.3e-15
    pnorm(z, lower = FALSE), z <= 22               6.0e-14     2.4e-13

This grid found two defects at large degrees of freedom, both fixed in stats.cpp:
  * betai took log(x) of the rounded x = df / (df + t^2), which for x = 1 - 3e-7 (df = 1e7, |t| ~ 1.7) has lost seven digits
    before a = df / 2 multiplies it: 3.6e-9 at df = 1e7, 2.4e-11 at df = 1e5.  It now takes log1p(-y), y = t^2 / (df + t^2).
  * betacf's fraction in x forms 1 - (1 - O(y)) at every other step when a is large and y = O(1 / a): 5.1e-10 at df = 1e7
    for |t| of 1.7 ... 4.  For a >= 100 betai now evaluates the even part of the fraction (betacf_even), which is written in
    y: 5.7e-14 at df = 1e7 afterwards.
The worst point left is df = 199.9 (a just below the Stirling switch at 100: the three lgamma values cancel).  Both
fractions stay far below their 10,000-iteration cap on the grid.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from plaid_amd import _lib
from plaid_amd.engine import plaid_test_finish
from tests.helpers import exact_stats as xs

mpmath = pytest.importorskip("mpmath")

DFS = [1, 1.5, 2, 3, 17.3, 199.9, 200, 200.1, 1e3, 1e5, 1e7]


def _f():
    f = _lib.load().plaidhip_debug_pvalue
    f.argtypes = [C.c_int, C.c_double, C.c_double]
    f.restype = C.c_double
    return f


def _rel(got, ref):
    ref = mpmath.mpf(ref)
    return float(abs(mpmath.mpf(got) - ref) / abs(ref)) if ref != 0 else abs(float(got))


def _t_at_p(p, df):
    """|t| with 2 pt(|t|, df) ~ p, by bisection in log t on the 50-digit function (2^-36 of the range is plenty for a grid end)"""
    lo, hi = math.log(1e-12), math.log(1e120)
    for _ in range(36):
        mid = 0.5 * (lo + hi)
        if xs.two_pt(math.exp(mid), df) > p:
            lo = mid
        else:
            hi = mid
    return math.exp(hi)


@functools.lru_cache(maxsize=None)
def _t_grid(df):
    """|t| from 1e-12 to where p reaches 1e-99 and one step beyond, and just either side of the continued fraction's
    switch x = (a + 1) / (a + b + 2), a = df / 2, b = 1 / 2, x = df / (df + t^2)"""
    t_end = _t_at_p(1e-99, df)
    ts = list(np.geomspace(1e-12, t_end, 40)) + [t_end * 1.05, 0.5, 1.0, 2.0, 5.0, 9.0]
    a = 0.5 * df
    xsw = (a + 1.0) / (a + 2.5)
    tsw = math.sqrt(df * (1.0 - xsw) / xsw)
    ts += [tsw * (1 - 1e-9), tsw, tsw * (1 + 1e-9), tsw * 0.9, tsw * 1.1]
    return ts


def _direct_side(a, b, y):
    """betai's choice: the fraction in x (True) or 1 - the fraction in y (False)"""
    return 1.0 - y < (a + 1.0) / (a + b + 2.0)


def _measure():
    f = _f()
    worst = {"pt": 0.0, "chisq": 0.0, "qnorm": 0.0, "pnorm": 0.0}
    at = {}

    def note(name, err, where):
        if err > worst[name]:
            worst[name], at[name] = err, where

    for df in DFS:
        for t in _t_grid(df):
            ref = xs.two_pt(t, df)
            if ref < mpmath.mpf(10) ** -110:
                continue
            note("pt", _rel(f(0, t, df), ref), (t, df))
    for k in (1, 2, 3):
        x_end = 2.0 * k * math.log(1e99)
        for x in list(np.geomspace(1e-12, x_end, 60)) + [x_end, 1.0, 9.2, 55.0, 460.0]:
            note("chisq", _rel(f(1, x, k), xs.chisq_upper_even(x, k)), (x, k))
    ps = list(np.geomspace(1e-99, 0.5, 120)) + [0.075, 0.0749999, 0.0750001, 0.925, 0.5, 0.3, 0.77,
                                               math.exp(-25.0), math.exp(-25.0) * (1 + 1e-9), math.exp(-25.0) * (1 - 1e-9)]
    ps += [1.0 - q for q in np.geomspace(1e-16, 0.4, 60)]
    for p in ps:
        ref = xs.qnorm(p)
        got = f(2, p, 0)
        note("qnorm", abs(got) if ref == 0 else _rel(got, ref), p)
    for z in list(np.linspace(-8.0, 22.0, 121)) + [0.0, 1e-9, 21.999]:
        note("pnorm", _rel(f(3, z, 0), xs.pnorm_upper(z)), z)
    return worst, at


def test_distribution_functions_within_four_times_their_measured_accuracy():
    worst, at = _measure()
    print("measured worst relative distance from the 50-digit value:", worst, "at", at)
    for name, w in worst.items():
        assert w <= xs.ASSERTED_ACC[name], (name, w, at[name], xs.ASSERTED_ACC[name])
        assert xs.ASSERTED_ACC[name] < 1e-10                       # worse than that would be a defect, not an accuracy


def test_the_references_agree_with_themselves_at_a_higher_precision():
    """two_pt() picks a side of the incomplete beta and a working precision: the same call at 90 digits, and the defining
    integral, agree to 45 digits where the hypergeometric series cancels most (large df, small t^2 / df)"""
    for t, df in [(21.0, 200.1), (1e-12, 1.0), (5.0, 1e3), (1e40, 1.5), (0.3, 1999.0), (40.0, 1500.0)]:
        a = xs.two_pt(t, df)
        with mpmath.workdps(90):
            tt, d = mpmath.mpf(t), mpmath.mpf(df)
            b = mpmath.betainc(d / 2, mpmath.mpf(1) / 2, 0, d / (d + tt * tt), regularized=True)
            c = xs._two_pt_quad(d / 2, d / (d + tt * tt))            # the large-df route, where both routes work
        assert _rel(a, b) < 1e-45 and _rel(c, b) < 1e-45, (t, df)
    for t, df in [(30.0, 1e7), (0.3, 1e5), (1e-12, 1e7), (22.0, 1e5), (0.01, 2001.0)]:
        with mpmath.workdps(110):
            tt, d = mpmath.mpf(t), mpmath.mpf(df)
            b = xs._two_pt_quad(d / 2, d / (d + tt * tt))
        assert _rel(xs.two_pt(t, df), b) < 1e-45, (t, df)
    with mpmath.workdps(60):
        q = 2 * mpmath.quad(lambda u: mpmath.gamma(2) / (mpmath.sqrt(3 * mpmath.pi) * mpmath.gamma(1.5))
                            * (1 + u * u / 3) ** -2, [2.5, mpmath.inf])
    assert _rel(xs.two_pt(2.5, 3), q) < 1e-40
    assert _rel(xs.chisq_upper_even(7.0, 2), mpmath.exp(-3.5) * 4.5) < 1e-45
    for p in (1e-99, 0.3, 1 - 1e-16):
        z = xs.qnorm(p)
        with mpmath.workdps(90):
            tail = mpmath.mpf(p) if p < 0.5 else 1 - mpmath.mpf(p)
            back = mpmath.erfc(abs(z) / mpmath.sqrt(2)) / 2
            assert abs(back - tail) <= mpmath.mpf(10) ** -45 * tail, p


def _betacf_mirror(a, b, x):
    """stats.cpp's betacf, operation for operation (Python floats are the same IEEE doubles): (value, iterations)"""
    tiny, eps = 1e-300, 1e-16
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    if abs(d) < tiny:
        d = tiny
    d = 1.0 / d
    h = d
    for m in range(1, 10001):
        m2 = 2.0 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        if abs(d) < tiny:
            d = tiny
        c = 1.0 + aa / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        if abs(d) < tiny:
            d = tiny
        c = 1.0 + aa / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        de = d * c
        h *= de
        if abs(de - 1.0) < eps:
            return h, m
    return h, 10001


def _betacf_even_mirror(a, b, x, y):
    """stats.cpp's betacf_even, operation for operation: (value, iterations)"""
    tiny, eps = 1e-300, 2.3e-16
    ayb = a * y - b * x + 1.0
    f = a * ayb / (a + 1.0)
    if abs(f) < tiny:
        f = tiny
    c, d = f, 0.0
    for m in range(1, 10001):
        den = a + 2.0 * m - 1.0
        an = (a + m - 1.0) * (a + b + m - 1.0) * m * (b - m) * x * x / (den * den)
        bn = m + m * (b - m) * x / den + (a + m) * (ayb + m * (2.0 - x)) / (a + 2.0 * m + 1.0)
        d = bn + an * d
        if abs(d) < tiny:
            d = tiny
        c = bn + an / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        de = c * d
        f *= de
        if abs(de - 1.0) < eps:
            return f, m
    return f, 10001


def test_the_continued_fractions_converge_before_their_cap_on_the_grid():
    """betacf's |del - 1| < 1e-16 holds in fp64 only for del == 1, betacf_even stops within one ulp: both must get there
    well before the 10,000-iteration cap at every grid point, on both sides of the switch"""
    most = (0, None)
    for df in DFS:
        a, b = 0.5 * df, 0.5
        for t in _t_grid(df):
            t2 = t * t
            x, y = df / (df + t2), t2 / (df + t2)
            if not (x > 0.0 and y > 0.0):
                continue
            if not _direct_side(a, b, y):
                _, it = _betacf_mirror(b, a, y)
            elif a >= 100.0:
                _, it = _betacf_even_mirror(a, b, x, y)
            else:
                _, it = _betacf_mirror(a, b, x)
            if it > most[0]:
                most = (it, (t, df))
    print("continued fractions: most iterations", most)
    assert most[0] < 1000, most


# ---------------------------------------------------------------------------------------------- plaid_test_finish
def _synthetic(m=9, g=500, seed=2):
    rng = np.random.default_rng(seed)
    k = rng.integers(2, 60, size=m)
    Gp = np.concatenate([[0], np.cumsum(k)]).astype(np.int32)
    mean = rng.normal(0.2, 0.3, m)
    sd = rng.uniform(0.5, 1.5, m)
    s1 = mean * k
    s2 = (k - 1) * sd * sd + k * mean * mean
    T = np.stack([s1, s2])
    tot1, tot2 = 0.05 * g, 3.0 * g
    SM = np.stack([rng.normal(0, 1, m), rng.normal(0.3, 1, m), rng.uniform(5, 50, m), rng.uniform(5, 50, m)])
    return g, Gp, T, tot1, tot2, SM, 13, 21


@pytest.mark.parametrize("metap", [0, 1])
@pytest.mark.parametrize("tests", range(1, 8))
def test_finish_on_synthetic_sufficient_statistics(tests, metap):
    """every `tests` mask and both meta-p methods: each p inside the interval of its exact sufficient statistics (a box of
    zero width: only the host's own roundings and the functions' accuracy), gsetFC = rowMeans of the effects present,
    p.meta inside the interval over the p-values the host itself returned, q.meta the plain BH restatement of p.meta"""
    g, Gp, T, tot1, tot2, SM, n0, n1 = _synthetic()
    m = len(Gp) - 1
    out = plaid_test_finish(g, Gp, T, tot1, tot2, SM if tests & 4 else None, n0, n1, tests, metap)
    nsep = 0
    for j in range(m):
        k = int(Gp[j + 1] - Gp[j])
        eff, pv = [], []
        if tests & 1:
            iv = xs.onesample_interval(k, T[0, j], 0.0, T[1, j], 0.0)
            nsep += iv is None
            assert iv and xs.in_interval(out[j, 1], iv), ("p.one", j, out[j, 1], iv)
            eff.append(T[0, j] / (1e-8 + k))
            pv.append(out[j, 1])
        else:
            assert np.isnan(out[j, 1])
        if tests & 2:
            iv = xs.twosample_interval(g, k, T[0, j], 0.0, T[1, j], 0.0, tot1, 0.0, tot2, 0.0)
            nsep += iv is None
            assert iv and xs.in_interval(out[j, 2], iv), ("p.two", j, out[j, 2], iv)
            eff.append(T[0, j] / (1e-8 + k) - (tot1 - T[0, j]) / (1e-8 + (g - k)))
            pv.append(out[j, 2])
        else:
            assert np.isnan(out[j, 2])
        if tests & 4:
            iv = xs.welch_interval(SM[0, j], 0.0, SM[1, j], 0.0, SM[2, j], 0.0, SM[3, j], 0.0, n0, n1)
            nsep += iv is None
            assert iv and xs.in_interval(out[j, 3], iv), ("p.lm", j, out[j, 3], iv)
            eff.append(SM[1, j] - SM[0, j])
            pv.append(out[j, 3])
        else:
            assert np.isnan(out[j, 3])
        np.testing.assert_allclose(out[j, 0], sum(eff) / len(eff), rtol=8 * xs.U, atol=0)
        if len(pv) == 1:
            assert out[j, 4] == pv[0]
        else:
            lo, hi = xs.combine_interval(pv, metap)
            assert lo <= out[j, 4] <= hi, ("p.meta", j, out[j, 4], lo, hi)
    assert nsep == 0
    assert np.array_equal(out[:, 5], xs.p_adjust_fdr(out[:, 4]))


def test_finish_clamps_and_nan():
    """NaN p -> 1 -> 1 - 1e-99; a p below 1e-99 -> 1e-99; Fisher with two and three p-values at the clamp; Stouffer with
    p = 1e-99 and p = 1 - 1e-99"""
    Gp = np.array([0, 50, 100, 101, 151], dtype=np.int32)
    g = 400
    # set 0: an enormous effect (p -> 0, clamped); set 1: no effect at all; set 2: one gene (var = 0 / 0 -> NaN -> 1);
    # set 3: moderate
    T = np.array([[50 * 10.0, 0.0, 3.0, 50 * 0.1], [50 * 100.0 + 49 * 1e-4, 49 * 1.0, 9.0, 49 * 1.0 + 50 * 0.01]])
    SM = np.array([[0.0, 1.0, np.nan, 0.0], [100.0, 1.0, 0.0, 0.5], [1.0, 4.0, 1.0, 9.0], [1.0, 4.0, 1.0, 9.0]])
    n0, n1 = 40, 40
    tot1, tot2 = 10.0, 5e3 + 400.0
    for metap in (0, 1):
        out = plaid_test_finish(g, Gp, T, tot1, tot2, SM, n0, n1, 7, metap)
        assert out[0, 1] == 1e-99 and out[0, 3] == 1e-99
        assert out[2, 1] == xs.P_HI and out[2, 3] == xs.P_HI          # NaN -> 1 -> the clamp (1 - 1e-99 == 1.0 in fp64)
        assert out[1, 1] == xs.P_HI and out[1, 3] == xs.P_HI          # t == 0 exactly
        for j in range(4):
            lo, hi = xs.combine_interval(list(out[j, 1:4]), metap)
            assert lo <= out[j, 4] <= hi, (metap, j, out[j, 4], lo, hi)
        assert np.array_equal(out[:, 5], xs.p_adjust_fdr(out[:, 4]))
    # two p-values at the clamp (tests = one + lm), three when p.two is clamped too
    out = plaid_test_finish(g, Gp, T, tot1, tot2, SM, n0, n1, 5, 0)
    assert out[0, 1] == 1e-99 and out[0, 3] == 1e-99
    ref = float(xs.chisq_upper_even(-4 * math.log(1e-99), 2))
    assert abs(out[0, 4] - ref) <= xs.ASSERTED_ACC["chisq"] * ref + 456 * 4 * xs.U * ref
    # p.two at the clamp too: a set 1e6 above a rest of variance 1e8 (dof ~ 930 by the reference's formula, t ~ 1800)
    T3 = T.copy()
    T3[:, 0] = [50e6, 49e6 + 50e12]
    out = plaid_test_finish(g, Gp, T3, 50e6, float(T3[1, 0] + 349e8), SM, n0, n1, 7, 0)
    assert list(out[0, 1:4]) == [1e-99] * 3
    lo, hi = xs.combine_interval([1e-99] * 3, 0)
    assert lo <= out[0, 4] <= hi and out[0, 4] > 0.0
    # Stouffer with p = 1e-99 against p = 1 - 1e-99: qnorm(1.0) is +Inf, as in R, and the meta-p 1 (z = -Inf)
    out = plaid_test_finish(g, Gp, T, tot1, tot2, SM, n0, n1, 5, 1)
    assert out[0, 4] < 1e-90 and out[1, 4] == 1.0 and out[2, 4] == 1.0


def test_p_adjust_fdr_against_the_plain_restatement():
    """through p.meta = the single p-value of tests = 4: ties, NaN entries (impossible after the clamp, so through the
    restatement's own checks) and m = 1"""
    p = np.array([0.01, 0.04, 0.04, 0.03, 0.5, 0.01, 1.0])
    assert np.allclose(xs.p_adjust_fdr(p), [0.035, 0.056, 0.056, 0.056, 7 * 0.5 / 6, 0.035, 1.0], rtol=1e-15)
    pn = np.array([0.01, np.nan, 0.04, np.nan, 0.03])
    q = xs.p_adjust_fdr(pn)
    assert np.isnan(q[[1, 3]]).all() and np.allclose(q[[0, 2, 4]], [0.03, 0.04, 0.04], rtol=1e-15)
    assert xs.p_adjust_fdr(np.array([0.2])).tolist() == [0.2]
    # the library's BH through plaid_test_finish: tests = 4 makes p.meta = p.lm, ties from repeated columns of SM
    rng = np.random.default_rng(3)
    for m in (1, 2, 7, 40):
        base = np.stack([rng.normal(0, 1, m), rng.normal(0.4, 1, m), rng.uniform(5, 50, m), rng.uniform(5, 50, m)])
        if m >= 7:
            base[:, 3] = base[:, 1]
            base[:, 5] = base[:, 1]
            base[0, 6] = np.nan                                            # a NaN statistic: p = 1 after the clamp
        Gp = np.arange(0, 3 * (m + 1), 3, dtype=np.int32)
        out = plaid_test_finish(3 * m, Gp, np.zeros((2, m)), 0.0, 0.0, base, 9, 11, 4, 0)
        assert np.array_equal(out[:, 4], out[:, 3])
        assert np.array_equal(out[:, 5], xs.p_adjust_fdr(out[:, 4]))
        if m >= 7:
            assert out[3, 5] == out[1, 5] == out[5, 5] and out[6, 3] == xs.P_HI
