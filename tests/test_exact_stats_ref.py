"""Self-tests of tests/helpers/exact_stats.py (host only): the exact group moments against fraction_sum and hand cases,
and the sensitivity of the bounds -- the one-pass variance and a mean 64 ulp off must both be caught."""
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import exact_ref as er
from tests.helpers import exact_stats as xs

mpmath = pytest.importorskip("mpmath")


def _cancelling(rows, n, seed):
    rng = np.random.default_rng(seed)
    return 1e6 + rng.normal(size=(rows, n)), (rng.random(n) < 0.4).astype(np.int32)


def test_group_moments_against_fractions_and_hand_cases():
    A, y = _cancelling(5, 37, 1)
    r = xs.group_moments(A, y)
    for grp in (0, 1):
        cols = np.flatnonzero(y == grp)
        for i in range(5):
            x = [Fraction(float(v)) for v in A[i, cols]]
            s = sum(x, Fraction(0))
            assert r["sum"][grp, i] == er.fraction_sum(A[i, cols])
            assert r["mean"][grp, i] == float(s / len(x))
            assert r["ssd"][grp, i] == float(sum(((v - s / len(x)) ** 2 for v in x), Fraction(0)))
            assert r["mag"][grp, i] == pytest.approx(np.abs(A[i, cols]).sum(), rel=1e-14)
    r = xs.group_moments(np.array([[1.0, 2.0, 4.0, 7.0], [np.nan, 1.0, np.inf, 3.0]]), np.array([0, 0, 1, 1]))
    assert r["sum"][0, 0] == 3.0 and np.isnan(r["sum"][0, 1]) and r["sum"][1, 1] == np.inf
    assert r["mean"][0, 0] == 1.5 and r["ssd"][0, 0] == 0.5 and r["mean"][1, 0] == 5.5 and r["ssd"][1, 0] == 4.5
    assert np.isnan(r["mean"][0, 1]) and np.isnan(r["ssd"][0, 1])
    assert r["mean"][1, 1] == np.inf and np.isnan(r["ssd"][1, 1])
    r = xs.group_moments(np.array([[1.0, 2.0]]), np.array([0, 0]))           # an empty group: NaN mean, the empty ssd
    assert np.isnan(r["mean"][1, 0]) and r["ssd"][1, 0] == 0.0 and r["n"].tolist() == [2, 0]


def _two_pass(A, y):
    """the device's operations in numpy: block partials of 128 columns, fl(1 / n_k), deviations from the rounded mean"""
    out_m, out_q = np.zeros((2, A.shape[0])), np.zeros((2, A.shape[0]))
    for grp in (0, 1):
        cols = np.flatnonzero(y == grp)
        s = np.zeros(A.shape[0])
        for b in range(0, A.shape[1], 128):
            part = np.zeros(A.shape[0])
            for c in cols[(cols >= b) & (cols < b + 128)]:
                part = part + A[:, c]
            s = s + part
        m = s * (1.0 / len(cols))
        q = np.zeros(A.shape[0])
        for c in cols:
            d = A[:, c] - m
            q = q + d * d
        out_m[grp], out_q[grp] = m, q
    return out_m, out_q


def test_bounds_hold_for_two_pass_and_catch_one_pass_and_a_shifted_mean():
    A, y = _cancelling(64, 300, 2)
    r = xs.group_moments(A, y)
    nk = r["n"][:, None].astype(np.float64)
    mb = xs.mean_bound(r["mag"], nk)
    qb = xs.ssd_bound(r["ssd"], nk, mb)
    m, q = _two_pass(A, y)
    er.assert_within(m, r["mean"], mb, "two-pass mean")
    er.assert_within(q, r["ssd"], qb, "two-pass ssd")
    # the one-pass form sum x^2 - n mean^2 in fp64 on the same data: outside the ssd bound nearly everywhere
    one = np.stack([(A[:, y == k] ** 2).sum(axis=1) - nk[k] * m[k] ** 2 for k in (0, 1)])
    assert er.bound_violations(one, r["ssd"], qb) > 0.9 * one.size
    # a mean 64 ulp off: outside the mean bound on well-conditioned data (bound ~ (n_k + 3) u |mean| / ... per element)
    rng = np.random.default_rng(3)
    B = rng.gamma(2.0, 1.0, size=(64, 9)) + 0.25
    yb = np.array([0, 1, 0, 1, 0, 1, 0, 1, 0])
    rb = xs.group_moments(B, yb)
    nb = rb["n"][:, None].astype(np.float64)
    off = rb["mean"] + 64 * np.spacing(rb["mean"])
    assert er.bound_violations(off, rb["mean"], xs.mean_bound(rb["mag"], nb)) == off.size
    er.assert_within(_two_pass(B, yb)[0], rb["mean"], xs.mean_bound(rb["mag"], nb), "well-conditioned mean")


def test_intervals_contain_the_50_digit_value_and_exclude_a_perturbed_one():
    iv = xs.welch_interval(0.1, 1e-15, 0.9, 1e-15, 30.0, 1e-13, 41.0, 1e-13, 25, 31)
    t, df = xs.welch_t_df(0.1, 0.9, 30.0, 41.0, 25, 31)
    p = float(xs.two_pt(abs(t), df))
    assert iv[0] <= p <= iv[1] and (iv[1] - iv[0]) / p < 1e-9
    assert not xs.in_interval(p * (1 + 1e-8), iv)
    assert xs.welch_interval(0.1, 0.0, 0.9, 0.0, 1e-20, 1e-19, 41.0, 0.0, 25, 31) is None          # the box reaches var <= 0
    assert xs.onesample_interval(5, 1.0, 0.0, 0.2, 1e-3) is None
    assert xs.clamp_p(float("nan")) == xs.P_HI and xs.clamp_p(0.0) == 1e-99


def _csr_two_pass(A, y):
    """csr_row_moments_kernel's operations in numpy on the rows of A (zeros are not stored): 64 lane sums of the stored
    values, a butterfly, s / n_k; stored deviations from the rounded mean the same way, then z * (m * m) added once"""
    rows = A.shape[0]
    out_m, out_q = np.zeros((2, rows)), np.zeros((2, rows))
    for grp in (0, 1):
        nk = float(np.sum(y == grp))
        for r in range(rows):
            v = A[r, (y == grp) & (A[r] != 0.0)]

            def lanes(x):
                acc = np.zeros(64)
                for k, t in enumerate(x):
                    acc[k % 64] += t
                o = 32
                while o >= 1:
                    acc = acc + acc[np.arange(64) ^ o]
                    o >>= 1
                return acc[0]

            m = lanes(v) / nk
            q = lanes((v - m) * (v - m))
            z = nk - len(v)
            out_m[grp, r], out_q[grp, r] = m, q + z * (m * m) if z > 0 else q
    return out_m, out_q


def test_csr_bounds_hold_for_the_implicit_zero_form():
    """MEAN_C_CSR and ssd_bound(implicit_zeros=True) on sparse rows (70 % implicit zeros) and on cancelling stored values"""
    rng = np.random.default_rng(8)
    for kind in ("gamma", "cancel"):
        A = rng.gamma(2.0, 1.0, size=(24, 200)) if kind == "gamma" else 1e6 + rng.normal(size=(24, 200))
        A[rng.random(A.shape) < 0.7] = 0.0
        A[3, :] = 0.0
        y = (rng.random(200) < 0.4).astype(np.int32)
        r = xs.group_moments(A, y)
        nk = r["n"][:, None].astype(np.float64)
        mb = xs.mean_bound(r["mag"], nk, xs.MEAN_C_CSR)
        m, q = _csr_two_pass(A, y)
        er.assert_within(m, r["mean"], mb, kind + " csr mean")
        er.assert_within(q, r["ssd"], xs.ssd_bound(r["ssd"], nk, mb, implicit_zeros=True), kind + " csr ssd")


@pytest.mark.parametrize("case", xs.CROSSPROD_CASES)
def test_no_set_of_the_gpu_cases_is_not_separable(case):
    """the zero-exclusion condition of the p.one / p.two GPU test, from the reference alone: for its exact seeds and
    shapes every set's error box stays inside var > 0, and the intervals are narrow enough to mean something"""
    X, y, Gp, Gi = xs.crossprod_case(*case)
    ivs = xs.crossprod_intervals(X, y, Gp, Gi)
    assert sum(a is None for a, _ in ivs) == 0 and sum(b is None for _, b in ivs) == 0
    for a, b in ivs:
        assert a[1] - a[0] <= 1e-6 * a[1] and b[1] - b[0] <= 1e-6 * b[1]
