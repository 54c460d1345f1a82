"""The exact references of tests/helpers/exact_ref.py have teeth and are not flaky (host only).

- set_sums equals fractions.Fraction sums rounded once, also where the terms cancel and span 1e+-300
- the fp64 bound accepts fp64 sums of the same terms in shuffled, pairwise and reversed order
- on well-conditioned sums it rejects fp32-rounded inputs, a dropped term of relative size 1e-10 and a 1 + 1e-12 scale
- col_medians is np.median where both are defined, and finite for two middle values near DBL_MAX
"""
import numpy as np
import pytest

from tests.helpers import exact_ref as er


def _csc(sets):
    Gp = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    Gi = np.concatenate([np.asarray(s, dtype=np.int64) for s in sets]).astype(np.int32)
    return Gp, Gi


def test_two_sum_and_two_prod_are_error_free():
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a = rng.normal(size=2000) * 10.0 ** rng.integers(-30, 30, size=2000)
    b = rng.normal(size=2000) * 10.0 ** rng.integers(-30, 30, size=2000)
    s, e = er.two_sum(a, b)
    p, f = er.two_prod(a, b)
    for i in range(0, 2000, 37):
        assert Fraction(s[i]) + Fraction(e[i]) == Fraction(a[i]) + Fraction(b[i])
        assert Fraction(p[i]) + Fraction(f[i]) == Fraction(a[i]) * Fraction(b[i])


def test_set_sums_equal_fraction_sums_rounded_once():
    cases = [
        [1e16, 1.0, -1e16],
        [1e300, 1e-300, -1e300, 3.0, -3.0],
        [1e-300, -1e300, 2.5, 1e300, -1e-300, 7e-310],
        [0.1] * 10 + [-1.0],
        [2.0 ** 53, 1.0, 1.0, -(2.0 ** 53)],
        [1e308, -1e308, 1e-308, 5e-324],
        [3.0, -3.0],
    ]
    rng = np.random.default_rng(1)
    for _ in range(40):                                   # mixed signs over 1e+-300
        k = int(rng.integers(1, 60))
        cases.append(list(rng.choice([-1.0, 1.0], size=k) * rng.random(k) * 10.0 ** rng.integers(-300, 300, size=k)))
    for _ in range(40):                                   # heavy cancellation at one scale
        x = rng.normal(size=50) * 1e6
        cases.append(list(x) + list(-x[:49]) + [rng.normal()])
    g = max(len(c) for c in cases)
    X = np.zeros((g, len(cases)))
    sets = []
    for j, c in enumerate(cases):
        X[: len(c), j] = c
    # one sample column per case: set j = the rows of case j, evaluated at every column; check the diagonal
    for j, c in enumerate(cases):
        sets.append(np.arange(len(c)))
    Gp, Gi = _csc(sets)
    ref, mag, k = er.set_sums(Gp, Gi, X)
    for j, c in enumerate(cases):
        assert ref[j, j] == er.fraction_sum(c), (j, c)
        assert k[j, j] == sum(1 for t in c if t != 0.0)
        assert mag[j, j] == pytest.approx(sum(abs(t) for t in c), rel=1e-12)


def test_weighted_set_sums_use_exact_products():
    from fractions import Fraction
    rng = np.random.default_rng(2)
    g, n = 300, 4
    X = rng.normal(size=(g, n)) * 1e3 + np.where(rng.random((g, n)) < 0.5, 1e6, -1e6)
    sets = [np.sort(rng.choice(g, size=int(s), replace=False)) for s in (1, 2, 17, 150, 300)]
    Gp, Gi = _csc(sets)
    w = rng.normal(size=len(Gi)) * (1.0 + 1e-9 * rng.random(len(Gi)))
    ref, _, _ = er.set_sums(Gp, Gi, X, weights=w)
    for j in range(len(sets)):
        for c in range(n):
            ex = sum((Fraction(float(w[t])) * Fraction(float(X[Gi[t], c])) for t in range(Gp[j], Gp[j + 1])), Fraction(0))
            assert ref[j, c] == float(ex)
    scale = np.array([0.1, 1.0 / 3.0, 7.0, 1e-8, 2.5])
    ref2, mag2, _ = er.set_sums(Gp, Gi, X, set_scale=scale)
    for j in range(len(sets)):
        for c in range(n):
            ex = sum((Fraction(float(scale[j])) * Fraction(float(X[Gi[t], c])) for t in range(Gp[j], Gp[j + 1])), Fraction(0))
            assert ref2[j, c] == float(ex)
    assert np.all(mag2 > 0)


def test_set_sums_propagate_nan_and_inf_like_ieee():
    X = np.array([[1.0, np.nan, np.inf, np.inf, -np.inf, 1e300],
                  [2.0, 1.0, 1.0, -np.inf, 1.0, 1e-300],
                  [3.0, 1.0, np.inf, 2.0, -np.inf, -1e300]])
    Gp, Gi = _csc([[0, 1, 2], [1, 2], []])
    ref, mag, k = er.set_sums(Gp, Gi, X)
    assert np.array_equal(ref[0, :5], [6.0, np.nan, np.inf, np.nan, -np.inf], equal_nan=True)
    assert ref[0, 5] == 1e-300                            # the fp64 sum in this order gives 0
    assert np.array_equal(ref[1, :5], [5.0, 2.0, np.inf, -np.inf, -np.inf]) and ref[1, 5] == -1e300 + 1e-300
    assert np.all(ref[2] == 0.0) and np.all(k[2] == 0) and np.all(mag[2] == 0.0)


def _well_conditioned(seed, g=4000, n=6, m=120):
    rng = np.random.default_rng(seed)
    X = rng.gamma(2.0, 1.0, size=(g, n)) + 0.5
    sets = [np.sort(rng.choice(g, size=int(s), replace=False)) for s in rng.integers(2, 500, size=m)]
    Gp, Gi = _csc(sets)
    return X, Gp, Gi, sets


def _fp64_sums(X, sets, how, rng):
    out = np.empty((len(sets), X.shape[1]))
    for j, s in enumerate(sets):
        t = X[s, :]
        if how == "shuffled":
            t = t[rng.permutation(len(s))]
            acc = np.zeros(X.shape[1])
            for row in t:
                acc = acc + row
            out[j] = acc
        elif how == "reversed":
            acc = np.zeros(X.shape[1])
            for row in t[::-1]:
                acc = acc + row
            out[j] = acc
        else:                                             # pairwise (numpy's blocked tree)
            out[j] = np.add.reduce(t, axis=0)
    return out


@pytest.mark.parametrize("how", ["shuffled", "reversed", "pairwise"])
def test_bound_accepts_fp64_sums_in_any_order(how):
    rng = np.random.default_rng(3)
    X, Gp, Gi, sets = _well_conditioned(3)
    ref, mag, k = er.set_sums(Gp, Gi, X)
    er.assert_fp64_bound(_fp64_sums(X, sets, how, rng), ref, mag, k, 0, how)
    # cancelling data: +-1e6 offsets that cancel to O(1)
    Xc = np.where(rng.random(X.shape) < 0.5, 1e6, -1e6) + rng.normal(size=X.shape)
    ref, mag, k = er.set_sums(Gp, Gi, Xc)
    assert np.median(mag / np.maximum(np.abs(ref), 1e-300)) > 10.0     # ill-conditioned: mag >> |sum|
    er.assert_fp64_bound(_fp64_sums(Xc, sets, how, rng), ref, mag, k, 0, how)
    # a scaled epilogue: fl(fl(sum) * w) is two more roundings on the fp64 side
    w = 1.0 / (1e-8 + np.diff(Gp).astype(float))
    got = _fp64_sums(X, sets, how, rng) * w[:, None]
    ref, mag, k = er.set_sums(Gp, Gi, X)
    er.assert_fp64_bound(got, ref * w[:, None], mag * w[:, None], k, 3, how)


def test_bound_rejects_fp32_inputs_dropped_terms_and_scaling():
    X, Gp, Gi, sets = _well_conditioned(4)
    ref, mag, k = er.set_sums(Gp, Gi, X)
    rng = np.random.default_rng(4)
    exact = _fp64_sums(X, sets, "pairwise", rng)
    er.assert_fp64_bound(exact, ref, mag, k, 0)
    # inputs staged through fp32
    f32 = _fp64_sums(X.astype(np.float32).astype(np.float64), sets, "pairwise", rng)
    assert er.fp64_bound_violations(f32, ref, mag, k, 3) > 0.5 * ref.size
    # one term of relative size 1e-10 dropped from every sum: one extra gene in every set, then left out
    Xt = np.vstack([X, 1e-10 * mag.mean(axis=0)[None, :]])
    extra = [np.append(s, X.shape[0]) for s in sets]
    Gpe, Gie = _csc(extra)
    ref_e, mag_e, k_e = er.set_sums(Gpe, Gie, Xt)
    er.assert_fp64_bound(_fp64_sums(Xt, extra, "pairwise", rng), ref_e, mag_e, k_e, 0)
    assert er.fp64_bound_violations(exact, ref_e, mag_e, k_e, 3) == ref.size
    # a result scaled by 1 + 1e-12
    assert er.fp64_bound_violations(exact * (1.0 + 1e-12), ref, mag, k, 3) == ref.size


def test_bound_demands_identical_nan_and_inf_patterns():
    ref = np.array([1.0, np.nan, np.inf, -np.inf, 0.0])
    mag = np.ones(5)
    k = np.ones(5, dtype=np.int64)
    er.assert_fp64_bound(ref.copy(), ref, mag, k, 0)
    for i, v in ((0, np.nan), (1, 1.0), (2, -np.inf), (3, np.nan), (4, np.inf)):
        got = ref.copy()
        got[i] = v
        assert er.fp64_bound_violations(got, ref, mag, k, 0) == 1


def test_col_medians_matches_numpy_and_r_rules():
    rng = np.random.default_rng(5)
    for m in (1, 2, 3, 10, 11, 1000, 1001):
        S = np.round(rng.normal(size=(m, 7)), 1)
        S[rng.random(S.shape) < 0.2] = 0.0
        S[:, 3] = np.abs(S[:, 3])
        med = er.col_medians(S, False)
        assert np.array_equal(med, np.median(S, axis=0) + 0.0)
        with np.errstate(all="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                nz = np.nanmedian(np.where(S == 0.0, np.nan, S), axis=0)
        assert np.array_equal(er.col_medians(S, True), np.where(np.isnan(nz), 0.0, nz) + 0.0)
    S = np.array([[1.0, np.nan, 0.0], [np.nan, np.nan, -0.0], [3.0, np.nan, 0.0]])
    assert np.array_equal(er.col_medians(S, False), [2.0, np.nan, 0.0], equal_nan=True)
    assert np.array_equal(er.col_medians(S, True), [2.0, 0.0, 0.0])
    assert er.resolve_ignore_zero(np.array([[-0.0, 1.0]])) is True         # min(x) == 0 holds for -0.0
    assert er.resolve_ignore_zero(np.array([[-1e-300, 0.0]])) is False
    assert er.resolve_ignore_zero(np.array([[np.nan, 0.0, 2.0]])) is True   # na.rm = TRUE
    assert er.bits(er.col_medians(np.array([[-0.0], [-0.0], [1.0]]), False))[0] == 0   # a zero median is +0.0


def test_col_medians_midpoint_near_dbl_max_is_finite():
    big = np.finfo(np.float64).max
    a, b = np.nextafter(big, 0.0), big
    S = np.array([[a, -a, a, 1.0], [b, -b, b, np.inf], [0.5 * b, -0.5 * b, np.inf, 1.0], [b, -b, np.inf, np.inf]])
    med = er.col_medians(S, False)
    assert np.isfinite(med[:2]).all()
    from fractions import Fraction
    assert med[0] == float((Fraction(a) + Fraction(b)) / 2) and med[1] == -med[0]
    assert med[2] == np.inf and med[3] == np.inf
    with np.errstate(over="ignore"):
        assert 0.5 * (a + b) == np.inf                    # what the plain formula gives
    # the oracles agree
    from oracle import c_oracle, plaid_oracle
    assert np.array_equal(plaid_oracle.normalize_medians(S, False)[1], med)
    assert np.array_equal(c_oracle.normalize_medians(S, False)[1], med)
