"""The reference of replaid.ssgsea.exact(single = FALSE) (tests/helpers/gsea_ks_walk.py), host only.

The literal walk over all N positions, the 2k-candidate form pinned in include/plaidhip.h and the same operations in exact
rationals must agree bit for bit at alpha 0 and 1, where every sum is exact; the first of two equal extremes wins; norm
and NaN follow replaid.ssgsea.exact's rules.
"""
import numpy as np
import pytest

from tests.helpers import gsea_ks_walk as kw


def _tied(g, n, seed=3):
    rng = np.random.default_rng(seed)
    X = np.round(rng.normal(0, 2, size=(g, n)), 0)
    X[rng.random((g, n)) < 0.05] = -0.0
    if n > 1:
        X[:, 1] = 4.0                                       # an all-equal column: the walk is the row order
    return X


def _sets(g, sizes, seed=11):
    rng = np.random.default_rng(seed)
    Gi, Gp = [], [0]
    for k in sizes:
        Gi.extend(sorted(rng.choice(g, size=min(k, g), replace=False)))
        Gp.append(len(Gi))
    return np.array(Gp, dtype=np.int32), np.array(Gi, dtype=np.int32)


def _same_bits(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    ok = ~np.isnan(a)
    assert np.array_equal(a[ok].view(np.int64), b[ok].view(np.int64)), what


@pytest.mark.parametrize("g,n", [(1, 3), (5, 4), (97, 9), (601, 5)])
@pytest.mark.parametrize("alpha", [0.0, 1.0])
@pytest.mark.parametrize("scale", [True, False])
def test_walk_candidates_and_rationals_agree_bit_for_bit(g, n, alpha, scale):
    X = _tied(g, n)
    Gp, Gi = _sets(g, [0, 1, 2, max(g - 1, 0), g, 7, 40, 300])
    cand = kw.candidates_max_dev(X, Gp, Gi, alpha, scale)
    _same_bits(kw.walk_max_dev(X, Gp, Gi, alpha, scale), cand, "walk vs candidates")
    if g <= 97:
        _same_bits(kw.fraction_max_dev(X, Gp, Gi, alpha, scale), cand, "rationals vs candidates")
    k = np.diff(Gp)
    assert np.isnan(cand[(k == 0) | (k == g)]).all()
    assert not np.isnan(cand[(k > 0) & (k < g)]).any()


@pytest.mark.parametrize("alpha", [0.25, 0.5, 2.0])
def test_other_alphas_agree_closely(alpha):
    X = _tied(97, 9)
    Gp, Gi = _sets(97, [1, 2, 96, 7, 40])
    a = kw.walk_max_dev(X, Gp, Gi, alpha)
    b = kw.candidates_max_dev(X, Gp, Gi, alpha)
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-15)


def test_equal_extremes_return_the_earlier_one():
    X = np.array([[4.0], [3.0], [2.0], [1.0]])              # row i is visited at position i + 1
    Gp = np.array([0, 2, 4], dtype=np.int32)
    Gi = np.array([0, 3, 1, 2], dtype=np.int32)
    # {0, 3}: hit, miss, miss, hit -> 0.5, 0, -0.5, 0;  {1, 2}: miss, hit, hit, miss -> -0.5, 0, 0.5, 0
    for fn in (kw.walk_max_dev, kw.candidates_max_dev, kw.fraction_max_dev):
        S = fn(X, Gp, Gi, 0.0, False)
        assert S[:, 0].tolist() == [0.5, -0.5], fn.__name__
        S = fn(X, Gp, Gi, 0.0, True)
        assert S[:, 0].tolist() == [0.125, -0.125], fn.__name__


def test_a_set_at_the_top_scores_one_and_at_the_bottom_minus_one():
    X = np.arange(10, 0, -1.0)[:, None]
    Gp = np.array([0, 3, 6], dtype=np.int32)
    Gi = np.array([0, 1, 2, 7, 8, 9], dtype=np.int32)
    S = kw.candidates_max_dev(X, Gp, Gi, 0.0, False)
    assert S[:, 0].tolist() == [1.0, -1.0]


def test_norm_and_nan_rules():
    X = _tied(97, 9)
    Gp, Gi = _sets(97, [1, 2, 7, 40, 96])
    plain = kw.candidates_max_dev(X, Gp, Gi, 0.25)
    _same_bits(kw.candidates_max_dev(X, Gp, Gi, 0.25, True, True), plain / (plain.max() - plain.min()), "norm")
    X[5, 3] = np.nan
    S = kw.candidates_max_dev(X, Gp, Gi, 0.0)
    assert np.isnan(S[:, 3]).all() and not np.isnan(np.delete(S, 3, axis=1)).any()
    assert np.isnan(kw.walk_max_dev(X, Gp, Gi, 0.0)[:, 3]).all()
    assert np.isnan(kw.candidates_max_dev(X, Gp, Gi, 0.0, True, True)).all()
    S, dmax, dmin = kw.candidates_max_dev(X, Gp, Gi, 0.25, with_extremes=True)
    ok = ~np.isnan(S)
    assert (np.abs(S[ok]) == np.maximum(dmax[ok], -dmin[ok])).all()
