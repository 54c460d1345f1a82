"""The references of replaid.gsva.exact against each other (host only): GSVA's literal walk, the pinned form of
include/plaidhip.h in numpy and the same operations in exact rationals (tests/helpers/gsva_walk.py); and the Python
entry's export and argument checks, which need no device."""
import numpy as np
import pytest

from tests.helpers import exact_ref as er
from tests.helpers import gsva_walk as gw

U = 2.0 ** -53


def _sized_sets(g, sizes, seed=17):
    rng = np.random.default_rng(seed)
    Gi, Gp = [], [0]
    for k in sizes:
        Gi.extend(sorted(rng.choice(g, size=k, replace=False)))
        Gp.append(len(Gi))
    return np.array(Gp, dtype=np.int32), np.array(Gi, dtype=np.int32)


def _tied(g, n, seed=3):
    """heavy ties, -0.0 beside 0.0, an all-equal column"""
    rng = np.random.default_rng(seed)
    X = np.round(rng.normal(0, 2, size=(g, n)), 0)
    X[rng.random((g, n)) < 0.05] = -0.0
    if n > 1:
        X[:, 1] = 4.0
    return X


@pytest.mark.parametrize("N", [60, 97, 512])
@pytest.mark.parametrize("tau", [0.0, 1.0])
def test_pinned_form_equals_exact_rationals_bit_for_bit(N, tau):
    V = _tied(N, 5)
    sizes = [k for k in (1, 2, 63, 64, 65, N // 2, N - 1) if 0 < k < N] + [0, N]
    Gp, Gi = _sized_sets(N, sizes)
    # the centre gene alone (even N: zero weight at tau > 0 -> NaN), for the first column
    centre = int(np.flatnonzero(gw.positions(V)[0][:, 0] == N + 1 - N // 2)[0])
    Gp = np.append(Gp, Gp[-1] + 1).astype(np.int32)
    Gi = np.append(Gi, centre).astype(np.int32)
    for max_diff in (True, False):
        b = gw.pinned(V, Gp, Gi, tau, max_diff)
        c = gw.fraction_pinned(V, Gp, Gi, tau, max_diff)
        er.assert_same_bits(b, c, f"N={N} tau={tau} max_diff={max_diff}")
        assert np.isnan(b[-3:-1]).all()                            # k = 0 and k = N
        assert np.isnan(b[-1, 0]) == (tau > 0 and N % 2 == 0)      # B == 0


@pytest.mark.parametrize("N", [60, 97, 512, 3001])
@pytest.mark.parametrize("tau", [0.0, 0.5, 1.0])
def test_pinned_form_against_the_literal_walk(N, tau):
    """Bound 2 (N + 8) u.  The literal running sum makes N additions of values of magnitude at most 1 (at most u each)
    plus the rounded increments (at most 2 u in total) per extreme; the pinned candidate makes three roundings; the score
    adds two extremes.  max_diff = FALSE: the magnitudes within the same bound, the sign equal wherever |mx_pos + mx_neg|
    exceeds it; the pairs below that are exempt from the sign check alone and may be at most 5 % of the finite pairs."""
    rng = np.random.default_rng(N)
    n = 6 if N < 1000 else 3
    V = np.round(rng.normal(0, 30, size=(N, n)), 0)
    Gp, Gi = _sized_sets(N, [int(k) for k in rng.integers(1, max(2, N // 4) + 1, size=30 if N < 1000 else 12)], seed=N + 1)
    bound = 2 * (N + 8) * U
    a = gw.literal_walk(V, Gp, Gi, tau, True)
    b, mxp, mxn = gw.pinned(V, Gp, Gi, tau, True, with_extremes=True)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    fin = ~np.isnan(a)
    print(f"N={N} tau={tau} max_diff=TRUE: worst |b - a| / bound = {np.abs(b[fin] - a[fin]).max() / bound:.3g}")
    assert (np.abs(b[fin] - a[fin]) <= bound).all()
    a0 = gw.literal_walk(V, Gp, Gi, tau, False)
    b0 = gw.pinned(V, Gp, Gi, tau, False)
    assert np.array_equal(np.isnan(a0), np.isnan(b0))
    err = np.abs(np.abs(b0[fin]) - np.abs(a0[fin]))
    assert (err <= bound).all()
    decided = fin & (np.abs(mxp + mxn) > bound)
    share = 1.0 - decided.sum() / fin.sum()
    print(f"N={N} tau={tau} max_diff=FALSE: worst / bound = {err.max() / bound:.3g}, exempt from the sign check {100 * share:.2f} %")
    assert share <= 0.05
    assert np.array_equal(np.sign(b0[decided]), np.sign(a0[decided]))


def test_equal_magnitudes_return_the_negative_extreme():
    V = np.array([[4.0], [3.0], [2.0], [1.0]])
    Gp = np.array([0, 2], dtype=np.int32)
    Gi = np.array([0, 3], dtype=np.int32)                          # first and last: +0.5 then -0.5
    assert gw.pinned(V, Gp, Gi, 0.0, False)[0, 0] == -0.5
    assert gw.literal_walk(V, Gp, Gi, 0.0, False)[0, 0] == -0.5
    assert gw.pinned(V, Gp, Gi, 0.0, True)[0, 0] == 0.0


def test_python_entry_is_exported_and_checks_its_arguments_without_a_device():
    import plaid_amd
    assert "replaid_gsva_exact" in plaid_amd.__all__ and callable(plaid_amd.replaid_gsva_exact)
    assert "gsva_exact_multi" in plaid_amd.__all__ and hasattr(plaid_amd.Context, "gsva_exact")
    X = plaid_amd.NamedMatrix(np.ones((4, 2)), ["a", "b", "c", "d"], ["s1", "s2"])
    G = plaid_amd.NamedMatrix(np.eye(4)[:, :2], ["a", "b", "c", "d"], ["set1", "set2"])
    for tau in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tau must be finite and >= 0"):
            plaid_amd.replaid_gsva_exact(X, G, tau=tau)
        with pytest.raises(ValueError, match="tau must be finite and >= 0"):
            plaid_amd.gsva_exact_multi(X.values, [0, 1, 2], [0, 1], tau=tau)
    with pytest.raises(ValueError, match="unknown row transform"):
        plaid_amd.replaid_gsva_exact(X, G, rowtf="kcdf")
    with pytest.raises(ValueError, match="unknown row transform"):
        plaid_amd.gsva_exact_multi(X.values, [0, 1, 2], [0, 1], rowtf="kcdf")
