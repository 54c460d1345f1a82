"""The host forms of replaid.ucell.exact and replaid.aucell.exact agree among themselves (tests/helpers/truncated_exact.py):
closed forms against literal forms in exact rationals, the numpy form against the rationals, the shifted-weight identity of
sparse columns, and a negative control for UCell's truncation rule.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import truncated_exact as te

SMALL = (63, 64, 65, 257)


def _members(Gp, Gi, j):
    return [int(i) for i in Gi[Gp[j]:Gp[j + 1]]]


@pytest.mark.parametrize("N", SMALL)
def test_closed_forms_equal_the_literal_forms(N):
    names, X, Gp, Gi = te.case(N)
    for c, name in enumerate(names):
        if name == "nan":
            continue
        x = X[:, c]
        for T in te.rank_values(N):
            for j in range(len(Gp) - 1):
                mem = _members(Gp, Gi, j)
                for K in (None, len(mem) + 3):
                    assert te.ucell_closed_fraction(x, mem, T, K) == te.ucell_literal_fraction(x, mem, T, K), (name, T, j, K)
                assert te.aucell_closed_fraction(x, mem, T) == te.aucell_literal_fraction(x, mem, T), (name, T, j)


@pytest.mark.parametrize("N", (63, 257))
def test_numpy_forms_are_the_rounded_rationals(N):
    """one division of exact integers: the fp64 result is the correctly rounded rational"""
    names, X, Gp, Gi = te.case(N)
    for T in te.rank_values(N):
        U = te.ucell_exact(X, Gp, Gi, T)
        A = te.aucell_exact(X, Gp, Gi, T)
        for c, name in enumerate(names):
            for j in range(len(Gp) - 1):
                mem = _members(Gp, Gi, j)
                if name == "nan":
                    assert np.isnan(U[j, c]) and np.isnan(A[j, c])
                    continue
                f = te.ucell_closed_fraction(X[:, c], mem, T)
                # 1 - q: q = U2 / (2 K T) rounded once, then one subtraction
                if f is None:
                    assert np.isnan(U[j, c])
                else:
                    q = float(1 - f) if f > 0 else None
                    if q is not None:
                        assert U[j, c] == 1.0 - q, (name, T, j)
                    else:
                        assert U[j, c] == 0.0
                f = te.aucell_closed_fraction(X[:, c], mem, T)
                if f is None:
                    assert np.isnan(A[j, c])
                else:
                    assert A[j, c] == float(f), (name, T, j)


@pytest.mark.parametrize("N", SMALL)
def test_shifted_weights_of_sparse_columns_give_the_dense_sums(N):
    """sum u over a set = sum of the stored non-zero entries' (u - u0) + k u0, and the lists hold what the dense lists hold"""
    names, X, Gp, Gi = te.case(N)
    rng = np.random.default_rng(5)
    Xs = te.to_csc(X, rng, explicit=0.05)
    shifted = 0
    for T in te.rank_values(N):
        lists, u0 = te.csc_lists(Xs, "ucell", T)
        dense = te.dense_lists(X, "ucell", T)
        for c, name in enumerate(names):
            if name == "nan":
                assert len(lists[c][0]) == 0
                continue
            w = np.full(N, u0[c])
            rows, vals = lists[c]
            w[rows] += vals
            full = np.zeros(N)
            full[dense[c][0]] = dense[c][1]
            assert np.array_equal(w, full), (name, T)
            assert (np.diff(rows) > 0).all()
            shifted += u0[c] > 0
            for j in range(len(Gp) - 1):
                mem = np.asarray(_members(Gp, Gi, j), dtype=np.int64)
                pos = {int(r): float(v) for r, v in zip(rows, vals)}
                assert sum(pos.get(int(i), 0.0) for i in mem) + len(mem) * u0[c] == full[mem].sum()
        al, _ = te.csc_lists(Xs, "aucell", T)
        ad = te.dense_lists(X, "aucell", T)
        for c in range(len(names)):
            assert np.array_equal(al[c][0], ad[c][0]) and np.array_equal(al[c][1], ad[c][1])
    assert shifted > 0, "no column whose zeros are weighted"


def test_pmin_is_not_ucells_rule():
    """the boundary tie group whose average rank is T + 0.5: UCell drops it as a whole (c = T + 1), pmin(d, T + 1) keeps
    T + 0.5 and the score moves"""
    N, T = 65, te.K_SET
    names, X, Gp, Gi = te.case(N)
    c = names.index("tie_half_above_T")
    x = X[:, c]
    group = np.nonzero(x == 50.0)[0]
    Gp1 = np.asarray([0, len(group)], dtype=np.int32)
    a = te.ucell_exact(x[:, None], Gp1, group.astype(np.int32), T)
    b = te.ucell_exact(x[:, None], Gp1, group.astype(np.int32), T, rule="pmin")
    assert a[0, 0] == 0.0 or a[0, 0] < b[0, 0]
    assert a[0, 0] != b[0, 0]
    assert te.ucell_closed_fraction(x, list(group), T) == te.ucell_literal_fraction(x, list(group), T)
    assert te.ucell_closed_fraction(x, list(group), T, rule="pmin") != te.ucell_literal_fraction(x, list(group), T)
    # at exactly T the group is weighted under both rules
    x = X[:, names.index("tie_at_T")]
    group = np.nonzero(x == 50.0)[0]
    assert (te.ucell_weights2(x, T)[group] == 2).all()
    assert np.array_equal(te.ucell_weights2(x, T), te.ucell_weights2(x, T, "pmin"))


@pytest.mark.parametrize("N", (65, 257))
def test_the_scores_are_not_all_alike(N):
    """the reference the GPU tests hold the device to tells the cases apart: weighted zeros, dropped and kept tie groups"""
    names, X, Gp, Gi = te.case(N)
    Xs = te.to_csc(X, np.random.default_rng(N), explicit=0.03)
    T = te.K_SET
    _, u0 = te.csc_lists(Xs, "ucell", N)
    assert u0[names.index("counts")] > 0 and u0[names.index("zero")] > 0
    _, u0 = te.csc_lists(Xs, "ucell", T)
    assert u0[names.index("counts")] == 0
    for name, kept in (("tie_at_T", True), ("tie_half_above_T", False), ("tie_above_T", False)):
        x = X[:, names.index(name)]
        assert (te.ucell_weights2(x, T)[x == 50.0] > 0).all() == kept


def test_total_and_clamps():
    up = np.array([0.5, 0.25, 0.25, np.nan, 0.5])
    down = np.array([0.25, 0.5, 0.25, 0.1, np.nan])
    assert np.array_equal(te.ucell_total(up, down, 1.0)[:3], [0.25, 0.0, 0.0])
    assert np.isnan(te.ucell_total(up, down, 1.0)[3:]).all()
    assert np.isnan(te.ucell_total(up, down, 0.0)[4])          # 0 * NaN: an empty down column makes total NaN
    assert te.ucell_total(np.array([0.25]), np.array([0.5]), 0.5)[0] == 0.0
    assert te.ucell_total(np.array([0.2500000000000001]), np.array([0.5]), 0.5)[0] > 0.0
    # auc is 0 exactly for one unweighted gene (U2 = 2 K T) and cannot go below with K >= k
    assert te.ucell_from_s2(0, 1, 1, 7) == 0.0
    assert te.ucell_from_s2(1, 1, 1, 7) == 1.0 - 13.0 / 14.0
    assert np.isnan(te.ucell_from_s2(0, 0, 0, 7))
    assert np.isnan(te.aucell_from_area(0, 0, 5)) and np.isnan(te.aucell_from_area(0, 3, 1))
    assert Fraction(te.aucell_from_area(6, 3, 4)) == 1
