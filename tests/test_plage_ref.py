"""tests/helpers/plage_ref.py against itself and numpy, without a GPU: the numpy restatement of the pinned PLAGE (power
iteration from the max-norm column, the orientation rule) is held to numpy.linalg.svd oriented by the same rule -- each
row certified against the extended-precision block, never trusted -- and the zscore restatement to 50-digit arithmetic
within the forward bound the GPU test uses."""
import numpy as np
import pytest

from tests.helpers import plage_ref as ref

SIZES = [1, 2, 3, 16, 17, 65, 257]
SAMPLES = [2, 3, 4, 65, 130]


def block(k, n, seed=0):
    rng = np.random.default_rng(1000 * k + n + seed)
    X, a = ref.planted(rng, k, n)
    return X + rng.normal(size=(k, 1)) * 3.0, a   # (row offsets: the standardization has something to remove)


def pair(sign, n=65):
    rng = np.random.default_rng(7 + n)
    f = rng.normal(size=n)
    return np.vstack([f + 0.3 * rng.normal(size=n), sign * f + 0.3 * rng.normal(size=n)])


@pytest.mark.parametrize("n", SAMPLES)
@pytest.mark.parametrize("k", SIZES)
def test_restatement_meets_the_oriented_svd_within_the_certified_angles(k, n):
    X, _ = block(k, n)
    Z, flag = ref.standardize(X)
    assert (flag == 0).all()
    Zl = ref.standardize_ld(X)
    r = ref.plage_set(Z)
    v_np, u_np, s2 = ref.svd_row(Z)
    c_dev, c_np = ref.certify(Zl, r["v"]), ref.certify(Zl, v_np)
    assert r["converged"] == 1 and r["residual"] <= ref.TOL and r["iterations"] <= 1000
    if c_dev["gap"] > 0 and c_np["gap"] > 0 and max(c_dev["sin"], c_np["sin"]) < 1:
        angle = np.arcsin(float(c_dev["sin"])) + np.arcsin(float(c_np["sin"]))
        assert float(np.linalg.norm(c_dev["w"] - c_np["w"])) <= angle + 8 * ref.U, (k, n, angle)
    else:   # (no separation to certify with, n = 3 at the most: the rows agree up to the gap-limited accuracy)
        assert n <= 4
        assert abs(abs(float(c_dev["w"] @ c_np["w"])) - 1) < 1e-6
    assert abs(r["lambda"] - s2) <= 1e-9 * s2
    assert abs(float(c_dev["norm"]) - 1) < 1e-12
    assert ref.orient(r["u"]) == 1.0 and ref.orient(u_np) == 1.0


def test_one_member_is_its_own_vector():
    X, _ = block(1, 65)
    Z, _ = ref.standardize(X)
    r = ref.plage_set(Z)
    assert r["iterations"] == 1 and r["converged"] == 1 and r["residual"] == 0.0
    assert r["u"].tolist() == [1.0] and r["lambda"] == ref.gram(Z)[0, 0]
    np.testing.assert_array_equal(r["v"], Z[0] / np.sqrt(r["lambda"]))


def test_pairs_and_the_orientation_rule():
    pos = ref.plage_set(ref.standardize(pair(+1.0))[0])
    assert pos["u"].sum() > 0 and (pos["u"] > 0).all()
    neg = ref.plage_set(ref.standardize(pair(-1.0))[0])
    assert neg["u"][0] > 0 > neg["u"][1]                       # sum u ~ 0: member 0 is made positive
    assert neg["explained"] > 0.9 and neg["converged"] == 1    # (the all-ones start would have stopped on lambda_2)
    ones = np.ones(2) / np.sqrt(2.0)
    C = ref.gram(ref.standardize(pair(-1.0))[0])
    assert float(ones @ C @ ones) < 0.1 * np.trace(C)
    mixed, a = block(17, 65)
    r = ref.plage_set(ref.standardize(mixed)[0])
    assert r["u"].sum() > 0 and (np.sign(r["u"]) == np.sign(a)).all()   # a quarter of the planted loadings is negative
    assert ref.orient([0.5, -0.5]) == 1.0 and ref.orient([-0.5, 0.5]) == -1.0 and ref.orient([-0.1, 0.7, -0.7]) == -1.0
    assert ref.orient([-0.6, -0.8]) == -1.0


def test_orthogonal_pair_keeps_the_start():
    X = np.array([[1.0, -1.0, 1.0, -1.0], [1.0, 1.0, -1.0, -1.0]])
    r = ref.plage_set(ref.standardize(X)[0])
    assert r["residual"] == 0.0 and r["iterations"] == 1 and abs(np.linalg.norm(r["v"]) - 1) < 4 * ref.U
    assert r["u"].tolist() == [1.0, 0.0]


def test_constant_and_flagged_rows():
    rng = np.random.default_rng(5)
    X = rng.normal(size=(6, 9))
    X[1, :] = 2.5
    X[4, 3] = np.nan
    X[5, 0] = np.inf
    _, _, flag = ref.moments(X)
    assert flag.tolist() == [0, 1, 0, 0, 2, 2]
    Gp, Gi = np.array([0, 3, 4, 6, 8]), np.array([2, 1, 0, 1, 0, 4, 5, 3])
    S, info, L = ref.plage(X, Gp, Gi)
    assert info[:, 0].tolist() == [2, 0, 2, 2]
    assert np.isfinite(S[0]).all() and np.isnan(S[1:]).all()
    assert L[1] == 0.0 and L[3] == 0.0 and np.isnan(L[4:8]).all()
    Sz, size = ref.zscore(X, Gp, Gi)
    assert size.tolist() == [2, 0, 2, 2] and np.isfinite(Sz[0]).all() and np.isnan(Sz[1:]).all()


@pytest.mark.parametrize("k,n", [(1, 2), (3, 3), (17, 65), (65, 130)])
def test_zscore_restatement_lies_within_the_forward_bound(k, n):
    X, _ = block(k, n, seed=3)
    S, size = ref.zscore(X, np.array([0, k]), np.arange(k))
    exact = ref.zscore_exact(X, range(k))
    bound = ref.zscore_bound(X, np.arange(k), k, exact)
    err = np.array([abs(float(e - float(s))) for e, s in zip(exact, S[0])])
    assert size[0] == k and (err <= bound).all() and bound.max() < 1e-9
