"""replaid.zscore on the device (plaidhip_zscore, kernels_plage.hip) against 50-digit arithmetic on the
same fp64 inputs, within the forward bound of tests/helpers/plage_ref.py (zscore_bound: the moments, z, the k-term sum in
any order, the epilogue -- computed from the input, no empirical factor).

g = 600 genes and n = 2, 3, 65, 130, 257 samples; sets of the effective sizes of plage_ref.SIZES (the edges are named there)
with members in drawn order, and the special sets of plage_ref.build_case: empty, constant rows only, one constant member,
a NaN row, an Inf row, two identical rows, a positive and a negative pair.  One case at g = 20,480 with three sets.  size and
the NaN pattern are exact; dgCMatrix input, every sharding through the hook and a repeated call return the same bits."""
import functools

import mpmath
import numpy as np
import pytest
import scipy.sparse as sp

from plaid_amd import engine
from tests.helpers import plage_hooks
from tests.helpers import plage_ref as ref

pytestmark = pytest.mark.gpu

SAMPLES = (2, 3, 65, 130, 257)


def same(a, b, what=""):
    assert a.shape == b.shape
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    assert not bad.any(), f"{what}: {int(bad.sum())} differ, first at {np.argwhere(bad)[0]}"


@functools.lru_cache(maxsize=None)
def case(n, g=600):
    if g == 600:
        return ref.build_case(n, ref.SEEDS[n])
    return ref.build_case(n, 1, g=g, sizes=(17, 65, 129), extras=False)


@functools.lru_cache(maxsize=None)
def ctx():
    return engine.Context(0)


def exact_rows(X, rows_needed):
    """row -> its z in 50 digits"""
    mpmath.mp.dps = 50
    n = X.shape[1]
    out = {}
    for i in rows_needed:
        x = [mpmath.mpf(float(t)) for t in X[i, :]]
        mean = mpmath.fsum(x) / n
        sd = mpmath.sqrt(mpmath.fsum([(t - mean) ** 2 for t in x]) / (n - 1))
        out[int(i)] = [(t - mean) / sd for t in x]
    return out


def check(c):
    X, Gp, Gi = c["X"], c["Gp"], c["Gi"]
    S, size = ctx().zscore(X, Gp, Gi)
    _, _, flag = ref.moments(X)
    kept = [ref.members(Gp, Gi, flag, s) for s in range(len(Gp) - 1)]
    zx = exact_rows(X, sorted({int(i) for rows, _, bad in kept if not bad for i in rows}))
    worst = 0.0
    for s, (rows, _, bad) in enumerate(kept):
        assert size[s] == len(rows), c["names"][s]
        if bad or len(rows) == 0:
            assert np.isnan(S[s]).all(), c["names"][s]     # the NaN pattern is exact
            continue
        assert np.isfinite(S[s]).all(), c["names"][s]
        rk = mpmath.sqrt(mpmath.mpf(len(rows)))
        exact = [mpmath.fsum([zx[int(i)][j] for i in rows]) / rk for j in range(X.shape[1])]
        bound = ref.zscore_bound(X, rows, int(Gp[s + 1] - Gp[s]), exact)
        err = np.array([abs(float(e - mpmath.mpf(float(v)))) for e, v in zip(exact, S[s])])
        worst = max(worst, float((err / bound).max()))
        print(f"zscore n={X.shape[1]} {c['names'][s]}: max err {err.max():.3e} bound {bound.max():.3e}")
        assert (err <= bound).all(), (c["names"][s], err.max(), bound.max())
        assert bound.max() < 1e-9          # (the allowance itself stays an fp64 one)
    return S, size


@pytest.mark.parametrize("n", SAMPLES)
def test_zscore_lies_within_the_forward_bound_of_exact_arithmetic(n):
    c = case(n)
    S, size = check(c)
    nm = c["names"]
    assert size[nm.index("empty")] == 0 and size[nm.index("constants")] == 0 and size[nm.index("one_constant")] == 16
    for k in ref.SIZES:
        assert size[nm.index(f"k{k}")] == k


def test_rows_past_16_bits():
    c = case(65, 20480)
    assert len(c["names"]) == 3 and c["X"].shape == (20480, 65)
    assert int(c["Gi"].max()) >= 16384
    check(c)


def sparse_case():
    c = case(65)
    rng = np.random.default_rng(11)
    X = np.asfortranarray(np.where(rng.random(c["X"].shape) < 0.6, 0.0, np.nan_to_num(c["X"], nan=1.5, posinf=2.5)))
    X[-3, 7] = np.nan                      # (a stored NaN)
    return X, c["Gp"], c["Gi"]


def test_bits_dgcmatrix_shards_and_repeats():
    X, Gp, Gi = sparse_case()
    S0, k0 = ctx().zscore(X, Gp, Gi)
    S1, k1 = ctx().zscore(X, Gp, Gi)
    same(S0, S1, "a second call")
    same(k0, k1)
    Ss, ks = ctx().zscore(sp.csc_matrix(X), Gp, Gi)
    same(S0, Ss, "dgCMatrix")
    same(k0, ks)
    assert np.isnan(S0).any() and np.isfinite(S0).any()
    for c in (case(65), case(3)):
        base, kb = plage_hooks.zscore(1, c["X"], c["Gp"], c["Gi"])
        same(base, ctx().zscore(c["X"], c["Gp"], c["Gi"])[0], "hook against context")
        for shards in (2, 3, 7):           # (7 > 3: more shards than columns)
            S, k = plage_hooks.zscore(shards, c["X"], c["Gp"], c["Gi"])
            same(base, S, f"{shards} shards")
            same(kb, k)
    Sm, km = engine.zscore_multi(sp.csc_matrix(X), Gp, Gi, devices=1)
    same(S0, Sm, "zscore_multi")
