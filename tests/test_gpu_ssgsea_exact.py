"""replaid.ssgsea.exact on the GPU (include/plaidhip.h: plaidhip_ssgsea_exact, _multi, the operand pass).

alpha = 0 and 1: A, B and C are sums of integers and half-integers below 2^53, exact in any order, so the scores must be
the pinned epilogue evaluated in numpy bit for bit.  Other alphas: within a bound derived below.  The operand pass must
reproduce colranks(ties = "last") and colranks(ties = "average", power = alpha) bit for bit; a dgCMatrix must score as its
dense form; the sharded engine, the mixed precision mode and the Python alignment must not change a bit.
"""

import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import exact_ref as er
from tests.helpers import ssgsea_walk as sw
from tests.helpers import sharded_hooks

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _sets(g, m, seed=11):
    """m sets over g genes with k in {0, 1, N - 1, N} among them (where g allows), the rest random sizes"""
    rng = np.random.default_rng(seed)
    sizes = [0, 1, max(g - 1, 0), g] + [int(rng.integers(1, max(2, min(g, 300)))) for _ in range(m - 4)]
    Gi, Gp = [], [0]
    for k in sizes:
        Gi.extend(sorted(rng.choice(g, size=min(k, g), replace=False)))
        Gp.append(len(Gi))
    return np.array(Gp, dtype=np.int32), np.array(Gi, dtype=np.int32)


def _tied(g, n, seed=3):
    """heavy ties, -0.0 beside 0.0, +-Inf, an all-equal column"""
    rng = np.random.default_rng(seed)
    X = np.round(rng.normal(0, 2, size=(g, n)), 0)
    X[rng.random((g, n)) < 0.05] = -0.0
    X[rng.random((g, n)) < 0.01] = np.inf
    X[rng.random((g, n)) < 0.01] = -np.inf
    if n > 1:
        X[:, 1] = 4.0
    return np.asfortranarray(X)


def same(got, exp, what=""):
    er.assert_same_bits(got, exp, what)


SHAPES = [(1, 1), (1, 37), (97, 37), (97, 2049), (3001, 37), (3001, 2049), (8193, 37), (20000, 37), (20000, 1)]


@pytest.mark.parametrize("g,n", SHAPES)
@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_exact_alphas_equal_the_pinned_epilogue(hip_ctx, g, n, alpha):
    X = _tied(g, n)
    Gp, Gi = _sets(g, 24)
    for scale in (True, False):
        got = hip_ctx.ssgsea_exact(X, Gp, Gi, alpha, scale, False)
        same(got, sw.closed_form(X, Gp, Gi, alpha, scale, False), f"g={g} n={n} alpha={alpha} scale={scale}")


@pytest.mark.parametrize("alpha", [0.25, 0.5, 2.0])
@pytest.mark.parametrize("g,n", [(97, 37), (3001, 64), (20000, 16)])
def test_other_alphas_within_the_derived_bound(hip_ctx, g, n, alpha):
    """Bound.  The device's w is r^alpha by 1/4-step square roots (a few ulp) or pow; the reference's is np.power: the two
    differ by at most e_w = 16 u relative.  P = fl(w q) adds u; A and B sum k positive terms with k - 1 roundings, so each
    is within ((k + 1) u + e_w) of its reference, and d1 = A / B within ((2 k + 8) u + 2 e_w) d1 (the division and the
    reference's own roundings included).  C is exact, so d2 agrees bit for bit; es = d1 - d2 and es / N add one rounding
    each on either side: 4 u (|d1| + |d2|)."""
    X = np.asfortranarray(np.round(np.random.default_rng(5).normal(8, 2, size=(g, n)), 1))
    Gp, Gi = _sets(g, 24)
    got = hip_ctx.ssgsea_exact(X, Gp, Gi, alpha, True, False)
    Q, W = sw.operands(X, alpha)
    k = np.diff(Gp)
    A, _, _ = er.set_sums(Gp, Gi, W * Q)
    B, _, _ = er.set_sums(Gp, Gi, W)
    Cs = sw.set_sums_exact(Gp, Gi, Q)
    ref = sw.pinned_epilogue(A, B, Cs, k, g, np.zeros(n, dtype=bool), True, False)
    with np.errstate(all="ignore"):
        d1 = np.abs(A / B)
        d2 = np.abs((g * (g + 1) / 2 - Cs) / (g - k)[:, None])
        bound = (((2 * k[:, None] + 8) * U + 32 * U) * d1 + 4 * U * (d1 + d2)) / g
    er.assert_within(got, ref, np.nan_to_num(bound, nan=0.0), f"g={g} alpha={alpha}")


def test_small_case_matches_the_running_sum_walk(hip_ctx):
    X = _tied(60, 7)
    X[~np.isfinite(X)] = 9.0
    Gp, Gi = _sets(60, 10)
    for alpha in (0.0, 0.25, 1.0, 2.0):
        got = hip_ctx.ssgsea_exact(X, Gp, Gi, alpha, True, False)
        walk = sw.walk_scores(X, Gp, Gi, alpha, True, False)
        assert np.array_equal(np.isnan(got), np.isnan(walk))
        ok = ~np.isnan(walk)
        np.testing.assert_allclose(got[ok], walk[ok], rtol=0, atol=1e-13)


# ------------------------------------------------------------------------------------------------- the operand pass
def _dev_operands(hip_ctx, X, alpha, csc=None):
    import torch
    dev = torch.device("cuda", 0)
    g, n = X.shape
    Q = torch.full((n, g), -1.0, dtype=torch.float64, device=dev)
    W = torch.full((n, g), -1.0, dtype=torch.float64, device=dev)
    P = torch.full((n, g), -1.0, dtype=torch.float64, device=dev)
    colnan = torch.full((n,), 7, dtype=torch.int32, device=dev)
    if csc is None:
        dX = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
        scratch = torch.empty(2 * g * n, dtype=torch.float64, device=dev)
        hip_ctx.dev_ssgsea_exact_operands(dX.data_ptr(), g, g, n, alpha, Q.data_ptr(), g, scratch.data_ptr(), colnan.data_ptr(),
                                          W.data_ptr(), P.data_ptr())
    else:
        Xs = csc
        nnz = int(Xs.indptr[-1])
        dXp = torch.from_numpy(Xs.indptr.astype(np.int32)).to(dev)
        dXi = torch.from_numpy(np.concatenate([Xs.indices, [0]]).astype(np.int32)).to(dev)         # (+1: never empty)
        dXx = torch.from_numpy(np.concatenate([Xs.data, [0.0]]).astype(np.float64)).to(dev)
        scratch = torch.empty(3 * nnz + 1, dtype=torch.float64, device=dev)
        mx = int(np.diff(Xs.indptr).max()) if n else 0
        hip_ctx.dev_ssgsea_exact_operands_csc(dXp.data_ptr(), dXi.data_ptr(), dXx.data_ptr(), g, n, mx, nnz, alpha,
                                              Q.data_ptr(), g, scratch.data_ptr(), colnan.data_ptr(), W.data_ptr(),
                                              P.data_ptr())
    torch.cuda.synchronize()
    return Q.cpu().numpy().T, W.cpu().numpy().T, P.cpu().numpy().T, colnan.cpu().numpy()


def _colranks_power(hip_ctx, X, power):
    import torch
    dev = torch.device("cuda", 0)
    g, n = X.shape
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
    R = torch.empty((n, g), dtype=torch.float64, device=dev)
    hip_ctx.dev_colranks_dense(dX.data_ptr(), g, g, n, R.data_ptr(), g, "average", False, power)
    torch.cuda.synchronize()
    return R.cpu().numpy().T


@pytest.mark.parametrize("g", [200, 3001, 25000])
def test_operands_equal_colranks(hip_ctx, g):
    n = 24
    Xt = np.asfortranarray(np.round(np.random.default_rng(7).normal(0, 3, size=(g, n)), 0))   # ties
    Xf = np.asfortranarray(np.random.default_rng(8).normal(8, 2, size=(g, n)))                # tie-free
    Xt[5, 3] = np.nan
    last = hip_ctx.colranks_dense(Xt, "last")
    for alpha in (0.0, 0.3, 1.0):
        Q, W, P, nanc = _dev_operands(hip_ctx, Xt, alpha)
        same(Q, last, f"q g={g}")
        assert nanc.tolist() == [1 if c == 3 else 0 for c in range(n)]
        if alpha != 0.0:
            same(W, _colranks_power(hip_ctx, Xt, alpha), f"w g={g} alpha={alpha}")
            same(P, W * Q, "p")
    for alpha in (0.25, 0.5, 2.0):   # 1/4-step exponents: the routine of the ranker that takes columns of g genes
        Q, W, P, _ = _dev_operands(hip_ctx, Xf, alpha)
        same(Q, hip_ctx.colranks_dense(Xf, "last"), "q tie-free")
        same(W, _colranks_power(hip_ctx, Xf, alpha), f"w g={g} alpha={alpha}")
        same(P, W * Q, "p")


def _sparse(g, n, density, seed):
    rng = np.random.default_rng(seed)
    D = np.round(rng.normal(0, 2, size=(g, n)), 0)
    D[rng.random((g, n)) >= density] = 0.0
    D[:, 0] = 0.0                                            # an empty column
    S = sp.csc_matrix(D)
    S.sort_indices()
    if S.nnz:                                                # stored zeros
        S.data[rng.random(S.nnz) < 0.1] = 0.0
    return S


@pytest.mark.parametrize("density", [0.0, 0.05, 0.6, 1.0])
def test_csc_operands_equal_the_dense_operands(hip_ctx, density):
    g, n = 3001, 40
    Xs = _sparse(g, n, density, 21)
    D = np.asfortranarray(Xs.toarray())
    for alpha in (0.0, 0.25, 1.0):
        a = _dev_operands(hip_ctx, D, alpha)
        b = _dev_operands(hip_ctx, D, alpha, csc=Xs)
        for x, y, what in zip(a, b, ("q", "w", "p", "colnan")):
            if alpha == 0.0 and what in ("w", "p"):
                continue
            same(y, x, f"{what} density={density} alpha={alpha}")


@pytest.mark.parametrize("density", [0.0, 0.05, 0.6, 1.0])
def test_dgcmatrix_scores_equal_the_dense_entry(hip_ctx, density):
    for g, n in ((3001, 40), (20000, 9)):
        Xs = _sparse(g, n, density, 31)
        Gp, Gi = _sets(g, 24)
        for alpha in (0.0, 0.25, 1.0):
            same(hip_ctx.ssgsea_exact(Xs, Gp, Gi, alpha), hip_ctx.ssgsea_exact(Xs.toarray(), Gp, Gi, alpha),
                 f"g={g} density={density} alpha={alpha}")


# ------------------------------------------------------------------------------------------------- norm, NaN
def test_norm_divides_by_the_range_and_nan_spreads(hip_ctx):
    g, n = 3001, 37
    X = np.asfortranarray(np.round(np.random.default_rng(9).normal(0, 2, size=(g, n)), 0))
    rng = np.random.default_rng(10)
    Gi, Gp = [], [0]
    for _ in range(20):
        Gi.extend(sorted(rng.choice(g, size=int(rng.integers(2, 300)), replace=False)))
        Gp.append(len(Gi))
    Gp, Gi = np.array(Gp, dtype=np.int32), np.array(Gi, dtype=np.int32)
    for alpha in (0.0, 0.25):
        plain = hip_ctx.ssgsea_exact(X, Gp, Gi, alpha, True, False)
        normed = hip_ctx.ssgsea_exact(X, Gp, Gi, alpha, True, True)
        same(normed, plain / (plain.max() - plain.min()), "norm")
    X[100, 4] = np.nan
    plain = hip_ctx.ssgsea_exact(X, Gp, Gi, 0.25, True, False)
    assert np.isnan(plain[:, 4]).all() and not np.isnan(np.delete(plain, 4, axis=1)).any()
    assert np.isnan(hip_ctx.ssgsea_exact(X, Gp, Gi, 0.25, True, True)).all()
    assert np.isnan(hip_ctx.ssgsea_exact(X, Gp, Gi, 0.0, True, False)[:, 4]).all(), "NaN column at alpha = 0 too"


# ------------------------------------------------------------------------------------------------- sharding
def _run_hook(nshards, X, Gp, Gi, alpha, norm, fail=-1):
    return sharded_hooks.score("ssgsea_exact", nshards, X, Gp, Gi, float(alpha), 1, int(norm), fail=fail)


@pytest.mark.parametrize("kind", ["dense", "csc"])
def test_sharded_engine_is_bit_identical(hip_ctx, kind):
    g, n = 3001, 23
    X = _tied(g, n) if kind == "dense" else _sparse(g, n, 0.05, 41)
    Gp, Gi = _sets(g, 24)
    for norm in (False, True):
        for alpha in (0.0, 0.25):
            exp = hip_ctx.ssgsea_exact(X, Gp, Gi, alpha, True, norm)
            for nshards in range(1, 6):
                rc, S = _run_hook(nshards, X, Gp, Gi, alpha, norm)
                assert rc == 0
                same(S, exp, f"{kind} nshards={nshards} norm={norm} alpha={alpha}")


def test_injected_shard_failure_returns_an_error(hip_ctx):
    from plaid_amd._lib import load
    g, n = 500, 12
    X = _tied(g, n)
    Gp, Gi = _sets(g, 10)
    for norm in (False, True):
        rc, _ = _run_hook(3, X, Gp, Gi, 0.25, norm, fail=1)
        assert rc != 0 and b"injected failure" in load().plaidhip_last_error_string()


# ------------------------------------------------------------------------------------------------- modes, alignment
def test_mixed_mode_does_not_change_a_bit(hip_ctx):
    g, n = 3001, 33
    X = _tied(g, n)
    Gp, Gi = _sets(g, 24)
    exp = [hip_ctx.ssgsea_exact(X, Gp, Gi, a) for a in (0.0, 0.25, 1.0)]
    hip_ctx.set_precision("mixed")
    try:
        got = [hip_ctx.ssgsea_exact(X, Gp, Gi, a) for a in (0.0, 0.25, 1.0)]
    finally:
        hip_ctx.set_precision("f64")
    for e, o in zip(exp, got):
        same(o, e, "mixed mode")


def test_python_alignment_equals_the_prealigned_call(hip_ctx):
    import plaid_amd
    g, n, m = 500, 8, 12
    rng = np.random.default_rng(12)
    X0 = rng.normal(8, 2, size=(g, n))                       # tie-free: the row order decides no tie
    genes = [f"g{i}" for i in range(g)]
    Gp, Gi = _sets(g, m)
    G0 = sp.csc_matrix((np.ones(len(Gi)), Gi, Gp), shape=(g, m))
    perm = rng.permutation(g)
    X1 = plaid_amd.NamedMatrix(X0[perm], [genes[i] for i in perm], [f"s{j}" for j in range(n)])
    extra = sp.csc_matrix((np.ones(m), (np.arange(m) % 5, np.arange(m))), shape=(5, m))
    G1 = plaid_amd.NamedMatrix(sp.vstack([G0, extra]).tocsc(), genes + [f"absent{i}" for i in range(5)],
                               [f"set{j}" for j in range(m)])
    for alpha in (0.0, 1.0, 0.25):
        got = plaid_amd.replaid_ssgsea_exact(X1, G1, alpha=alpha, ctx=hip_ctx)
        exp = hip_ctx.ssgsea_exact(X0[perm], *plaid_amd.aligned_pattern(X1, G1), alpha)
        same(got.values, exp, f"alignment alpha={alpha}")
        if alpha != 0.25:
            same(got.values, sw.closed_form(X0, Gp, Gi, alpha), "alignment vs the closed form")
