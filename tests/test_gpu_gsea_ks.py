"""replaid.ssgsea.exact(single = FALSE) on the GPU (include/plaidhip.h: plaidhip_ssgsea_exact_ks, _multi,
plaidhip_dev_gsea_ks_f64; kernels_ks.hip).

alpha = 0 and 1: every cw_t and B is a sum of integers or half-integers, each candidate is two correctly rounded divisions
and a subtraction, so the device must return the bits of the pinned form in numpy (tests/helpers/gsea_ks_walk.py).  Other
alphas: within the bound derived at the test.  The kernel has ONE route for every set size; its internal boundaries are
the 64 lanes of a wavefront, the 64 bits of a map word and the 4,096 positions of a scan step, and sets are placed at
each of them and one above.  A dgCMatrix must score as its dense form; sharding, the mixed precision mode and the Python
alignment must not change a bit.
"""

import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import exact_ref as er
from tests.helpers import gsea_ks_walk as kw
from tests.helpers import sharded_hooks
from tests.test_gpu_ssgsea_exact import SHAPES, _sets, _sparse, _tied

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
KS_MAX_GENES = 131072   # PLAIDHIP_GSEA_KS_MAX_GENES


def same(got, exp, what=""):
    er.assert_same_bits(got, exp, what)


def _sized_sets(g, sizes, seed=17):
    rng = np.random.default_rng(seed)
    Gi, Gp = [], [0]
    for k in sizes:
        Gi.extend(sorted(rng.choice(g, size=k, replace=False)))
        Gp.append(len(Gi))
    return np.array(Gp, dtype=np.int32), np.array(Gi, dtype=np.int32)


# ------------------------------------------------------------------------------------------------- 1. exact alphas
@pytest.mark.parametrize("g,n", SHAPES)
@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_exact_alphas_equal_the_pinned_candidates(hip_ctx, g, n, alpha):
    X = _tied(g, n)
    Gp, Gi = _sets(g, 24)
    for scale in (True, False):
        got = hip_ctx.ssgsea_exact(X, Gp, Gi, alpha, scale, False, single=False)
        same(got, kw.candidates_max_dev(X, Gp, Gi, alpha, scale), f"g={g} n={n} alpha={alpha} scale={scale}")


def test_equal_extremes_return_the_earlier_one(hip_ctx):
    X = np.asfortranarray([[4.0], [3.0], [2.0], [1.0]])
    Gp = np.array([0, 2, 4], dtype=np.int32)
    Gi = np.array([0, 3, 1, 2], dtype=np.int32)
    assert hip_ctx.ssgsea_exact(X, Gp, Gi, 0.0, False, False, single=False)[:, 0].tolist() == [0.5, -0.5]
    assert hip_ctx.ssgsea_exact(X, Gp, Gi, 1.0, True, False, single=False)[:, 0].tolist() == \
        kw.candidates_max_dev(X, Gp, Gi, 1.0, True)[:, 0].tolist()


def test_small_case_matches_the_literal_walk(hip_ctx):
    X = _tied(60, 7)
    X[~np.isfinite(X)] = 9.0
    Gp, Gi = _sets(60, 10)
    for alpha in (0.0, 1.0):
        same(hip_ctx.ssgsea_exact(X, Gp, Gi, alpha, True, False, single=False), kw.walk_max_dev(X, Gp, Gi, alpha), "walk")


# ------------------------------------------------------------------------------------------------- 2. the route's seams
@pytest.mark.parametrize("g", [64, 65, 4096, 4097, 8192, 8193])
@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_set_sizes_and_column_lengths_at_the_kernel_seams(hip_ctx, g, alpha):
    """one route for every k: sets of 63 / 64 / 65 (a wavefront of lanes), 127 / 128 / 129, 4,095 / 4,096 / 4,097 members
    (a scan step of 64 words) where g allows, in columns whose map ends at, and one past, a word and a scan step"""
    n = 9
    X = _tied(g, n)
    sizes = [k for k in (1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, g - 2, g - 1) if 0 < k < g] + [0, g]
    Gp, Gi = _sized_sets(g, sizes)
    for scale in (True, False):
        got = hip_ctx.ssgsea_exact(X, Gp, Gi, alpha, scale, False, single=False)
        same(got, kw.candidates_max_dev(X, Gp, Gi, alpha, scale), f"g={g} alpha={alpha} scale={scale}")


def test_the_gene_bound_and_one_above(hip_ctx):
    from plaid_amd._lib import EUNSUPPORTED, PlaidHipError
    g, n = KS_MAX_GENES, 3
    X = np.asfortranarray(np.round(np.random.default_rng(2).normal(0, 50, size=(g, n)), 0))
    Gp, Gi = _sized_sets(g, [1, 64, 5000, g - 1])
    for alpha in (0.0, 1.0):
        same(hip_ctx.ssgsea_exact(X, Gp, Gi, alpha, True, False, single=False), kw.candidates_max_dev(X, Gp, Gi, alpha),
             f"g={g} alpha={alpha}")
    X1 = np.asfortranarray(np.vstack([X, np.ones((1, n))]))
    with pytest.raises(PlaidHipError) as e:
        hip_ctx.ssgsea_exact(X1, Gp, Gi, 0.0, True, False, single=False)
    assert e.value.code == EUNSUPPORTED
    assert hip_ctx.ssgsea_exact(X1, Gp, Gi, 0.0).shape == (4, n)          # single = TRUE has no such bound


# ------------------------------------------------------------------------------------------------- 3. other alphas
@pytest.mark.parametrize("alpha", [0.25, 0.5, 2.0])
@pytest.mark.parametrize("g,n", [(97, 37), (3001, 64), (20000, 16)])
def test_other_alphas_within_the_derived_bound(hip_ctx, g, n, alpha):
    """Bound.  The device's w is within e_w = 16 u (relative) of np.power.  cw_t and B sum at most k positive terms in
    some order: each within ((k + 1) u + e_w) of the reference's.  Both quotients cw / B and miss are at most 1, so a
    candidate is within b = (2 k + 8) u + 2 e_w + 8 u of the reference's (b / N with scale).  Two candidates can change
    places only when their magnitudes are within 2 b, so |got| is within 2 b of |ref| for EVERY finite pair.  The sign
    must be the reference's wherever its |max(d) + min(d)| exceeds 4 b; the pairs below that are exempt from the sign
    check alone and may be at most 1 % of the finite pairs."""
    X = np.asfortranarray(np.round(np.random.default_rng(5).normal(8, 2, size=(g, n)), 1))
    Gp, Gi = _sets(g, 24)
    got = hip_ctx.ssgsea_exact(X, Gp, Gi, alpha, True, False, single=False)
    ref, dmax, dmin = kw.candidates_max_dev(X, Gp, Gi, alpha, True, with_extremes=True)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    k = np.diff(Gp).astype(np.float64)[:, None] * np.ones((1, n))
    b = ((2 * k + 8) * U + 2 * 16 * U + 8 * U) / g
    fin = ~np.isnan(ref)
    err = np.abs(np.abs(got[fin]) - np.abs(ref[fin]))
    print(f"g={g} alpha={alpha}: finite pairs {int(fin.sum())}, worst | |got| - |ref| | / 2b = {(err / (2 * b[fin])).max():.3g}")
    assert (err <= 2 * b[fin]).all()
    decided = fin & (np.abs(dmax + dmin) > 4 * b)
    exempt = int(fin.sum()) - int(decided.sum())
    print(f"  pairs exempt from the sign check: {exempt}")
    assert exempt <= 0.01 * fin.sum()
    assert np.array_equal(np.sign(got[decided]), np.sign(ref[decided]))


# ------------------------------------------------------------------------------------------------- 4. dgCMatrix
@pytest.mark.parametrize("density", [0.05, 0.6])
def test_dgcmatrix_scores_equal_the_dense_form(hip_ctx, density):
    for g, n in ((3001, 40), (20000, 9)):
        Xs = _sparse(g, n, density, 31)                       # stored zeros and an empty column
        Gp, Gi = _sets(g, 24)
        for alpha in (0.0, 0.25, 1.0):
            dense = hip_ctx.ssgsea_exact(Xs.toarray(), Gp, Gi, alpha, single=False)
            same(hip_ctx.ssgsea_exact(Xs, Gp, Gi, alpha, single=False), dense, f"g={g} density={density} alpha={alpha}")
            if alpha != 0.25:
                same(dense, kw.candidates_max_dev(Xs.toarray(), Gp, Gi, alpha), "dense form vs the pinned candidates")


# ------------------------------------------------------------------------------------------------- 5. sharding, modes
def _run_hook(nshards, X, Gp, Gi, alpha, norm, fail=-1):
    return sharded_hooks.score("ssgsea_exact_ks", nshards, X, Gp, Gi, float(alpha), 1, int(norm), fail=fail)


@pytest.mark.parametrize("kind", ["dense", "csc"])
def test_sharded_engine_is_bit_identical(hip_ctx, kind):
    g, n = 3001, 23
    X = _tied(g, n) if kind == "dense" else _sparse(g, n, 0.05, 41)
    Gp, Gi = _sets(g, 24)
    for norm in (False, True):
        for alpha in (0.0, 0.25):
            exp = hip_ctx.ssgsea_exact(X, Gp, Gi, alpha, True, norm, single=False)
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


def test_multi_on_one_device_equals_the_context_call(hip_ctx):
    import plaid_amd
    g, n = 3001, 23
    Gp, Gi = _sets(g, 24)
    for X in (_tied(g, n), _sparse(g, n, 0.05, 43)):
        for alpha, norm in ((0.0, False), (0.25, True)):
            same(plaid_amd.ssgsea_exact_multi(X, Gp, Gi, alpha, True, norm, devices=1, single=False),
                 hip_ctx.ssgsea_exact(X, Gp, Gi, alpha, True, norm, single=False), f"multi alpha={alpha} norm={norm}")


def test_mixed_mode_does_not_change_a_bit(hip_ctx):
    g, n = 3001, 33
    X = _tied(g, n)
    Gp, Gi = _sets(g, 24)
    exp = [hip_ctx.ssgsea_exact(X, Gp, Gi, a, single=False) for a in (0.0, 0.25, 1.0)]
    hip_ctx.set_precision("mixed")
    try:
        got = [hip_ctx.ssgsea_exact(X, Gp, Gi, a, single=False) for a in (0.0, 0.25, 1.0)]
    finally:
        hip_ctx.set_precision("f64")
    for e, o in zip(exp, got):
        same(o, e, "mixed mode")


# ------------------------------------------------------------------------------------------------- 6. alignment, single
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
        got = plaid_amd.replaid_ssgsea_exact(X1, G1, alpha=alpha, single=False, ctx=hip_ctx)
        exp = hip_ctx.ssgsea_exact(X0[perm], *plaid_amd.aligned_pattern(X1, G1), alpha, single=False)
        same(got.values, exp, f"alignment alpha={alpha}")
        if alpha != 0.25:
            same(got.values, kw.candidates_max_dev(X0, Gp, Gi, alpha), "alignment vs the pinned candidates")
        one = plaid_amd.replaid_ssgsea_exact(X1, G1, alpha=alpha, single=True, ctx=hip_ctx)
        same(one.values, hip_ctx.ssgsea_exact(X0[perm], *plaid_amd.aligned_pattern(X1, G1), alpha), "single = TRUE")
        same(plaid_amd.replaid_ssgsea_exact(X1, G1, alpha=alpha, ctx=hip_ctx).values, one.values, "the default is single = TRUE")


# ------------------------------------------------------------------------------------------------- 7. norm, NaN
def test_norm_divides_by_the_range_and_nan_spreads(hip_ctx):
    g, n = 3001, 37
    X = np.asfortranarray(np.round(np.random.default_rng(9).normal(0, 2, size=(g, n)), 0))
    Gp, Gi = _sized_sets(g, [int(k) for k in np.random.default_rng(10).integers(2, 300, size=20)])
    for alpha in (0.0, 0.25):
        plain = hip_ctx.ssgsea_exact(X, Gp, Gi, alpha, True, False, single=False)
        normed = hip_ctx.ssgsea_exact(X, Gp, Gi, alpha, True, True, single=False)
        same(normed, plain / (plain.max() - plain.min()), "norm")
    X[100, 4] = np.nan
    for alpha in (0.0, 0.25):
        plain = hip_ctx.ssgsea_exact(X, Gp, Gi, alpha, True, False, single=False)
        assert np.isnan(plain[:, 4]).all() and not np.isnan(np.delete(plain, 4, axis=1)).any()
        assert np.isnan(hip_ctx.ssgsea_exact(X, Gp, Gi, alpha, True, True, single=False)).all()


# ------------------------------------------------------------------------------------------------- the device entry
def test_dev_entry_scores_the_device_operands(hip_ctx):
    import torch
    dev = torch.device("cuda", 0)
    g, n = 3001, 19
    X = _tied(g, n)
    X[7, 2] = np.nan
    Gp, Gi = _sets(g, 24)
    m = len(Gp) - 1
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
    dGp, dGi = torch.from_numpy(Gp).to(dev), torch.from_numpy(Gi).to(dev)
    for alpha in (0.0, 1.0):
        Q, W, P = (torch.empty((n, g), dtype=torch.float64, device=dev) for _ in range(3))
        colnan = torch.empty((n,), dtype=torch.int32, device=dev)
        scratch = torch.empty(2 * g * n, dtype=torch.float64, device=dev)
        S = torch.full((n, m + 3), -7.0, dtype=torch.float64, device=dev)
        hip_ctx.dev_ssgsea_exact_operands(dX.data_ptr(), g, g, n, alpha, Q.data_ptr(), g, scratch.data_ptr(), colnan.data_ptr(),
                                          W.data_ptr(), P.data_ptr())
        hip_ctx.dev_gsea_ks(Q.data_ptr(), g, colnan.data_ptr(), g, n, dGp.data_ptr(), dGi.data_ptr(), m, alpha, True,
                            S.data_ptr(), m + 3, W=W.data_ptr() if alpha else None)
        torch.cuda.synchronize()
        out = S.cpu().numpy().T
        same(out[:m], hip_ctx.ssgsea_exact(X, Gp, Gi, alpha, True, False, single=False), f"dev entry alpha={alpha}")
        assert (out[m:] == -7.0).all()
