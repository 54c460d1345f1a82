"""replaid.aucell and replaid.scse against the exact references of tests/helpers/gsva_ref.py, at their derived fp64
bounds -- `pytest -m gpu`.  (map_kernel ops 1 ... 5, col_abs_sums_kernel, affine_kernel, and the sharded engine.)

replaid.aucell: weights 1.08 pmax((r - (max(r) - K)) / K, 0) of the average ranks; K = 1, ceil(0.05 g), g and g + 7; tie
groups astride the thresholds; dense X and a dgCMatrix whose zeros tie.  A set with no member in the top K scores
exactly 0, which decides normalize_medians' ignore.zero: the reference applies the rule, and the test reads the device's
zero pattern off the result.

replaid.scse: sum and mean, removeLog2 TRUE / FALSE / NULL (both outcomes), dense X and a dgCMatrix with stored zeros
and negative values, 1, 2 and 3 shards.  Without removeLog2 the bound is fully derived.  With it, every term is a
device 2^x; the allowance for one such value is gsva_ref.EXP2_ULPS = 3 u, the project's figure for its pow routines.
test_device_exp2_within_its_allowance measures the device's exp2 on its own -- not through the cases it licenses --
against 50 digits: 1.78 u measured, 2.78 u with the 1 u the rule adds, inside the 3 u.

Every test prints the largest |error| / bound it met (`pytest -s`)."""
import functools

import numpy as np
import pytest

from tests.helpers import exact_ref as er
from tests.helpers import gsva_cases as gc
from tests.helpers import gsva_ref as gr
from tests.helpers import sharded_hooks

pytestmark = pytest.mark.gpu
AUCELL, SCSE = sharded_hooks.AUCELL, sharded_hooks.SCSE


def _dense(X):
    return X.toarray() if hasattr(X, "toarray") else X


@functools.lru_cache(maxsize=None)
def _aucell_reference(g, sparse, K):
    X, Gp, Gi = gc.aucell_case(g, sparse)
    return gr.aucell_ref(_dense(X), Gp, Gi, K)


@pytest.mark.parametrize("ki", range(4))
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("g", gc.AUCELL_G)
def test_aucell_within_the_bound(hip_ctx, g, sparse, ki):
    K = gc.aucell_ks(g)[ki]
    X, Gp, Gi = gc.aucell_case(g, sparse)
    N, B, T, iz = _aucell_reference(g, sparse, K)
    assert iz == (K < g)                                       # K >= g: every weight is positive, no score is 0
    S = hip_ctx.aucell(X, Gp, Gi, K)
    print(f"RATIO aucell g={g} sparse={sparse} K={K}: {gr.ratio(S, N, B):.3g}")
    er.assert_within(S, N, B, f"aucell g={g} sparse={sparse} K={K}")
    # The device's raw zeros, read off the result: a raw 0 leaves as fl(fl(0 - med_c) + add), one value per column, and
    # every positive raw score leaves above it.  The device's zero pattern is the reference's, so min(S) == 0 exactly
    # where the reference says so, and ignore.zero resolved alike on both sides.
    for c in range(S.shape[1]):
        z = T[:, c] == 0.0
        if z.any():
            v = S[z, c]
            assert np.all(er.bits(v) == er.bits(v[:1])), (c, "raw zeros must leave as one value")
            assert np.all(S[~z, c] > v[0]), (c, "a positive raw score left at or below the zeros' value")


def test_aucell_sharded_within_the_same_bound(hip_ctx):
    g, sparse = 257, True
    K = gc.aucell_ks(g)[1]
    X, Gp, Gi = gc.aucell_case(g, sparse)
    N, B, _, _ = _aucell_reference(g, sparse, K)
    for nshards in (2, 3):
        rc, S, _ = sharded_hooks.scorer(nshards, AUCELL, X, Gp, Gi, auc_max_rank=K)
        assert rc == 0
        er.assert_within(S, N, B, f"aucell {nshards} shards")


# ------------------------------------------------------------------ replaid.scse
@functools.lru_cache(maxsize=None)
def _scse_reference(kind, sparse, remove_log2, score_mean):
    X, Gp, Gi = gc.scse_case(kind, sparse)
    return gr.scse_ref(X, Gp, Gi, remove_log2, score_mean)


@pytest.mark.parametrize("score_mean", [False, True])
@pytest.mark.parametrize("remove_log2", [True, False, None])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("kind", gc.SCSE_KINDS)
def test_scse_within_the_bound_one_shard_and_several(hip_ctx, kind, sparse, remove_log2, score_mean):
    X, Gp, Gi = gc.scse_case(kind, sparse)
    ref, B, removed = _scse_reference(kind, sparse, remove_log2, score_mean)
    if remove_log2 is None:
        assert removed == (kind == "nonneg")                   # both outcomes of NULL are met
    what = f"scse {kind} sparse={sparse} removeLog2={remove_log2} mean={score_mean}"
    S = hip_ctx.scse(X, Gp, Gi, remove_log2, score_mean)
    assert bool(hip_ctx.last_scse_removed_log2) == removed
    print(f"RATIO {what}: {gr.ratio(S, ref, B):.3g}")
    er.assert_within(S, ref, B, what)
    for nshards in (2, 3):
        rc, Sn, rem = sharded_hooks.scorer(nshards, SCSE, X, Gp, Gi, remove_log2=remove_log2, score_mean=score_mean)
        assert rc == 0 and bool(rem) == removed
        print(f"RATIO {what} {nshards} shards: {gr.ratio(Sn, ref, B):.3g}")
        er.assert_within(Sn, ref, B, f"{what} {nshards} shards")


def test_device_exp2_within_its_allowance(hip_ctx):
    """The device's 2^x on its own, against 50 digits.  A dense X whose gene 0 is -1 in every sample, singleton sets,
    scoreMean = FALSE, removeLog2 = TRUE: gene 0 keeps its -1 (only x > 0 is transformed), so its score is fl(-1 * f) =
    -f, the device's column factor f = fl(100 / (sum |V| + 1e-8)) itself, bit for bit; every other score is fl(v f) with
    v the device's 2^x.  v = score / f then carries one rounding of the device's (the product) beside exp2's own error;
    the quotient is taken in long double.  The largest |v - 2^x| / (u 2^x) seen, plus 1 u, must fit in the
    allowance EXP2_ULPS = 3 u that the removeLog2 cases use.

    Measured on an MI355X: 1.78 (the product's rounding included) over the 3,192 exponents below, so 2.78 with the
    1 u added: the starting allowance of 3 u stays."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    g, n = 400, 8
    rng = np.random.default_rng(2)
    X = rng.uniform(0.0, 19.5, size=(g, n))
    X[1:40, :] = rng.uniform(0.0, 1.0, size=(39, n))           # small exponents too
    X[40:60, :] = np.maximum(np.round(X[40:60, :]), 1.0)       # and integers: exact powers of two
    X[0, :] = -1.0
    Gp = np.arange(g + 1, dtype=np.int32)
    Gi = np.arange(g, dtype=np.int32)
    S = hip_ctx.scse(np.asfortranarray(X), Gp, Gi, True, False)
    assert bool(hip_ctx.last_scse_removed_log2)
    f = -S[0, :]
    assert np.all(f > 0)
    v = (S[1:, :].astype(gr.ld) / f.astype(gr.ld)[None, :])
    worst = 0.0
    for (i, c), x in np.ndenumerate(X[1:, :]):
        exact = mp.mpf(2) ** mp.mpf(float(x))
        vi = v[i, c]
        hi = float(vi)
        got = mp.mpf(hi) + mp.mpf(float(vi - gr.ld(hi)))
        worst = max(worst, float(abs(got - exact) / exact) / er.U)
    print(f"EXP2 largest |v_dev - 2^x| / (u 2^x) over {v.size} values, the product's 1 u included: {worst:.3f}")
    assert worst + 1.0 <= gr.EXP2_ULPS                         # (allowance >= the measured value plus 1 u)
    assert np.all(S[40:60, :] == np.exp2(X[40:60, :]) * f[None, :])     # integer exponents: exact powers of two
