"""replaid.gsva.exact on the GPU (include/plaidhip.h: plaidhip_gsva_exact, _multi, plaidhip_dev_gsva_ks_f64;
kernels_ks.hip: gsva_ks_kernel).

tau = 0 and 1: every cw_t and B is a sum of integers or half-integers and a candidate is two correctly rounded divisions
and a subtraction, so the device must return the bits of the pinned form in numpy (tests/helpers/gsva_walk.py).  Other
tau: within the bound derived at the test.  The walk has ONE route for every set size; its seams are the 64 lanes of a
wavefront, the 64 bits of a map word and the 4,096 positions of a scan step.  The row transforms must score as
rowtf = "none" on the transformed matrix; a dgCMatrix as its dense form; sharding, the mixed precision mode and the
Python alignment must not change a bit.
"""

import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import exact_ref as er
from tests.helpers import gsva_walk as gw
from tests.helpers import sharded_hooks
from tests.test_gpu_ssgsea_exact import SHAPES, _sets, _sparse, _tied

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
KS_MAX_GENES = 131072   # PLAIDHIP_GSEA_KS_MAX_GENES
ROWTF = {"z": 0, "ecdf": 1, "none": 2}


def same(got, exp, what=""):
    er.assert_same_bits(got, exp, what)


def _sized_sets(g, sizes, seed=17, extra=()):
    rng = np.random.default_rng(seed)
    Gi, Gp = [], [0]
    for k in sizes:
        Gi.extend(sorted(rng.choice(g, size=k, replace=False)))
        Gp.append(len(Gi))
    for rows in extra:
        Gi.extend(sorted(rows))
        Gp.append(len(Gi))
    return np.array(Gp, dtype=np.int32), np.array(Gi, dtype=np.int32)


# ------------------------------------------------------------------------------------------------- 1. exact tau
@pytest.mark.parametrize("g,n", SHAPES)
@pytest.mark.parametrize("tau", [0.0, 1.0])
def test_exact_taus_equal_the_pinned_form(hip_ctx, g, n, tau):
    X = _tied(g, n)
    Gp, Gi = _sets(g, 24)
    for max_diff in (True, False):
        got = hip_ctx.gsva_exact(X, Gp, Gi, tau, "none", max_diff)
        same(got, gw.pinned(X, Gp, Gi, tau, max_diff), f"g={g} n={n} tau={tau} max_diff={max_diff}")


def test_equal_magnitudes_return_the_negative_extreme(hip_ctx):
    X = np.asfortranarray([[4.0], [3.0], [2.0], [1.0]])
    Gp = np.array([0, 2, 4], dtype=np.int32)
    Gi = np.array([0, 3, 1, 2], dtype=np.int32)
    assert hip_ctx.gsva_exact(X, Gp, Gi, 0.0, "none", False)[:, 0].tolist() == [-0.5, -0.5]
    # (first and last gene: +0.5 then -0.5; the two middle genes: -0.5 then +0.5)
    assert hip_ctx.gsva_exact(X, Gp, Gi, 0.0, "none", True)[:, 0].tolist() == [0.0, 0.0]


def test_small_case_against_the_literal_walk(hip_ctx):
    """the bound of tests/test_gsva_exact_ref.py (2 (N + 8) u) between the device and GSVA's loop"""
    N = 60
    X = _tied(N, 7)
    X[~np.isfinite(X)] = 9.0
    Gp, Gi = _sets(N, 10)
    for tau in (0.0, 1.0):
        got = hip_ctx.gsva_exact(X, Gp, Gi, tau, "none", True)
        ref = gw.literal_walk(X, Gp, Gi, tau, True)
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        fin = ~np.isnan(ref)
        assert (np.abs(got[fin] - ref[fin]) <= 2 * (N + 8) * U).all()


# ------------------------------------------------------------------------------------------------- 2. the walk's seams
@pytest.mark.parametrize("g", [64, 65, 4096, 4097, 8192, 8193])
@pytest.mark.parametrize("tau", [0.0, 1.0])
def test_set_sizes_and_column_lengths_at_the_kernel_seams(hip_ctx, g, tau):
    """sets of 63 / 64 / 65, 127 / 128 / 129, 4,095 / 4,096 / 4,097, N - 1, 0 and N members where g allows, in columns
    whose map ends at, and one past, a word and a scan step.  Even N: the centre gene (q = N / 2) weighs 0 at tau > 0; the
    one-member set on it scores NaN at tau = 1 and is finite at tau = 0 (odd N has no such gene)."""
    n = 9
    X = _tied(g, n)
    sizes = [k for k in (1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, g - 2, g - 1) if 0 < k < g] + [0, g]
    centre = int(np.flatnonzero(gw.positions(X)[0][:, 0] == g + 1 - g // 2)[0])   # of column 0
    other = (centre + 1) % g
    Gp, Gi = _sized_sets(g, sizes, extra=([centre], [centre, other]))
    for max_diff in (True, False):
        got = hip_ctx.gsva_exact(X, Gp, Gi, tau, "none", max_diff)
        same(got, gw.pinned(X, Gp, Gi, tau, max_diff), f"g={g} tau={tau} max_diff={max_diff}")
    assert np.isnan(got[-2, 0]) == (tau > 0 and g % 2 == 0)
    assert not np.isnan(got[-1, 0])


def test_the_gene_bound_and_one_above(hip_ctx):
    from plaid_amd._lib import EUNSUPPORTED, PlaidHipError
    g, n = KS_MAX_GENES, 3
    X = np.asfortranarray(np.round(np.random.default_rng(2).normal(0, 50, size=(g, n)), 0))
    Gp, Gi = _sized_sets(g, [1, 64, 5000, g - 1])
    for tau in (0.0, 1.0):
        same(hip_ctx.gsva_exact(X, Gp, Gi, tau, "none", True), gw.pinned(X, Gp, Gi, tau, True), f"g={g} tau={tau}")
    X1 = np.asfortranarray(np.vstack([X, np.ones((1, n))]))
    for rowtf in ("none", "z"):
        with pytest.raises(PlaidHipError) as e:
            hip_ctx.gsva_exact(X1, Gp, Gi, 0.0, rowtf, True)
        assert e.value.code == EUNSUPPORTED


def test_nan_column_scores_nan(hip_ctx):
    g, n = 3001, 9
    X = np.asfortranarray(np.round(np.random.default_rng(9).normal(0, 2, size=(g, n)), 0))
    X[100, 4] = np.nan
    Gp, Gi = _sets(g, 12)
    for tau in (0.0, 1.0):
        got = hip_ctx.gsva_exact(X, Gp, Gi, tau, "none", True)
        assert np.isnan(got[:, 4]).all()
        same(got, gw.pinned(X, Gp, Gi, tau, True), "NaN column")


# ------------------------------------------------------------------------------------------------- 3. row transforms
def _exact_z_rows(g, n, seed=7):
    """integer rows whose mean and sd are exactly representable: a at t places and -a at t others (mean 0, whatever way it
    is divided), n - 1 = 2 * 4^j and t a power of 4, so that the sum of squared deviations 2 t a^2 over n - 1 is the
    square of a binary fraction; every sum on the way is an integer.  Rows with the same (t, a) transform to the same bits
    on any route, rows with another (t, a) to values 1e-10 (relative) or more away (the 1e-8 beside the sd), far beyond a
    rounding: the per-sample order of the device's transform is the order of the host's."""
    rng = np.random.default_rng(seed)
    assert n - 1 in (8, 32, 128, 512, 2048)
    ts = [t for t in (1, 4, 16, 64, 256) if 2 * t <= n]
    X = np.zeros((g, n))
    for i in range(g):
        t, a = ts[rng.integers(len(ts))], float(rng.integers(1, 6))
        at = rng.choice(n, size=2 * t, replace=False)
        X[i, at[:t]] = a
        X[i, at[t:]] = -a
    return np.asfortranarray(X)


@pytest.mark.parametrize("tau", [0.0, 1.0])
def test_ecdf_scores_as_none_on_the_transformed_matrix(hip_ctx, tau):
    """no existing entry point exposes the device's transformed matrix: v is computed on the host as the oracle's
    replaid_gsva does.  ecdf(x)(x_i) = #{x <= x_i} / n is an integer over n: exact, and the device's (without the factor
    1 / n) has the same order"""
    g, n = 3001, 37
    X = np.asfortranarray(np.round(np.random.default_rng(21).normal(0, 2, size=(g, n)), 0))
    Gp, Gi = _sets(g, 24)
    V = np.asfortranarray(gw.row_transform(X, "ecdf"))
    for max_diff in (True, False):
        got = hip_ctx.gsva_exact(X, Gp, Gi, tau, "ecdf", max_diff)
        same(got, hip_ctx.gsva_exact(V, Gp, Gi, tau, "none", max_diff), "ecdf vs none on the host's transform")
        same(got, gw.pinned(V, Gp, Gi, tau, max_diff), "ecdf vs the pinned form")


@pytest.mark.parametrize("tau", [0.0, 1.0])
@pytest.mark.parametrize("n", [33, 513])
def test_z_scores_as_none_on_the_transformed_matrix(hip_ctx, tau, n):
    g = 3001
    X = _exact_z_rows(g, n)
    Gp, Gi = _sets(g, 24)
    V = np.asfortranarray(gw.row_transform(X, "z"))
    assert np.isfinite(V).all()
    for max_diff in (True, False):
        got = hip_ctx.gsva_exact(X, Gp, Gi, tau, "z", max_diff)
        same(got, hip_ctx.gsva_exact(V, Gp, Gi, tau, "none", max_diff), "z vs none on the host's transform")
        same(got, gw.pinned(V, Gp, Gi, tau, max_diff), "z vs the pinned form")


# ------------------------------------------------------------------------------------------------- 4. other tau
@pytest.mark.parametrize("tau", [0.25, 0.5, 2.0])
@pytest.mark.parametrize("g,n", [(97, 37), (3001, 64), (20000, 16)])
def test_other_taus_within_the_derived_bound(hip_ctx, g, n, tau):
    """Bound.  The device's w is within e_w = 16 u (relative) of np.power (1/4-step roots or pow).  cw_t and B sum at most
    k non-negative terms in some order: each within ((k + 1) u + e_w) of the reference's.  Both quotients cw / B and miss
    are at most 1, so a candidate is within b = (2 k + 8) u + 2 e_w + 8 u of the reference's, and so are mx_pos and
    mx_neg, a max and a min over candidates.  max_diff = TRUE adds them: 2 b, plus one rounding of a sum of magnitude at
    most 1 on either side (2 u); no sign exemption.  max_diff = FALSE returns one of them: the magnitude within b; the
    choice between them (the sign) is decided wherever the reference's |mx_pos + mx_neg| exceeds 2 b, the pairs below that
    are exempt from the sign check alone and may be at most 5 % of the finite pairs."""
    X = np.asfortranarray(np.round(np.random.default_rng(5).normal(8, 2, size=(g, n)), 1))
    Gp, Gi = _sets(g, 24)
    k = np.diff(Gp).astype(np.float64)[:, None] * np.ones((1, n))
    b = (2 * k + 8) * U + 2 * 16 * U + 8 * U
    ref, mxp, mxn = gw.pinned(X, Gp, Gi, tau, True, with_extremes=True)
    got = hip_ctx.gsva_exact(X, Gp, Gi, tau, "none", True)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    fin = ~np.isnan(ref)
    err = np.abs(got[fin] - ref[fin])
    print(f"g={g} tau={tau}: finite pairs {int(fin.sum())}, worst |got - ref| / (2b + 2u) = {(err / (2 * b[fin] + 2 * U)).max():.3g}")
    assert (err <= 2 * b[fin] + 2 * U).all()
    got0 = hip_ctx.gsva_exact(X, Gp, Gi, tau, "none", False)
    ref0 = gw.pinned(X, Gp, Gi, tau, False)
    assert np.array_equal(np.isnan(got0), np.isnan(ref0))
    err0 = np.abs(np.abs(got0[fin]) - np.abs(ref0[fin]))
    assert (err0 <= b[fin]).all()
    decided = fin & (np.abs(mxp + mxn) > 2 * b)
    share = 1.0 - decided.sum() / fin.sum()
    print(f"  max_diff = FALSE: worst / b = {(err0 / b[fin]).max():.3g}, exempt from the sign check {100 * share:.2f} %")
    assert share <= 0.05
    assert np.array_equal(np.sign(got0[decided]), np.sign(ref0[decided]))


# ------------------------------------------------------------------------------------------------- 5. dgCMatrix
@pytest.mark.parametrize("density", [0.05, 0.6])
@pytest.mark.parametrize("rowtf", ["none", "ecdf", "z"])
def test_dgcmatrix_scores_equal_the_dense_form(hip_ctx, density, rowtf):
    """stored zeros and an empty column; integer values and 64 samples, so that the row moments of "z" are the same
    binary fractions whether summed over all entries or over the stored ones"""
    for g, n in ((3001, 64), (20000, 64)):
        Xs = _sparse(g, n, density, 31)
        Gp, Gi = _sets(g, 24)
        for tau in (0.0, 0.25, 1.0):
            dense = hip_ctx.gsva_exact(Xs.toarray(), Gp, Gi, tau, rowtf, True)
            same(hip_ctx.gsva_exact(Xs, Gp, Gi, tau, rowtf, True), dense, f"g={g} density={density} tau={tau} {rowtf}")
            if tau != 0.25 and rowtf != "z":
                same(dense, gw.pinned(gw.row_transform(Xs.toarray(), rowtf), Gp, Gi, tau, True), "dense form vs the pinned form")


# ------------------------------------------------------------------------------------------------- 6. sharding, modes
def _run_hook(nshards, X, Gp, Gi, tau, rowtf, max_diff, fail=-1):
    return sharded_hooks.score("gsva_exact", nshards, X, Gp, Gi, float(tau), ROWTF[rowtf], int(max_diff), fail=fail)


@pytest.mark.parametrize("kind", ["dense", "csc"])
@pytest.mark.parametrize("rowtf", ["none", "z"])
def test_sharded_engine_is_bit_identical(hip_ctx, kind, rowtf):
    """1, 2, 3 and 7 shards; the z transform of dense X cuts whole 128-column blocks, so 7 shards of 513 columns leave the
    last two empty; 5 columns over 7 shards leave empty shards on the other routes.  A dgCMatrix under "z": integer values
    and 64 samples, so that the rows' moments are exact however the stored values are split over the shards"""
    g = 3001
    Gp, Gi = _sets(g, 24)
    for n in ((513, 5) if rowtf == "none" else (513,) if kind == "dense" else (64, 5)):
        if kind == "dense":
            X = _exact_z_rows(g, n) if rowtf == "z" else _tied(g, n)
        else:
            X = _sparse(g, n, 0.05, 41)
        for tau, max_diff in ((0.0, True), (0.25, True), (1.0, False)):
            exp = hip_ctx.gsva_exact(X, Gp, Gi, tau, rowtf, max_diff)
            for nshards in (1, 2, 3, 7):
                rc, S = _run_hook(nshards, X, Gp, Gi, tau, rowtf, max_diff)
                assert rc == 0
                same(S, exp, f"{kind} {rowtf} n={n} nshards={nshards} tau={tau}")


def test_ecdf_over_several_shards_is_refused(hip_ctx):
    from plaid_amd._lib import load
    g, n = 500, 12
    X = _tied(g, n)
    Gp, Gi = _sets(g, 10)
    rc, _ = _run_hook(2, X, Gp, Gi, 1.0, "ecdf", True)
    assert rc != 0 and b"not sharded by sample" in load().plaidhip_last_error_string()
    rc, S = _run_hook(1, X, Gp, Gi, 1.0, "ecdf", True)
    assert rc == 0
    same(S, hip_ctx.gsva_exact(X, Gp, Gi, 1.0, "ecdf", True), "one shard")


def test_injected_shard_failure_returns_an_error(hip_ctx):
    from plaid_amd._lib import load
    g, n = 500, 300
    X = _exact_z_rows(g, 513)[:, :n]
    Gp, Gi = _sets(g, 10)
    for rowtf in ("none", "z"):
        rc, _ = _run_hook(3, X, Gp, Gi, 0.25, rowtf, True, fail=1)
        assert rc != 0 and b"injected failure" in load().plaidhip_last_error_string()


def test_multi_on_one_device_equals_the_context_call(hip_ctx):
    import plaid_amd
    g, n = 3001, 23
    Gp, Gi = _sets(g, 24)
    for X in (_tied(g, n), _sparse(g, n, 0.05, 43)):
        for tau, max_diff in ((0.0, False), (0.25, True)):
            same(plaid_amd.gsva_exact_multi(X, Gp, Gi, tau, "none", max_diff, devices=1),
                 hip_ctx.gsva_exact(X, Gp, Gi, tau, "none", max_diff), f"multi tau={tau}")


def test_mixed_mode_does_not_change_a_bit(hip_ctx):
    g, n = 3001, 33
    Xn, Xz = _tied(g, n), _exact_z_rows(g, n)
    Gp, Gi = _sets(g, 24)
    cases = [(Xn, "none", t) for t in (0.0, 0.25, 1.0)] + [(Xz, "z", 1.0), (Xz, "ecdf", 1.0)]
    exp = [hip_ctx.gsva_exact(X, Gp, Gi, t, tf) for X, tf, t in cases]
    hip_ctx.set_precision("mixed")
    try:
        got = [hip_ctx.gsva_exact(X, Gp, Gi, t, tf) for X, tf, t in cases]
    finally:
        hip_ctx.set_precision("f64")
    for e, o in zip(exp, got):
        same(o, e, "mixed mode")


# ------------------------------------------------------------------------------------------------- 7. alignment
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
    for tau in (0.0, 1.0, 0.25):
        got = plaid_amd.replaid_gsva_exact(X1, G1, tau=tau, rowtf="none", ctx=hip_ctx)
        exp = hip_ctx.gsva_exact(X0[perm], *plaid_amd.aligned_pattern(X1, G1), tau, "none")
        same(got.values, exp, f"alignment tau={tau}")
        assert list(got.rownames) == list(G1.colnames) and list(got.colnames) == list(X1.colnames)
        if tau != 0.25:
            same(got.values, gw.pinned(X0, Gp, Gi, tau), "alignment vs the pinned form")
    Xs = plaid_amd.NamedMatrix(sp.csc_matrix(np.round(X0[perm])), X1.rownames, X1.colnames)
    same(plaid_amd.replaid_gsva_exact(Xs, G1, tau=1, rowtf="none", ctx=hip_ctx).values,
         plaid_amd.replaid_gsva_exact(plaid_amd.NamedMatrix(np.round(X0[perm]), X1.rownames, X1.colnames), G1, tau=1,
                                      rowtf="none", ctx=hip_ctx).values, "sparse through the public entry")
    with pytest.raises(ValueError):
        plaid_amd.replaid_gsva_exact(X1, G1, tau=-1.0, ctx=hip_ctx)


# ------------------------------------------------------------------------------------------------- the device entry
def test_dev_entry_scores_the_device_ranks(hip_ctx):
    import torch
    dev = torch.device("cuda", 0)
    g, n = 3001, 19
    X = _tied(g, n)
    X[7, 2] = np.nan
    Gp, Gi = _sets(g, 24)
    m = len(Gp) - 1
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
    dGp, dGi = torch.from_numpy(Gp).to(dev), torch.from_numpy(Gi).to(dev)
    Q = torch.empty((n, g), dtype=torch.float64, device=dev)
    colnan = torch.empty((n,), dtype=torch.int32, device=dev)
    scratch = torch.empty(2 * g * n, dtype=torch.float64, device=dev)
    hip_ctx.dev_ssgsea_exact_operands(dX.data_ptr(), g, g, n, 0.0, Q.data_ptr(), g, scratch.data_ptr(), colnan.data_ptr())
    for tau in (0.0, 1.0, 0.5):
        for max_diff in (True, False):
            S = torch.full((n, m + 3), -7.0, dtype=torch.float64, device=dev)
            hip_ctx.dev_gsva_ks(Q.data_ptr(), g, colnan.data_ptr(), g, n, dGp.data_ptr(), dGi.data_ptr(), m, tau, max_diff,
                                S.data_ptr(), m + 3)
            torch.cuda.synchronize()
            out = S.cpu().numpy().T
            same(out[:m], hip_ctx.gsva_exact(X, Gp, Gi, tau, "none", max_diff), f"dev entry tau={tau}")
            assert (out[m:] == -7.0).all()
