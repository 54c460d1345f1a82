"""replaid.ucell / aucell / scse / gsva over several devices (plaidhip_*_multi, multi.cpp).

A 1-GPU box reaches the multi-device engine with ndev >= 2 through a test hook that runs it with `nshards` contexts on
device 0.  The context entries (plaidhip_ucell ... plaidhip_gsva_csc) are the same engine with one shard, so the
comparisons below say: every sharding equals the one-shard run.  Dense X bit for bit (the gsva row moments are chained
across the shards in the one-shard order); a dgCMatrix must agree with the one-shard run and with the oracle within the
suite's tolerance, and `removed_log2` must be the one-shard run's.
"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import sharded_hooks

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-9
UCELL, AUCELL, SCSE, GSVA = 3, 4, 5, 6


def close(a, b):
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL)


def same(a, b):
    assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _oracle():
    from oracle import plaid_oracle
    return plaid_oracle


run = sharded_hooks.scorer


def _ctx_args(X):
    return X if not sp.issparse(X) else sp.csc_matrix(X)


def _expected(hip_ctx, case, X, Gp, Gi, kf):
    """what the context entry gives for one case: (S, removed_log2 or None)"""
    kind, p = case
    Xa = _ctx_args(X)
    if kind == "ucell":
        return hip_ctx.ucell(Xa, Gp, Gi, kf, p["rmax"]), None
    if kind == "aucell":
        return hip_ctx.aucell(Xa, Gp, Gi, p["auc_max_rank"]), None
    if kind == "scse":
        S = hip_ctx.scse(Xa, Gp, Gi, p["remove_log2"], p["score_mean"])
        return S, int(hip_ctx.last_scse_removed_log2)
    if sp.issparse(X):
        Xs = sp.csc_matrix(X)
        return hip_ctx.gsva_csc(Xs.indptr, Xs.indices, Xs.data, X.shape[0], Gp, Gi, p["tau"], "z"), None
    return hip_ctx.gsva(X, Gp, Gi, p["tau"], "z"), None


def _oracle_scores(case, X, Gp, Gi):
    kind, p = case
    g, m = X.shape[0], len(Gp) - 1
    rn = [str(k) for k in range(g)]
    G = sp.csc_matrix((np.ones(len(Gi)), Gi, Gp), shape=(g, m))
    o = _oracle()
    with np.errstate(all="ignore"):
        if kind == "ucell":
            return o.replaid_ucell(X, rn, G, rn, rmax=p["rmax"])
        if kind == "aucell":
            return o.replaid_aucell(X, rn, G, rn, auc_max_rank=p["auc_max_rank"])
        if kind == "scse":
            return o.replaid_scse(X, rn, G, rn, remove_log2=p["remove_log2"], score_mean=p["score_mean"])
        return o.replaid_gsva(X, rn, G, rn, tau=p["tau"], rowtf="z")


def _run_case(nshards, case, X, Gp, Gi, kf, fail=-1):
    kind, p = case
    method = {"ucell": UCELL, "aucell": AUCELL, "scse": SCSE, "gsva": GSVA}[kind]
    return run(nshards, method, X, Gp, Gi, fail=fail, k_full=kf, **p)


CASES = ([("ucell", dict(rmax=1500.0)), ("ucell", dict(rmax=100.3)), ("aucell", dict(auc_max_rank=450.0))]
         + [("scse", dict(remove_log2=rl, score_mean=sm)) for rl in (None, True, False) for sm in (False, True)]
         + [("gsva", dict(tau=0.0)), ("gsva", dict(tau=0.5))])


def _sets(g, m=60):
    from plaid_amd import synth as sy
    Gp, Gi = sy.geneset_csc(g, m, kmin=3, kmax=300, sort_by_size=False)
    kf = np.diff(Gp).astype(np.float64)
    return Gp, Gi, kf


def _dense_inputs(g, n):
    """tied dense X (scse's removeLog2 = NULL: FALSE), and a non-negative one with zeros and max < 20 (TRUE)"""
    from plaid_amd import synth as sy
    X = sy.dense_columns(g, 0, n, tied=True)
    Xz = np.where(np.random.default_rng(n).random(X.shape) < 0.2, 0.0, np.abs(X))
    return [X, np.asfortranarray(Xz)]


def _ns(nshards):
    return sorted({n for n in (1, nshards - 1, 2 * nshards + 1, 37, 300) if n >= 1})


@pytest.mark.parametrize("g", [9000, 9001])
@pytest.mark.parametrize("nshards", [1, 2, 3, 5])
def test_dense_sharded_scorers_equal_the_context_entries(hip_ctx, nshards, g):
    Gp, Gi, kf = _sets(g)
    for n in _ns(nshards):
        for X in _dense_inputs(g, n):
            for case in CASES:
                rc, S, removed = _run_case(nshards, case, X, Gp, Gi, kf)
                assert rc == 0, (case, n)
                exp, exp_removed = _expected(hip_ctx, case, X, Gp, Gi, kf)
                assert np.array_equal(S, exp, equal_nan=True), (case, n, nshards, g)
                if exp_removed is not None:
                    assert removed == exp_removed, (case, n)


def _sparse_inputs(g, n):
    from plaid_amd import synth as sy
    Xp, Xi, Xx = sy.sparse_columns(g, 0, n)
    return sp.csc_matrix((Xx, Xi, Xp), shape=(g, n))


@pytest.mark.parametrize("g", [9000, 9001])
@pytest.mark.parametrize("nshards", [1, 2, 3, 5])
def test_sparse_sharded_scorers_agree_with_context_and_oracle(hip_ctx, nshards, g):
    Gp, Gi, kf = _sets(g)
    for n in _ns(nshards):
        Xs = _sparse_inputs(g, n)
        for case in CASES:
            rc, S, removed = _run_case(nshards, case, Xs, Gp, Gi, kf)
            assert rc == 0, (case, n)
            exp, exp_removed = _expected(hip_ctx, case, Xs, Gp, Gi, kf)
            close(S, exp)
            if exp_removed is not None:
                assert removed == exp_removed, (case, n)
            if n in (37, 300) or nshards == 3:
                close(S, _oracle_scores(case, Xs, Gp, Gi))
            if case[0] != "scse":   # (scse's sparse crossprod may add in arrival order; the others' is dense)
                rc2, S2, _ = _run_case(nshards, case, Xs, Gp, Gi, kf)    # deterministic for a given sharding
                assert rc2 == 0 and np.array_equal(S, S2, equal_nan=True), (case, n)


@pytest.mark.parametrize("nshards", [2, 3, 5])
def test_scse_remove_log2_is_decided_for_the_whole_matrix(hip_ctx, nshards):
    """removeLog2 = NULL (R/plaid.R:160-161) from min / max of ALL entries: a matrix whose only zeros are implicit, and
    one where the first shards store every entry (alone they would decide FALSE) while later shards have implicit zeros"""
    g = 501
    Gp, Gi, kf = _sets(g, 40)
    n = 4 * nshards + 1
    rng = np.random.default_rng(nshards)
    only_implicit = _sparse_inputs(g, n)
    assert only_implicit.data.min() > 0
    full = np.round(rng.uniform(0.5, 9.0, size=(g, n)), 1)
    lo, hi = 0, (n + nshards - 1) // nshards                         # the first shard of the plain split: all stored
    full[:, hi:] = np.where(rng.random((g, n - hi)) < 0.9, 0.0, full[:, hi:])
    mixed = sp.csc_matrix(full)
    assert np.all(np.diff(mixed.indptr)[lo:hi] == g) and mixed.nnz < g * n
    stored_only = sp.csc_matrix(np.round(rng.uniform(0.5, 9.0, size=(g, n)), 1))   # no zero at all: FALSE
    for Xs, want in ((only_implicit, 1), (mixed, 1), (stored_only, 0)):
        for sm in (False, True):
            case = ("scse", dict(remove_log2=None, score_mean=sm))
            rc, S, removed = _run_case(nshards, case, Xs, Gp, Gi, kf)
            assert rc == 0
            exp, exp_removed = _expected(hip_ctx, case, Xs, Gp, Gi, kf)
            assert removed == exp_removed == want
            close(S, exp)
            close(S, _oracle_scores(case, Xs, Gp, Gi))


def test_pbmc_fixture_at_three_shards_against_the_oracle(hip_ctx, pbmc, golden_dir):
    import plaid_amd
    d, e = pbmc
    X = sp.csc_matrix((d["x"], d["i"], d["p"]), shape=tuple(d["dim"]))
    Xn = plaid_amd.NamedMatrix(X, d["rownames"], d["colnames"])
    matG = plaid_amd.gmt2mat(plaid_amd.read_gmt(os.path.join(golden_dir, "hallmarks.gmt")))
    Gp, Gi = plaid_amd.aligned_pattern(Xn, matG)
    G = sp.csc_matrix(matG.values)
    kf = np.asarray((G != 0).sum(axis=0), dtype=np.float64).ravel()
    o = _oracle()
    rx, rg = list(d["rownames"]), list(matG.rownames)
    for Xin in (X, X.toarray()):
        rc, S, _ = run(3, UCELL, Xin, Gp, Gi, k_full=kf, rmax=1500.0)
        assert rc == 0
        close(S, o.replaid_ucell(X, rx, G, rg, rmax=1500))
        rc, S, _ = run(3, AUCELL, Xin, Gp, Gi, auc_max_rank=float(np.ceil(0.05 * X.shape[0])))
        assert rc == 0
        close(S, o.replaid_aucell(X, rx, G, rg))
        for sm in (False, True):
            rc, S, removed = run(3, SCSE, Xin, Gp, Gi, remove_log2=None, score_mean=sm)
            assert rc == 0 and removed == 1
            close(S, o.replaid_scse(X, rx, G, rg, score_mean=sm))
        # replaid.gsva: many genes of this fixture have z values that are equal in exact arithmetic (few small counts);
        # their ranks, and so the scores, follow the rounding of each implementation's row sums.  The one-device CSC
        # entry itself is ~2e-3 (relative) from the oracle here; a sharded dgCMatrix adds in yet another order, and a few
        # scores move against the CSC entry (seen: 2e-6 absolute).  Dense X: the chained sums are the one-device bits.
        for tau in (0.0, 0.5):
            rc, S, _ = run(3, GSVA, Xin, Gp, Gi, tau=tau)
            assert rc == 0
            if sp.issparse(Xin):
                np.testing.assert_allclose(S, hip_ctx.gsva_csc(X.indptr, X.indices, X.data, X.shape[0], Gp, Gi, tau, "z"),
                                           rtol=1e-4, atol=1e-5)
            else:
                same(S, hip_ctx.gsva(Xin, Gp, Gi, tau, "z"))


@pytest.mark.parametrize("nshards", [2, 3, 5])
def test_a_failing_shard_makes_the_call_fail(hip_ctx, nshards):
    from plaid_amd._lib import load
    g, n = 2001, 300
    Gp, Gi, kf = _sets(g, 30)
    X = _dense_inputs(g, n)[0]
    Xs = _sparse_inputs(g, n)
    for case in (CASES[0], CASES[2], CASES[3], CASES[-1]):
        for Xin in (X, Xs):
            for fail in (0, nshards - 1):
                rc, _, _ = _run_case(nshards, case, Xin, Gp, Gi, kf, fail=fail)
                assert rc != 0, case
                assert b"injected failure" in load().plaidhip_last_error_string()
    rc, S, _ = _run_case(nshards, CASES[-1], X, Gp, Gi, kf)                 # and the engine is usable afterwards
    assert rc == 0 and np.array_equal(S, hip_ctx.gsva(X, Gp, Gi, CASES[-1][1]["tau"], "z"), equal_nan=True)


def test_public_entries_with_one_device(hip_ctx):
    import plaid_amd
    g, n = 3001, 37
    Gp, Gi, kf = _sets(g)
    X = _dense_inputs(g, n)[1]
    Xs = _sparse_inputs(g, n)
    for devices in (1, [0]):
        same(plaid_amd.ucell_multi(X, Gp, Gi, kf, 1500.0, devices=devices), hip_ctx.ucell(X, Gp, Gi, kf, 1500.0))
        same(plaid_amd.aucell_multi(X, Gp, Gi, 150.0, devices=devices), hip_ctx.aucell(X, Gp, Gi, 150.0))
        S, removed = plaid_amd.scse_multi(X, Gp, Gi, None, True, devices=devices)
        same(S, hip_ctx.scse(X, Gp, Gi, None, True))
        assert removed == hip_ctx.last_scse_removed_log2
        same(plaid_amd.gsva_multi(X, Gp, Gi, 0.5, "z", devices=devices), hip_ctx.gsva(X, Gp, Gi, 0.5, "z"))
        close(plaid_amd.ucell_multi(Xs, Gp, Gi, kf, 1500.0, devices=devices), hip_ctx.ucell(Xs, Gp, Gi, kf, 1500.0))
        close(plaid_amd.gsva_multi(Xs, Gp, Gi, 0.0, devices=devices),
              hip_ctx.gsva_csc(Xs.indptr, Xs.indices, Xs.data, g, Gp, Gi, 0.0, "z"))
    for f in (lambda: plaid_amd.ucell_multi(X, Gp, Gi, kf, devices=[0, 0]),
              lambda: plaid_amd.aucell_multi(X, Gp, Gi, 150.0, devices=[0, 0]),
              lambda: plaid_amd.scse_multi(X, Gp, Gi, devices=[0, 0]),
              lambda: plaid_amd.gsva_multi(X, Gp, Gi, devices=[0, 0])):
        with pytest.raises(plaid_amd.PlaidHipError, match="twice"):
            f()
    plaid_amd.multi_finalize()


def test_gsva_ecdf_is_not_sharded(hip_ctx):
    import plaid_amd
    g, n = 3001, 37
    Gp, Gi, kf = _sets(g)
    X = _dense_inputs(g, n)[0]
    before = hip_ctx.gsva(X, Gp, Gi, 0.0, "ecdf")
    with pytest.raises(plaid_amd.PlaidHipError, match="ecdf"):
        plaid_amd.gsva_multi(X, Gp, Gi, rowtf="ecdf", devices=1)
    rc, _, _ = run(2, GSVA, X, Gp, Gi, rowtf=1)
    assert rc != 0
    same(hip_ctx.gsva(X, Gp, Gi, 0.0, "ecdf"), before)
    rn = [str(k) for k in range(g)]
    G = sp.csc_matrix((np.ones(len(Gi)), Gi, Gp), shape=(g, len(Gp) - 1))
    close(before, _oracle().replaid_gsva(X, rn, G, rn, rowtf="ecdf"))
