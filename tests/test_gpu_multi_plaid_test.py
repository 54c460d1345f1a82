"""plaid.test over several devices (plaidhip_plaid_test_multi, multi.cpp).

A 1-GPU box reaches the multi-device engine with ndev >= 2 through a test hook that runs it with `nshards` contexts on
device 0.  plaidhip_plaid_test / plaidhip_plaid_test_csc are the same engine with one shard, so the comparisons below
say: every sharding equals the one-shard run.  Dense X bit for bit, NaNs included, for every `tests` mask, both meta-p
methods and with gsetX given or computed (the shards are cut at 128-column blocks and every sum over the samples is
chained from shard to shard in the one-shard order).  A dgCMatrix adds its shards' sums in shard order: it must agree
with the one-shard run and with the oracle within the suite's plaid.test tolerances.
"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers.plaid_test_sharded import run

pytestmark = pytest.mark.gpu

RTOL_ENTRY, RTOL_ORACLE = 1e-9, 1e-7          # tests/test_gpu_parity.py: the sharded plaid.test's tolerances
COLS = ["gsetFC", "p.one", "p.two", "p.lm", "p.meta", "q.meta"]
ALL_TESTS = [(t, mp) for t in range(1, 8) for mp in (0, 1)]
SOME_TESTS = [(7, 0), (4, 1), (5, 1), (3, 0)]


def _oracle():
    from oracle import plaid_oracle
    return plaid_oracle


def same(a, b, what=""):
    assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), what


def _sets(g, m=120, seed=3):
    from plaid_amd import synth
    return synth.geneset_csc(g, m, kmin=3, kmax=200, seed=seed)


def _dense(g, n, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.gamma(2.0, 1.0, size=(g, n))
    X[rng.random(X.shape) < 0.3] = 0.0
    X[7, :] = X[8, :]
    return X


def _gsetX(m, n, seed=9):
    rng = np.random.default_rng(seed)
    S = rng.normal(size=(m, n))
    S[2, 5 % n] = np.nan                       # a NaN score: its set's Welch statistics are NaN on every route
    return np.asfortranarray(S)


def _labels(n, kind, seed=1):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return (rng.random(n) < 0.4).astype(np.int32)
    if kind == "first_block":                  # every y == 1 column in the first 128: later shards have none
        y = np.zeros(n, dtype=np.int32)
        y[rng.choice(128, 40, replace=False)] = 1
        return y
    return np.zeros(n, dtype=np.int32)         # n1 == 0: group 1 is empty (NaN means)


# (g, n, labels): odd g with n not a multiple of 128; n < 128 * nshards (empty shards); a shard without y == 1; n1 == 0;
# shards large enough for the pipelined upload (the crossprod runs panel by panel behind the DMA)
DENSE_CASES = [(2001, 1000, "random"), (1500, 200, "random"), (1200, 700, "first_block"), (999, 333, "none"),
               (5001, 2300, "random")]


@pytest.mark.parametrize("nshards", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("case", range(len(DENSE_CASES)))
def test_dense_equals_the_single_device_entry_bit_for_bit(hip_ctx, case, nshards):
    g, n, kind = DENSE_CASES[case]
    Gp, Gi = _sets(g)
    m = len(Gp) - 1
    X = _dense(g, n)
    y = _labels(n, kind)
    S = _gsetX(m, n)
    grid = ALL_TESTS if case == 0 else SOME_TESTS
    for tests, mp in grid:
        for gx in (None, S):
            exp = hip_ctx.plaid_test(X, y, Gp, Gi, gx, tests, mp)
            rc, got = run(nshards, X, y, Gp, Gi, gx, tests, mp)
            assert rc == 0
            same(got, exp, f"tests={tests} metap={mp} gsetX={'given' if gx is not None else 'NULL'}")
            if kind == "none":                 # group 1 empty: its means, and so the effect sizes, are NaN
                assert np.isnan(got[:, 0]).all()


def _csc_case(g=1800, n=900, seed=21):
    rng = np.random.default_rng(seed)
    X = rng.gamma(2.0, 1.5, size=(g, n))
    X[rng.random(X.shape) < 0.95] = 0.0        # ~5 % stored
    X[3, :] = 0.0
    X[:, 11] = 0.0
    Xs = sp.csc_matrix(X)
    Xs.sort_indices()
    y = (rng.random(n) < 0.35).astype(np.int32)
    return Xs, y


@pytest.mark.parametrize("nshards", [1, 2, 3, 4])
def test_csc_agrees_with_the_csc_entry_and_the_oracle(hip_ctx, nshards):
    Xs, y = _csc_case()
    g, n = Xs.shape
    Gp, Gi = _sets(g, 80, seed=4)
    m = len(Gp) - 1
    G = sp.csc_matrix((np.ones(len(Gi)), Gi, Gp), shape=(g, m))
    rn = [str(k) for k in range(g)]
    S = _gsetX(m, n)
    S[2, 5] = 0.25
    po = _oracle()
    for tests, mp in ((7, 0), (1 | 4, 1), (2, 0)):
        for gx in (None, S):
            exp = hip_ctx.plaid_test_csc(Xs.indptr, Xs.indices, Xs.data, g, y, Gp, Gi, gx, tests, mp)
            rc, got = run(nshards, Xs, y, Gp, Gi, gx, tests, mp)
            assert rc == 0
            names = [nm for b, nm in ((1, "one"), (2, "two"), (4, "lm")) if tests & b]
            ora = po.plaid_test(Xs, rn, y, G, rn, gx, metap_method="stouffer" if mp else "fisher", tests=tuple(names))
            for k, nm in enumerate(COLS):
                np.testing.assert_allclose(got[:, k], exp[:, k], rtol=RTOL_ENTRY, atol=1e-300, err_msg=f"{tests} {nm}")
                if nm in ora:
                    np.testing.assert_allclose(got[:, k], ora[nm], rtol=RTOL_ORACLE, atol=1e-300, err_msg=f"{tests} {nm}")
                else:
                    assert np.isnan(got[:, k]).all()


def _aligned(X, xrn, G, grn):
    """X[gg, ], G[gg, ] as plaid_amd.plaid_test aligns them (R/plaid.R:403-405)"""
    posx = {}
    for k, nm in enumerate(xrn):
        posx.setdefault(nm, k)
    seen, grow, xrow = set(), [], []
    for k, nm in enumerate(grn):
        if nm in seen:
            continue
        seen.add(nm)
        if nm in posx:
            grow.append(k)
            xrow.append(posx[nm])
    Xs = sp.csc_matrix(X)[xrow, :].tocsc()
    Xs.sort_indices()
    Gs = sp.csc_matrix(G)[grow, :].tocsc()
    Gs.eliminate_zeros()
    Gs.sort_indices()
    return Xs, Gs


@pytest.mark.parametrize("nshards", [2, 3])
def test_vignette_fixture_through_the_multi_path(hip_ctx, pbmc, golden_dir, nshards):
    """the vignette's known answers (doc/plaid-vignette.html:857-869, tests = c("one", "lm"), stouffer) through the
    sharded engine, dgCMatrix and dense, as tests/test_gpu_parity.py checks the single-device entry"""
    import plaid_amd
    d, _ = pbmc
    X = sp.csc_matrix((d["x"], d["i"], d["p"]), shape=tuple(d["dim"]))
    rn = list(d["rownames"])
    matG = plaid_amd.gmt2mat(plaid_amd.read_gmt(os.path.join(golden_dir, "hallmarks.gmt")))
    y = (d["celltype"] == "B").astype(np.int32)
    Xs, Gs = _aligned(X, rn, matG.values, matG.rownames)
    Gp, Gi = Gs.indptr.astype(np.int32), Gs.indices.astype(np.int32)
    kat = {"HALLMARK_INTERFERON_GAMMA_RESPONSE": (0.003668116, 8.246828e-06, 3.868049e-07, 1.934024e-05),
           "HALLMARK_ALLOGRAFT_REJECTION": (0.102407488, 1.071307e-05, 4.781538e-05, 1.195384e-03),
           "HALLMARK_P53_PATHWAY": (0.038355508, 1.906952e-04, 8.369509e-05, 1.394918e-03),
           "HALLMARK_INTERFERON_ALPHA_RESPONSE": (0.032562973, 9.261621e-03, 1.491854e-03, 1.864818e-02),
           "HALLMARK_PEROXISOME": (0.016625538, 4.052692e-02, 3.080580e-03, 3.032190e-02),
           "HALLMARK_G2M_CHECKPOINT": (0.012385507, 6.049535e-02, 3.638628e-03, 3.032190e-02)}
    Xd = Xs.toarray()
    same(run(nshards, Xd, y, Gp, Gi, None, 1 | 4, 1)[1], hip_ctx.plaid_test(Xd, y, Gp, Gi, None, 1 | 4, 1))
    for Xin in (Xs, Xd):
        rc, out = run(nshards, Xin, y, Gp, Gi, None, 1 | 4, 1)
        assert rc == 0
        o = np.argsort(out[:, 4], kind="stable")
        names = [matG.colnames[j] for j in o[:6]]
        assert names == list(kat)
        for j, nm in zip(o[:6], names):
            np.testing.assert_allclose(out[j, [1, 3, 4, 5]], kat[nm], rtol=2e-6, err_msg=nm)


def test_public_entry_with_one_device(hip_ctx):
    import plaid_amd
    g, n = 1201, 450
    Gp, Gi = _sets(g, 60)
    X = _dense(g, n)
    y = _labels(n, "random")
    S = _gsetX(len(Gp) - 1, n)
    for devices in (1, [0]):
        same(plaid_amd.plaid_test_multi(X, y, Gp, Gi, devices=devices), hip_ctx.plaid_test(X, y, Gp, Gi))
        same(plaid_amd.plaid_test_multi(X, y, Gp, Gi, gsetX=S, tests=4, metap_method=1, devices=devices),
             hip_ctx.plaid_test(X, y, Gp, Gi, S, 4, 1))
    Xs, ys = _csc_case(900, 400)
    Gp2, Gi2 = _sets(900, 40)
    np.testing.assert_allclose(plaid_amd.plaid_test_multi(Xs, ys, Gp2, Gi2, devices=1),
                               hip_ctx.plaid_test_csc(Xs.indptr, Xs.indices, Xs.data, 900, ys, Gp2, Gi2),
                               rtol=RTOL_ENTRY, atol=1e-300)
    with pytest.raises(plaid_amd.PlaidHipError, match="twice"):
        plaid_amd.plaid_test_multi(X, y, Gp, Gi, devices=[0, 0])
    plaid_amd.multi_finalize()


@pytest.mark.parametrize("nshards", [2, 4])
def test_a_failing_shard_makes_the_call_fail(hip_ctx, nshards):
    from plaid_amd._lib import load
    g, n = 1001, 600
    Gp, Gi = _sets(g, 50)
    X = _dense(g, n)
    Xs, _ = _csc_case(g, n)
    y = _labels(n, "random")
    for Xin in (X, Xs):
        for tests in (7, 3):
            for fail in (0, nshards - 1):
                rc, _ = run(nshards, Xin, y, Gp, Gi, None, tests, 0, fail=fail)
                assert rc != 0
                assert b"injected failure" in load().plaidhip_last_error_string()
    rc, out = run(nshards, X, y, Gp, Gi)                                     # and the engine is usable afterwards
    assert rc == 0
    same(out, hip_ctx.plaid_test(X, y, Gp, Gi))
