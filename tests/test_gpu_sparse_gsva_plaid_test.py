"""replaid.gsva and plaid.test on a CSC matrix without densifying it (plaidhip_gsva_csc / plaidhip_plaid_test_csc): the
row view built on the device, its row moments and ECDF, against the oracle and the dense entries -- `pytest -m gpu`."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-9


def close(a, b, rtol=RTOL, atol=ATOL):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


def _oracle():
    from oracle import plaid_oracle
    return plaid_oracle


def _pattern(G):
    G = sp.csc_matrix(G)
    G.sort_indices()
    return G.indptr.astype(np.int32), G.indices.astype(np.int32)


def _edge_case_matrix(rounded, seed=11, g=2000, n=300):
    """~90 % zeros with the edge cases of the row view: genes 0 / 1 identical, gene 2 all zero, gene 3 stored in every
    cell, cell 5 empty, explicit stored zeros, negative values in some genes.  Returns (CSC, dup pair)."""
    rng = np.random.default_rng(seed)
    X = rng.gamma(2.0, 1.5, size=(g, n))
    if rounded:
        X = np.round(X, 1)
    X[rng.random(X.shape) < 0.9] = 0.0
    neg = rng.random(g) < 0.1
    X[neg, :] *= np.where(rng.random((int(neg.sum()), n)) < 0.5, -1.0, 1.0)
    X[1, :] = X[0, :]
    X[2, :] = 0.0
    X[3, :] = rng.gamma(2.0, 1.5, size=n) + (0.0 if not rounded else 0.05)
    if rounded:
        X[3, :] = np.round(X[3, :], 1)
    X[:, 5] = 0.0
    Xs = sp.csc_matrix(X)
    # explicit stored zeros: a few (row, column) pairs that are zero in X but stored
    extra_r = np.array([10, 11, 12, 40, 41, 2], dtype=np.int64)
    extra_c = np.array([0, 1, 2, 7, 7, 9], dtype=np.int64)
    keep = X[extra_r, extra_c] == 0.0
    coo = Xs.tocoo()
    rows = np.concatenate([coo.row, extra_r[keep]])
    cols = np.concatenate([coo.col, extra_c[keep]])
    vals = np.concatenate([coo.data, np.zeros(int(keep.sum()))])
    Xs = sp.csc_matrix((vals, (rows, cols)), shape=X.shape)
    Xs.sort_indices()
    assert Xs.nnz > sp.csc_matrix(X).nnz            # the stored zeros survived
    return Xs, (0, 1)


def _sets_with_dup_singletons(g, m, dup, seed=5):
    """m random sets plus two singleton sets holding the duplicated genes (the last two columns)"""
    rng = np.random.default_rng(seed)
    Gd = (rng.random((g, m)) < 0.03).astype(float)
    single = np.zeros((g, 2))
    single[dup[0], 0] = 1.0
    single[dup[1], 1] = 1.0
    return sp.csc_matrix(np.hstack([Gd, single]))


# ---------------------------------------------------------------- 1. gsva z on CSC vs the oracle
@pytest.mark.parametrize("tau", [0, 0.5])
def test_gsva_csc_z_matches_oracle_with_edge_cases(hip_ctx, tau):
    Xs, dup = _edge_case_matrix(rounded=False)
    g, n = Xs.shape
    G = _sets_with_dup_singletons(g, 60, dup)
    Gp, Gi = _pattern(G)
    rn = [f"g{k}" for k in range(g)]
    S = hip_ctx.gsva_csc(Xs.indptr, Xs.indices, Xs.data, g, Gp, Gi, tau, "z")
    close(S, _oracle().replaid_gsva(Xs, rn, G, rn, tau=tau))
    assert np.array_equal(S[-2, :], S[-1, :])       # identical genes: bitwise-identical score rows


# ---------------------------------------------------------------- 2. gsva ecdf: the dense entry's bits
@pytest.mark.parametrize("tau", [0, 0.5])
def test_gsva_csc_ecdf_is_bitwise_the_dense_entry(hip_ctx, tau):
    Xs, dup = _edge_case_matrix(rounded=True, seed=12)
    g, n = Xs.shape
    G = _sets_with_dup_singletons(g, 60, dup, seed=6)
    Gp, Gi = _pattern(G)
    S = hip_ctx.gsva_csc(Xs.indptr, Xs.indices, Xs.data, g, Gp, Gi, tau, "ecdf")
    D = hip_ctx.gsva(Xs.toarray(), Gp, Gi, tau, "ecdf")
    assert np.array_equal(S, D)
    rn = [f"g{k}" for k in range(g)]
    close(S, _oracle().replaid_gsva(Xs, rn, G, rn, tau=tau, rowtf="ecdf"))


# ---------------------------------------------------------------- 3. a row longer than 65,536 entries
def test_gsva_csc_long_rows(hip_ctx):
    rng = np.random.default_rng(13)
    g, n = 600, 70000
    nnz_col = 30
    rows = np.concatenate([np.sort(rng.choice(np.arange(1, g), nnz_col, replace=False)) for _ in range(n)])
    ptr = np.arange(0, (n + 1) * nnz_col, nnz_col)
    vals = np.round(rng.gamma(2.0, 1.5, size=rows.size), 2)
    X = sp.csc_matrix((vals, rows, ptr), shape=(g, n)).tolil()
    X[0, :] = np.round(rng.gamma(2.0, 1.5, size=(1, n)), 2) + 0.01     # gene 0 stored in every cell
    Xs = sp.csc_matrix(X)
    Xs.sort_indices()
    assert np.diff(Xs.tocsr().indptr).max() == n > 65536
    Gd = (rng.random((g, 40)) < 0.05).astype(float)
    Gd[0, 0] = 1.0
    G = sp.csc_matrix(Gd)
    Gp, Gi = _pattern(G)
    S = hip_ctx.gsva_csc(Xs.indptr, Xs.indices, Xs.data, g, Gp, Gi, 0.0, "ecdf")
    assert np.array_equal(S, hip_ctx.gsva(Xs.toarray(), Gp, Gi, 0.0, "ecdf"))
    Xz = Xs.copy()
    Xz.data = Xz.data + rng.random(Xz.nnz) * 1e-3                     # continuous: no exact ties between genes
    rn = [f"g{k}" for k in range(g)]
    close(hip_ctx.gsva_csc(Xz.indptr, Xz.indices, Xz.data, g, Gp, Gi, 0.0, "z"), _oracle().replaid_gsva(Xz, rn, G, rn))


# ---------------------------------------------------------------- 4. run-to-run bits at size
def test_gsva_csc_is_deterministic_at_size(hip_ctx):
    from plaid_amd import synth
    g, n = 20000, 4096
    Xp, Xi, Xx = synth.sparse_columns(g, 0, n, density=0.05)
    Gp, Gi = synth.geneset_csc(g, 500)
    a = hip_ctx.gsva_csc(Xp, Xi, Xx, g, Gp, Gi, 0.0, "z")
    b = hip_ctx.gsva_csc(Xp, Xi, Xx, g, Gp, Gi, 0.0, "z")
    assert np.all(np.isfinite(a))
    assert np.array_equal(a, b)


# ---------------------------------------------------------------- 5. plaid.test on CSC
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
    return Xs, Gs


_COLS = ["gsetFC", "p.one", "p.two", "p.lm", "p.meta", "q.meta"]


@pytest.mark.parametrize("metap", ["fisher", "stouffer"])
def test_plaid_test_csc_fixture_matches_oracle_and_vignette(hip_ctx, pbmc, golden_dir, metap):
    import plaid_amd
    d, _ = pbmc
    X = sp.csc_matrix((d["x"], d["i"], d["p"]), shape=tuple(d["dim"]))
    rn = list(d["rownames"])
    matG = plaid_amd.gmt2mat(plaid_amd.read_gmt(os.path.join(golden_dir, "hallmarks.gmt")))
    y = (d["celltype"] == "B").astype(np.int32)
    Xs, Gs = _aligned(X, rn, matG.values, matG.rownames)
    Gp, Gi = _pattern(Gs)
    mm = 1 if metap == "stouffer" else 0
    out = hip_ctx.plaid_test_csc(Xs.indptr, Xs.indices, Xs.data, Xs.shape[0], y, Gp, Gi, None, 7, mm)
    exp = _oracle().plaid_test(X, rn, y, sp.csc_matrix(matG.values), matG.rownames, None, metap_method=metap,
                               tests=("one", "two", "lm"))
    for k, nm in enumerate(_COLS):
        np.testing.assert_allclose(out[:, k], exp[nm], rtol=1e-7, atol=1e-300, err_msg=nm)
    if metap == "stouffer":
        # doc/plaid-vignette.html:857-869: tests = c("one", "lm"), sorted by p.meta
        out2 = hip_ctx.plaid_test_csc(Xs.indptr, Xs.indices, Xs.data, Xs.shape[0], y, Gp, Gi, None, 1 | 4, mm)
        o = np.argsort(out2[:, 4], kind="stable")
        names = [matG.colnames[j] for j in o[:6]]
        kat = {"HALLMARK_INTERFERON_GAMMA_RESPONSE": (0.003668116, 8.246828e-06, 3.868049e-07, 1.934024e-05),
               "HALLMARK_ALLOGRAFT_REJECTION": (0.102407488, 1.071307e-05, 4.781538e-05, 1.195384e-03),
               "HALLMARK_P53_PATHWAY": (0.038355508, 1.906952e-04, 8.369509e-05, 1.394918e-03),
               "HALLMARK_INTERFERON_ALPHA_RESPONSE": (0.032562973, 9.261621e-03, 1.491854e-03, 1.864818e-02),
               "HALLMARK_PEROXISOME": (0.016625538, 4.052692e-02, 3.080580e-03, 3.032190e-02),
               "HALLMARK_G2M_CHECKPOINT": (0.012385507, 6.049535e-02, 3.638628e-03, 3.032190e-02)}
        assert names == list(kat)
        for j, nm in zip(o[:6], names):
            np.testing.assert_allclose(out2[j, [1, 3, 4, 5]], kat[nm], rtol=2e-6, err_msg=nm)


def _synthetic_test_case(seed=17):
    rng = np.random.default_rng(seed)
    g, n, m = 700, 90, 25
    X = rng.gamma(2.0, 1.5, size=(g, n))
    X[rng.random(X.shape) < 0.85] = 0.0
    X[3, :] = 0.0
    X[4, :] = X[5, :]
    X[:, 7] = 0.0
    Xs = sp.csc_matrix(X)
    y = (rng.random(n) < 0.4).astype(np.int32)
    G = sp.csc_matrix((rng.random((g, m)) < 0.05).astype(float))
    return Xs, y, G


@pytest.mark.parametrize("tests", range(1, 8))
@pytest.mark.parametrize("given", [False, True])
def test_plaid_test_csc_synthetic_every_mask(hip_ctx, tests, given):
    Xs, y, G = _synthetic_test_case()
    g, n = Xs.shape
    Gp, Gi = _pattern(G)
    rn = [f"g{k}" for k in range(g)]
    names = [t for b, t in ((1, "one"), (2, "two"), (4, "lm")) if tests & b]
    gsetX = None
    if given:
        gsetX = np.asfortranarray(np.random.default_rng(3).normal(size=(G.shape[1], n)))
    for mm, metap in ((0, "fisher"), (1, "stouffer")):
        out = hip_ctx.plaid_test_csc(Xs.indptr, Xs.indices, Xs.data, g, y, Gp, Gi, gsetX, tests, mm)
        dense = hip_ctx.plaid_test(Xs.toarray(), y, Gp, Gi, gsetX, tests, mm)
        exp = _oracle().plaid_test(Xs, rn, y, G, rn, gsetX, metap_method=metap, tests=tuple(names))
        for k, nm in enumerate(_COLS):
            if nm in exp:
                close(out[:, k], exp[nm])
                close(out[:, k], dense[:, k])
            else:
                assert np.all(np.isnan(out[:, k])) and np.all(np.isnan(dense[:, k]))


def test_plaid_test_csc_errors_and_empty_shapes(hip_ctx):
    import plaid_amd
    Xs, y, G = _synthetic_test_case()
    g, n = Xs.shape
    Gp, Gi = _pattern(G)
    with pytest.raises(plaid_amd.PlaidHipError):
        hip_ctx.plaid_test_csc(Xs.indptr, Xs.indices, Xs.data, g, y * 2, Gp, Gi)
    bad_p = Xs.indptr.copy()
    bad_p[10] = bad_p[11] + 1                                 # not monotone
    with pytest.raises(plaid_amd.PlaidHipError):
        hip_ctx.plaid_test_csc(bad_p, Xs.indices, Xs.data, g, y, Gp, Gi)
    # n == 0: whatever the dense entry returns (NaN statistics); m == 0: nothing
    e = np.zeros(0)
    out0 = hip_ctx.plaid_test_csc(np.zeros(1, np.int32), e.astype(np.int32), e, g, np.zeros(0, np.int32), Gp, Gi)
    np.testing.assert_array_equal(out0, hip_ctx.plaid_test(np.zeros((g, 0)), np.zeros(0, np.int32), Gp, Gi))
    outm = hip_ctx.plaid_test_csc(Xs.indptr, Xs.indices, Xs.data, g, y, np.zeros(1, np.int32), np.zeros(0, np.int32))
    assert outm.shape == (0, 6)
    assert hip_ctx.plaid_test(Xs.toarray(), y, np.zeros(1, np.int32), np.zeros(0, np.int32)).shape == (0, 6)
    assert hip_ctx.gsva_csc(np.zeros(1, np.int32), e.astype(np.int32), e, g, Gp, Gi).shape == (G.shape[1], 0)


# ---------------------------------------------------------------- 6. the R-like API never densifies a sparse X
class _NoDense(sp.csc_matrix):
    def toarray(self, *a, **k):
        raise AssertionError("toarray called on a sparse input")

    def todense(self, *a, **k):
        raise AssertionError("todense called on a sparse input")

    def __array__(self, *a, **k):
        raise AssertionError("__array__ called on a sparse input")


def test_api_routes_sparse_input_without_densifying(hip_ctx, pbmc, golden_dir):
    import plaid_amd
    d, _ = pbmc
    X = sp.csc_matrix((d["x"], d["i"], d["p"]), shape=tuple(d["dim"]))
    matG = plaid_amd.gmt2mat(plaid_amd.read_gmt(os.path.join(golden_dir, "hallmarks.gmt")))
    y = (d["celltype"] == "B").astype(int)
    plain = plaid_amd.NamedMatrix(X, d["rownames"], d["colnames"])
    guarded = plaid_amd.NamedMatrix(X, d["rownames"], d["colnames"])
    guarded.values = _NoDense(plain.values)                      # every route below must leave the slots as they are
    for rowtf in ("z", "ecdf"):
        a = plaid_amd.replaid_gsva(guarded, matG, rowtf=rowtf, ctx=hip_ctx)
        b = plaid_amd.replaid_gsva(plain, matG, rowtf=rowtf, ctx=hip_ctx)
        assert np.array_equal(a.values, b.values) and a.rownames == b.rownames
    a = plaid_amd.plaid_test(guarded, y, matG, ctx=hip_ctx)
    b = plaid_amd.plaid_test(plain, y, matG, ctx=hip_ctx)
    assert np.array_equal(a.values, b.values) and a.rownames == b.rownames
