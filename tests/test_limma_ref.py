"""plaid.limma on the host, without a GPU: the two restatements of tests/helpers/limma_ref.py against identities that depend
on neither, plaidhip_limma_design on ten fixed designs, and plaidhip_limma_finish against the 50-digit restatement on inputs
that take every branch of the empirical-Bayes step.

The tolerances of the last two are MEASURED, as DESIGN.md section 20 records: the worst relative deviation over these inputs
on the development host (glibc x86-64), times 8 for libm differences between hosts, and in no case looser than 1e-9."""
import numpy as np
import pytest

from plaid_amd import _lib, engine
from tests.helpers import limma_ref as lr

# worst deviation measured, and what is asserted: 8 times it
MEASURED = {"u": 5.3e-16, "df_prior": 2.4e-16, "s2_prior": 1.1e-15, "t": 2.3e-14, "p": 2.2e-14}
FACTOR = 8
BOUND = {k: FACTOR * v for k, v in MEASURED.items()}
assert all(b <= 1e-9 for b in BOUND.values())


# ---- 1. limma_np against identities that depend on neither restatement ---------------------------------------------------------
def test_limma_np_with_one_ok_row_is_the_pooled_t_test():
    import scipy.stats as st
    rng = np.random.default_rng(1)
    n = 13
    y = (rng.random(n) < 0.5).astype(float)
    y[:2] = [0, 1]
    X = rng.normal(size=(3, n)) + 0.8 * y
    X[0, 4] = np.nan
    X[2, 0] = np.nan
    res = lr.limma_np(X, np.column_stack([np.ones(n), y]), K=[0.0, 1.0])
    assert res["nok"] == 1 and res["df_prior"] == 0
    ref = st.ttest_ind(X[1, y == 1], X[1, y == 0], equal_var=True)
    np.testing.assert_allclose(res["t"][1, 0], ref.statistic, rtol=1e-12)
    np.testing.assert_allclose(res["p"][1, 0], ref.pvalue, rtol=1e-12)
    assert np.isnan(res["t"][[0, 2], 0]).all()


def test_limma_np_with_a_covariate_is_least_squares_on_the_explicit_design():
    rng = np.random.default_rng(2)
    n = 17
    y = (np.arange(n) % 2).astype(float)
    b = rng.normal(size=n)
    D = np.column_stack([np.ones(n), y, b])
    X = rng.normal(size=(20, n)) + np.outer(rng.normal(size=20), y) + np.outer(rng.normal(size=20), b)
    res = lr.limma_np(X, D, K=[0.0, 1.0, 0.0])
    Qn, Rn = np.linalg.qr(D)                                  # the normal equations' solution by another route
    beta = np.linalg.solve(Rn, Qn.T @ X.T)
    np.testing.assert_allclose(res["logFC"][:, 0], beta[1], rtol=1e-11, atol=1e-13)
    r = X.T - D @ beta
    np.testing.assert_allclose(res["s2"], (r * r).sum(axis=0) / (n - 3), rtol=1e-11)
    np.testing.assert_allclose(res["AveExpr"], X.mean(axis=1), rtol=1e-13)


def test_the_two_restatements_agree():
    X, Y, B = lr.branch_case("finite", rows=24)
    D, use = lr.contrast_design(Y, B, 1)
    a, b = lr.limma_mp(X, D, use, [0.0, 1.0, 0.0]), lr.limma_np(X, D, use, [0.0, 1.0, 0.0])
    assert a["branch"] == "finite" and a["nok"] == b["nok"] == 24
    assert lr.dev_rel(b["df_prior"], a["df_prior"]) < 1e-9 and lr.dev_rel(b["s2_prior"], a["s2_prior"]) < 1e-11
    assert lr.dev_t(b["t"][:, 0], [float(r["t"][0]) for r in a["rows"]]) < 1e-10
    assert lr.dev_p(b["p"][:, 0], [float(r["p"][0]) for r in a["rows"]]) < 1e-10


# ---- 2. plaidhip_limma_design ---------------------------------------------------------------------------------------------------
def designs():
    rng = np.random.default_rng(7)

    def groups(n, k):
        g = np.arange(n) % k
        rng.shuffle(g)
        return g

    def cov(n):
        b = rng.normal(size=n)
        return b - b.mean()

    out = []
    g = groups(12, 2)
    out.append(("two-group", np.column_stack([np.ones(12), g]), None, [[0.0], [1.0]]))
    g = groups(31, 2)
    out.append(("two-group n=31", np.column_stack([np.ones(31), g]), None, None))
    g = groups(15, 2)
    out.append(("two-group + centred covariate", np.column_stack([np.ones(15), g, cov(15)]), None, [[0.0], [1.0], [0.0]]))
    g = groups(40, 2)
    out.append(("two-group + two covariates", np.column_stack([np.ones(40), g, cov(40), cov(40)]), None, None))
    g = groups(18, 3)
    cell = np.column_stack([(g == k).astype(float) for k in range(3)])
    out.append(("three-group cell means", cell, None, [[-1.0, -1.0, 0.0], [1.0, 0.0, -1.0], [0.0, 1.0, 1.0]]))
    out.append(("p = 1", np.ones((9, 1)), None, None))
    out.append(("p = 1, scaled", np.full((5, 1), -2.5), None, [[3.0]]))
    out.append(("p = 32", rng.normal(size=(45, 32)), None, None))
    out.append(("n_f = p + 1", np.column_stack([np.ones(5), rng.normal(size=(5, 3))]), None, None))
    g = groups(30, 2)
    use = (np.arange(30) % 3 != 1).astype(np.int8)
    D = np.column_stack([np.ones(30), g, cov(30)])
    D[use == 0] = np.nan                                    # (an unused row may hold anything)
    out.append(("use drops a third", D, use, [[0.0], [1.0], [0.0]]))
    return out


DESIGNS = designs()
assert len(DESIGNS) == 10


@pytest.mark.parametrize("name,D,use,K", DESIGNS, ids=[d[0] for d in DESIGNS])
def test_limma_design(name, D, use, K):
    d = engine.limma_design(D, use, K)
    n, p = D.shape
    sel = np.arange(n) if use is None else np.flatnonzero(use)
    Q, R = d["Q"], d["R"]
    assert d["nf"] == len(sel) and not Q[np.setdiff1d(np.arange(n), sel)].any()
    assert not np.tril(R, -1).any()
    eps = p * n * 2.0 ** -53
    assert np.linalg.norm(Q.T @ Q - np.eye(p)) <= eps * np.sqrt(p)                        # ||I||_F
    assert np.linalg.norm(Q[sel] @ R - D[sel]) <= eps * np.linalg.norm(D[sel])
    ref = lr.mp_design(D, use, K)
    worst = max(lr.dev_rel(a, float(b)) for a, b in zip(d["u"], ref["u"]))
    print(f"[measure] limma_design {name}: worst relative deviation of u {worst:.3g}")
    assert worst <= BOUND["u"]
    Kc = np.eye(p) if K is None else np.asarray(K, dtype=float)
    np.testing.assert_allclose(R.T @ d["v"], Kc, rtol=0, atol=64 * p * 2.0 ** -53 * max(1.0, np.abs(Kc).max()))


# ---- 3. plaidhip_limma_finish against limma_mp, given exact E, M and RSS --------------------------------------------------------
@pytest.mark.parametrize("name", lr.BRANCH_CASES)
def test_limma_finish_against_50_digits(name):
    X, Y, B = lr.branch_case(name)
    D, use = lr.contrast_design(Y, B, 0)
    K = np.array([[0.0, 0.3], [1.0, -1.0], [0.0, 2.0]])
    des = lr.mp_design(D, use, K)
    fits = lr.mp_fit(X, des)
    ref = lr.mp_finish(fits, des)
    assert ref["branch"] == lr.EXPECTED_BRANCH[name], ref["branch"]
    rows, p, q = X.shape[0], 3, 2
    E = np.full((p + 1, rows), np.nan)
    rss = np.full((1, rows), np.nan)
    for r, f in enumerate(fits):
        if f is not None:
            E[:p, r], E[p, r], rss[0, r] = [float(e) for e in f[0]], float(f[1]), float(f[2])
    v = np.array([[float(x) for x in vj] for vj in des["v"]]).T
    out, hyper = engine.limma_finish(E, rss, [des["nf"]], v, [float(x) for x in des["u"]])
    assert hyper[0, 0] == des["nf"] - p and hyper[0, 3] == ref["nok"]
    ok = [r for r, f in enumerate(fits) if f is not None]
    assert np.isnan(out[[r for r in range(rows) if r not in ok]]).all() and not np.isnan(out[ok][:, [0, 1, 2, 3, 5]]).any()
    dev = {"df_prior": lr.dev_rel(hyper[0, 1], float(ref["df_prior"])), "s2_prior": lr.dev_rel(hyper[0, 2], float(ref["s2_prior"]))}
    t_ref = np.full((rows, q), np.nan)
    p_ref = np.full((rows, q), np.nan)
    for r in ok:
        t_ref[r], p_ref[r] = [float(x) for x in ref["rows"][r]["t"]], [float(x) for x in ref["rows"][r]["p"]]
    flat = lr.flat_rows(X, use)
    dev["t"] = 0.0
    for j in range(q):
        scale = np.array([float(ref["rows"][r]["mag"][j] / ref["rows"][r]["se"][j]) if fits[r] is not None else 0.0
                          for r in range(rows)])
        dev["t"] = max(dev["t"], lr.dev_t(out[:, 2, j, 0], t_ref[:, j], flat, scale))
    dev["p"] = lr.dev_p(out[:, 3, :, 0], p_ref)
    print(f"[measure] limma_finish {name} ({ref['branch']}): " + ", ".join(f"{k} {x:.3g}" for k, x in dev.items()))
    for k, x in dev.items():
        assert x <= BOUND[k], (k, x)
    for j in range(q):
        np.testing.assert_array_equal(out[:, 4, j, 0], lr.bh(out[:, 3, j, 0]))
        np.testing.assert_array_equal(out[ok, 5, j, 0], rss[0, ok] / (des["nf"] - p))
        np.testing.assert_array_equal(out[ok, 1, j, 0], E[p, ok])


def test_limma_finish_is_the_same_on_one_thread_and_on_many():
    """more rows than one host thread takes: the tails and Benjamini-Hochberg are dealt out, the result is the small call's"""
    rng = np.random.default_rng(5)
    rows, p, q = 70000, 2, 2
    E = rng.normal(size=(p + 1, rows))
    rss = rng.chisquare(6, size=(1, rows))
    v, u = rng.normal(size=(p, q)), np.array([0.4, 0.7])
    big, hb = engine.limma_finish(E, rss, [8], v, u)
    for lo in (0, 40000):
        small, _ = engine.limma_finish(E[:, lo:lo + 1000], rss[:, lo:lo + 1000], [8], v, u)
        np.testing.assert_array_equal(big[lo:lo + 1000, [0, 1, 5]], small[:, [0, 1, 5]])
    # t, P.Value and adj.P.Val of every row and both contrasts, from the returned hyper-parameters: a row or a column dealt to
    # the wrong thread would show here
    import scipy.stats as st
    d, d0, s0, nok = hb[0]
    s2 = rss[0] / d
    post = np.full(rows, s0) if np.isinf(d0) else (d * s2 + d0 * s0) / (d + d0)
    dft = nok * d if np.isinf(d0) else min(d + d0, nok * d)
    for j in range(q):
        fc = v[0, j] * E[0] + v[1, j] * E[1]
        np.testing.assert_allclose(big[:, 0, j, 0], fc, rtol=1e-13, atol=1e-15)
        t = big[:, 0, j, 0] / (u[j] * np.sqrt(post))
        np.testing.assert_allclose(big[:, 2, j, 0], t, rtol=1e-13)
        np.testing.assert_allclose(big[:, 3, j, 0], 2 * st.t.sf(np.abs(big[:, 2, j, 0]), dft), rtol=1e-9, atol=1e-300)
        np.testing.assert_array_equal(big[:, 4, j, 0], lr.bh(big[:, 3, j, 0]))
    assert hb[0, 3] == rows and np.isfinite(big[:, :4]).all() and (big[:, 4] >= big[:, 3] * (1 - 2.0 ** -52)).all()


def test_the_tile_is_the_headers():
    assert engine.limma_tile() == 8 and _lib.load().plaidhip_limma_tile() == 8
