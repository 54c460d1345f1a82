"""The exact references of tests/helpers/gsva_ref.py and the inputs of tests/helpers/gsva_cases.py, checked on the host:
against 50-digit arithmetic at a tiny size, against the fp64 oracle, the z bound against numpy's own z, the separation
precondition for EVERY z input the GPU tests use (zero ambiguous pairs), and the sensitivity of every bound: a rank off
by 1/2, or a sign 0 -> -1, must break it."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import exact_ref as er
from tests.helpers import gsva_cases as gc
from tests.helpers import gsva_ref as gr

U = er.U
mp = None


def _need_mp():
    """mpmath for the 50-digit tests alone: the other tests of this file need nothing but numpy and scipy"""
    global mp
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50


def _oracle():
    from oracle import plaid_oracle
    return plaid_oracle


def _G(Gp, Gi, g):
    return sp.csc_matrix((np.ones(len(Gi)), Gi, Gp), shape=(g, len(Gp) - 1)), [str(k) for k in range(g)]


# ------------------------------------------------------------------ 50 digits, tiny
def _mp_median(v):
    v = sorted(v)
    k = len(v)
    return v[k // 2] if k % 2 else (v[k // 2 - 1] + v[k // 2]) / 2


def _mp_normalize(S, ignore_zero):
    m, n = len(S), len(S[0])
    med = []
    for c in range(n):
        col = [S[j][c] for j in range(m) if not (ignore_zero and S[j][c] == 0)]
        med.append(_mp_median(col) if col else mp.mpf(0))
    add = sum(med) / n
    return [[(S[j][c] - med[c]) + add for c in range(n)] for j in range(m)]


def _mp_ranks(col):
    """average ranks by counting: (#{<} + 1 + #{<=}) / 2"""
    return [(sum(1 for y in col if y < x) + 1 + sum(1 for y in col if y <= x)) / mp.mpf(2) for x in col]


def _mp_sets(Gp, Gi, W, wset):
    n = len(W[0])
    return [[wset[j] * sum(W[i][c] for i in Gi[Gp[j]:Gp[j + 1]]) for c in range(n)] for j in range(len(Gp) - 1)]


def _tiny(seed=3, g=14, n=5):
    rng = np.random.default_rng(seed)
    X = rng.gamma(2.0, 1.5, size=(g, n))
    X[1] = X[0]
    X[2] = gc.CONST
    Gp, Gi = gc.sets(g, 4, seed, kmin=1, kmax=6, force=(2,))
    return X, Gp, Gi


def _close_to_mp(ref, exact, what):
    exact = np.array([[float(v) for v in row] for row in exact])
    scale = np.abs(exact).max()
    assert np.abs(ref - exact).max() <= 4 * U * scale, what


@pytest.mark.parametrize("rowtf", ["z", "ecdf"])
@pytest.mark.parametrize("tau", gc.TAUS)
def test_gsva_ref_against_50_digits(tau, rowtf):
    _need_mp()
    X, Gp, Gi = _tiny()
    if rowtf == "ecdf":
        X = np.round(X, 0)
    g, n = X.shape
    M = [[mp.mpf(float(v)) for v in row] for row in X]
    if rowtf == "z":
        Z = []
        for row in M:
            mu = sum(row) / n
            sd = mp.sqrt(sum((v - mu) ** 2 for v in row) / (n - 1))
            Z.append([(v - mu) / (mp.mpf(1e-8) + sd) for v in row])
        assert all(v == 0 for v in Z[2])
        assert np.abs(np.array([[float(v) for v in r] for r in Z]) - gr.z_exact(X).astype(np.float64)).max() < 1e-15
    else:
        Z = [[mp.mpf(sum(1 for y in row if y <= v)) for v in row] for row in M]
    W = [[None] * n for _ in range(g)]
    p = mp.mpf(1.0 + tau)
    for c in range(n):
        r = _mp_ranks([abs(Z[i][c]) for i in range(g)])
        for i in range(g):
            W[i][c] = mp.sign(Z[i][c]) * r[i] ** p
    wmax = max(abs(v) for row in W for v in row)
    wset = [mp.mpf(float(v)) for v in gr._w(Gp)]
    S = [[v / wmax for v in row] for row in _mp_sets(Gp, Gi, W, wset)]
    N, B = gr.gsva_ref(X, Gp, Gi, tau, rowtf)
    _close_to_mp(N, _mp_normalize(S, False), (tau, rowtf))
    assert np.all(B > 0) and B.max() < 1e-13


@pytest.mark.parametrize("K", [1.0, 3.0, 14.0, 21.0])
def test_aucell_ref_against_50_digits(K):
    _need_mp()
    X, Gp, Gi = _tiny(seed=4)
    X = np.round(X, 0)
    g, n = X.shape
    R = [_mp_ranks([mp.mpf(float(v)) for v in X[:, c]]) for c in range(n)]
    rmax = max(max(col) for col in R)
    W = [[mp.mpf(1.08) * max((R[c][i] - (rmax - mp.mpf(K))) / mp.mpf(K), 0) for c in range(n)] for i in range(g)]
    S = _mp_sets(Gp, Gi, W, [mp.mpf(float(v)) for v in gr._w(Gp)])
    iz = min(v for row in S for v in row) == 0
    N, B, T, iz_ref = gr.aucell_ref(X, Gp, Gi, K)
    assert iz_ref == iz
    _close_to_mp(N, _mp_normalize(S, iz), K)


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("score_mean", [False, True])
@pytest.mark.parametrize("remove_log2", [True, False])
def test_scse_ref_against_50_digits(remove_log2, score_mean, sparse):
    _need_mp()
    X, Gp, Gi = _tiny(seed=5)
    X[X < 1.5] = 0.0
    X[4] *= -1.0
    g, n = X.shape
    Xin = gc._with_stored_zeros(X, [(r, c) for r, c in zip(*np.nonzero(X == 0.0))][:3]) if sparse else X
    stored = np.zeros(X.shape, dtype=bool)
    if sparse:
        stored[Xin.indices, np.repeat(np.arange(n), np.diff(Xin.indptr))] = True
    V = [[mp.mpf(float(v)) for v in row] for row in X]
    if remove_log2:
        V = [[mp.mpf(2) ** V[i][c] if (stored[i, c] if sparse else V[i][c] > 0) else V[i][c] for c in range(n)]
             for i in range(g)]
    w = [mp.mpf(float(v)) for v in gr._w(Gp)]
    if score_mean:
        S = _mp_sets(Gp, Gi, V, w)
        den = [sum(abs(V[i][c]) for i in range(g)) / g + mp.mpf(1e-8) for c in range(n)]
        exact = [[S[j][c] / den[c] for c in range(n)] for j in range(len(w))]
    else:
        S = _mp_sets(Gp, Gi, V, [mp.mpf(1)] * len(w))
        den = [sum(abs(V[i][c]) for i in range(g)) + mp.mpf(1e-8) for c in range(n)]
        exact = [[S[j][c] / den[c] * 100 for c in range(n)] for j in range(len(w))]
    ref, B, removed = gr.scse_ref(Xin, Gp, Gi, remove_log2, score_mean)
    assert removed == remove_log2
    _close_to_mp(ref, exact, (remove_log2, score_mean, sparse))


# ------------------------------------------------------------------ the fp64 oracle, to 1e-12
def _assert_1e12(ref, exp, what):
    np.testing.assert_allclose(ref, exp, rtol=1e-12, atol=1e-12, err_msg=str(what))


@pytest.mark.parametrize("name", ["g257", "n105", "n129"])
def test_gsva_ref_matches_the_oracle_dense(name):
    X, Gp, Gi, _ = gc.dense_case(name)
    G, rn = _G(Gp, Gi, X.shape[0])
    for tau in gc.TAUS:
        N, _ = gr.gsva_ref(X, Gp, Gi, tau, "z")
        _assert_1e12(N, _oracle().replaid_gsva(X, rn, G, rn, tau=tau), (name, tau))


@pytest.mark.parametrize("rowtf", ["z", "ecdf"])
def test_gsva_ref_matches_the_oracle_csc(rowtf):
    Xs, Gp, Gi, _ = gc.csc_case("const", rounded=rowtf == "ecdf")
    G, rn = _G(Gp, Gi, Xs.shape[0])
    for tau in (0.0, 0.5):
        N, _ = gr.gsva_ref(Xs.toarray(), Gp, Gi, tau, rowtf)
        _assert_1e12(N, _oracle().replaid_gsva(Xs, rn, G, rn, tau=tau, rowtf=rowtf), (rowtf, tau))


@pytest.mark.parametrize("sparse", [False, True])
def test_aucell_ref_matches_the_oracle(sparse):
    X, Gp, Gi = gc.aucell_case(257, sparse)
    G, rn = _G(Gp, Gi, 257)
    D = X.toarray() if sparse else X
    for K in gc.aucell_ks(257):
        N, _, _, _ = gr.aucell_ref(D, Gp, Gi, K)
        _assert_1e12(N, _oracle().replaid_aucell(X, rn, G, rn, auc_max_rank=K), (sparse, K))


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("kind", gc.SCSE_KINDS)
def test_scse_ref_matches_the_oracle(kind, sparse):
    X, Gp, Gi = gc.scse_case(kind, sparse)
    G, rn = _G(Gp, Gi, X.shape[0])
    for rl in (None, True, False):
        for sm in (False, True):
            ref, _, removed = gr.scse_ref(X, Gp, Gi, rl, sm)
            assert removed == (rl if rl is not None else kind == "nonneg")
            _assert_1e12(ref, _oracle().replaid_scse(X, rn, G, rn, remove_log2=rl, score_mean=sm), (kind, sparse, rl, sm))


# ------------------------------------------------------------------ the z bound and the precondition, every GPU input
@pytest.mark.parametrize("kind,name", gc.Z_INPUTS)
def test_every_z_input_is_separated_and_covered(kind, name):
    """zero ambiguous pairs (the precondition of the GPU tests, asserted and never skipped), and z_delta covers numpy's
    fp64 z, which sums pairwise and not in the device's order.  The margin is printed: gap / (2 (delta_a + delta_b))"""
    X, ties = gc.z_input(kind, name)
    Z = gr.z_exact(X)
    delta = gr.z_delta(X)
    amb, margin = gr.separated(Z, delta, ties)
    print(f"SEPARATED {kind} {name}: ambiguous {amb}, smallest margin {margin:.3g}, largest delta {delta.max():.3g}")
    assert amb == 0, (kind, name, amb, margin)
    assert margin > 4.0                                        # (not thin: another seed otherwise)
    for rows in ties:                                          # the declared ties are what they claim to be
        assert np.all(Z[rows] == Z[rows[0]])
        if len(rows) == 1:
            assert np.all(Z[rows[0]] == 0)
    with np.errstate(all="ignore"):
        Zn = (X - X.mean(axis=1, keepdims=True)) / (1e-8 + X.std(axis=1, ddof=1, keepdims=True))
    err = np.abs(Zn - Z.astype(np.float64))
    assert np.all(err <= delta), float((err / delta).max())
    free = np.setdiff1d(np.arange(X.shape[0]), [r for rows in ties if len(rows) == 1 for r in rows])
    assert delta[free].max() < 1e-10 and np.median(delta) < 1e-12   # of order n u mean|x| / sd, as derived


def test_separated_counts_what_it_should():
    Z = np.array([[1.0, 2.0], [1.0, 2.0], [0.0, 0.0], [3.0, 5.0], [3.0 + 1e-13, 1e-13]]).astype(gr.ld)
    d = np.full(Z.shape, 1e-13)
    amb, margin = gr.separated(Z[:4], d[:4], ([0, 1], [2]))
    assert amb == 0 and margin == pytest.approx(5e12)          # |z| = 1 over 2 delta (a declared zero's delta counts as 0)
    assert gr.separated(Z[:4], d[:4], ([2],))[0] == 2          # the undeclared tie of rows 0 / 1, once per column
    assert gr.separated(Z[:4], d[:4], ([0, 1],))[0] == 2       # the undeclared zeros of row 2
    assert gr.separated(Z[:4], d[:4], ([0, 3], [2]))[0] == 2   # declared together with another row: still undeclared ties
    # row 4: 3 + 1e-13 beside 3 (column 0), |z| = 1e-13 <= 2 delta and closer than 4 delta to the declared zero (column 1)
    assert gr.separated(Z, d, ([0, 1], [2]))[0] == 3


# ------------------------------------------------------------------ sensitivity
def _member(Gp, Gi, ties, j=0):
    """a member of set j outside the declared ties"""
    skip = {r for grp in ties for r in grp}
    return next(int(i) for i in Gi[Gp[j]:Gp[j + 1]] if int(i) not in skip)


@pytest.mark.parametrize("kind,name", gc.Z_INPUTS)
def test_gsva_bound_catches_half_a_rank_and_a_flipped_sign(kind, name):
    """the fp64 restatement is within the bound; with ONE rank off by 1/2, or the constant gene's sign 0 turned -1, it is
    not -- at every case and exponent.  And every bound is below 1/4 of the smallest raw move such an error can make"""
    if kind == "dense":
        X, Gp, Gi, ties = gc.dense_case(name)
    else:
        Xs, Gp, Gi, ties = gc.csc_case(name)
        X = Xs.toarray()
    i = _member(Gp, Gi, ties)
    for tau in gc.TAUS:
        N, B, _, _, wmax = gc.gsva_reference(kind, name, tau)
        assert er.bound_violations(gr.gsva_fp64(X, Gp, Gi, tau), N, B) == 0
        assert er.bound_violations(gr.gsva_fp64(X, Gp, Gi, tau, bump=(i, 1, "rank")), N, B) > 0
        assert er.bound_violations(gr.gsva_fp64(X, Gp, Gi, tau, bump=(2, 1, "sign")), N, B) > 0
        assert np.all(B < 0.25 * gr.gsva_min_move(Gp, tau, wmax)[:, None]), (name, tau)


@pytest.mark.parametrize("name", ["edge", "long"])
def test_gsva_ecdf_bound_catches_half_a_rank(name):
    Xs, Gp, Gi, ties = gc.csc_case(name, rounded=True)
    X = Xs.toarray()
    i = _member(Gp, Gi, ties)
    for tau in (0.0, 0.5):
        N, B, _, _, wmax = gc.gsva_reference("csc", name, tau, "ecdf")
        assert er.bound_violations(gr.gsva_fp64(X, Gp, Gi, tau, "ecdf"), N, B) == 0
        assert er.bound_violations(gr.gsva_fp64(X, Gp, Gi, tau, "ecdf", bump=(i, 1, "rank")), N, B) > 0
        assert np.all(B < 0.25 * gr.gsva_min_move(Gp, tau, wmax)[:, None])


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("g", gc.AUCELL_G)
def test_aucell_bound_catches_half_a_rank(g, sparse):
    """a top-ranked member's rank + 1/2 moves its weight by 1.08 / (2 K): outside the bound, which stays below 1/4 of that"""
    X, Gp, Gi = gc.aucell_case(g, sparse)
    D = X.toarray() if sparse else X
    top = int(Gi[Gp[-2]])                                      # the singleton set's gene: the unique maximum of column 2
    for K in gc.aucell_ks(g):
        N, B, T, iz = gr.aucell_ref(D, Gp, Gi, K)
        assert iz == (K < g)
        assert er.bound_violations(gr.aucell_fp64(D, Gp, Gi, K), N, B) == 0
        assert er.bound_violations(gr.aucell_fp64(D, Gp, Gi, K, bump=(top, 2)), N, B) > 0
        assert np.all(B < 0.25 * (1.08 * 0.5 / K) * gr._w(Gp)[:, None]), (g, K)


@pytest.mark.parametrize("sparse", [False, True])
def test_scse_bound_catches_fp32_inputs(sparse):
    """removeLog2 = FALSE, the fully derived bound: X rounded to fp32 (2^-24 relative on every term) is outside it"""
    X, Gp, Gi = gc.scse_case("signed", sparse)
    X32 = X.copy()
    if sparse:
        X32.data = X32.data.astype(np.float32).astype(np.float64)
    else:
        X32 = X32.astype(np.float32).astype(np.float64)
    G, rn = _G(Gp, Gi, X.shape[0])
    for sm in (False, True):
        ref, B, _ = gr.scse_ref(X, Gp, Gi, False, sm)
        assert er.bound_violations(_oracle().replaid_scse(X, rn, G, rn, remove_log2=False, score_mean=sm), ref, B) == 0
        bad = er.bound_violations(_oracle().replaid_scse(X32, rn, G, rn, remove_log2=False, score_mean=sm), ref, B)
        assert bad > 0.5 * ref.size
