"""replaid.ucell.exact and replaid.aucell.exact on the GPU (include/plaidhip.h: plaidhip_ucell_exact, plaidhip_aucell_exact,
their _multi forms, plaidhip_dev_truncated_ranks_f64 / _csc_f64; kernels_trunc.hip).

Every quantity before the one division is an exact integer, so the device returns the bits of the numpy form of
tests/helpers/truncated_exact.py: equality is the assertion, NaN positions included.  The case matrix of every N holds
normal, tied, count-like and signed columns, a constant, an all-zero and a NaN column, boundary tie groups whose average
rank is T, T + 0.5 and above T, columns with 1, < T, T and > T stored values and the zero-filling column of AUCell; its sets
have 0, 1, k, 63, 64, 65, 200 and N members.  auc itself cannot fall below 0 when K >= k (U2 <= 2 K T - K^2 + K - S2), so
its clamp is met at exactly 0 (one unweighted gene) and just above; total's clamp is met on both sides."""
import numpy as np
import pytest

import plaid_amd
from plaid_amd import _lib
from tests.helpers import truncated_exact as te
from tests.helpers import truncated_hooks as th

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(N):
    """the case matrix of N rows, its CSC form with some zeros stored, and down sets (the up sets in reverse order: the empty
    set pairs with the full one)"""
    if N not in _CASES:
        names, X, Gp, Gi = te.case(N)
        Xs = te.to_csc(X, np.random.default_rng(N), explicit=0.03)
        sizes = np.diff(Gp)[::-1]
        Dp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        Di = np.concatenate([Gi[Gp[j]:Gp[j + 1]] for j in range(len(Gp) - 2, -1, -1)]).astype(np.int32)
        _CASES[N] = (names, X, Xs, Gp, Gi, Dp, Di)
    return _CASES[N]


def _ranks(N):
    return te.rank_values(N) if N <= 257 else [2, te.K_SET, N - 1, N]


@pytest.mark.parametrize("N", te.SIZES + (te.BIG,))
def test_scores_have_the_bits_of_the_numpy_form(hip_ctx, N):
    names, X, Xs, Gp, Gi, _, _ = _case(N)
    assert N != te.BIG or np.diff(Xs.indptr).max() > 20352
    for T in _ranks(N):
        ref = te.ucell_exact(X, Gp, Gi, T)
        assert np.isnan(ref[:, names.index("nan")]).all() and np.isnan(ref[0]).all()
        te.assert_same_bits(hip_ctx.ucell_exact(X, Gp, Gi, max_rank=T)["UpScore"], ref, f"ucell dense N={N} T={T}")
        te.assert_same_bits(hip_ctx.ucell_exact(Xs, Gp, Gi, max_rank=T)["UpScore"], ref, f"ucell dgCMatrix N={N} T={T}")
        ref = te.aucell_exact(X, Gp, Gi, T)
        te.assert_same_bits(hip_ctx.aucell_exact(X, Gp, Gi, T), ref, f"aucell dense N={N} A={T}")
        te.assert_same_bits(hip_ctx.aucell_exact(Xs, Gp, Gi, T), ref, f"aucell dgCMatrix N={N} A={T}")


@pytest.mark.parametrize("N", (65, 257))
@pytest.mark.parametrize("sparse", (False, True))
def test_down_sets_w_neg_and_impute(hip_ctx, N, sparse):
    names, X, Xs, Gp, Gi, Dp, Di = _case(N)
    V = Xs if sparse else X
    T = te.K_SET + 1
    m = len(Gp) - 1
    kf = np.diff(Gp) + (np.arange(m) + 1) % 3 * 2.0           # larger than k for two sets in three, the empty one among them
    kd = np.diff(Dp) + 1.0
    for w_neg in (0.0, 1.0, 0.5):
        out = hip_ctx.ucell_exact(V, Gp, Gi, Dp, Di, max_rank=T, w_neg=w_neg)
        up, down = te.ucell_exact(X, Gp, Gi, T), te.ucell_exact(X, Dp, Di, T)
        te.assert_same_bits(out["UpScore"], up, "up")
        te.assert_same_bits(out["DownScore"], down, "down")
        total = te.ucell_total(up, down, w_neg)
        te.assert_same_bits(out["TotalScore"], total, f"total w_neg={w_neg}")
        assert np.isnan(total[m - 1]).all() and np.isnan(total[0]).all()    # an empty down (or up) column
        if w_neg == 1.0:
            ok = ~np.isnan(total)
            assert (total[ok] == 0.0).any() and (total[ok] > 0.0).any()     # both sides of the clamp
    out = hip_ctx.ucell_exact(V, Gp, Gi, Dp, Di, max_rank=T, w_neg=0.5, k_full=kf, k_full_down=kd)
    up, down = te.ucell_exact(X, Gp, Gi, T, kf), te.ucell_exact(X, Dp, Di, T, kd)
    assert not np.isnan(up[0, :3]).any()                                   # K = 2 with no aligned member: a score, not NaN
    te.assert_same_bits(out["UpScore"], up, "up, imputed")
    te.assert_same_bits(out["DownScore"], down, "down, imputed")
    te.assert_same_bits(out["TotalScore"], te.ucell_total(up, down, 0.5), "total, imputed")


def test_clamps(hip_ctx):
    """auc at exactly 0 and just above; total clamped and just above"""
    N, T = 64, 5
    x = np.arange(N, dtype=np.float64)                        # row N - 1 has d = 1
    X = np.asfortranarray(np.stack([x, x[::-1]], axis=1))
    Gp = np.array([0, 1, 2, 3], dtype=np.int32)
    Gi = np.array([0, N - T, N - 1], dtype=np.int32)            # in column 0: unweighted, d = T (u = 1), d = 1
    Dp = np.array([0, 1, 2, 3], dtype=np.int32)
    Di = np.array([N - 1, N - 1, N - T], dtype=np.int32)
    for V in (X, te.to_csc(X)):
        out = hip_ctx.ucell_exact(V, Gp, Gi, Dp, Di, max_rank=T, w_neg=1.0)
        up, down = te.ucell_exact(X, Gp, Gi, T), te.ucell_exact(X, Dp, Di, T)
        assert up[0, 0] == 0.0 and 0.0 < up[1, 0] < 0.21 and up[2, 0] == 1.0
        te.assert_same_bits(out["UpScore"], up, "up")
        total = te.ucell_total(up, down, 1.0)
        assert total[0, 0] == 0.0 and total[1, 0] == 0.0 and total[2, 0] > 0.0      # 0 - 1, 0.2 - 1, 1 - 0.2
        te.assert_same_bits(out["TotalScore"], total, "total")
        just = hip_ctx.ucell_exact(V, Gp, Gi, Dp, Di, max_rank=T, w_neg=0.125)["TotalScore"]
        te.assert_same_bits(just, te.ucell_total(up, down, 0.125), "total, w_neg = 1/8")
        assert just[1, 0] > 0.0


def _dev_lists(ctx, X, Xs, mode, T):
    import torch
    dev = torch.device("cuda", 0)
    g, n = X.shape
    i32 = dict(dtype=torch.int32, device=dev)
    colnan, counts, Wp = torch.empty(n, **i32), torch.empty(n, **i32), torch.empty(n + 1, **i32)
    out = []
    # dense
    cap = n * min(g, 2 * T - 1 if mode == "ucell" else T - 1)
    Wi = torch.full((max(cap, 1) + 8,), -7, **i32)
    Wx = torch.full((max(cap, 1) + 8,), -7.0, dtype=torch.float64, device=dev)
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
    R = torch.empty((n, g), dtype=torch.float64, device=dev)
    ctx.dev_truncated_ranks(dX.data_ptr(), g, g, n, mode, T, R.data_ptr(), colnan.data_ptr(), counts.data_ptr(), Wp.data_ptr(),
                            Wi.data_ptr(), Wx.data_ptr(), cap)
    torch.cuda.synchronize()
    out.append((Wp.cpu().numpy(), Wi.cpu().numpy(), Wx.cpu().numpy(), np.zeros(n), cap))
    # CSC
    nnz = int(Xs.indptr[-1])
    cap = nnz if mode == "ucell" else n * min(g, T - 1)
    Wi = torch.full((max(cap, 1) + 8,), -7, **i32)
    Wx = torch.full((max(cap, 1) + 8,), -7.0, dtype=torch.float64, device=dev)
    dp, di = torch.from_numpy(Xs.indptr.astype(np.int32)).to(dev), torch.from_numpy(Xs.indices.astype(np.int32)).to(dev)
    dx = torch.from_numpy(Xs.data).to(dev)
    scratch = torch.empty(2 * max(nnz, 1), dtype=torch.float64, device=dev)
    u0 = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    ctx.dev_truncated_ranks_csc(dp.data_ptr(), di.data_ptr(), dx.data_ptr(), g, n, int(np.diff(Xs.indptr).max()), nnz, mode, T,
                                scratch.data_ptr(), colnan.data_ptr(), counts.data_ptr(), u0.data_ptr(), Wp.data_ptr(),
                                Wi.data_ptr(), Wx.data_ptr(), cap)
    torch.cuda.synchronize()
    out.append((Wp.cpu().numpy(), Wi.cpu().numpy(), Wx.cpu().numpy(), u0.cpu().numpy(), cap))
    return out


@pytest.mark.parametrize("N", (63, 65, 257))
def test_columns_with_0_1_below_T_and_T_stored_values(hip_ctx, N):
    """the CSC form without explicit zeros: the all-zero column stores nothing, the others exactly 1, T - 3, T and T + 5
    values; then a matrix with no stored value at all (no rank pass runs).  Scores and the lists of the device entry."""
    names, X, _, Gp, Gi, _, _ = _case(N)
    K = te.K_SET
    Xs = te.to_csc(X)
    lens = dict(zip(names, np.diff(Xs.indptr)))
    assert (lens["zero"], lens["nnz_1"], lens["nnz_below_T"], lens["nnz_T"], lens["nnz_above_T"]) == (0, 1, K - 3, K, K + 5)
    empty = te.to_csc(np.zeros((N, 5)))
    assert empty.indptr[-1] == 0
    for V, D in ((Xs, X), (empty, np.zeros((N, 5), order="F"))):
        for T in (1, K - 1, K, K + 1, N):
            te.assert_same_bits(hip_ctx.ucell_exact(V, Gp, Gi, max_rank=T)["UpScore"], te.ucell_exact(D, Gp, Gi, T), f"ucell T={T}")
            te.assert_same_bits(hip_ctx.aucell_exact(V, Gp, Gi, T), te.aucell_exact(D, Gp, Gi, T), f"aucell A={T}")
        for mode in ("ucell", "aucell"):
            for T in (K, N):
                _, (Wp, Wi, Wx, gu0, cap) = _dev_lists(hip_ctx, D, V, mode, T)
                want, u0 = te.csc_lists(V, mode, T)
                assert Wp[0] == 0 and Wp[-1] == sum(len(r) for r, _ in want) <= cap
                for c, (rows, w) in enumerate(want):
                    assert np.array_equal(Wi[Wp[c]:Wp[c + 1]], rows) and np.array_equal(Wx[Wp[c]:Wp[c + 1]], w), (mode, T, c)
                assert (Wi[Wp[-1]:] == -7).all()
                assert np.array_equal(gu0, u0 if mode == "ucell" else np.zeros(V.shape[1]))
    # the zeros of an empty column are weighted in UCell mode when (N + 1) / 2 <= T, and fill AUCell's positions in row order
    lists, u0 = te.csc_lists(empty, "ucell", N)
    assert u0[0] == N + 1 - (N + 1) / 2 and len(lists[0][0]) == 0
    lists, _ = te.csc_lists(empty, "aucell", K)
    assert np.array_equal(lists[0][0], np.arange(K - 1))


@pytest.mark.parametrize("N", (65, 257))
@pytest.mark.parametrize("mode", ("ucell", "aucell"))
def test_compressed_columns(hip_ctx, N, mode):
    """plaidhip_dev_truncated_ranks_f64 / _csc_f64: the lists themselves -- rows ascending inside a column, weights equal,
    nothing written behind the last entry"""
    names, X, Xs, _, _, _, _ = _case(N)
    for T in (2, te.K_SET, N):
        dense, sparse = _dev_lists(hip_ctx, X, Xs, mode, T)
        want_d = te.dense_lists(X, mode, T)
        want_s, u0 = te.csc_lists(Xs, mode, T)
        for what, (Wp, Wi, Wx, gu0, cap), want in (("dense", dense, want_d), ("csc", sparse, want_s)):
            assert Wp[0] == 0 and Wp[-1] == sum(len(r) for r, _ in want) <= cap, (what, T)
            for c, (rows, w) in enumerate(want):
                assert np.array_equal(Wi[Wp[c]:Wp[c + 1]], rows), (what, T, names[c])
                assert np.array_equal(Wx[Wp[c]:Wp[c + 1]], w), (what, T, names[c])
            assert (Wi[Wp[-1]:] == -7).all() and (Wx[Wp[-1]:] == -7.0).all()
        assert np.array_equal(sparse[3], u0 if mode == "ucell" else np.zeros(len(names)))
    with pytest.raises(_lib.PlaidHipError):   # slots too small for what the columns may take: refused, nothing launched
        hip_ctx.dev_truncated_ranks(1, N, N, 4, mode, 5, 1, 1, 1, 1, 1, 1, 3)


@pytest.mark.parametrize("nshards", (1, 2, 3, 7, 40))
def test_every_sharding_returns_the_one_device_bits(hip_ctx, nshards):
    N, T = 257, te.K_SET + 1
    names, X, Xs, Gp, Gi, Dp, Di = _case(N)
    assert nshards <= 7 or nshards > len(names)
    kf = np.diff(Gp) + 1.0
    kd = np.diff(Dp) + 2.0
    for V in (X, Xs):
        one = hip_ctx.ucell_exact(V, Gp, Gi, Dp, Di, max_rank=T, w_neg=0.5, k_full=kf, k_full_down=kd)
        status, out = th.ucell_exact(nshards, V, Gp, Gi, Dp, Di, max_rank=T, w_neg=0.5, k_full=kf, k_full_down=kd)
        assert status == _lib.OK
        for k in one:
            te.assert_same_bits(out[k], one[k], f"{k}, {nshards} shards")
        status, S = th.aucell_exact(nshards, V, Gp, Gi, T)
        assert status == _lib.OK
        te.assert_same_bits(S, hip_ctx.aucell_exact(V, Gp, Gi, T), f"aucell, {nshards} shards")
    status, _ = th.aucell_exact(3, X, Gp, Gi, T, fail=1)
    assert status == _lib.EHIP


def test_multi_entries_on_one_device():
    N, T = 65, 9
    names, X, Xs, Gp, Gi, Dp, Di = _case(N)
    te.assert_same_bits(plaid_amd.aucell_exact_multi(Xs, Gp, Gi, T, devices=1), te.aucell_exact(X, Gp, Gi, T), "aucell_multi")
    out = plaid_amd.ucell_exact_multi(X, Gp, Gi, max_rank=T, devices=[0])
    te.assert_same_bits(out["UpScore"], te.ucell_exact(X, Gp, Gi, T), "ucell_multi")
    plaid_amd.multi_finalize()


def test_r_level_wrappers(hip_ctx):
    """replaid_ucell_exact / replaid_aucell_exact: alignment by name, impute's k_full from the un-aligned sets"""
    import scipy.sparse as sp
    N = 257
    names, X, Xs, Gp, Gi, Dp, Di = _case(N)
    rows = [f"g{i}" for i in range(N)]
    cols = [f"c{i}" for i in range(X.shape[1])]
    m = len(Gp) - 1
    G = sp.csc_matrix((np.ones(len(Gi)), Gi, Gp), shape=(N, m))
    extra = sp.csc_matrix(np.ones((2, m)))                                   # two genes X lacks, in every set
    matG = plaid_amd.NamedMatrix(sp.vstack([G, extra]).tocsc(), rows + ["absent1", "absent2"], [f"s{j}" for j in range(m)])
    for V in (X, Xs):
        Xn = plaid_amd.NamedMatrix(V, rows, cols)
        got = plaid_amd.replaid_ucell_exact(Xn, matG, maxRank=20, impute=True, ctx=hip_ctx)
        te.assert_same_bits(got["UpScore"].values, te.ucell_exact(X, Gp, Gi, 20, np.diff(Gp) + 2), "impute")
        got = plaid_amd.replaid_ucell_exact(Xn, matG, maxRank=20, ctx=hip_ctx)
        te.assert_same_bits(got["UpScore"].values, te.ucell_exact(X, Gp, Gi, 20), "no impute")
        A = int(np.ceil(0.05 * N))
        te.assert_same_bits(plaid_amd.replaid_aucell_exact(Xn, matG, ctx=hip_ctx).values, te.aucell_exact(X, Gp, Gi, A), "aucell")
    with pytest.raises(ValueError):
        plaid_amd.replaid_aucell_exact(plaid_amd.NamedMatrix(X, rows, cols), matG, aucMaxRank=N + 1, ctx=hip_ctx)
