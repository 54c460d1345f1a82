"""Every fp64 crossprod route against an exact reference, at the fp64 error bound of each score -- `pytest -m gpu`.

The bound is (k + c) 2^-53 mag per element (tests/helpers/exact_ref.py): k nonzero terms summed in any order, c the
roundings after the sum.  The epilogue of the crossprod kernels is alpha * (sum * w) + beta * (k * w) with
w = fl(1 / (1e-8 + k)) (mean) or 1 (sum); the tests restate it with the same fp64 w, so for alpha = 1, beta = 0:
  sum:  c = 1  (the reference's own rounding to fp64)
  mean: c = 3  (reference rounding, the test's fl(ref * w), the kernel's fl(sum * w); mag scaled by w)
Two kinds of data: well-conditioned (bound ~1e-13 relative) and signed +-1e6 offsets that cancel (mag >> |S|), where a
relative tolerance means nothing.  A mixed-precision run (fp32 staging) must FAIL the bound: the tests see it."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import exact_ref as er
from tests.helpers.gsva_ref import _long_sums, _normalized_ref, _w
from tests.helpers.pow_ref import pow_allowance_u

pytestmark = pytest.mark.gpu


def _sets(g, m, seed, kmax=500):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, min(g, kmax) + 1, size=m)
    sizes[0] = 1
    sizes[-1] = min(g, kmax)
    sets = [np.sort(rng.choice(g, size=int(s), replace=False)) for s in sizes]
    sets[1 % m] = np.array([g - 1])                        # the last gene (odd g: staged on its own)
    Gp = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    Gi = np.concatenate(sets).astype(np.int32)
    return Gp, Gi


def _data(kind, g, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "well":
        return rng.gamma(2.0, 1.0, size=(g, n)) + 0.25
    return np.where(rng.random((g, n)) < 0.5, 1e6, -1e6) + rng.normal(size=(g, n))


def _check_mean_and_sum(got_mean, got_sum, Gp, Gi, X, what):
    ref, mag, k = er.set_sums(Gp, Gi, X)
    w = _w(Gp)[:, None]
    er.assert_fp64_bound(got_sum, ref, mag, k, 1, what + " sum")
    er.assert_fp64_bound(got_mean, ref * w, mag * w, k, 3, what + " mean")


@pytest.mark.parametrize("kernel", ["pair", "single"])
@pytest.mark.parametrize("g,n,m", [(10224, 9, 130), (10226, 5, 130), (20448, 1, 200), (20449, 33, 300), (30001, 5, 150),
                                   (45000, 9, 90), (333, 1, 40)])
def test_dense_kernels_within_the_fp64_bound(pinned_ctx, kernel, g, n, m):
    """the pair kernel and the one-column kernel, odd n, at and above the LDS limit (1 ... 3 gene slices), set sizes
    1 ... 500, raw sums and means (normalize = FALSE), well-conditioned and cancelling data"""
    ctx = pinned_ctx(spmm_dense_kernel=kernel)
    Gp, Gi = _sets(g, m, g + n)
    for kind in ("well", "cancel"):
        X = _data(kind, g, n, g * 7 + n)
        _check_mean_and_sum(ctx.plaid_dense(X, Gp, Gi, "mean", False), ctx.plaid_dense(X, Gp, Gi, "sum", False), Gp, Gi, X,
                            f"{kernel} {kind}")


def test_dense_device_entry_with_even_stride_and_odd_genes():
    """dev_spmm_dense with ldx = g + 1 (even) and odd g, pair kernel: stride padding untouched, scores within the bound"""
    import torch
    import plaid_amd
    g, n, m = 20449, 5, 90
    Gp, Gi = _sets(g, m, 3)
    dev = torch.device("cuda", 0)
    ctx = plaid_amd.Context(0)
    gs = None
    try:
        ctx.set_option("spmm_dense_kernel", "pair")
        gs = ctx.geneset(g, Gp, Gi)
        for kind in ("well", "cancel"):
            X = _data(kind, g, n, 5)
            Xd = torch.zeros((n, g + 1), dtype=torch.float64, device=dev)
            Xd[:, :g] = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
            Sd = torch.full((n, m + 3), -7.0, dtype=torch.float64, device=dev)
            fl = torch.zeros(4, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            ctx.dev_spmm_dense(gs, Xd.data_ptr(), g + 1, n, Sd.data_ptr(), m + 3, "sum", 1.0, 0.0, fl.data_ptr())
            ctx.synchronize()
            S = Sd.cpu().numpy()
            assert np.all(S[:, m:] == -7.0)
            ref, mag, k = er.set_sums(Gp, Gi, X)
            er.assert_fp64_bound(S[:, :m].T, ref, mag, k, 1, kind)
    finally:
        if gs is not None:
            gs.close()
        ctx.close()


def test_mixed_precision_fails_the_fp64_bound():
    """sensitivity: the opt-in mixed mode (dense X staged as fp32, default kernel choice) must be CAUGHT by the bound on
    well-conditioned data -- the same check passes the fp64 default on the same input"""
    import plaid_amd
    g, n, m = 20000, 9, 300
    Gp, Gi = _sets(g, m, 11)
    X = _data("well", g, n, 13)
    ref, mag, k = er.set_sums(Gp, Gi, X)
    ctx = plaid_amd.Context(0)
    try:
        er.assert_fp64_bound(ctx.plaid_dense(X, Gp, Gi, "sum", False), ref, mag, k, 1, "f64")
        ctx.set_precision("mixed")
        mixed = ctx.plaid_dense(X, Gp, Gi, "sum", False)
        ctx.set_precision("f64")
    finally:
        ctx.close()
    assert er.fp64_bound_violations(mixed, ref, mag, k, 1) > 0.5 * mixed.size


# ---------------------------------------------------------------- sparse X
def _sparse(g, n, dens, seed, signed):
    rng = np.random.default_rng(seed)
    if signed:
        vals = np.where(rng.random((g, n)) < 0.5, 1e6, -1e6) + rng.normal(size=(g, n))
    else:
        vals = rng.gamma(2.0, 1.0, size=(g, n)) + 0.01
    X = np.where(rng.random((g, n)) < dens, vals, 0.0)
    X[:, n - 1] = 0.0                                      # a sample without stored values
    return sp.csc_matrix(X), X


@pytest.mark.parametrize("route", [("scatter", "chunk"), ("scatter", "column"), ("gather", "chunk")])
@pytest.mark.parametrize("g,n,m,dens", [(500, 3, 40, 0.05), (20000, 9, 700, 0.05), (20000, 5, 24000, 0.03),
                                        (30001, 4, 300, 0.3), (64, 2, 5, 1.0)])
def test_sparse_kernels_within_the_fp64_bound(pinned_ctx, route, g, n, m, dens):
    """dgCMatrix X through the scatter kernel with fp64 accumulators (both item orders) and the gather kernel"""
    kern, order = route
    ctx = pinned_ctx(spmm_sparse_kernel=kern, scatter_fixed="off", scatter_order=order)
    Gp, Gi = _sets(g, m, g + m, kmax=300)
    for signed in (False, True):
        Xs, X = _sparse(g, n, dens, g + n + int(signed), signed)
        got_m = ctx.plaid_csc(Xs.indptr, Xs.indices, Xs.data, g, Gp, Gi, "mean", False)
        got_s = ctx.plaid_csc(Xs.indptr, Xs.indices, Xs.data, g, Gp, Gi, "sum", False)
        _check_mean_and_sum(got_m, got_s, Gp, Gi, X, f"{route} signed={signed}")


@pytest.mark.parametrize("sets", [1023, 1024, 1025, 17408, 17409])
def test_scatter_chunk_boundaries_within_the_fp64_bound(pinned_ctx, sets):
    """either side of a block of 1,024 sets and of one LDS chunk of 17,408: fp64 accumulators and the gather kernel"""
    g = 600
    Gp, Gi = _sets(g, sets, sets, kmax=90 if sets > 4000 else 400)
    for kern in ("scatter", "gather"):
        ctx = pinned_ctx(spmm_sparse_kernel=kern, scatter_fixed="off")
        for signed in (False, True):
            Xs, X = _sparse(g, 24, 0.3, sets + int(signed), signed)
            got_m = ctx.plaid_csc(Xs.indptr, Xs.indices, Xs.data, g, Gp, Gi, "mean", False)
            got_s = ctx.plaid_csc(Xs.indptr, Xs.indices, Xs.data, g, Gp, Gi, "sum", False)
            _check_mean_and_sum(got_m, got_s, Gp, Gi, X, f"{kern} signed={signed}")


# ---------------------------------------------------------------- the fixed-point predicate of the scatter kernel
def _predicate(Gp, Xp, Xx, xmax=None):
    """host restatement of scatter_fixed_ok (kernels_spmm.hip): (fixed point allowed, e, qm) -- e + qm >= 40 is the
    guarantee 2^-(e + 1) / min_nz <= 2^-40"""
    kmax = int(np.diff(Gp).max())
    kbits = 1
    while (1 << kbits) <= kmax:
        kbits += 1
    seen_max = float(Xx.max())
    xm = seen_max if xmax is None else xmax
    q = int(np.frexp(xm)[1])
    e = 63 - (q + kbits)
    qm = int(np.frexp(Xx[Xx > 0].min())[1])
    fine = qm + e >= 40
    colsum = float(np.add.reduceat(Xx, Xp[:-1][np.diff(Xp) > 0]).max())
    if not fine and colsum > 0:
        qs = int(np.frexp(colsum)[1])
        if qs < q + kbits:
            e = 63 - qs
            fine = qm + e >= 40
    return fine and seen_max <= xm, e, qm


def _fixed_case(target, big_set, seed):
    """stored values >= 0 with max 1.5 (q = 1) and the smallest positive value placed so that e + qm == target.  Sets of
    <= 100 genes (kbits 7, e = 55; column sums far above 2^8: no column-sum branch) or, with `big_set`, one set of 5,000
    genes (kbits 13: e = 49 misses) and column sums in [2^10, 2^11) (the column-sum branch: e = 52).  Set 0 sums small,
    off-grid values only"""
    rng = np.random.default_rng(seed)
    g, n = 8000, 6
    sets = [np.sort(rng.choice(g, size=int(s), replace=False)) for s in rng.integers(1, 101, size=300)]
    sets[0] = np.arange(100)
    if big_set:
        sets[1] = np.sort(rng.choice(g, size=5000, replace=False))
    Gp = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    Gi = np.concatenate(sets).astype(np.int32)
    X = np.zeros((g, n))
    nnz_col = 1300 if big_set else 2500
    for c in range(n):
        rows = np.sort(rng.choice(np.arange(100, g), size=nnz_col, replace=False))
        X[rows, c] = rng.uniform(0.5, 1.2, size=nnz_col)
    X[107, 0] = 1.5                                        # xmax: q = 1
    e = 52 if big_set else 55
    qm = target - e                                        # smallest positive value in [2^(qm - 1), 2^qm)
    small = np.ldexp(rng.uniform(1.0, 2.0, size=(100, n)), qm - 1)
    small[0, 0] = np.ldexp(1.0, qm - 1)
    X[:100, :] = small
    Xs = sp.csc_matrix(X)
    Xs.sort_indices()
    ok, e_got, qm_got = _predicate(Gp, Xs.indptr, Xs.data)
    if big_set:
        cs = np.asarray(Xs.sum(axis=0)).ravel()
        assert 2.0 ** 10 <= cs.max() < 2.0 ** 11
    assert e_got == e and e_got + qm_got == target and ok == (target >= 40), (e_got, qm_got)
    return Gp, Gi, Xs, X, e


def _scatter_raw(ctx, torch, gs, Xs, m, bounded_xmax=None):
    dev = torch.device("cuda", 0)
    dp, di, dx = (torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                  for a in (Xs.indptr.astype(np.int32), Xs.indices.astype(np.int32), Xs.data))
    n = Xs.shape[1]
    S = torch.empty((n, m), dtype=torch.float64, device=dev)
    fl = torch.zeros(4, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    if bounded_xmax is None:
        ctx.dev_spmm_csc(gs, dp.data_ptr(), di.data_ptr(), dx.data_ptr(), n, S.data_ptr(), m, "sum", 1.0, 0.0, fl.data_ptr(),
                         None, nnz=len(Xs.data))
    else:   # alpha is divided by *rmax: alpha = rmax leaves the raw sum
        rm = torch.full((1,), bounded_xmax, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.dev_spmm_csc_ranks(gs, dp.data_ptr(), di.data_ptr(), dx.data_ptr(), n, S.data_ptr(), m, rm.data_ptr(), "sum",
                               bounded_xmax, 0.0, fl.data_ptr(), nnz=len(Xs.data))
    ctx.synchronize()
    return S.cpu().numpy().T


@pytest.mark.parametrize("big_set", [False, True])
@pytest.mark.parametrize("bounded", [False, True])
def test_scatter_fixed_point_predicate_at_its_boundary(pinned_ctx, big_set, bounded):
    """e + qm = 40: fixed point allowed -- every score within 2^-40 relative of the exact sum (and not the fp64 sums);
    e + qm = 39: fixed point refused -- every score within the fp64 bound, which the 2^-e grid would break (checked on
    the host).  Through the plain entry and the bounded entry with a declared xmax; with sets of <= 100 genes and through
    the column-sum branch (one set of 5,000 genes)"""
    import torch
    ctx = pinned_ctx(spmm_sparse_kernel="scatter", scatter_fixed="on")
    xmax = 1.5 if bounded else None
    for target in (40, 39):
        Gp, Gi, Xs, X, e = _fixed_case(target, big_set, 100 * target + 2 * int(big_set) + int(bounded))
        m, g = len(Gp) - 1, X.shape[0]
        gs = ctx.geneset(g, Gp, Gi)
        ref, mag, k = er.set_sums(Gp, Gi, X)
        got = _scatter_raw(ctx, torch, gs, Xs, m, xmax)
        # the 2^-e grid, on the host: rounding every stored value to it breaks the fp64 bound (set 0's small values)
        Xq = np.ldexp(np.round(np.ldexp(X, e)), -e)
        refq, _, _ = er.set_sums(Gp, Gi, Xq)
        assert er.fp64_bound_violations(refq, ref, mag, k, 1) > 0
        if target == 40:
            assert np.all(np.abs(got - ref) <= (2.0 ** -40 + 2.0 ** -52) * np.abs(ref))
            ctx.set_option("scatter_fixed", "off")
            f64 = _scatter_raw(ctx, torch, gs, Xs, m, xmax)
            ctx.set_option("scatter_fixed", "on")
            er.assert_fp64_bound(f64, ref, mag, k, 1, "fp64 accumulators")
            # the fixed-point route ran: each value rounded half-even to the 2^-e grid, exact integer sums, one
            # conversion -- the exact sum of the grid values rounded once, bit for bit (fp64 atomics would not give it)
            er.assert_same_bits(got, refq, "fixed point = exact sums of the grid values")
        else:
            er.assert_fp64_bound(got, ref, mag, k, 1, f"e + qm = {target}")
        gs.close()


# ---------------------------------------------------------------- weighted crossprod
@pytest.mark.parametrize("g", [700, 20480, 20481, 33000])
def test_weighted_crossprod_within_the_fp64_bound(hip_ctx, g):
    """t(W) %*% Y with signed, cancelling weights and explicit stored zeros; dense and CSC Y, host and device entries.
    Terms w * y are rounded on the device: c = 2 (the products add <= u mag, the reference rounds once)"""
    import torch
    rng = np.random.default_rng(g)
    m, n = 60, 7
    sets = [np.sort(rng.choice(g, size=int(s), replace=False)) for s in rng.integers(1, min(g, 600), size=m)]
    Wp = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    Wi = np.concatenate(sets).astype(np.int32)
    Wx = rng.normal(size=len(Wi)) * np.where(rng.random(len(Wi)) < 0.5, 1e3, 1.0)
    Wx[::17] = 0.0                                         # explicit stored zeros
    Y = _data("cancel", g, n, g + 1)
    Y[rng.random(Y.shape) < 0.5] = 0.0
    Yz = sp.csc_matrix(Y)
    Yz.data[::13] = 0.0                                    # explicit stored zeros in Y as well
    Y2 = Yz.toarray()
    ref, mag, k = er.set_sums(Wp, Wi, Y, weights=Wx)
    er.assert_fp64_bound(hip_ctx.crossprod_weighted(Wp, Wi, Wx, g, Y=Y), ref, mag, k, 2, "dense Y")
    ref2, mag2, k2 = er.set_sums(Wp, Wi, Y2, weights=Wx)
    er.assert_fp64_bound(hip_ctx.crossprod_weighted(Wp, Wi, Wx, g, Yp=Yz.indptr, Yi=Yz.indices, Yx=Yz.data), ref2, mag2,
                         k2, 2, "CSC Y")
    dev = torch.device("cuda", 0)

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    dWp, dWi, dWx = t(Wp), t(Wi), t(Wx)
    dY = t(Y.T)                                            # column-major g x n
    S = torch.empty((n, m), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    hip_ctx.dev_crossprod_weighted(dWp.data_ptr(), dWi.data_ptr(), dWx.data_ptr(), g, m, dY.data_ptr(), g, n,
                                   S.data_ptr(), m)
    hip_ctx.synchronize()
    er.assert_fp64_bound(S.cpu().numpy().T, ref, mag, k, 2, "device dense Y")
    dYp, dYi, dYx = t(Yz.indptr.astype(np.int32)), t(Yz.indices.astype(np.int32)), t(Yz.data)
    S2 = torch.empty((n, m), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    hip_ctx.dev_crossprod_weighted_csc(dWp.data_ptr(), dWi.data_ptr(), dWx.data_ptr(), g, m, dYp.data_ptr(),
                                       dYi.data_ptr(), dYx.data_ptr(), n, S2.data_ptr(), m)
    hip_ctx.synchronize()
    er.assert_fp64_bound(S2.cpu().numpy().T, ref2, mag2, k2, 2, "device CSC Y")


# ---------------------------------------------------------------- rank-valued routes
@pytest.mark.parametrize("sparse", [False, True])
def test_replaid_sing_within_the_fp64_bound_of_exact_rank_sums(hip_ctx, sparse):
    """replaid.sing = mean over the set of (rank / g - 0.5) (R/plaid.R:215-217), in the default staging.  The ranks are
    exact (pinned elsewhere); the reference takes the exact integer sums R of the oracle's ranks and evaluates
    w (R / g - 0.5 k) in long double.  The device rounds 1 / g, R w, (1 / g)(R w), k w and the final add, the reference
    once more: c = 7 over mag = w (R / g + 0.5 k)"""
    from plaid_amd import synth as sy
    from oracle import plaid_oracle as po
    g, n, m = 12001, 9, 400
    Gp, Gi = _sets(g, m, 21)
    if sparse:
        Xp, Xi, Xx = sy.sparse_columns(g, 0, n)
        Xs = sp.csc_matrix((Xx, Xi, Xp), shape=(g, n))
        got = hip_ctx.sing_csc(Xs.indptr, Xs.indices, Xs.data, g, Gp, Gi)
        ranks = po._dense(po.colranks(Xs, ties_method="min"))
    else:
        X = sy.dense_columns(g, 0, n, tied=True)
        got = hip_ctx.sing_dense(X, Gp, Gi)
        ranks = po._dense(po.colranks(X, ties_method="min"))
    R, _, _ = er.set_sums(Gp, Gi, ranks)                   # integers < 2^53: exact
    kk = np.diff(Gp).astype(np.float64)[:, None]
    w = _w(Gp)[:, None]
    ld = np.longdouble
    exact = (w.astype(ld) * (R.astype(ld) / ld(g) - ld(0.5) * kk.astype(ld))).astype(np.float64)
    mag = w * (R / g + 0.5 * kk)
    er.assert_fp64_bound(got, exact, mag, np.zeros(R.shape, dtype=np.int64), 7, "sing")


# ---------------------------------------------------------------- normalised rank routes: replaid.ssgsea and replaid.ucell
def _rank_case(sparse, seed):
    from plaid_amd import synth as sy
    g, n, m = 12001, 9, 400
    Gp, Gi = _sets(g, m, seed)
    if sparse:
        Xp, Xi, Xx = sy.sparse_columns(g, 0, n)
        X = sp.csc_matrix((Xx, Xi, Xp), shape=(g, n))
    else:
        X = sy.dense_columns(g, 0, n, tied=True)
    return g, Gp, Gi, X


def _ssgsea_within_the_bound(hip_ctx, sparse, alpha):
    """replaid.ssgsea in the default staging: mean over the set of (r^(1 + alpha) / max(r^(1 + alpha)) - 0.5), then
    normalize_medians (R/plaid.R:245-253).  Reference: the oracle's average ranks (sparse: zeros stay 0), their powers in
    long double, exact sums P, T = w (P / max - 0.5 k) in long double.

    The device sums its weights and applies alpha * (sum * w) + beta * (k * w) with alpha = fl(1 / max), beta = -0.5.
    Relative to mag = w (P / max + 0.5 k), c counts: the device's r^(1 + alpha) (a = pow_ref.pow_allowance_u(1 + alpha) u
    per weight, and so on the sum and on its max: 2 a; a = 3 for 1.25 -- root4_pos' 2 u and one product --, 4.5 for 1.75:
    two square roots and three products), fl(1 / max) 1, sum * w 1, alpha * (...) 1, k * w 1, the final add 1, the
    reference's sum P and T 2: c = 6 + 2 a = 12 for alpha = 0.25 and 15 for alpha = 0.75; alpha = 0 has exact weights
    and max: c = 6.  The sum itself: (k - 1) roundings in fp64 -- or, where
    the scatter kernel's predicate (restated on the host) allows fixed point for these bounded weights, 2^-40 of P, the
    grid's guarantee (then the k term is replaced).  The medians step adds the bound of _normalized_ref"""
    from oracle import plaid_oracle as po
    g, Gp, Gi, X = _rank_case(sparse, 31)
    got = hip_ctx.ssgsea_csc(X.indptr, X.indices, X.data, g, Gp, Gi, alpha) if sparse else hip_ctx.ssgsea_dense(X, Gp, Gi, alpha)
    ld = np.longdouble
    R = po._dense(po.colranks(X, keep_zero=True, ties_method="average"))
    W = np.power(R.astype(ld), ld(1.0 + alpha))
    wmax = W.max()
    P, _, k = _long_sums(Gp, Gi, W)
    kk = np.diff(Gp).astype(np.float64)[:, None]
    w = _w(Gp)[:, None]
    T = (w.astype(ld) * (P / wmax - ld(0.5) * kk.astype(ld))).astype(np.float64)
    Pf = P.astype(np.float64)
    mag = w * (Pf / float(wmax) + 0.5 * kk)
    c = 6 + 2 * pow_allowance_u(np.float64(1.0) + np.float64(alpha))      # (an exponent of 1: no allowance)
    assert c == {0.0: 6, 0.25: 12, 0.75: 15}[alpha]
    E = (k + c) * er.U * mag
    if sparse:
        Wx = np.concatenate([W.astype(np.float64)[X.indices[X.indptr[j]:X.indptr[j + 1]], j] for j in range(X.shape[1])])
        fixed, _, _ = _predicate(Gp, X.indptr, Wx, xmax=float(wmax))   # (the stored values' weights, by column)
        if fixed:
            E = E + 2.0 ** -40 * w * Pf / float(wmax)
    N, B = _normalized_ref(T, E)
    assert abs(T.min()) > 10 * E.max()                         # ignore.zero auto resolves as on the device (min(S) != 0)
    er.assert_within(got, N, B, f"ssgsea alpha={alpha} sparse={sparse}")
    assert B.max() < 1e-11 * np.abs(N).max()                   # (the bound stays far below the 1e-5 bar)


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("alpha", [0.0, 0.25])
def test_replaid_ssgsea_within_the_bound_of_exact_rank_sums(hip_ctx, sparse, alpha):
    _ssgsea_within_the_bound(hip_ctx, sparse, alpha)


def test_replaid_ssgsea_alpha_075_within_the_bound_of_its_larger_allowance(hip_ctx):
    """alpha = 0.75: the exponent 1.75 is pow_quarters' q = 7, whose weights exceed 3 u (3.90 u over the domain, by IEEE
    operations alone): held at the c = 15 that its derived 4.5 u gives"""
    _ssgsea_within_the_bound(hip_ctx, False, 0.75)


@pytest.mark.parametrize("sparse", [False, True])
def test_replaid_ucell_within_the_bound_of_exact_rank_sums(hip_ctx, sparse):
    """replaid.ucell: v = pmin(max(r) - r, rmax + 1) of average ranks (half-integers, exact), plaid(mean) with medians,
    then 1 - S / rmax + (k + 1) / (2 rmax) (R/plaid.R:276-282).  Raw scores: the sum of v ((k - 1) roundings), sum * w
    and the reference: c = 2 over mag = w sum v.  The medians add _normalized_ref's bound; the affine step
    fl(fl(N * fl(-1 / rmax)) + add_j) rounds 1 / rmax, the product and the sum, the reference once more"""
    from oracle import plaid_oracle as po
    g, Gp, Gi, X = _rank_case(sparse, 37)
    rmax = 1500.0
    kf = np.diff(Gp).astype(np.float64)
    got = hip_ctx.ucell(X, Gp, Gi, kf, rmax)
    R = po._dense(po.colranks(X, ties_method="average"))
    V = np.minimum(R.max() - R, rmax + 1.0)
    P, mag, k = er.set_sums(Gp, Gi, V)
    w = _w(Gp)[:, None]
    ld = np.longdouble
    T = (P.astype(ld) * w.astype(ld)).astype(np.float64)
    E = (k + 2) * er.U * mag * w
    assert T.min() > 10 * E.max()
    N, B = _normalized_ref(T, E)
    addj = 1.0 + (kf + 1.0) / (2.0 * rmax)                     # the device's fp64 row terms
    U = (N.astype(ld) * (ld(-1.0) / ld(rmax)) + addj.astype(ld)[:, None]).astype(np.float64)
    BU = B / rmax + 2.0 * er.U * np.abs(N) / rmax + 2.0 * er.U * np.abs(U)
    er.assert_within(got, U, BU, f"ucell sparse={sparse}")
