"""The pair crossprod's register-partial form (`pytest -m gpu`, through the C ABI).

A collection with more than 10,224 genes (two or more gene slices) and at most 6,144 sets (96 tiles = 12 wavefronts x 8)
gets a pair plan for 12 wavefronts; the kernel then runs at 768 threads and a lane keeps its partial sums of the slices
before in registers, one pair per tile, where the 1,024-thread form stores them to a per-workgroup scratch and loads them
back.  PLAIDHIP_OPT_SPMM_DENSE_KERNEL = 4 ("pair_scratch") pins the scratch form on the same plan.  A tile's schedule does
not depend on the wavefront that walks it, so the two forms must agree BIT FOR BIT, flag words included; one of them is
also held to the CPU oracle at the parity tests' tolerance (oracle/fullsize.py RTOL / ATOL).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_SLICE = 10224      # genes of one LDS slice of the pair kernel
REG_TILES = 12 * 8     # tiles the register-partial form holds: 12 wavefronts x 8 register pairs


def _tol():
    from oracle.fullsize import ATOL, RTOL
    return RTOL, ATOL


def _eligible(g, m):
    return g > MAX_SLICE and (m + 63) // 64 <= REG_TILES


def _plan(g, Gp, Gi):
    """the library's own view of the plan: (eligible, most tiles on one wavefront, wavefronts with tiles)"""
    from plaid_amd import _lib
    fn = _lib.load().plaidhip_debug_pair_plan_check
    fn.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]
    fn.restype = C.c_int
    out = (C.c_int64 * 8)()
    Gp = np.ascontiguousarray(Gp, dtype=np.int32)
    Gi = np.ascontiguousarray(Gi, dtype=np.int32)
    assert fn(g, len(Gp) - 1, Gp.ctypes.data, Gi.ctypes.data, 16, out) == 0
    assert out[2] == int(Gp[-1]) and out[4] == 0
    return bool(out[5]), int(out[6]), int(out[7])


def _sets(g, m, seed=5, kmin=15, kmax=60):
    from plaid_amd import synth
    return synth.geneset_csc(g, m, seed=seed, kmin=kmin, kmax=kmax)


def _x(g, n, seed=1):
    return np.asfortranarray(np.random.default_rng(seed).normal(8.0, 2.0, size=(g, n)))


def _both_forms(pin, g, Gp, Gi, X, stat="mean", ldx=None, lds=None, csc=False):
    """scores (m x n) and flag words of the default form and of the pinned scratch form, on one geneset"""
    import torch
    dev = torch.device("cuda", 0)
    n = X.shape[1]
    m = len(Gp) - 1
    ldx = g if ldx is None else ldx
    lds = m if lds is None else lds
    res = []
    ctx = pin()
    gs = ctx.geneset(g, Gp, Gi)
    try:
        if csc:
            import scipy.sparse as sp
            Xs = sp.csc_matrix(X)
            dXp = torch.from_numpy(Xs.indptr.astype(np.int32)).to(dev)
            dXi = torch.from_numpy(Xs.indices.astype(np.int32)).to(dev)
            dXx = torch.from_numpy(Xs.data.astype(np.float64)).to(dev)
        else:
            Xh = np.full((n, ldx), -77.0)          # rows of this array are the columns of X, ldx apart
            Xh[:, :g] = X.T
            dX = torch.from_numpy(Xh).to(dev)
        for mode in ("auto", "pair_scratch"):
            ctx = pin(spmm_dense_kernel=mode, spmm_sparse_kernel="gather")
            S = torch.full((n, lds), -55.0, dtype=torch.float64, device=dev)
            flags = torch.zeros(4, dtype=torch.int32, device=dev)
            if csc:
                ctx.dev_spmm_csc(gs, dXp.data_ptr(), dXi.data_ptr(), dXx.data_ptr(), n, S.data_ptr(), lds, stat, 1.0, 0.0,
                                 flags.data_ptr(), nnz=int(Xs.nnz))
            else:
                ctx.dev_spmm_dense(gs, dX.data_ptr(), ldx, n, S.data_ptr(), lds, stat, 1.0, 0.0, flags.data_ptr())
            torch.cuda.synchronize()
            Sh = S.cpu().numpy()
            assert np.all(Sh[:, m:] == -55.0)      # nothing written between the columns of S
            res.append((np.ascontiguousarray(Sh[:, :m].T), flags.cpu().numpy()[:3].copy()))
    finally:
        gs.close()
    return res


def _check(pin, g, Gp, Gi, X, expect_regp, stat="mean", **kw):
    from oracle import c_oracle
    regp, most, waves = _plan(g, Gp, Gi)
    assert regp == expect_regp == _eligible(g, len(Gp) - 1)
    if regp:
        assert most <= 8 and waves == 12
    (Sa, fa), (Sb, fb) = _both_forms(pin, g, Gp, Gi, X, stat=stat, **kw)
    assert np.array_equal(Sa.view(np.int64), Sb.view(np.int64)), "register-partial and scratch forms differ in bits"
    assert np.array_equal(fa, fb)
    rtol, atol = _tol()
    ref = c_oracle.crossprod_dense(X, Gp, Gi, stat, threads=8)
    np.testing.assert_allclose(Sa, ref, rtol=rtol, atol=atol, equal_nan=True)
    return Sa, fa


@pytest.mark.parametrize("g,regp", [(10224, False), (10225, True), (20000, True), (20449, True), (30001, True)])
def test_gene_counts_one_to_three_slices(pinned_ctx, g, regp):
    """10,224: one slice, the old form; 10,225: a second slice of one gene; 20,449 / 30,001: three slices (odd counts), a
    partial sum crosses two hand-overs"""
    Gp, Gi = _sets(g, 130, kmax=300)
    _check(pinned_ctx, g, Gp, Gi, _x(g, 4), regp)


@pytest.mark.parametrize("m,regp", [(1, True), (63, True), (64, True), (65, True), (700, True), (768, True),
                                    (6144, True), (6145, False)])
def test_set_counts(pinned_ctx, m, regp):
    """one lane, a tile short of / at / past 64 lanes, fewer tiles than wavefronts (700: 11), one tile per wavefront (768),
    the most the registers hold (6,144 sets = 96 tiles) and one tile more, which falls back to the scratch form"""
    g = 20000
    Gp, Gi = _sets(g, m, kmax=40 if m > 1000 else 120)
    _check(pinned_ctx, g, Gp, Gi, _x(g, 3), regp)


def test_one_long_set_among_short_ones(pinned_ctx):
    """a 2,000-gene set among 15-gene sets: tile lengths very unequal, so the cost balance would pile the short tiles on
    the other wavefronts and the cap of 8 tiles per wavefront binds"""
    g, m = 20000, 6100
    rng = np.random.default_rng(9)
    sizes = np.full(m, 15)
    sizes[0] = 2000
    Gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    Gi = np.concatenate([np.sort(rng.choice(g, size=k, replace=False)) for k in sizes]).astype(np.int32)
    regp, most, _ = _plan(g, Gp, Gi)
    assert regp and most == 8
    _check(pinned_ctx, g, Gp, Gi, _x(g, 3), True)


@pytest.mark.parametrize("n", [1, 3, "2cu+3"])
def test_sample_counts(pinned_ctx, n):
    """odd counts: the last pair has no column B; 2 x CUs + 3: every workgroup walks two or more pairs, and the register
    slots of the pair before must not leak into the next"""
    import torch
    if n == "2cu+3":
        n = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 3
    g = 20000
    Gp, Gi = _sets(g, 200, kmax=200)
    _check(pinned_ctx, g, Gp, Gi, _x(g, n), True)


def test_stat_sum(pinned_ctx):
    g = 20449
    Gp, Gi = _sets(g, 130, kmax=300)
    _check(pinned_ctx, g, Gp, Gi, _x(g, 3), True, stat="sum")


def test_leading_dimensions(pinned_ctx):
    """S with a leading dimension above m, X with an odd one above g (every other column 8 bytes off 16-byte alignment)"""
    g, m = 20000, 130
    Gp, Gi = _sets(g, m, kmax=300)
    _check(pinned_ctx, g, Gp, Gi, _x(g, 5), True, ldx=g + 7, lds=m + 5)


def test_nan_zero_column_and_negatives_with_flags(pinned_ctx):
    g, m = 20449, 200
    Gp, Gi = _sets(g, m, kmax=200)
    X = _x(g, 5) - 8.0          # negative values
    X[:, 2] = 0.0               # a zero column: exact zero scores
    X[Gi[Gp[7]], 3] = np.nan    # one NaN, member of set 7
    S, f = _check(pinned_ctx, g, Gp, Gi, X, True)
    assert list(f) == [1, 1, 1]                       # has_neg, has_zero, has_nan
    assert np.isnan(S[7, 3]) and np.all(S[:, 2] == 0.0)


def test_csc_x_through_the_pair_kernel(pinned_ctx):
    g, m = 20449, 200
    Gp, Gi = _sets(g, m, kmax=200)
    X = _x(g, 5)
    X[np.random.default_rng(4).random(X.shape) < 0.6] = 0.0
    _check(pinned_ctx, g, Gp, Gi, X, True, csc=True)
