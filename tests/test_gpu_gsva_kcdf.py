"""GSVA's Gaussian kernel CDF estimate on the GPU (include/plaidhip.h: plaidhip_gsva_kcdf, rowtf = 3 "gauss" of
plaidhip_gsva_exact and _multi; kernels_kcdf.hip).

Everything is bit for bit: the pinned form is sequential and correctly rounded, so the device must return the bits of the
numpy form (tests/helpers/gsva_kcdf.py) fed with the library's own table.  The kernel's seams are the fast table index
(an estimate that must agree with the pinned expression on, beside and between integers, at v = +-10 and beyond), the 64
lanes of a wavefront, the sub-group widths 64 .. 1024 (each asserted and run) and the chunks of samples that pass through LDS.  "gauss" must score
as rowtf = "none" on V; a dgCMatrix as its dense form; sharding, the mixed precision mode and the Python alignment must
not change a bit.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import exact_ref as er
from tests.helpers import gsva_kcdf as gk
from tests.helpers import gsva_walk as gw
from tests.helpers import sharded_hooks
from tests.test_gpu_ssgsea_exact import _sets

pytestmark = pytest.mark.gpu


def same(got, exp, what=""):
    er.assert_same_bits(got, exp, what)


@pytest.fixture(scope="module")
def table():
    import plaid_amd
    return plaid_amd.gsva_kcdf_table()


def _rows(g, n, seed=5, nan_row=False):
    """g rows cycling through: normal, heavily tied (-0.0 beside 0.0), constant, seam rows with h = 2^p and 5 * 2^p
    (n >= 16), an outlier row (|v| > 10), a wide-range row; nan_row: the last row holds a NaN"""
    rng = np.random.default_rng(seed)
    X = np.empty((g, n))
    for i in range(g):
        kind = i % 8
        if kind in (0, 4):
            X[i] = rng.normal(7, 2, size=n)
        elif kind == 1:
            X[i] = np.round(rng.normal(0, 2, size=n), 0)
            X[i, rng.random(n) < 0.1] = -0.0
        elif kind == 2:
            X[i] = 3.25
        elif kind == 3 and n >= 16:
            X[i] = gk.seam_row(n, 1, int(rng.integers(0, 4)), rng)
        elif kind == 5 and n >= 16:
            X[i] = gk.seam_row(n, 5, int(rng.integers(0, 3)), rng)
        elif kind == 6:
            X[i] = rng.normal(0, 1, size=n)
            X[i, n // 2] = 40.0
        else:
            X[i] = rng.normal(0, 1, size=n) * 10.0 ** rng.integers(-3, 4, size=n)
    if nan_row:
        X[g - 1, n // 3] = np.nan
    return np.asfortranarray(X)


# ------------------------------------------------------------------------------------------------- 1. the transform alone
@pytest.mark.parametrize("g,n", [(1, 2), (8, 2), (64, 63), (65, 64), (3001, 65), (24, 257), (1, 65), (64, 130), (16, 2049),
                                 (9, 1100)])
def test_kcdf_equals_the_pinned_form(hip_ctx, table, g, n):
    X = _rows(g, n, seed=g + n, nan_row=g >= 8)
    same(hip_ctx.gsva_kcdf(X), gk.pinned(X, table), f"g={g} n={n}")


def _width_rule(nj):
    """kcdf_sum_kernel's sub-group width, restated: the widest power of two in [64, 1024] that pads the nj test columns
    by at most 4 % more than the best of them"""
    pad = {w: -(-nj // w) * w for w in (64, 128, 256, 512, 1024)}
    return max(w for w in pad if pad[w] * 100 <= min(pad.values()) * 104)


def _width_hook(nj):
    from plaid_amd._lib import load
    fn = load().plaidhip_debug_gsva_kcdf_width
    fn.argtypes, fn.restype = [C.c_int32], C.c_int
    return fn(nj)


# (g, n, W): every width, one and several chunks of W samples (the last one partial), g = 1 and g that 1024 / W does
# not divide; the shapes the transform is for, 20,000 x 2,000 and 20,000 x 10,000, take W = 1024 (asserted below)
WIDTHS = [(1, 63, 64), (3, 300, 64), (1, 65, 128), (9, 1100, 128), (1, 256, 256), (7, 250, 256), (5, 760, 256),
          (1, 512, 512), (3, 500, 512), (3, 1500, 512), (3, 1000, 1024), (1, 1024, 1024), (3, 2000, 1024), (2, 3000, 1024)]


def test_the_width_rule():
    for nj in list(range(1, 2200)) + [3000, 4000, 10000, 100000]:
        assert _width_hook(nj) == _width_rule(nj), nj
    assert _width_hook(2000) == 1024 and _width_hook(10000) == 1024
    assert {w for _, _, w in WIDTHS} == {64, 128, 256, 512, 1024}


@pytest.mark.parametrize("g,n,width", WIDTHS)
def test_every_sub_group_width(hip_ctx, table, g, n, width):
    assert _width_hook(n) == width
    assert g == 1 or g % (1024 // width) != 0 or width == 1024
    # (fewer than 8 rows: a normal, a beside-integer seam, an on-integer seam, a tied and an outlier row first)
    X = np.asfortranarray(_rows(8, n, seed=n)[[0, 5, 3, 1, 6, 7, 2, 4][:g]]) if g < 8 else _rows(g, n, seed=n)
    same(hip_ctx.gsva_kcdf(X), gk.pinned(X, table), f"g={g} n={n} W={width}")


def test_bandwidths_equal_the_pinned_moments(hip_ctx):
    """h alone, bit for bit: V hardly depends on the last bits of h, so the sequential sums, the uncontracted d * d + ss
    and the correctly rounded division and square root of kcdf_row_moments_kernel are pinned here"""
    from plaid_amd._lib import load
    fn = load().plaidhip_debug_gsva_kcdf_bandwidths
    fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p], C.c_int
    for g, n in ((1, 2), (65, 63), (3001, 65), (300, 257), (64, 2049)):
        X = _rows(g, n, seed=g + n, nan_row=g > 1)
        if g > 20:
            X[9] = np.arange(n) * 1e-170                            # squares underflow: h == 0
            X[10] = np.arange(n) * 1e300                            # squares overflow: h == inf
            X[11, n // 2] = np.inf
        H = np.empty(g)
        assert fn(hip_ctx.handle, X.ctypes.data, g, n, H.ctypes.data) == 0
        same(H, gk.bandwidths(X), f"h g={g} n={n}")


def test_special_rows(hip_ctx, table):
    """a constant row is n / 2 exactly; NaN and infinite rows are NaN rows; a row whose squared deviations underflow
    (h == 0 with unequal values: v = +-inf) and rows of huge and tiny scale follow the form"""
    n = 65
    X = _rows(16, n)
    X[3, 5] = np.nan
    X[4, 6] = np.inf
    X[5, 7] = -np.inf
    X[6] = 1.0
    X[6, 10] = 1.0 + 2.0 ** -52
    X[7] = np.arange(n) * 1e-170
    X[8] = np.arange(n) * 1e150
    X[9] = np.arange(n) * 1e300
    V = hip_ctx.gsva_kcdf(X)
    same(V, gk.pinned(X, table), "special rows")
    assert (V[2] == n / 2).all() and (V[10] == n / 2).all()          # (_rows: every row 8 k + 2 is constant)
    assert np.isnan(V[3:6]).all() and np.isfinite(V[6:10]).all()


def test_seam_rows_alone_with_the_fast_index_and_without(hip_ctx, table):
    """rows made for the index seams (d / h exact: on integers, v = +-10; h = 5 * 2^p: one rounding beside integers),
    then the same call with the fast index switched off (the exact operations for every term): the same bits"""
    from plaid_amd._lib import load
    rng = np.random.default_rng(21)
    n = 257
    X = np.asfortranarray([gk.seam_row(n, m, p, rng) for m in (1, 5) for p in (0, 1, 2, 5)] * 2)
    X[8:] *= 3.0                                                      # (h = 3 * 2^p, 15 * 2^p: rounded quotients)
    exp = gk.pinned(X, table)
    same(hip_ctx.gsva_kcdf(X), exp, "seam rows")
    Xn = _rows(64, 130, seed=3)
    expn = gk.pinned(Xn, table)
    lib = load()
    assert lib.plaidhip_debug_gsva_kcdf_set_mode(1) == 0
    try:
        same(hip_ctx.gsva_kcdf(X), exp, "seam rows, exact operations only")
        same(hip_ctx.gsva_kcdf(Xn), expn, "mixed rows, exact operations only")
    finally:
        lib.plaidhip_debug_gsva_kcdf_set_mode(0)
    same(hip_ctx.gsva_kcdf(Xn), expn, "mixed rows")


def test_kcdf_of_a_dgcmatrix_equals_its_dense_form(hip_ctx, table):
    g, n = 301, 65
    rng = np.random.default_rng(31)
    for density in (0.05, 0.6):
        D = np.round(rng.normal(0, 2, size=(g, n)), 0)
        D[rng.random((g, n)) >= density] = 0.0
        D[:, 0] = 0.0                                                 # an empty column
        S = sp.csc_matrix(D)
        S.sort_indices()
        S.data[rng.random(S.nnz) < 0.1] = 0.0                        # stored zeros
        dense = np.asfortranarray(S.toarray())
        V = hip_ctx.gsva_kcdf(S)
        same(V, hip_ctx.gsva_kcdf(dense), f"dgCMatrix density={density}")
        same(V, gk.pinned(dense, table), f"dgCMatrix density={density} vs the pinned form")


def test_fewer_than_two_samples_are_refused(hip_ctx):
    from plaid_amd._lib import PlaidHipError
    X = np.asfortranarray(np.arange(12.0).reshape(12, 1))
    Gp, Gi = _sets(12, 5)
    with pytest.raises(ValueError):
        hip_ctx.gsva_kcdf(X)
    with pytest.raises(PlaidHipError):
        hip_ctx.gsva_exact(X, Gp, Gi, 1.0, "gauss", True)
    import plaid_amd
    with pytest.raises(PlaidHipError):
        plaid_amd.gsva_exact_multi(X, Gp, Gi, 1.0, "gauss", True, devices=1)
    rc, _ = _run_hook(2, X, Gp, Gi, 1.0, True)
    assert rc != 0


# ------------------------------------------------------------------------------------------------- 2. the statistic
@pytest.mark.parametrize("g,n", [(97, 37), (3001, 65), (500, 300)])
def test_gauss_scores_as_none_on_v_and_as_the_pinned_walk(hip_ctx, table, g, n):
    X = _rows(g, n, seed=g, nan_row=False)
    Gp, Gi = _sets(g, 24)
    V = hip_ctx.gsva_kcdf(X)
    same(V, gk.pinned(X, table), "V")
    for tau in (0.0, 1.0):
        for max_diff in (True, False):
            got = hip_ctx.gsva_exact(X, Gp, Gi, tau, "gauss", max_diff)
            same(got, hip_ctx.gsva_exact(V, Gp, Gi, tau, "none", max_diff), f"g={g} n={n} tau={tau} vs none on V")
            same(got, gw.pinned(V, Gp, Gi, tau, max_diff), f"g={g} n={n} tau={tau} vs the pinned walk")


def test_a_nan_row_scores_nan_everywhere(hip_ctx):
    g, n = 97, 37
    X = _rows(g, n, nan_row=True)
    Gp, Gi = _sets(g, 10)
    assert np.isnan(hip_ctx.gsva_exact(X, Gp, Gi, 1.0, "gauss", True)).all()


def _sparse_x(g, n, density, seed):
    rng = np.random.default_rng(seed)
    D = np.round(rng.normal(0, 2, size=(g, n)), 0)
    D[rng.random((g, n)) >= density] = 0.0
    D[:, 0] = 0.0
    S = sp.csc_matrix(D)
    S.sort_indices()
    if S.nnz:
        S.data[rng.random(S.nnz) < 0.1] = 0.0
    return S


@pytest.mark.parametrize("density", [0.05, 0.6])
def test_dgcmatrix_scores_as_its_dense_form(hip_ctx, density):
    g, n = 3001, 65
    S = _sparse_x(g, n, density, 41)
    dense = np.asfortranarray(S.toarray())
    Gp, Gi = _sets(g, 24)
    for tau, max_diff in ((0.0, True), (1.0, True), (1.0, False)):
        same(hip_ctx.gsva_exact(S, Gp, Gi, tau, "gauss", max_diff), hip_ctx.gsva_exact(dense, Gp, Gi, tau, "gauss", max_diff),
             f"density={density} tau={tau}")


# ------------------------------------------------------------------------------------------------- 3. sharding, modes
def _run_hook(nshards, X, Gp, Gi, tau, max_diff):
    """plaidhip_gsva_exact_multi's engine with nshards contexts on one device (the library's debug hook), rowtf = 3"""
    return sharded_hooks.score("gsva_exact", nshards, X, Gp, Gi, float(tau), 3, int(max_diff))


@pytest.mark.parametrize("kind", ["dense", "csc"])
def test_sharded_engine_is_bit_identical(hip_ctx, kind):
    """1, 2, 3 and 7 shards: every shard takes all of X and sums over k in the one order; 5 columns over 7 shards leave
    shards empty"""
    g = 301
    Gp, Gi = _sets(g, 24)
    for n in (130, 5):
        X = _rows(g, n, seed=n) if kind == "dense" else _sparse_x(g, n, 0.3, 43)
        for tau, max_diff in ((0.0, True), (1.0, False)):
            exp = hip_ctx.gsva_exact(X, Gp, Gi, tau, "gauss", max_diff)
            for nshards in (1, 2, 3, 7):
                rc, S = _run_hook(nshards, X, Gp, Gi, tau, max_diff)
                assert rc == 0
                same(S, exp, f"{kind} n={n} nshards={nshards} tau={tau}")


def test_shards_of_more_than_a_thousand_columns(hip_ctx, table):
    """4,000 samples over 2 shards: each shard's 2,000 test columns take W = 1024 and two tiles per gene, the sums run
    over all 4,000 samples in four chunks; V against the numpy form on a subset of the columns"""
    g, n = 5, 4000
    assert _width_hook(n) == 1024 and _width_hook(n // 2) == 1024
    X = np.asfortranarray(_rows(8, n, seed=4)[[0, 5, 3, 1, 6]])
    Gp, Gi = _sets(g, 8)
    cols = np.r_[0:8, 1020:1030, 1995:2005, 3064:3080, 3990:4000]
    V = hip_ctx.gsva_kcdf(X)
    same(V[:, cols], gk.pinned(X, table, cols=cols), "V, 4,000 samples")
    for tau, max_diff in ((0.0, True), (1.0, False)):
        exp = hip_ctx.gsva_exact(X, Gp, Gi, tau, "gauss", max_diff)
        same(exp, hip_ctx.gsva_exact(V, Gp, Gi, tau, "none", max_diff), "gauss vs none on V")
        for nshards in (2, 3):
            rc, S = _run_hook(nshards, X, Gp, Gi, tau, max_diff)
            assert rc == 0
            same(S, exp, f"n={n} nshards={nshards} tau={tau}")


def test_multi_on_one_device_equals_the_context_call(hip_ctx):
    import plaid_amd
    g, n = 301, 65
    Gp, Gi = _sets(g, 24)
    for X in (_rows(g, n), _sparse_x(g, n, 0.3, 47)):
        for tau, max_diff in ((0.0, False), (1.0, True)):
            same(plaid_amd.gsva_exact_multi(X, Gp, Gi, tau, "gauss", max_diff, devices=1),
                 hip_ctx.gsva_exact(X, Gp, Gi, tau, "gauss", max_diff), f"multi tau={tau}")


def test_mixed_mode_does_not_change_a_bit(hip_ctx):
    g, n = 301, 65
    X = _rows(g, n)
    Gp, Gi = _sets(g, 24)
    exp = [hip_ctx.gsva_exact(X, Gp, Gi, t, "gauss") for t in (0.0, 1.0)]
    expv = hip_ctx.gsva_kcdf(X)
    hip_ctx.set_precision("mixed")
    try:
        got = [hip_ctx.gsva_exact(X, Gp, Gi, t, "gauss") for t in (0.0, 1.0)]
        gotv = hip_ctx.gsva_kcdf(X)
    finally:
        hip_ctx.set_precision("f64")
    for e, o in zip(exp + [expv], got + [gotv]):
        same(o, e, "mixed mode")


# ------------------------------------------------------------------------------------------------- 4. alignment
def test_python_alignment_equals_the_prealigned_call(hip_ctx, table):
    import plaid_amd
    g, n, m = 500, 18, 12
    rng = np.random.default_rng(12)
    X0 = rng.normal(8, 2, size=(g, n))
    genes = [f"g{i}" for i in range(g)]
    Gp, Gi = _sets(g, m)
    G0 = sp.csc_matrix((np.ones(len(Gi)), Gi, Gp), shape=(g, m))
    perm = rng.permutation(g)
    X1 = plaid_amd.NamedMatrix(X0[perm], [genes[i] for i in perm], [f"s{j}" for j in range(n)])
    extra = sp.csc_matrix((np.ones(m), (np.arange(m) % 5, np.arange(m))), shape=(5, m))
    G1 = plaid_amd.NamedMatrix(sp.vstack([G0, extra]).tocsc(), genes + [f"absent{i}" for i in range(5)],
                               [f"set{j}" for j in range(m)])
    for tau in (0.0, 1.0):
        got = plaid_amd.replaid_gsva_exact(X1, G1, tau=tau, rowtf="gauss", ctx=hip_ctx)
        exp = hip_ctx.gsva_exact(X0[perm], *plaid_amd.aligned_pattern(X1, G1), tau, "gauss")
        same(got.values, exp, f"alignment tau={tau}")
        assert list(got.rownames) == list(G1.colnames) and list(got.colnames) == list(X1.colnames)
        same(got.values, gw.pinned(gk.pinned(X0[perm], table), *plaid_amd.aligned_pattern(X1, G1), tau),
             "alignment vs the pinned forms")
    with pytest.raises(ValueError):
        plaid_amd.replaid_gsva_exact(X1, G1, rowtf="kcdf", ctx=hip_ctx)
