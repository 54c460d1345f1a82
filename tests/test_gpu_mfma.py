"""The dense-G matrix-core backend of the crossprod (spmm_dense_kernel = "mfma", plaid_amd/csrc/kernels_mfma.hip) held to
exact sums at a derived bound -- `pytest -m gpu`.

Reference: tests/helpers/exact_ref.py::set_sums (error-free sums, rounded once).  Bound: tests/helpers/mfma_ref.py::mfma_bound,
3 k 2^-23 mag + the fp64 term + 3 k 2^-126, derived there from the split (24 bits), 3 k fp32 additions of one ulp each and
the c fp64 roundings of the epilogue; tests/test_mfma_ref.py shows on the host that it sees a dropped `lo` plane and a
dropped K step.  No tolerance here is fitted: every comparison is mfma_bound (scaled by the epilogue's exact factors where
there is one) or an equality.

  a. the bound on five kinds of data (positive, cancelling, signed, O(1) mixed with 1e-45 ... 1e-30, half-integer ranks),
     set sizes 0 ... 400 with {g - 1} and {0, g - 1}, at shapes on the kernel's edges;
  b. the device entry with odd leading dimensions, sentinels, replaid.sing's epilogue in both alpha forms, flag words;
  c. the launcher's sample loop (n = 4097) and second panel (n = 8193);
  d. one prepared collection across routes and other collections;
  e. NaN, +-Inf and finite values past the bf16 range: the fp64 route's pattern element for element (the fix-up kernel).
"""
import numpy as np
import pytest

from tests.helpers import exact_ref as er
from tests.helpers import mfma_ref as mr
from tests.helpers.gsva_ref import _long_sums, _normalized_ref, _w

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


def _measure(capsys, what, got, ref, bound):
    with np.errstate(all="ignore"):
        fin = np.isfinite(got) & np.isfinite(ref) & (bound > 0)
        worst = float(np.max(np.abs(got - ref)[fin] / bound[fin])) if fin.any() else 0.0
    with capsys.disabled():
        print(f"\n[measure] {what}: worst error / bound {worst:.3g}")


def _check_sum_and_mean(capsys, what, got_sum, got_mean, Gp, ref, mag, k):
    """c = 1 for the sum (the reference's rounding; 1 * s + 0 is exact), c = 3 for the mean (w's own two roundings are in
    the device's w too: the product, and the reference's product and sum), as tests/test_gpu_exact_sums.py counts them"""
    w = _w(Gp)[:, None]
    for name, got, r, mg, c in (("sum", got_sum, ref, mag, 1), ("mean", got_mean, ref * w, mag * w, 3)):
        bound = mr.mfma_bound(mg, k, c)
        _measure(capsys, f"{what} {name}", got, r, bound)
        er.assert_within(got, r, bound, f"mfma {what} {name}")


# ---------------------------------------------------------------- a. the bound, at the kernel's edges
SHAPES = [
    (1, 1, 1),          # one gene padded to gk = 64 (nk = 2, 63 zero columns), one sample of 256 rows, one set of 256
    (31, 127, 63),      # below the K step; the last row of the first 128-sample wave row unused; the first 64-set wave column short
    (33, 129, 65),      # one gene into the second K step; one sample in the second wave row; one set in the second wave column
    (64, 255, 255),     # gk = g = 64, no padding; one short of the tile both ways
    (65, 256, 256),     # gk = 128 (nk = 4, 63 padded); exactly one tile both ways
    (129, 257, 257),    # gk = 192 (nk = 6: an odd multiple of the pad); one sample and one set into the second tiles
    (2049, 513, 65),    # gk = 2112 (nk = 66), set size 400; one sample into the THIRD sample tile
    (2049, 1, 257),     # many K steps on one sample, two set tiles
    (129, 513, 1),      # three sample tiles on one set ({g - 1}: the last gene alone)
    (64, 127, 256),     # no gene padding, a full set tile, a short wave row
]


@pytest.mark.parametrize("g,n,m", SHAPES)
def test_within_the_derived_bound_at_the_kernel_edges(pinned_ctx, g, n, m, capsys):
    """plaid_dense(sum / mean, normalize = FALSE) on the mfma backend against set_sums at mfma_bound, all five data kinds
    of mfma_ref.data; every column its own draw, so a value from the wrong sample, plane or K step changes a sum.  On
    positive data with g >= 31 some score must differ from the fp64 route's bits: the backend really ran"""
    Gp, Gi, names = mr.sets(g, m, 100 * g + m)
    for kind in mr.KINDS:
        X = np.asfortranarray(mr.data(kind, g, n, 7 * g + n))
        ref, mag, k = er.set_sums(Gp, Gi, X)
        ctx = pinned_ctx(spmm_dense_kernel="mfma")
        got_sum = ctx.plaid_dense(X, Gp, Gi, "sum", False)
        got_mean = ctx.plaid_dense(X, Gp, Gi, "mean", False)
        _check_sum_and_mean(capsys, f"g={g} n={n} m={m} {kind}", got_sum, got_mean, Gp, ref, mag, k)
        if names["empty"] is not None:
            assert np.all(got_sum[names["empty"]] == 0.0) and np.all(got_mean[names["empty"]] == 0.0)
        if kind == "well" and g >= 31:
            f64 = pinned_ctx().plaid_dense(X, Gp, Gi, "sum", False)
            er.assert_fp64_bound(f64, ref, mag, k, 1, "fp64 route")
            assert np.any(er.bits(got_sum) != er.bits(f64)), "the mfma backend returned the fp64 scores: it did not run"
        if kind == "half_ranks":
            with capsys.disabled():
                print(f"[measure] g={g} n={n} m={m} half_ranks: largest |error| {float(np.max(np.abs(got_sum - ref))):.3g} "
                      f"(exact split; fp32 adds half-integers below 2^23 exactly)")


# ---------------------------------------------------------------- the device entry, laid out by the test
class _Dev:
    """X with ldx > g, 8 bytes into its allocation, NaN in the padding rows g ... ldx of every column and around the matrix
    (never to be read: one of them in a sum would show); S with lds > m and sentinels"""

    def __init__(self, X, ldx, m, lds):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        g, n = X.shape
        assert ldx > g and lds > m
        self.g, self.n, self.ldx, self.m, self.lds = g, n, ldx, m, lds
        host = np.full((n, ldx), np.nan)
        host[:, :g] = X.T
        self.buf = torch.full((n * ldx + 2,), float("nan"), dtype=torch.float64, device=self.dev)
        self.buf[1:1 + n * ldx] = torch.from_numpy(host.ravel()).to(self.dev)
        self.before = self.buf.clone()
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + 8
        self.S = torch.empty((n, lds), dtype=torch.float64, device=self.dev)
        self.fl = torch.zeros(4, dtype=torch.int32, device=self.dev)
        torch.cuda.synchronize()

    def run(self, ctx, gs, stat, alpha=1.0, beta=0.0, alpha_div=None):
        """one dev_spmm_dense: (scores m x n, the three flag words); nothing outside m x n of S and nothing of X may change"""
        torch = self.torch
        self.S.fill_(SENTINEL)
        self.fl.zero_()
        torch.cuda.synchronize()
        ctx.dev_spmm_dense(gs, self.ptr, self.ldx, self.n, self.S.data_ptr(), self.lds, stat, alpha, beta, self.fl.data_ptr(),
                           alpha_div)
        ctx.synchronize()
        torch.cuda.synchronize()
        S = self.S.cpu().numpy()
        assert np.all(S[:, self.m:] == SENTINEL), "written outside m x n of S"
        assert torch.equal(self.buf.view(torch.int64), self.before.view(torch.int64)), "X or its surroundings were written"
        fl = self.fl.cpu().numpy()
        assert fl[3] == 0
        return np.ascontiguousarray(S[:, :self.m].T), fl[:3].copy()


def test_device_entry_odd_strides_sing_epilogue_and_flag_words(pinned_ctx, capsys):
    """g = 129, n = 257, m = 65 through dev_spmm_dense with ldx = g + 3 (odd: every other column only 8-byte aligned) and
    lds = m + 5.  replaid.sing's epilogue alpha = 1 / g, beta = -0.5 on the mean statistic, as a host scalar and as
    alpha = 1 with the device scalar alpha_div = g: the exact value w (s / g - k / 2) in long double; the fp32 error of the
    sum reaches the score through the exact factors w / g, the seven fp64 roundings are counted over w (mag / g + k / 2) as
    test_replaid_sing_within_the_fp64_bound_of_exact_rank_sums counts them.  Flag words equal the fp64 route's, on data
    where they are unambiguous (no empty set): positive columns [0, 0, 0], with a zero column [0, 1, 0], with a strictly
    negative column too [1, 1, 0]"""
    import torch
    g, n, m = 129, 257, 65
    Gp, Gi, names = mr.sets(g, m, 5)
    X = mr.data("normal", g, n, 17)
    ref, mag, k = er.set_sums(Gp, Gi, X)
    kk = np.diff(Gp).astype(np.float64)[:, None]
    w = _w(Gp)[:, None]
    ld = np.longdouble
    exact = (w.astype(ld) * (ref.astype(ld) / ld(g) - ld(0.5) * kk.astype(ld))).astype(np.float64)
    bound = (w / g) * mr.mfma_bound(mag, k, 0) + er.fp64_bound(w * (mag / g + 0.5 * kk), np.zeros(k.shape, dtype=np.int64), 7)
    d = _Dev(X, g + 3, m, m + 5)
    gdev = torch.full((1,), float(g), dtype=torch.float64, device=d.dev)
    torch.cuda.synchronize()
    gs = pinned_ctx().geneset(g, Gp, Gi)
    try:
        for alpha, div in ((1.0 / g, None), (1.0, gdev.data_ptr())):
            S64, f64 = d.run(pinned_ctx(), gs, "mean", alpha, -0.5, div)
            S, f = d.run(pinned_ctx(spmm_dense_kernel="mfma"), gs, "mean", alpha, -0.5, div)
            _measure(capsys, f"device entry, sing epilogue, alpha_div={div is not None}", S, exact, bound)
            er.assert_within(S, exact, bound, f"mfma sing epilogue alpha_div={div is not None}")
            er.assert_fp64_bound(S64, exact, w * (mag / g + 0.5 * kk), k, 7, "fp64 sing epilogue")
            assert np.array_equal(f, f64), (f, f64)
            assert list(f64) == [1, 1, 0]                       # (the empty set scores 0, every other set is below 0)
    finally:
        gs.close()
    # flag words on unambiguous data: the collection without its empty set (set 0)
    assert names["empty"] == 0 and Gp[1] == 0
    Gp2 = Gp[1:].copy()
    Xp = mr.data("well", g, 5, 23)
    cases = [("positive", Xp.copy(), [0, 0, 0])]
    Xz = Xp.copy()
    Xz[:, 1] = 0.0
    cases.append(("zero column", Xz.copy(), [0, 1, 0]))
    Xz[:, 3] = -Xz[:, 3]
    cases.append(("zero and negative columns", Xz, [1, 1, 0]))
    gs = pinned_ctx().geneset(g, Gp2, Gi)
    try:
        for what, Xc, expect in cases:
            dd = _Dev(Xc, g + 3, m - 1, m + 4)
            r2, m2, k2 = er.set_sums(Gp2, Gi, Xc)
            for stat in ("sum", "mean"):
                S64, f64 = dd.run(pinned_ctx(), gs, stat)
                S, f = dd.run(pinned_ctx(spmm_dense_kernel="mfma"), gs, stat)
                assert list(f64) == expect and np.array_equal(f, f64), (what, stat, f, f64)
                sc = _w(Gp2)[:, None] if stat == "mean" else 1.0
                er.assert_within(S, r2 * sc, mr.mfma_bound(m2 * sc, k2, 3 if stat == "mean" else 1), f"mfma {what} {stat}")
                assert np.all(S[:, 1] == 0.0) or what == "positive"
    finally:
        gs.close()


# ---------------------------------------------------------------- c. the launcher's loops
@pytest.mark.parametrize("n", [4097, 8193])
def test_sample_loop_and_second_panel(pinned_ctx, n, capsys):
    """g = 64, m = 3 through the device entry (one call over all columns).  n = 4097: rows_pad = 4352 > 4096, so
    split3_bf16_kernel's workgroups loop over samples.  n = 8193: a second panel of one column, X + 8192 ldx and
    S + 8192 lds.  Every column is its own draw of signed data; every column within the bound, the last one looked at on
    its own (column 8192 is the first of panel 2)"""
    g, m = 64, 3
    rng = np.random.default_rng(n)
    lists = [rng.choice(g, size=33, replace=False), np.array([g - 1]), np.array([0, g - 1])]
    Gp = np.concatenate([[0], np.cumsum([len(s) for s in lists])]).astype(np.int32)
    Gi = np.concatenate(lists).astype(np.int32)
    X = mr.data("normal", g, n, 3 * n)
    ref, mag, k = er.set_sums(Gp, Gi, X)
    d = _Dev(X, g + 3, m, m + 5)
    gs = pinned_ctx().geneset(g, Gp, Gi)
    try:
        S, f = d.run(pinned_ctx(spmm_dense_kernel="mfma"), gs, "sum")
        S64, f64 = d.run(pinned_ctx(), gs, "sum")
    finally:
        gs.close()
    bound = mr.mfma_bound(mag, k, 1)
    _measure(capsys, f"n={n}", S, ref, bound)
    er.assert_within(S[:, n - 1:], ref[:, n - 1:], bound[:, n - 1:], f"the last column of n={n}")
    er.assert_within(S, ref, bound, f"n={n}")
    er.assert_fp64_bound(S64, ref, mag, k, 1, "fp64 route")
    assert np.array_equal(f, f64)


# ---------------------------------------------------------------- d. one prepared collection across routes
def test_a_prepared_collection_across_routes_and_other_collections(pinned_ctx):
    """The dense bf16 membership is built on the collection's first mfma call and the workspace is shared by every
    collection of the context: a collection first used by the fp64 route, then by mfma, then again after ANOTHER collection
    with another gene count (another gk, another workspace layout) ran mfma on the same context, gives the bits of a fresh
    collection's first mfma call; the fp64 route in between keeps its bits"""
    gA, nA, mA = 129, 130, 65
    gB, nB, mB = 65, 257, 63
    GpA, GiA, _ = mr.sets(gA, mA, 1)
    GpB, GiB, _ = mr.sets(gB, mB, 2)
    XA = mr.data("cancel", gA, nA, 3)
    XB = mr.data("well", gB, nB, 4)
    dA = _Dev(XA, gA + 3, mA, mA + 5)
    dB = _Dev(XB, gB + 3, mB, mB + 5)
    refA, magA, kA = er.set_sums(GpA, GiA, XA)
    refB, magB, kB = er.set_sums(GpB, GiB, XB)
    fresh = pinned_ctx().geneset(gA, GpA, GiA)
    gsA = pinned_ctx().geneset(gA, GpA, GiA)
    gsB = pinned_ctx().geneset(gB, GpB, GiB)
    try:
        S_fresh, f_fresh = dA.run(pinned_ctx(spmm_dense_kernel="mfma"), fresh, "sum")
        er.assert_within(S_fresh, refA, mr.mfma_bound(magA, kA, 1), "fresh collection")
        S64, f64 = dA.run(pinned_ctx(), gsA, "sum")
        er.assert_fp64_bound(S64, refA, magA, kA, 1, "fp64 first")
        S1, f1 = dA.run(pinned_ctx(spmm_dense_kernel="mfma"), gsA, "sum")
        SB, _ = dB.run(pinned_ctx(spmm_dense_kernel="mfma"), gsB, "sum")
        er.assert_within(SB, refB, mr.mfma_bound(magB, kB, 1), "the other collection")
        S2, f2 = dA.run(pinned_ctx(spmm_dense_kernel="mfma"), gsA, "sum")
        S64b, _ = dA.run(pinned_ctx(), gsA, "sum")
        for S, f, what in ((S1, f1, "after the fp64 route"), (S2, f2, "after another collection")):
            er.assert_same_bits(S, S_fresh, what)
            assert np.array_equal(f, f_fresh)
        er.assert_same_bits(S64b, S64, "fp64 after mfma")
    finally:
        for gs in (fresh, gsA, gsB):
            gs.close()


# ---------------------------------------------------------------- e. values the split cannot carry
def _special_case():
    """g = 129, n = 7, 64 sets of mfma_ref.sets and one more, {0, 5, 11, 20}.  Signed data with, per sample:
    0 nothing; 1 NaN in gene g - 1 (sets {g - 1} and {0, g - 1}); 2 +Inf in gene 0 and -Inf in gene 5 (the added set holds
    both: NaN); 3 +Inf in gene 7; 4 -Inf in gene g - 1 and NaN in gene 9; 5 the finite 1e39 in gene 0 and -1e39 in gene 11
    (the added set holds both); 6 a finite value just below the range's end in gene 7 (its bf16 head rounds to Inf)"""
    g, n = 129, 7
    Gp, Gi, names = mr.sets(g, 64, 9)
    Gi = np.concatenate([Gi, np.array([0, 5, 11, 20], dtype=np.int32)]).astype(np.int32)
    Gp = np.concatenate([Gp, [len(Gi)]]).astype(np.int32)
    X = mr.data("normal", g, n, 29)
    X[g - 1, 1] = np.nan
    X[0, 2], X[5, 2] = np.inf, -np.inf
    X[7, 3] = np.inf
    X[g - 1, 4], X[9, 4] = -np.inf, np.nan
    X[0, 5], X[11, 5] = 1e39, -1e39
    X[7, 6] = -3.397e38
    return g, n, Gp, Gi, names, np.asfortranarray(X)


def _same_specials(got, exp, what):
    for name, fn in (("NaN", np.isnan), ("+Inf", lambda a: a == np.inf), ("-Inf", lambda a: a == -np.inf)):
        assert np.array_equal(fn(got), fn(exp)), f"{what}: the {name} pattern differs in {int(np.sum(fn(got) != fn(exp)))} scores"


def test_non_finite_values_reach_exactly_the_sets_that_hold_them(pinned_ctx, capsys):
    """plaid_dense and the device entry.  The NaN / +Inf / -Inf pattern is the fp64 route's and set_sums', element for
    element; every other score is within mfma_bound of the exact sum of the finite entries (set_sums' mag and k count only
    those); the flag words are the fp64 route's.  A finite value whose bf16 head would be Inf (1e39, -1e39, -3.397e38) is
    added in fp64 behind the matrix core: never a NaN anywhere in its sample, and the score is the exact sum of the OTHER
    members at mfma_bound plus the fp64 sum of such values in gene order (two more fp64 roundings over their magnitude)"""
    g, n, Gp, Gi, names, X = _special_case()
    m = len(Gp) - 1
    ref, mag, k = er.set_sums(Gp, Gi, X)
    assert np.isnan(ref[m - 1, 2]) and np.isnan(ref[names["last"], 1]) and ref[names["ends"], 2] == np.inf
    assert ref[names["last"], 4] == -np.inf and not np.isfinite(ref).all(axis=0)[1:5].any()
    assert np.isfinite(ref[:, [0, 5, 6]]).all() and np.isfinite(ref).any(axis=0).all()
    f64 = {st: pinned_ctx().plaid_dense(X, Gp, Gi, st, False) for st in ("sum", "mean")}
    ctx = pinned_ctx(spmm_dense_kernel="mfma")
    got = {st: ctx.plaid_dense(X, Gp, Gi, st, False) for st in ("sum", "mean")}
    for st in ("sum", "mean"):
        _same_specials(got[st], f64[st], f"plaid_dense {st} against the fp64 route")
        _same_specials(got[st], ref, f"plaid_dense {st} against set_sums")
    _check_sum_and_mean(capsys, "specials", got["sum"], got["mean"], Gp, ref, mag, k)
    # the finite values past the range: samples 5 and 6
    big = ~mr.splittable(X) & np.isfinite(X)
    assert big.sum() == 3
    X0 = np.where(big, 0.0, X)
    ref0, mag0, k0 = er.set_sums(Gp, Gi, X0)
    sp = np.zeros((m, n))
    for j in range(m):
        idx = np.sort(Gi[Gp[j]:Gp[j + 1]])
        for c in (5, 6):
            for i in idx[big[idx, c]]:
                sp[j, c] += X[i, c]                          # (fp64, in gene order, as the fix-up adds them)
    assert sp[m - 1, 5] == 0.0 and sp[names["ends"], 5] == 1e39
    cols = [5, 6]
    bound = mr.mfma_bound(mag0, k0, 1) + er.fp64_bound(np.abs(sp) + mag0, np.zeros(k0.shape, dtype=np.int64), 2)
    er.assert_within(got["sum"][:, cols], (ref0 + sp)[:, cols], bound[:, cols], "finite values past the bf16 range")
    assert np.isfinite(got["sum"][:, [0, 5, 6]]).all() and np.isfinite(got["mean"][:, [0, 5, 6]]).all()
    # the device entry: the same through odd strides, with the flag words
    d = _Dev(X, g + 3, m, m + 5)
    gs = pinned_ctx().geneset(g, Gp, Gi)
    try:
        for st in ("sum", "mean"):
            S64, fl64 = d.run(pinned_ctx(), gs, st)
            S, fl = d.run(pinned_ctx(spmm_dense_kernel="mfma"), gs, st)
            _same_specials(S, S64, f"device entry {st}")
            er.assert_same_bits(S, got[st], f"device entry {st} against plaid_dense")
            assert np.array_equal(fl, fl64) and list(fl64) == [1, 1, 1], (st, fl, fl64)
    finally:
        gs.close()


def test_non_finite_values_in_a_singleton_only_collection_keep_the_flag_words(pinned_ctx):
    """a staged-out value scores 0 inside the matrix core: in a collection of singletons on positive data a NaN must give
    [0, 0, 1], not has_zero -- and +Inf [0, 0, 0], -Inf [1, 0, 0], as on the fp64 route"""
    g, n = 33, 3
    Gp = np.arange(g + 1, dtype=np.int32)
    Gi = np.arange(g, dtype=np.int32)
    for value, expect in ((np.nan, [0, 0, 1]), (np.inf, [0, 0, 0]), (-np.inf, [1, 0, 0]), (1e39, [0, 0, 0])):
        X = mr.data("well", g, n, 31)
        X[g - 1, 1] = value
        d = _Dev(X, g + 3, g, g + 5)
        gs = pinned_ctx().geneset(g, Gp, Gi)
        try:
            S64, f64 = d.run(pinned_ctx(), gs, "sum")
            S, f = d.run(pinned_ctx(spmm_dense_kernel="mfma"), gs, "sum")
        finally:
            gs.close()
        assert list(f64) == expect and np.array_equal(f, f64), (value, f, f64)
        er.assert_same_bits(S[g - 1, 1], value, "the planted value, alone in its set")
        ref, mag, k = er.set_sums(Gp, Gi, X)
        fin = np.isfinite(X) & mr.splittable(X)
        er.assert_within(np.where(fin, S, 0.0), np.where(fin, ref, 0.0), mr.mfma_bound(mag, k, 1), f"the other scores, {value}")


def test_rank_scorers_keep_the_fp64_routes_pattern(pinned_ctx, capsys):
    """replaid.sing and replaid.ssgsea(alpha = 0.25) on the mfma backend, on the planted matrix: the crossprod sees rank
    weights, where +-Inf and 1e39 are ordinary values and NaN stays NaN.  The pattern is the fp64 route's element for
    element.  Every other score: replaid.sing within (w / g) mfma_bound + the seven fp64 roundings of the exact
    w (R / g - k / 2) from the device's own (exact, integer) ranks; replaid.ssgsea, where the fp64 route leaves finite
    scores at all, within the bound of _ssgsea_within_the_bound (tests/test_gpu_exact_sums.py: c = 12 for alpha = 0.25)
    with (w / max) mfma_bound in place of the fp64 sum's k u mag, through normalize_medians' Lipschitz bound"""
    g, n, Gp, Gi, names, X = _special_case()
    kk = np.diff(Gp).astype(np.float64)[:, None]
    w = _w(Gp)[:, None]
    ld = np.longdouble
    base = pinned_ctx()
    s64 = base.sing_dense(X, Gp, Gi)
    e64 = base.ssgsea_dense(X, Gp, Gi, 0.25)
    Rmin = base.colranks_dense(X, "min")
    Ravg = base.colranks_dense(X, "average")
    ctx = pinned_ctx(spmm_dense_kernel="mfma")
    s = ctx.sing_dense(X, Gp, Gi)
    e = ctx.ssgsea_dense(X, Gp, Gi, 0.25)
    _same_specials(s, s64, "replaid.sing")
    _same_specials(e, e64, "replaid.ssgsea")
    assert np.array_equal(np.isnan(Rmin), np.isnan(X)) and np.isnan(s64).any() and np.isfinite(s64[:, 0]).all()
    # replaid.sing
    R, mag, k = er.set_sums(Gp, Gi, Rmin)
    with np.errstate(invalid="ignore"):
        exact = (w.astype(ld) * (R.astype(ld) / ld(g) - ld(0.5) * kk.astype(ld))).astype(np.float64)
    zero = np.zeros(k.shape, dtype=np.int64)
    fp64_part = er.fp64_bound(w * (mag / g + 0.5 * kk), zero, 7)
    er.assert_within(s64, exact, fp64_part, "fp64 replaid.sing")
    bound = (w / g) * mr.mfma_bound(mag, k, 0) + fp64_part
    _measure(capsys, "replaid.sing with NaN / Inf planted", s, exact, bound)
    er.assert_within(s, exact, bound, "mfma replaid.sing")
    # replaid.ssgsea(alpha = 0.25)
    if np.isfinite(e64).any():
        with np.errstate(invalid="ignore"):
            W = np.power(Ravg.astype(ld), ld(1.25))
        wmax = np.nanmax(W)
        P, magP, kP = _long_sums(Gp, Gi, W)
        with np.errstate(invalid="ignore"):
            T = (w.astype(ld) * (P / wmax - ld(0.5) * kk.astype(ld))).astype(np.float64)
        magT = w * (magP / float(wmax) + 0.5 * kk)
        E64 = (kP + 12) * er.U * magT
        N, B64 = _normalized_ref(T, E64)
        er.assert_within(e64, N, B64, "fp64 replaid.ssgsea")
        E = (w / float(wmax)) * mr.mfma_bound(magP, kP, 0) + E64
        N, B = _normalized_ref(T, E)
        _measure(capsys, "replaid.ssgsea(0.25) with NaN / Inf planted", e, N, B)
        er.assert_within(e, N, B, "mfma replaid.ssgsea")
    else:
        with capsys.disabled():
            print("\n[measure] replaid.ssgsea(0.25): a NaN makes max(rX) NaN, every score of both routes is NaN")
