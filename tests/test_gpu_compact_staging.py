"""The two compact stagings of the dense crossprod past one trip of their persistent loop -- `pytest -m gpu`.

spmm_colquad_u16 (2 * rank as u16, four sample columns per LDS entry, integer sums: the default of every rank-valued
crossprod with 8,192 < genes <= 20,448) and spmm_colpair_mixed (two columns as fp32, four-term fp32 partial sums folded
into fp64 accumulators: replaid.gsva(tau = 0), ranks_f32 = 1 and the whole of PLAIDHIP_PRECISION_MIXED) launch
min(CUs, quads or pairs) workgroups that WALK their quads or pairs: stage from registers, gather, request the next quad's
first items into registers, load the late items behind the barrier, meet the barrier that lets the next trip overwrite the
LDS, and carry the words that decide the fp64 fallback across all trips.  With more than 4 x CUs (2 x CUs) samples every
workgroup makes a second trip; these tests hold both kernels there

  * on rank inputs: bit for bit to an INTEGER reference (tests/helpers/compact_ref.py::rank_sums), never only to another
    device route -- and the fp64 route on the same input to the same bits and flag words (include/plaidhip.h's contract);
  * on arbitrary doubles in mixed mode: within the derived bound compact_ref.mixed_bound of the exact sums
    (exact_ref.set_sums), on well-conditioned and on cancelling data.

Every column is an independent draw, so a value taken from the wrong quad, the wrong trip or a stale register changes a
sum; plaidhip_debug_spec_fell_back says whether the u16 scores stand (0) or the fp64 kernel behind them recomputed (1) --
without it a quad kernel that wrongly reports a non-rank would pass every comparison.
"""
import numpy as np
import pytest

from tests.helpers import compact_ref as cr
from tests.helpers import exact_ref as er

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
LO, HI = 8192, 20448           # the compact stagings take LO < genes <= HI (one gene slice, 16 wavefronts)


def _cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _n(spec):
    """sample counts given in CUs: "2cu+3" -> 2 * CUs + 3"""
    if isinstance(spec, int):
        return spec
    a, b = spec.split("cu+")
    return int(a) * _cu() + int(b)


# ---------------------------------------------------------------- inputs and references, computed once per shape
_RANKS = {}


def _rank_case(g, n):
    """(R g x n: average ranks of tied data, every column an independent draw; Gp, Gi, names; exact sums, k) -- the last
    shape is kept, the tests of one shape stand together"""
    key = (g, n)
    if key not in _RANKS:
        from oracle import c_oracle
        _RANKS.clear()
        rng = np.random.default_rng(1000 * g + n)
        X = np.asfortranarray(rng.integers(0, 3000, size=(g, n)).astype(np.float64))    # ~g / 3000 genes per tie group
        R = c_oracle.colranks_dense_mt(X, "average", threads=8)
        assert R.min() >= 1.0 and R.max() <= g and np.any(R != np.rint(R)) and np.all(2 * R == np.rint(2 * R))
        Gp, Gi, names = cr.sets(g, g + 1)
        sums, k = cr.rank_sums(Gp, Gi, R)
        _RANKS[key] = (R, Gp, Gi, names, sums, k)
    return _RANKS[key]


def _assert_columns_differ_across_trips(R, cols_per_pass):
    """the first column of every quad (pair) differs from the first column of the quad CU quads later -- the one the same
    workgroup stages next -- in at least g / 2 rows"""
    g, n = R.shape
    step = cols_per_pass * _cu()
    for c in range(0, n - step, cols_per_pass):
        assert np.count_nonzero(R[:, c] != R[:, c + step]) >= g / 2, (c, c + step)


class _Dev:
    """device memory laid out by the test: R with ldr > g, 8 bytes into its allocation, NaN in the padding rows g ... ldr of
    every column (neither summed nor mistaken for non-ranks); S with lds = m + 3 and sentinels"""

    def __init__(self, R, ldr, m):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        g, n = R.shape
        assert ldr > g
        self.g, self.n, self.ldr, self.m, self.lds = g, n, ldr, m, m + 3
        host = np.full((n, ldr), np.nan)
        host[:, :g] = R.T
        self.buf = torch.full((n * ldr + 2,), float("nan"), dtype=torch.float64, device=self.dev)
        self.buf[1:1 + n * ldr] = torch.from_numpy(host.ravel()).to(self.dev)
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + 8
        self.S = torch.empty((n, self.lds), dtype=torch.float64, device=self.dev)
        self.fl = torch.zeros(4, dtype=torch.int32, device=self.dev)
        torch.cuda.synchronize()

    def poke(self, row, col, value):
        """R[row, col] = value; returns the value that was there"""
        i = 1 + col * self.ldr + row
        old = float(self.buf[i])
        self.buf[i] = value
        self.torch.cuda.synchronize()
        return old

    def run(self, ctx, gs, entry, stat, alpha=1.0, beta=0.0, alpha_div=None):
        """one crossprod through dev_spmm_ranks / dev_spmm_dense: (scores m x n, the three flag words); nothing outside
        m x n of S may change"""
        self.S.fill_(SENTINEL)
        self.fl.zero_()
        self.torch.cuda.synchronize()
        call = ctx.dev_spmm_ranks if entry == "ranks" else ctx.dev_spmm_dense
        call(gs, self.ptr, self.ldr, self.n, self.S.data_ptr(), self.lds, stat, alpha, beta, self.fl.data_ptr(), alpha_div)
        ctx.synchronize()
        self.torch.cuda.synchronize()
        S = self.S.cpu().numpy()
        assert np.all(S[:, self.m:] == SENTINEL), "written outside m x n of S"
        fl = self.fl.cpu().numpy()
        assert fl[3] == 0
        return np.ascontiguousarray(S[:, :self.m].T), fl[:3].copy()


ROUTES = [("u16", 2, "ranks"), ("fp32", 1, "ranks"), ("fp64", 0, "dense")]


def _check_rank_routes(pin, R, Gp, Gi, sums, k, ldr, stats=("sum", "mean")):
    """the three routes on one device matrix: each bit for bit the integer reference, the same flag words; the fallback
    indicator 0 after the u16 route wherever the quad kernel takes the shape"""
    g = R.shape[0]
    m = len(Gp) - 1
    d = _Dev(R, ldr, m)
    gs = pin().geneset(g, Gp, Gi)
    try:
        for stat in stats:
            exp = cr.expected_bits(sums, k, stat)
            flags = {}
            for name, opt, entry in ROUTES:
                ctx = pin(ranks_f32=opt)
                S, flags[name] = d.run(ctx, gs, entry, stat)
                er.assert_same_bits(S, exp, f"{name} {stat} g={g} n={R.shape[1]} ldr={ldr}")
                if name == "u16" and LO < g <= HI:
                    assert not ctx.debug_spec_fell_back(), "the u16 kernel reported a non-rank on a clean rank matrix"
            assert np.array_equal(flags["u16"], flags["fp64"]) and np.array_equal(flags["fp32"], flags["fp64"]), flags
            assert list(flags["fp64"]) == [0, 1, 0]          # (the empty set scores 0; ranks are positive)
    finally:
        gs.close()
        pin()
    return d


# ---------------------------------------------------------------- 3. rank inputs, bit for bit
@pytest.mark.parametrize("g", [8193, 8194, 10240, 14338, 18434, 20447, 20448, 8192, 20449])
def test_gene_seams_of_the_staging(pinned_ctx, g):
    """n = 5 (one trip, quad tail 1, pair tail 1).  Ten items of 1,024 gene pairs per thread, an odd last gene by thread 0:
    8193 = four items exactly + the last gene; 8194 one thread in item 4; 10240 five full items, the late items 6..9 all
    out of range; 14338 / 18434 one thread in the late items 7 / 9; 20447 odd, 20448 the maximum (item 9 with 1,008
    threads); 8192 and 20449 take the general kernels and must give the same exact bits.  ldr = g + 7: odd for even g, so
    every other column is 8 bytes off 16-byte alignment"""
    R, Gp, Gi, names, sums, k = _rank_case(g, 5)
    _check_rank_routes(pinned_ctx, R, Gp, Gi, sums, k, g + 7)


@pytest.mark.parametrize("g,n", [(8194, 1), (8194, 2), (8194, 3), (8194, 4), (8194, "2cu+3"), (8194, "4cu+5"),
                                 (20447, 1), (20447, 2), (20447, 3), (20447, 4), (20447, "2cu+3"), (20447, "4cu+5"),
                                 (8193, "8cu+1")])
def test_sample_counts_past_one_trip(pinned_ctx, g, n):
    """1 ... 4: every quad and pair tail.  2 CU + 3: every workgroup of the fp32 kernel walks two pairs or more and the last
    pair has no column B.  4 CU + 5: every workgroup of the u16 kernel walks two quads and the last quad has one column.
    8 CU + 1 at 8,193 genes: three trips for some workgroups, two for the others, the odd last gene on every trip"""
    n = _n(n)
    R, Gp, Gi, names, sums, k = _rank_case(g, n)
    _assert_columns_differ_across_trips(R, 4)
    _assert_columns_differ_across_trips(R, 2)
    _check_rank_routes(pinned_ctx, R, Gp, Gi, sums, k, g + 7)


def test_largest_admissible_values(pinned_ctx):
    """g = 20448, n = 5: one column of 32,767.5 throughout (the largest 2x a u16 holds), one of zeros, the rest true ranks.
    The set of every gene sums to 20,448 x 32,767.5 exactly: the u16 kernel's 32-bit accumulators (1.34e9 < 2^32) and the
    fp32 kernel's four-term partials (131,070, one fractional bit) must both be exact.  The zero column sets has_zero, and
    no flag word differs from the fp64 route's"""
    g = HI
    R, Gp, Gi, names, _, _ = _rank_case(g, 5)
    R = R.copy()
    R[:, 1] = 32767.5
    R[:, 3] = 0.0
    sums, k = cr.rank_sums(Gp, Gi, R)
    assert sums[names["all"], 1] == 20448 * 32767.5 == 670029840.0 and np.all(sums[:, 3] == 0.0)
    _check_rank_routes(pinned_ctx, R, Gp, Gi, sums, k, g + 7)


def test_replaid_sing_epilogue_past_one_trip(pinned_ctx):
    """n = 4 CU + 5, g = 8194: alpha = 1 / g, beta = -0.5, and the alpha_div form with a device scalar; the compact stagings
    give the bits of dev_spmm_dense under ranks_f32 = 0, and all lie within the fp64 bound of the long-double value
    w (R / g - k / 2) with the c = 7 that test_replaid_sing_within_the_fp64_bound_of_exact_rank_sums derives"""
    import torch
    g = 8194
    n = _n("4cu+5")
    R, Gp, Gi, names, sums, k = _rank_case(g, n)
    m = len(Gp) - 1
    ld = np.longdouble
    kk = k.astype(np.float64)[:, None]
    w = cr.set_weight(k)[:, None]
    exact = (w.astype(ld) * (sums.astype(ld) / ld(g) - ld(0.5) * kk.astype(ld))).astype(np.float64)
    mag = w * (sums / g + 0.5 * kk)
    d = _Dev(R, g + 7, m)
    gdev = torch.full((1,), float(g), dtype=torch.float64, device=d.dev)
    torch.cuda.synchronize()
    gs = pinned_ctx().geneset(g, Gp, Gi)
    try:
        for alpha, div in ((1.0 / g, None), (1.0, gdev.data_ptr())):
            out = {}
            for name, opt, entry in ROUTES:
                ctx = pinned_ctx(ranks_f32=opt)
                out[name] = d.run(ctx, gs, entry, "mean", alpha, -0.5, div)
                if name == "u16":
                    assert not ctx.debug_spec_fell_back()
            for name in ("u16", "fp32"):
                er.assert_same_bits(out[name][0], out["fp64"][0], f"sing epilogue {name} div={div is not None}")
                assert np.array_equal(out[name][1], out["fp64"][1])
            er.assert_fp64_bound(out["fp64"][0], exact, mag, np.zeros(sums.shape, dtype=np.int64), 7, "sing epilogue")
            assert list(out["fp64"][1]) == [1, 1, 0]
    finally:
        gs.close()


def test_replaid_scorers_default_staging_past_one_trip(pinned_ctx):
    """4 CU + 5 samples, g = 8194, 200 sets: the default staging and ranks_f32 = 0 agree bit for bit on replaid.sing,
    replaid.ssgsea(alpha = 0), replaid.ucell (integer rmax + 1) and replaid.gsva(tau = 0, "z") -- the fp32 kernel on signed
    ranks (PLAIDHIP_X_EXACT_F32).  With the device-entry cases above this puts their default routes on an exact footing
    past one trip"""
    g = 8194
    n = _n("4cu+5")
    rng = np.random.default_rng(g + n)
    X = np.asfortranarray(np.round(rng.normal(8.0, 2.0, size=(g, n)), 1))      # ties; every column its own draw
    Gp, Gi, _ = cr.sets(g, 17, m_random=196)
    assert len(Gp) - 1 == 200
    kf = np.diff(Gp).astype(np.float64)
    outs = {}
    for opt in (2, 0):
        ctx = pinned_ctx(ranks_f32=opt)
        outs[opt] = {"sing": ctx.sing_dense(X, Gp, Gi), "ssgsea": ctx.ssgsea_dense(X, Gp, Gi, 0.0)}
        if opt == 2:
            assert not ctx.debug_spec_fell_back()
        outs[opt]["ucell"] = ctx.ucell(X, Gp, Gi, kf, 1500.0)
        if opt == 2:
            assert not ctx.debug_spec_fell_back()
        outs[opt]["gsva"] = ctx.gsva(X, Gp, Gi, 0.0, "z")
    for what in outs[0]:
        assert outs[2][what].shape == (200, n)
        er.assert_same_bits(outs[2][what], outs[0][what], what)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -3.0, 40000.0, 0.25])
def test_a_non_rank_on_a_later_trip_falls_back_to_fp64(pinned_ctx, bad):
    """default staging, n = 4 CU + 5, g = 8193: one value that is not a rank -- in the last column, in a middle row of column
    4 CU + 1 (second trip), in row g - 1 (the odd last gene, staged by thread 0) of a second-trip column, and in column 1
    (the FIRST trip of a workgroup that makes a second: the check words must survive the later trip) -- must give the
    bits, NaN pattern and flag words of dev_spmm_dense under ranks_f32 = 0, with the fallback indicator at 1.  The bad runs
    use replaid.sing's epilogue (negative scores: the quad kernel's private has_neg is set); the clean raw sums afterwards
    must be exact again with has_neg clear -- the private flag words were reset -- and the indicator back at 0"""
    g = 8193
    cu = _cu()
    n = 4 * cu + 5
    R, Gp, Gi, names, sums, k = _rank_case(g, n)
    m = len(Gp) - 1
    d = _Dev(R, g + 7, m)
    gs = pinned_ctx().geneset(g, Gp, Gi)
    try:
        for row, col in ((g // 2 + 1, n - 1), (g // 2, 4 * cu + 1), (g - 1, 4 * cu + 2), (g // 2 + 2, 1)):
            old = d.poke(row, col, bad)
            assert old == R[row, col]
            ctx = pinned_ctx(ranks_f32=2)
            S1, f1 = d.run(ctx, gs, "ranks", "mean", 1.0 / g, -0.5)
            assert ctx.debug_spec_fell_back(), (bad, row, col)
            S0, f0 = d.run(pinned_ctx(ranks_f32=0), gs, "dense", "mean", 1.0 / g, -0.5)
            er.assert_same_bits(S1, S0, f"non-rank {bad} at ({row}, {col})")
            assert np.array_equal(np.isnan(S1), np.isnan(S0)) and np.array_equal(f1, f0), (bad, row, col, f1, f0)
            hit = np.zeros((m, n), dtype=bool)
            for j in range(m):
                hit[j, col] = row in Gi[Gp[j]:Gp[j + 1]]
            assert hit.sum() >= 2                                        # (the set of every gene and one more at least)
            if bad != bad:
                assert np.array_equal(np.isnan(S1), hit) and f1[2] == 1
            else:
                assert not np.isnan(S1).any() and f1[2] == 0
            d.poke(row, col, old)
        ctx = pinned_ctx(ranks_f32=2)
        S, f = d.run(ctx, gs, "ranks", "sum")
        assert not ctx.debug_spec_fell_back()
        er.assert_same_bits(S, sums, "clean matrix after the fallbacks")
        assert list(f) == [0, 1, 0]
    finally:
        gs.close()


# ---------------------------------------------------------------- 4. mixed mode: arbitrary doubles within mixed_bound
def _mixed_and_f64(X, Gp, Gi):
    """plaid_dense sum and mean (normalize = FALSE) on a private context: fp64, mixed, and fp64 again"""
    import plaid_amd
    ctx = plaid_amd.Context(0)
    try:
        f64 = [ctx.plaid_dense(X, Gp, Gi, st, False) for st in ("sum", "mean")]
        ctx.set_precision("mixed")
        try:
            mixed = [ctx.plaid_dense(X, Gp, Gi, st, False) for st in ("sum", "mean")]
        finally:
            ctx.set_precision("f64")
        again = [ctx.plaid_dense(X, Gp, Gi, st, False) for st in ("sum", "mean")]
    finally:
        ctx.close()
    return f64, mixed, again


@pytest.mark.parametrize("g,n", [(8193, 5), (10240, 5), (20448, 5), (8194, 1), (8194, "2cu+3")])
def test_mixed_mode_within_the_derived_bound(g, n, capsys):
    """both data kinds of test_gpu_exact_sums.py, the sets of the rank tests (the set of every gene included: on positive
    data it is what catches fp32 accumulation across chunks, tests/test_compact_staging_ref.py).  c = 1 for the sum, c = 3
    for the mean, as in _check_mean_and_sum.  At least one score differs from the fp64 result (the staging really ran), and
    after set_precision("f64") the fp64 bits are back.  (Through the host entry plaid_dense, which uploads an X of more than
    8 MB in panels and launches per panel: the one launch over 2 CU + 3 columns is the device-entry test below)"""
    n = _n(n)
    Gp, Gi, names = cr.sets(g, g + 2)
    w = cr.set_weight(np.diff(Gp))[:, None]
    for kind in ("well", "cancel"):
        X = cr.data(kind, g, n, 7 * g + n)
        ref, mag, k = er.set_sums(Gp, Gi, X)
        f64, mixed, again = _mixed_and_f64(X, Gp, Gi)
        er.assert_fp64_bound(f64[0], ref, mag, k, 1, f"fp64 {kind} sum")
        for (what, c, r, mg), got, base, back in zip((("sum", 1, ref, mag), ("mean", 3, ref * w, mag * w)), mixed, f64, again):
            bound = cr.mixed_bound(mg, k, c)
            ok = bound > 0
            ratio = float((np.abs(got - r)[ok] / bound[ok]).max())
            with capsys.disabled():
                print(f"\n[mixed bound] g={g} n={n} {kind} {what}: largest error / bound = {ratio:.4f} "
                      f"(set of every gene: {float((np.abs(got - r) / bound)[names['all']].max()):.4f})")
            er.assert_within(got, r, bound, f"mixed {kind} {what} g={g} n={n}")
            assert np.any(er.bits(got) != er.bits(base)), "mixed mode returned the fp64 scores: the fp32 staging did not run"
            er.assert_same_bits(back, base, "fp64 after mixed")


@pytest.mark.parametrize("kind", ["well", "cancel"])
def test_mixed_mode_device_entry_past_one_trip(kind, capsys):
    """g = 8194, n = 2 CU + 3 through dev_spmm_dense on a private mixed context: ONE launch over all columns, so every
    workgroup of the fp32 kernel walks two pairs or more and the last pair has no column B.  (The host entry above uploads
    a large X in panels and launches per panel: its launches are narrower than its n.)  Same sets, bound and references;
    odd leading dimension, offset base pointer, NaN padding rows, sentinels around S"""
    import plaid_amd
    g = 8194
    n = _n("2cu+3")
    Gp, Gi, names = cr.sets(g, g + 2)
    m = len(Gp) - 1
    w = cr.set_weight(np.diff(Gp))[:, None]
    X = cr.data(kind, g, n, 7 * g + n + 1)
    ref, mag, k = er.set_sums(Gp, Gi, X)
    d = _Dev(X, g + 7, m)
    ctx = plaid_amd.Context(0)
    gs = ctx.geneset(g, Gp, Gi)
    try:
        f64 = {st: d.run(ctx, gs, "dense", st) for st in ("sum", "mean")}
        ctx.set_precision("mixed")
        try:
            mixed = {st: d.run(ctx, gs, "dense", st) for st in ("sum", "mean")}
        finally:
            ctx.set_precision("f64")
        back = {st: d.run(ctx, gs, "dense", st) for st in ("sum", "mean")}
    finally:
        gs.close()
        ctx.close()
    er.assert_fp64_bound(f64["sum"][0], ref, mag, k, 1, f"fp64 {kind} sum")
    er.assert_fp64_bound(f64["mean"][0], ref * w, mag * w, k, 3, f"fp64 {kind} mean")
    for st, c, r, mg in (("sum", 1, ref, mag), ("mean", 3, ref * w, mag * w)):
        got = mixed[st][0]
        bound = cr.mixed_bound(mg, k, c)
        ratio = np.abs(got - r) / bound
        with capsys.disabled():
            print(f"\n[mixed bound] device entry g={g} n={n} {kind} {st}: largest error / bound = {float(ratio.max()):.4f} "
                  f"(set of every gene: {float(ratio[names['all']].max()):.4f})")
        er.assert_within(got, r, bound, f"mixed device entry {kind} {st}")
        assert np.any(er.bits(got) != er.bits(f64[st][0])), "the fp32 staging did not run"
        assert np.array_equal(mixed[st][1], f64[st][1])
        er.assert_same_bits(back[st][0], f64[st][0], "fp64 after mixed")
    assert list(f64["sum"][1]) == ([0, 1, 0] if kind == "well" else [1, 1, 0])


def test_mixed_mode_specials_of_the_fp32_cast(pinned_ctx):
    """g = 8194, n = 5 through the device entry of a private mixed context: one NaN and one +Inf in members of known sets
    propagate to exactly those scores, 1e39 (finite, past the fp32 range) becomes +Inf in its sets, 1e-46 (below half the
    smallest fp32 subnormal) contributes 0 -- the singleton {g - 1} scores exactly 0 --, everything else stays within the
    bound, and the flag words are those of the fp64 route (include/plaidhip.h, next to PLAIDHIP_PRECISION_MIXED)"""
    import plaid_amd
    g, n = 8194, 5
    Gp, Gi, names = cr.sets(g, g + 2)
    m = len(Gp) - 1
    X = cr.data("well", g, n, 41)
    member = lambda j: int(Gi[Gp[j]])                          # noqa: E731  (a member of set j)
    g_nan, g_inf, g_big = member(5), member(9), member(12)
    assert len({g_nan, g_inf, g_big, g - 1}) == 4
    X[g_nan, 1] = np.nan
    X[g_inf, 2] = np.inf
    X[g_big, 3] = 1e39
    X[g - 1, 0] = 1e-46
    Xref = X.copy()
    Xref[g_big, 3] = np.inf                                    # what the cast makes of it
    Xref[g - 1, 0] = 0.0
    ref, mag, k = er.set_sums(Gp, Gi, Xref)
    assert np.isnan(ref[5, 1]) and ref[9, 2] == np.inf and ref[12, 3] == np.inf and np.isnan(ref[names["all"], 1])
    d = _Dev(X, g + 7, m)
    ctx = plaid_amd.Context(0)
    gs = ctx.geneset(g, Gp, Gi)
    try:
        S64, f64 = d.run(ctx, gs, "dense", "sum")
        ctx.set_precision("mixed")
        try:
            S32, f32 = d.run(ctx, gs, "dense", "sum")
        finally:
            ctx.set_precision("f64")
        Sback, fback = d.run(ctx, gs, "dense", "sum")
    finally:
        gs.close()
        ctx.close()
    er.assert_within(S32, ref, cr.mixed_bound(mag, k, 1), "mixed specials")
    assert S32[names["last"], 0] == 0.0 and S64[names["last"], 0] == 1e-46
    assert np.isfinite(S64[12, 3]) and S64[12, 3] > 9e38 and S32[12, 3] == np.inf
    assert np.array_equal(np.isnan(S32), np.isnan(S64)) and np.isnan(S32).sum() == np.isnan(ref).sum()
    assert np.array_equal(f32, f64) and list(f64) == [0, 1, 1]
    er.assert_same_bits(Sback, S64, "fp64 after mixed")
    assert np.array_equal(fback, f64)
