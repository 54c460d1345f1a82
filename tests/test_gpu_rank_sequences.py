"""The rank kernels past a workgroup's first column (`pytest -m gpu`).

Every rank kernel here walks several columns per workgroup once a launch has more columns than workgroups, and carries
state across: the bucket ranker's prefetched successor (have_next, xc_n / rc_n / cnt_n), its histograms and hand-over flag,
the sorting networks' LDS key area and NaN counter, the densify scratch column, the partitioned ranker's LDS counters.  The
other rank tests give a workgroup ONE hard column, or many benign ones.  These deal decks (tests/helpers/rank_decks.py) in
which, for the grid the launcher uses, every kind of column follows every kind inside some workgroup, and make two
assertions per case, both bit for bit with equal NaN positions:

  (a) power 1: the whole launch equals the C oracle (rank_decks.ranks_ref / csc_ranks_ref);
  (b) the whole launch -- with the column maxima and power 1.25 where the route has them -- equals the concatenation of
      launches over chunks of at most `grid` columns: single-trip launches, which the other tests pin.

The grids are restated from launch_ranks, launch_bucket, launch_network and launch_colranks_partitioned
(plaid_amd/csrc/kernels_rank.hip); each test first asserts that its deck shows every ordered pair FOR THAT GRID -- a
condition on the input: if a launcher's grid changes, the deck must change with it."""
import numpy as np
import pytest

from tests.helpers import rank_decks as rd

pytestmark = pytest.mark.gpu

TRIPS, TAIL = 3, 37
ORDINARY = tuple(k for k in rd.KINDS if k != "forced")


def _cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _same_bits(A, B):
    """equal bit patterns, or NaN in both"""
    import torch
    return bool(((A.view(torch.int64) == B.view(torch.int64)) | (torch.isnan(A) & torch.isnan(B))).all().item())


def _empty(shape):
    import torch
    return torch.full(shape, -7.0, dtype=torch.float64, device=torch.device("cuda", 0))


def _chunks(n, grid):
    return [(c0, min(grid, n - c0)) for c0 in range(0, n, grid)]


# ---------------------------------------------------------------------------------------------------------- launch forms
def _handed(fbs):
    """columns handed to the sorting network over a series of launches, from Context.debug_rank_fallbacks after each:
    (by the bucket ranker, by the partitioned ranker); a launcher that kept no list counts 0"""
    return tuple(sum(max(f[k], 0) for f in fbs) for k in (0, 1))


def _dense_launch(ctx, Xd, g, cols, ties, signed, power, colmax):
    """dev_colranks_dense over the column ranges `cols` of Xd ((n, g) row-major == g x n column-major): ranks, maxima"""
    import torch
    n = Xd.shape[0]
    R = _empty((n, g))
    cm = _empty((n,)) if colmax else None
    torch.cuda.synchronize()
    fbs = []
    for c0, nc in cols:
        ctx.dev_colranks_dense(Xd.data_ptr() + c0 * g * 8, g, g, nc, R.data_ptr() + c0 * g * 8, g, ties, signed, power,
                               cm.data_ptr() + c0 * 8 if colmax else None)
        fbs.append(ctx.debug_rank_fallbacks())
    ctx.synchronize()
    return R, cm, _handed(fbs)


def _csc_launch(ctx, Xp, Xx, max_col_nnz, cols, ties, signed, power, colmax):
    """dev_colranks_csc over column ranges: Xp is cut at column boundaries (its entries are offsets into Xx and Rx)"""
    import torch
    n = Xp.shape[0] - 1
    Rx = _empty((max(int(Xx.shape[0]), 1),))
    cm = _empty((n,)) if colmax else None
    torch.cuda.synchronize()
    fbs = []
    for c0, nc in cols:
        ctx.dev_colranks_csc(Xp.data_ptr() + c0 * 4, Xx.data_ptr(), nc, max_col_nnz, Rx.data_ptr(), ties, signed, power,
                             cm.data_ptr() + c0 * 8 if colmax else None)
        fbs.append(ctx.debug_rank_fallbacks())
    ctx.synchronize()
    return Rx[:Xx.shape[0]], cm, _handed(fbs)


def _densify_launch(ctx, Xp, Xi, Xx, g, cols, ties, signed, power, colmax):
    """dev_colranks_csc_dense over column ranges"""
    import torch
    n = Xp.shape[0] - 1
    R = _empty((n, g))
    cm = _empty((n,)) if colmax else None
    torch.cuda.synchronize()
    fbs = []
    for c0, nc in cols:
        ctx.dev_colranks_csc_dense(Xp.data_ptr() + c0 * 4, Xi.data_ptr(), Xx.data_ptr(), g, nc, R.data_ptr() + c0 * g * 8, g,
                                   ties, signed, power, cm.data_ptr() + c0 * 8 if colmax else None)
        fbs.append(ctx.debug_rank_fallbacks())
    ctx.synchronize()
    return R, cm, _handed(fbs)


def _check_dense(ctx, X, grid, combos, power=1.25):
    """(a) and (b) for a dense deck; returns the hand-over counts of the last whole power-1 launch"""
    g, n = X.shape
    Xd = _dev(X.T)
    fb = None
    for ties, signed in combos:
        R, _, fb = _dense_launch(ctx, Xd, g, [(0, n)], ties, signed, 1.0, False)
        got = R.cpu().numpy().T
        ref = rd.ranks_ref(X, ties, signed)
        bad = np.flatnonzero(~np.all((got == ref) | (np.isnan(got) & np.isnan(ref)), axis=0))
        assert bad.size == 0, (ties, signed, "first wrong columns", bad[:8], "trip", bad[:8] // grid)
        R1, c1, f1 = _dense_launch(ctx, Xd, g, [(0, n)], ties, signed, power, True)
        R2, c2, f2 = _dense_launch(ctx, Xd, g, _chunks(n, grid), ties, signed, power, True)
        assert _same_bits(R1, R2) and _same_bits(c1, c2), (ties, signed, power)
        assert fb == f1 == f2, (ties, signed, "handed over: whole launch, with power, chunk by chunk", fb, f1, f2)
    print(f"columns handed over (bucket ranker, partitioned ranker): {fb}")
    return fb


# ------------------------------------------------------------------------- dense columns: the persistent bucket ranker
_DECKS = {}


def _dense_deck(g, grid, trips=TRIPS):
    """one deck per (g, grid), shared by the cases that use it (never written to)"""
    key = (g, grid, trips)
    if key not in _DECKS:
        _DECKS.clear()                                           # (one deck at a time: they are up to 170 MB)
        kinds = rd.deck(rd.KINDS, grid, trips, TAIL)
        _DECKS[key] = (kinds, rd.dense_deck(kinds, g, g))
    return _DECKS[key]


@pytest.mark.parametrize("signed", [False, True])
def test_persistent_bucket_12288_every_ties_rule(pinned_ctx, signed):
    """`auto`, g = 12,288: colranks_bucket_kernel<512,24>, persistent with prefetch.  launch_bucket: its 97 KB of LDS put
    one workgroup on a CU, so grid = min(n, CU); 3 CU + 37 columns.  All three ties rules, signed and unsigned."""
    grid = _cu()
    kinds, X = _dense_deck(12288, grid)
    assert len(kinds) == TRIPS * grid + TAIL and rd.pairs_seen(kinds, grid) == rd.all_pairs(rd.KINDS)
    fb = _check_dense(pinned_ctx(rank_kernel="auto"), X, grid, [(tm, signed) for tm in ("average", "min", "max")])
    assert fb[0] >= kinds.count("forced")                        # the forced columns did go to the sorting network


@pytest.mark.parametrize("option,g", [("auto", 12289), ("auto", 20352), ("bucket512", 20352)])
def test_persistent_bucket_long_columns(pinned_ctx, option, g):
    """`auto`, g = 12,289 and 20,352: colranks_bucket_kernel<1024,20>; `bucket512`, g = 20,352: <512,40>.  launch_bucket: one
    workgroup per CU (LDS), grid = min(n, CU); 3 CU + 37 columns"""
    grid = _cu()
    kinds, X = _dense_deck(g, grid)
    assert len(kinds) == TRIPS * grid + TAIL and rd.pairs_seen(kinds, grid) == rd.all_pairs(rd.KINDS)
    fb = _check_dense(pinned_ctx(rank_kernel=option), X, grid, [("average", False), ("min", True)])
    assert fb[0] >= kinds.count("forced")


# ------------------------------------------------------------------------------------- CSC stored values (sparse_colranks)
def test_persistent_bucket_csc_lengths(pinned_ctx):
    """dev_colranks_csc, `auto`, max_col_nnz = 20,352: colranks_bucket_kernel<1024,20> on CSC columns, grid = min(n, CU)
    (launch_ranks / launch_bucket); 3 CU + 37 columns whose stored-value counts -- 0, 1, 2, 63, 64, 65, 257, 8,192, 8,193,
    12,289, 20,352 -- follow each other in every order: an empty column as the prefetched successor (cnt_n == 0: not taken
    over), a short column after a long one"""
    grid, mx = _cu(), 20352
    lens = rd.csc_lengths(mx, grid, TRIPS, TAIL)
    kinds = rd.deck(rd.KINDS, grid, TRIPS, TAIL)
    assert rd.pairs_seen(lens, grid) == rd.all_pairs(list(rd.CSC_LENGTHS) + [mx])
    assert rd.pairs_seen(kinds, grid) == rd.all_pairs(rd.KINDS)
    Xp, Xx = rd.csc_values(lens, kinds, 11)
    dXp, dXx = _dev(Xp), _dev(Xx)
    ctx = pinned_ctx(rank_kernel="auto")
    n = len(lens)
    for ties, signed in (("average", False), ("min", True)):
        Rx, _, fb = _csc_launch(ctx, dXp, dXx, mx, [(0, n)], ties, signed, 1.0, False)
        got, ref = Rx.cpu().numpy(), rd.csc_ranks_ref(Xp, Xx, ties, signed)
        col = np.repeat(np.arange(n), np.diff(Xp))
        bad = np.unique(col[~((got == ref) | (np.isnan(got) & np.isnan(ref)))])
        assert bad.size == 0, (ties, signed, "first wrong columns", bad[:8], "lengths", [lens[c] for c in bad[:8]])
        R1, c1, f1 = _csc_launch(ctx, dXp, dXx, mx, [(0, n)], ties, signed, 1.25, True)
        R2, c2, f2 = _csc_launch(ctx, dXp, dXx, mx, _chunks(n, grid), ties, signed, 1.25, True)
        assert _same_bits(R1, R2) and _same_bits(c1, c2), (ties, signed)
        assert fb == f1 == f2, (ties, signed, "handed over: whole launch, with power, chunk by chunk", fb, f1, f2)


# ------------------------------------------------------------------------------ densify-and-rank (dev_colranks_csc_dense)
@pytest.mark.parametrize("option,g,per_cu", [("auto", 200, 2), ("auto", 300, 2), ("auto", 12289, 1), ("network", 12289, 2)])
def test_densify_route_reuses_its_scratch_column(pinned_ctx, option, g, per_cu):
    """dev_colranks_csc_dense: one scratch column per workgroup, zeroed and filled per column.  launch_ranks caps the grid at
    2 CU for this route (grid_cap).  `auto` g = 200: colranks_f64_kernel<false> (LDS network, launch_network); `auto`
    g = 300: colranks_bucket_kernel<256,8> on 2 CU workgroups; `auto` g = 12,289: <1024,20>, which launch_bucket cuts to one
    workgroup per CU; `network` g = 12,289: colranks_regs_kernel on 2 CU.  3 grid + 37 columns: empty, one entry, full and
    5 % columns (stored zeros, negatives) in every order -- a full column's values must not show through an empty one"""
    grid = per_cu * _cu()
    pats = rd.deck(rd.DENSIFY_PATTERNS, grid, TRIPS, TAIL)
    kinds = rd.deck(rd.KINDS, grid, TRIPS, TAIL)
    assert rd.pairs_seen(pats, grid) == rd.all_pairs(rd.DENSIFY_PATTERNS)
    assert rd.pairs_seen(kinds, grid) == rd.all_pairs(rd.KINDS)
    Xp, Xi, Xx = rd.densify_deck(pats, kinds, g, g)
    X = rd.csc_toarray(Xp, Xi, Xx, g)
    dXp, dXi, dXx = _dev(Xp), _dev(Xi), _dev(Xx)
    ctx = pinned_ctx(rank_kernel=option)
    n = len(pats)
    for ties, signed in (("average", False), ("min", True)):
        R, _, fb = _densify_launch(ctx, dXp, dXi, dXx, g, [(0, n)], ties, signed, 1.0, False)
        got, ref = R.cpu().numpy().T, rd.ranks_ref(X, ties, signed)
        bad = np.flatnonzero(~np.all((got == ref) | (np.isnan(got) & np.isnan(ref)), axis=0))
        assert bad.size == 0, (ties, signed, "first wrong columns", bad[:8], [pats[c] for c in bad[:8]])
        R1, c1, f1 = _densify_launch(ctx, dXp, dXi, dXx, g, [(0, n)], ties, signed, 1.25, True)
        R2, c2, f2 = _densify_launch(ctx, dXp, dXi, dXx, g, _chunks(n, grid), ties, signed, 1.25, True)
        assert _same_bits(R1, R2) and _same_bits(c1, c2), (ties, signed)
        assert fb == f1 == f2, (ties, signed, "handed over: whole launch, with power, chunk by chunk", fb, f1, f2)


# --------------------------------------------------------------------------- columns beyond the LDS: network, partitioned
def test_network_on_global_keys(pinned_ctx):
    """`network`, g = 20,481 (more than the 20,448 keys the LDS holds): colranks_f64_kernel<true>, one global key slice per
    workgroup; launch_network: grid = min(n, 2 CU); 2 grid + 37 columns"""
    grid = 2 * _cu()
    kinds, X = _dense_deck(20481, grid, 2)
    assert len(kinds) == 2 * grid + TAIL and rd.pairs_seen(kinds, grid) == rd.all_pairs(rd.KINDS)
    _check_dense(pinned_ctx(rank_kernel="network"), X, grid, [("average", False), ("min", True)])


def test_partitioned_ranker(pinned_ctx):
    """`auto`, g = 20,353: launch_colranks_partitioned; rank_part_count / scatter / finish run on min(n, 2 CU) workgroups with
    their counters in LDS (and the segments go through the persistent bucket ranker); 2 grid + 37 columns"""
    grid = 2 * _cu()
    kinds, X = _dense_deck(20353, grid, 2)
    assert len(kinds) == 2 * grid + TAIL and rd.pairs_seen(kinds, grid) == rd.all_pairs(rd.KINDS)
    fb = _check_dense(pinned_ctx(rank_kernel="auto"), X, grid, [("average", False), ("min", True)])
    assert fb[1] == 0                                            # no kind here leaves an open interval above 20,352 keys


# ----------------------------------------------------------------------------------- hand-over to the sorting networks
def test_handover_lds_network_by_list(pinned_ctx):
    """`auto`, g = 300, every second column forced: colranks_bucket_kernel<256,8> (one column per workgroup) hands 3 CU + 18
    columns to colranks_f64_kernel<false>, which walks the device-side list on min(n, CU) workgroups (fb_grid in
    launch_ranks): three trips and more.  The list is in order of arrival, so which columns share a workgroup is not
    fixed; the deck property is asserted for both halves at grid CU, and the count from the device says the list was as
    long as intended.  6 CU + 37 columns"""
    grid = _cu()
    g, n = 300, 6 * grid + 37
    forced = rd.deck(("forced", "forced_nan"), grid, TRIPS, n // 2 - TRIPS * grid)            # the odd columns
    plain = rd.deck(ORDINARY, grid, TRIPS, n - n // 2 - TRIPS * grid)                         # the even columns
    assert rd.pairs_seen(forced, grid) == rd.all_pairs(("forced", "forced_nan"))
    assert rd.pairs_seen(plain, grid) == rd.all_pairs(ORDINARY)
    kinds = [None] * n
    kinds[1::2], kinds[0::2] = forced, plain
    X = rd.dense_deck(kinds, g, 300)
    n_forced = len(forced)
    assert n_forced == 3 * grid + 18 > grid
    fb = _check_dense(pinned_ctx(rank_kernel="auto"), X, grid, [("average", False), ("min", True)])
    # (near_one, two histogram levels cannot separate it either, is only handed over in long columns: not at g = 300)
    assert fb[0] == n_forced, fb


def test_handover_regs_network_by_list(pinned_ctx):
    """dev_colranks_csc, `auto`, max_col_nnz = 12,289, CSC columns of 259, 300, 8,193 and 12,289 stored values, ALL forced:
    colranks_bucket_kernel<1024,20> (grid CU, every column leaves its loop early) hands all 2 CU + 37 columns to
    colranks_regs_kernel, which keeps ONE network size (L = 14) for columns of every length and walks the list on
    min(n, CU) workgroups (fb_grid in launch_ranks).  The list is in order of arrival: the deck property asserted below
    holds for the bucket kernel's loop only; which lengths follow each other in the regs kernel is not fixed -- with four
    lengths in equal shares over more than two trips per workgroup, short after long is all but certain, not asserted"""
    grid, mx = _cu(), 12289
    lengths = (259, 300, 8193, 12289)
    lens = rd.deck(lengths, grid, 2, TAIL)
    assert rd.pairs_seen(lens, grid) == rd.all_pairs(lengths)
    n = len(lens)
    kinds = ["forced" if (k < 300 or c % 3 == 0) else "forced_nan" for c, k in enumerate(lens)]
    Xp, Xx = rd.csc_values(lens, kinds, 12)
    dXp, dXx = _dev(Xp), _dev(Xx)
    ctx = pinned_ctx(rank_kernel="auto")
    for ties, signed in (("average", False), ("min", True)):
        Rx, _, fb = _csc_launch(ctx, dXp, dXx, mx, [(0, n)], ties, signed, 1.0, False)
        print(f"columns handed over (bucket ranker, partitioned ranker): {fb}")
        assert fb[0] == n == 2 * grid + 37 > grid, fb
        got, ref = Rx.cpu().numpy(), rd.csc_ranks_ref(Xp, Xx, ties, signed)
        col = np.repeat(np.arange(n), np.diff(Xp))
        bad = np.unique(col[~((got == ref) | (np.isnan(got) & np.isnan(ref)))])
        assert bad.size == 0, (ties, signed, "first wrong columns", bad[:8], "lengths", [lens[c] for c in bad[:8]])
        R1, c1, f1 = _csc_launch(ctx, dXp, dXx, mx, [(0, n)], ties, signed, 1.25, True)
        R2, c2, f2 = _csc_launch(ctx, dXp, dXx, mx, _chunks(n, grid), ties, signed, 1.25, True)
        assert _same_bits(R1, R2) and _same_bits(c1, c2), (ties, signed)
        assert fb == f1 == f2, (ties, signed, "handed over: whole launch, with power, chunk by chunk", fb, f1, f2)


def _adversarial(g, rng):
    """the `adversarial` kind of tests/test_gpu_sparse_ranks.py: the 1,024 rows rank_part_count_kernel samples hold the small
    values, so every splitter lies below the bulk, whose open interval is too long for the bucket ranker"""
    x = 100.0 + rng.random(g)
    x[(np.arange(1024, dtype=np.int64) * g) >> 10] = rng.random(1024)
    return x


def test_handover_from_the_partitioned_ranker(pinned_ctx):
    """`auto`, g = 22,000: one splitter (the sample median, below 1), so the open interval above it holds about 21,488 keys
    > 20,352 and rank_part_count_kernel hands the column to the sorting network.  At g > 20,448 launch_network takes its
    global-key branch, colranks_f64_kernel<true>, whose grid is its own: min(n, 2 CU) workgroups walk the list, whatever
    fb_grid launch_colranks_partitioned passes.  2 CU + 37 adversarial columns (every third with NaN) with ordinary ones
    between: 2 (2 CU + 37) columns, so that the list is longer than the 2 CU workgroups that walk it, and the partition
    kernels (2 CU workgroups too) skip handed-over columns (`continue`) between ordinary ones.  The single-trip launches of
    (b) take 2 CU columns each, CU of them handed over.  g = 22,000 is the first size tried: the count matches there"""
    grid = 2 * _cu()
    g, n_forced = 22000, grid + 37
    n = 2 * n_forced
    rng = np.random.default_rng(22)
    plain = (list(ORDINARY) * (n_forced // len(ORDINARY) + 1))[:n_forced]
    X = np.empty((g, n), order="F")
    for c in range(n):
        X[:, c] = _adversarial(g, rng) if c % 2 == 1 else rd.column(plain[c // 2], g, rng)
    X[5::1000, 3::6] = np.nan                                    # (22 NaN in a handed-over column: its interval stays too long)
    fb = _check_dense(pinned_ctx(rank_kernel="auto"), X, grid, [("average", False), ("min", True)])
    assert fb[1] == n_forced > grid, fb


# --------------------------------------------------------------------------------------------- colmax_zero_group_kernel
def test_colmax_zero_group_past_one_trip(pinned_ctx):
    """`auto`, g = 300, signed, power 1.3 (no quarter exponent: the bucket ranker's pow() loop leaves the maximum of a column
    of zeros at its start value and colmax_zero_group_kernel repairs it).  launch_ranks gives it min((n + 3) / 4, 8 CU)
    blocks of four wavefronts, one column each: a wavefront's columns are 32 CU apart.  2 x 32 CU + 37 columns; all-zero and
    zero-plus-NaN columns among the ordinary kinds"""
    stride = 32 * _cu()
    kinds_all = rd.KINDS + ("all_zero", "zero_nan")
    kinds = rd.deck(kinds_all, stride, 2, TAIL)
    assert len(kinds) == 2 * stride + TAIL and rd.pairs_seen(kinds, stride) == rd.all_pairs(kinds_all)
    g = 300
    X = rd.dense_deck(kinds, g, 13)
    n = X.shape[1]
    Xd = _dev(X.T)
    ctx = pinned_ctx(rank_kernel="auto")
    for ties, signed in (("average", False), ("min", True)):
        R, _, _ = _dense_launch(ctx, Xd, g, [(0, n)], ties, signed, 1.0, False)
        got, ref = R.cpu().numpy().T, rd.ranks_ref(X, ties, signed)
        assert np.array_equal(got, ref, equal_nan=True), (ties, signed)
    for ties in ("average", "min"):
        R1, c1, f1 = _dense_launch(ctx, Xd, g, [(0, n)], ties, True, 1.3, True)
        R2, c2, f2 = _dense_launch(ctx, Xd, g, _chunks(n, stride), ties, True, 1.3, True)
        assert _same_bits(R1, R2) and _same_bits(c1, c2) and f1 == f2, (ties, f1, f2)
        # the repaired maxima themselves: the common weight of z tied zeros, and -inf where nothing has a rank (the device's
        # pow() is within 3 ulp of the exact power -- rank_bucket.h -- and numpy's within 1: 4 ulp)
        cm = c1.cpu().numpy()
        for kind in ("all_zero", "zero_nan", "all_nan"):
            for c in [i for i, k in enumerate(kinds) if k == kind][:: max(1, kinds.count(kind) // 16)]:
                z = int((X[:, c] == 0.0).sum())
                want = -np.inf if z == 0 else (1.0 if ties == "min" else 0.5 * (z + 1)) ** 1.3
                assert cm[c] == want or abs(cm[c] - want) <= 4 * np.spacing(want), (kind, c, cm[c], want)


# ------------------------------------------------------------------- the densify entry behind the torch.distributed form
def _long_column_shard(rng, g, n):
    """a CSC matrix with one column of 20,353 stored values (one more than the stored-values route takes) among sparse ones"""
    import scipy.sparse as sp
    X = np.round(rng.gamma(2.0, 1.5, size=(g, n)), 1)
    X[rng.random(X.shape) < 0.9] = 0.0
    X[:, 2] = np.round(rng.gamma(2.0, 1.5, size=g), 1) + 0.1
    X[rng.choice(g, size=g - 20353, replace=False), 2] = 0.0
    Xs = sp.csc_matrix(X)
    assert np.diff(Xs.indptr).max() == 20353
    return X, Xs


def test_hip_phase_engine_colranks_csc_dense_long_column():
    """HipPhaseEngine.colranks_csc_dense on a shard of g = 20,400 with a column of 20,353 stored values: the shard leaves the
    stored-values route (20,352 at most) for Context.dev_colranks_csc_dense; equal to the oracle on toarray()"""
    import torch
    import plaid_amd
    from plaid_amd import sharded, synth as sy
    g, n = 20400, 9
    X, Xs = _long_column_shard(np.random.default_rng(4), g, n)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    ctx = plaid_amd.Context(0, stream.cuda_stream)
    Gp, Gi = sy.geneset_csc(g, 20, kmin=5, kmax=50)
    gs = ctx.geneset(g, Gp, Gi)
    try:
        eng = sharded.HipPhaseEngine(ctx, gs, dev)
        shard = sharded.CscShard.from_scipy(Xs, 0, n, device=dev)
        assert shard.max_col_nnz == 20353 > ctx.limit("sparse_rank_column")
        for ties, signed in (("average", False), ("min", True)):
            with torch.cuda.stream(stream):
                R = eng.colranks_csc_dense(shard, ties, signed)
                Rp = eng.colranks_csc_dense(shard, ties, signed, rows=(1, 4))
            torch.cuda.synchronize()
            ref = rd.ranks_ref(X, ties, signed)
            assert np.array_equal(R.cpu().numpy()[:, :g].T, ref), (ties, signed)
            assert np.array_equal(Rp.cpu().numpy()[:, :g].T, ref[:, 1:4]), (ties, signed)
    finally:
        gs.close()
        ctx.close()


def test_sharded_sing_csc_long_column():
    """sharded_sing_csc on that shard (panels of four cells, the long column in the first): equal to ctx.sing_csc bit for
    bit and to the oracle within the score tolerance; modelled on test_sharded_sing_csc_hip_phase_engine"""
    import scipy.sparse as sp
    import torch
    import plaid_amd
    from plaid_amd import sharded, synth as sy
    from oracle import plaid_oracle as po
    g, n, m = 20400, 9, 60
    X, Xs = _long_column_shard(np.random.default_rng(4), g, n)
    Gp, Gi = sy.geneset_csc(g, m, kmin=5, kmax=300)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    ctx = plaid_amd.Context(0, stream.cuda_stream)
    gs = ctx.geneset(g, Gp, Gi)
    try:
        eng = sharded.HipPhaseEngine(ctx, gs, dev)
        shard = sharded.CscShard.from_scipy(Xs, 0, n, device=dev)
        with torch.cuda.stream(stream):
            S = sharded.sharded_sing_csc(eng, shard, panel_bytes=4 * (g + 1) * 8)
        torch.cuda.synchronize()
        G = sp.csc_matrix((np.ones(len(Gi)), Gi, Gp), shape=(g, m))
        rn = [str(k) for k in range(g)]
        np.testing.assert_allclose(S.cpu().numpy().T, po.replaid_sing(X, rn, G, rn), rtol=1e-5, atol=1e-9)
        assert np.array_equal(S.cpu().numpy().T, ctx.sing_csc(Xs.indptr, Xs.indices, Xs.data, g, Gp, Gi))
    finally:
        gs.close()
        ctx.close()
