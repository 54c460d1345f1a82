"""tests/helpers/rank_decks.py against itself and scipy (host only): the decks that tests/test_gpu_rank_sequences.py deals to
the rank kernels show every ordered pair of column kinds inside some workgroup, the forced hand-over column does what
rank_bucket.h says it must, and ranks_ref is rank() per column."""
import numpy as np
import pytest

from tests.helpers import rank_decks as rd


def test_pair_cycle_holds_every_ordered_pair_once():
    for k in (1, 2, 3, 4, 11, 14):
        cyc = rd.pair_cycle(k)
        assert len(cyc) == k * k
        pairs = {(cyc[i], cyc[(i + 1) % (k * k)]) for i in range(k * k)}
        assert pairs == {(a, b) for a in range(k) for b in range(k)}


@pytest.mark.parametrize("grid", [1, 7, 256, 304, 512])
def test_deck_covers_all_pairs(grid):
    """trips = 3 for every grid; the tail of the GPU tests (37) where 2 grid + 37 successions hold the 196 pairs of the 14
    kinds, and the shortest tail that does on the small grids"""
    k2 = len(rd.KINDS) ** 2
    tail = max(37, k2 - 2 * grid)
    kinds = rd.deck(rd.KINDS, grid, 3, tail)
    assert len(kinds) == 3 * grid + tail
    assert rd.pairs_seen(kinds, grid) == rd.all_pairs(rd.KINDS)
    # the columns of one workgroup follow consecutive entries of the cycle
    cyc = [rd.KINDS[i] for i in rd.pair_cycle(len(rd.KINDS))]
    for w in (0, grid // 2, grid - 1):
        mine = kinds[w::grid]
        starts = [s for s in range(k2) if all(cyc[(s + t) % k2] == mine[t] for t in range(len(mine)))]
        assert starts, w
    # one column short of the pairs: refused, not dealt incompletely
    with pytest.raises(ValueError):
        rd.deck(rd.KINDS, grid, 0, grid + k2 - 1)
    # the CSC lengths and the densify patterns are dealt by the same rule
    lens = rd.csc_lengths(20352, grid, 3, tail)
    want = [v for v in rd.CSC_LENGTHS] + [20352]
    assert rd.pairs_seen(lens, grid) == rd.all_pairs(want)
    pats = rd.deck(rd.DENSIFY_PATTERNS, grid, 3, tail)
    assert rd.pairs_seen(pats, grid) == rd.all_pairs(rd.DENSIFY_PATTERNS)


def test_pairs_seen_notices_a_missing_pair():
    kinds = rd.deck(rd.KINDS, 7, 3, 182)
    kinds[7 * 5 + 3] = "constant" if kinds[7 * 5 + 3] != "constant" else "rounded"    # breaks two pairs that occur once each
    assert rd.pairs_seen(kinds, 7) != rd.all_pairs(rd.KINDS)


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("g", [259, 300, 8193, 12289, 20352, 22000])
def test_forced_column_shares_one_fine_bucket(g, signed):
    """the key map and PH_D32 of rank_bucket.h restated: the clustered keys of the forced column share (key - lo) >> 32
    -- the value every fine bucket index is computed from -- are more than kFallbackCount = 256, and are not all equal"""
    for kind in ("forced", "forced_nan") if g >= 300 else ("forced",):     # (NaN take keys away: not at the shortest length)
        x = rd.column(kind, g, np.random.default_rng(g))
        x = x[~np.isnan(x)]
        key = rd.key_of(x, signed)
        lo, hi = key.min(), key.max()
        rbits = int(hi - lo).bit_length()
        assert rbits > 32                                   # d_shr = rbits - 32, d_shl = 0
        d32 = (key - lo) >> np.uint64(rbits - 32)
        cluster = np.abs(x) < 2.0
        assert cluster.sum() == len(x) - 2 > 256
        assert len(np.unique(d32[cluster])) == 1
        assert len(np.unique((key - lo)[cluster] >> np.uint64(32))) == 1
        assert len(np.unique(key[cluster])) == 4
        # the key map keeps the order of the doubles
        o = np.argsort(np.abs(x) if signed else x, kind="stable")
        assert np.all(np.diff(key[o].astype(object)) >= 0)


def test_ranks_ref_is_rankdata_per_column():
    from scipy.stats import rankdata
    g, grid = 301, 1
    kinds = rd.deck(rd.KINDS, grid, 3, len(rd.KINDS) ** 2 - 2)
    X = rd.dense_deck(kinds, g, 5)
    assert {k for k, c in zip(kinds, range(X.shape[1])) if np.isnan(X[:, c]).any()} >= {"nan1", "all_nan", "one_valid"}
    for ties in ("average", "min", "max"):
        for signed in (False, True):
            R = rd.ranks_ref(X, ties, signed)
            assert np.array_equal(np.isnan(R), np.isnan(X))
            for c in range(X.shape[1]):
                ok = ~np.isnan(X[:, c])
                v = X[ok, c]
                want = rankdata(np.abs(v) if signed else v, method=ties)
                if signed:
                    want = np.sign(v) * want
                assert np.array_equal(R[ok, c], want), (kinds[c], ties, signed)


def test_csc_ranks_ref_is_rankdata_per_column():
    from scipy.stats import rankdata
    grid = 3
    lens = rd.csc_lengths(300, grid, 3, 70)                 # the lengths below 300 and 300 itself
    assert set(lens) == {0, 1, 2, 63, 64, 65, 257, 300}
    kinds = rd.deck(rd.KINDS, grid, 3, len(rd.KINDS) ** 2)[:len(lens)]
    Xp, Xx = rd.csc_values(lens, kinds, 6)
    assert np.isnan(Xx).any()
    for ties, signed in (("average", False), ("min", True), ("max", False)):
        R = rd.csc_ranks_ref(Xp, Xx, ties, signed)
        assert np.array_equal(np.isnan(R), np.isnan(Xx))
        for c in range(len(lens)):
            v = Xx[Xp[c]:Xp[c + 1]]
            ok = ~np.isnan(v)
            want = rankdata(np.abs(v[ok]) if signed else v[ok], method=ties)
            if signed:
                want = np.sign(v[ok]) * want
            assert np.array_equal(R[Xp[c]:Xp[c + 1]][ok], want), (c, ties, signed)


def test_densify_deck_patterns_and_toarray():
    import scipy.sparse as sp
    g, grid = 300, 2
    pats = rd.deck(rd.DENSIFY_PATTERNS, grid, 3, 12)
    kinds = (list(rd.KINDS) * 2)[:len(pats)]
    Xp, Xi, Xx = rd.densify_deck(pats, kinds, g, 7)
    nnz = np.diff(Xp)
    for c, pat in enumerate(pats):
        assert {"empty": nnz[c] == 0, "one": nnz[c] == 1, "full": nnz[c] == g, "sparse5": 0 < nnz[c] < g // 4}[pat], (c, pat)
        assert len(np.unique(Xi[Xp[c]:Xp[c + 1]])) == nnz[c]
        if pat == "sparse5":
            v = Xx[Xp[c]:Xp[c + 1]]
            assert (v == 0.0).any() and (v < 0.0).any()
    X = rd.csc_toarray(Xp, Xi, Xx, g)
    ref = sp.csc_matrix((Xx, Xi, Xp), shape=(g, len(pats))).toarray()
    assert np.array_equal(X, ref, equal_nan=True)
