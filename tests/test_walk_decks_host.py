"""tests/helpers/walk_decks.py on the host: the decks of tests/test_gpu_walk_tasks.py meet their conditions for 64, 256 and
304 CUs before a device is asked -- every ordered pair of kinds inside a workgroup (wavefront) at each stride, the partial
permutation block and the short list tile after full ones, the planted B = 0 pairs NaN, every ordinary kind finite, the
planted genes where the docstrings say they stand.  No GPU."""
import numpy as np
import pytest

from tests.helpers import gsea_edge_ref as er
from tests.helpers import gsea_perm_ref as ref
from tests.helpers import rank_decks as rd
from tests.helpers import walk_decks as wd

CUS = [64, 256, 304]


@pytest.mark.parametrize("cu", CUS)
@pytest.mark.parametrize("stride_of,kinds", [(wd.ks_stride, wd.KS_KINDS), (wd.pair_stride, wd.GSEA_KINDS),
                                             (wd.null_stride, wd.GSEA_KINDS)])
def test_every_kind_follows_every_kind_at_the_stride(cu, stride_of, kinds):
    stride = stride_of(cu)
    names, idx = wd.deal(kinds, stride)
    assert len(names) == stride + len(kinds) ** 2 + 7 and rd.pairs_seen(names, stride) == rd.all_pairs(kinds)
    assert [kinds[i] for i in idx] == names
    Gp, Gi = wd.deck_pattern(kinds, idx)
    ml = wd.member_lists(kinds)
    for j in (0, 1, stride - 1, stride, len(names) - 1):
        assert np.array_equal(Gi[Gp[j]:Gp[j + 1]], ml[names[j]])


def test_a_deck_too_short_for_its_pairs_raises():
    with pytest.raises(ValueError):
        rd.deck(wd.KS_KINDS, 64, 1, len(wd.KS_KINDS) ** 2 - 1)


@pytest.mark.parametrize("cu", CUS)
def test_pairs_of_two_lists_cross_from_the_nan_list_and_into_it(cu):
    """gsea_obs_kernel / gsea_edge_kernel with two lists, one NaN: pair e = l m + j is followed by e + stride, so the ordinary
    list shows every ordered pair of kinds, and a wavefront goes from the NaN list to the ordinary one (NaN first) or into
    it (NaN last)"""
    stride = wd.pair_stride(cu)
    names, _ = wd.deal(wd.GSEA_KINDS, stride)
    for listnan in ((True, False), (False, True)):
        pk = wd.pair_kinds(names, listnan)
        seen = rd.pairs_seen(pk, stride)
        assert {(a, b) for (a, na), (b, nb) in seen if not na and not nb} == rd.all_pairs(wd.GSEA_KINDS)
        crossing = (True, False) if listnan[0] else (False, True)
        assert any((na, nb) == crossing for (a, na), (b, nb) in seen)


@pytest.mark.parametrize("cu", CUS)
def test_the_partial_block_and_the_short_tile_follow_full_ones(cu):
    """B = 130 placements and c = 9 lists: three blocks, the last of 2; two list tiles, the last of 1 list"""
    names, _ = wd.deal(wd.GSEA_KINDS, wd.null_stride(cu))
    blk, tile, j, nb, nl = wd.null_tasks(len(names), 9, 130)
    assert len(j) == 3 * 2 * len(names) and sorted(set(nb.tolist())) == [2, 64] and sorted(set(nl.tolist())) == [1, 8]
    t = 2 * len(names) * 2 + len(names) + 5                  # block 2, tile 1, set 5
    assert (blk[t], tile[t], j[t]) == (2, 1, 5)
    got = wd.null_successions(names, 9, 130, wd.null_stride(cu))
    assert got["block"] > 0 and got["tile"] > 0 and got["from_nan"] > 0, got
    one = wd.null_tasks(len(names), 8, 64)                   # B = 64, c = 8: task = set
    assert np.array_equal(one[2], np.arange(len(names))) and set(one[3].tolist()) == {64} and set(one[4].tolist()) == {8}
    assert set(wd.null_tasks(len(names), 9, 130, weighted=False)[1].tolist()) == {0}     # unweighted: one walk serves all lists


def test_the_planted_genes_stand_where_the_kinds_need_them():
    X = wd.columns()
    assert sorted(np.flatnonzero(np.isnan(X).any(axis=0)).tolist()) == list(wd.NAN_COLS) and np.isnan(X).sum() == 2
    ok = ~np.isnan(X)
    assert np.array_equal(X[ok], np.round(X[ok])) and len(np.unique(X[:, 1])) < wd.N      # integers, with ties
    gg, ml = wd.gene_groups(), wd.member_lists(wd.KS_KINDS + ("zero_w",))
    assert set(ml["high"]) <= set(gg["high"]) and set(ml["low"]) <= set(gg["low"])
    for entry, first, second in (("ks", "high", "low"), ("mad", "low", "high")):
        assert (wd.bits_of(X, ml[first], entry) < 64).all()                               # the first word of the first scan step
        assert (wd.bits_of(X, ml[second], entry) >= wd.STEP).all()                        # the second scan step only
        b = wd.bits_of(X, ml["both"], entry)
        assert (b < wd.STEP).any(axis=0).all() and (b >= wd.STEP).any(axis=0).all()
        assert (wd.bits_of(X, ml["centre"], entry) == (wd.N // 2 if entry == "ks" else wd.N // 2 - 1)).all()
    assert [len(ml[k]) for k in ("empty", "full", "one", "k64", "k65", "centre")] == [0, wd.N, 1, 64, 65, 1]
    assert all(len(np.unique(r)) == len(r) for r in ml.values())
    w = wd.gsea_weights(8, True)
    assert (w[ml["zero_w"]] == 0).all() and (w[ml["one"]] > 0).all() and w.max() < 2**20 and np.array_equal(w, np.round(w))
    assert (wd.gsea_weights(8, False) == 1).all()


def _finite_but(rows, kinds, nan_kinds, nan_cols, what):
    for i, k in enumerate(kinds):
        for c in range(rows.shape[1]):
            want_nan = k in nan_kinds or c in nan_cols
            assert np.isnan(rows[i, c]) == want_nan, (what, k, c, rows[i, c])
    assert wd.nan_only_where(rows, kinds, nan_kinds, nan_cols), what
    spoiled = np.array(rows)
    ordinary = min(c for c in range(rows.shape[1]) if c not in nan_cols)
    spoiled[kinds.index("k64"), ordinary] = np.nan
    assert not wd.nan_only_where(spoiled, kinds, nan_kinds, nan_cols)


def test_the_ks_and_mad_references_are_nan_only_where_planted():
    for alpha in (0.0, 1.0):
        _finite_but(wd.ssgsea_ks_ref(alpha), wd.KS_KINDS, ("empty", "full"), wd.NAN_COLS, f"ssgsea alpha {alpha}")
    for max_diff in (True, False):
        _finite_but(wd.gsva_ks_ref(0.0, max_diff), wd.KS_KINDS, ("empty", "full"), wd.NAN_COLS, "gsva tau 0")
        # tau = 1: the centre gene alone weighs 0, B = 0 and the score is NaN in every column
        _finite_but(wd.gsva_ks_ref(1.0, max_diff), wd.KS_KINDS, ("empty", "full", "centre"), wd.NAN_COLS, "gsva tau 1")
    s = wd.sing_ref()
    assert sorted(s) == ["UpDispersion", "UpScore"]
    _finite_but(s["UpScore"], wd.KS_KINDS, ("empty", "full"), wd.NAN_COLS, "sing score")
    _finite_but(s["UpDispersion"], wd.KS_KINDS, ("empty",), wd.NAN_COLS, "sing dispersion")    # k = N: an ordinary pair


@pytest.mark.parametrize("ncol,nan_lists,weighted,B", [(2, (0,), False, 2), (2, (1,), True, 2), (8, (0, 3), True, 64),
                                                      (8, (3, 7), True, 64), (8, (0, 3), False, 64), (9, (3,), True, 130)])
def test_the_gsea_references_are_nan_only_where_planted(ncol, nan_lists, weighted, B):
    stat, w, P, Gp, Gi, want = wd.gsea_case(ncol, nan_lists, weighted, B)
    assert P.shape == (wd.N, B) and all(sorted(P[:, b].tolist()) == list(range(wd.N)) for b in (0, B - 1))
    for st in (er.STD, er.POS, er.NEG):
        out, null, le_len, le_idx = want[st]
        _finite_but(out[:, 0, :], wd.GSEA_KINDS, wd.NAN_KINDS, nan_lists, "ES")
        for b in (0, B - 1):
            _finite_but(null[:, b, :], wd.GSEA_KINDS, wd.NAN_KINDS, nan_lists, "null")
        assert (le_len[[wd.GSEA_KINDS.index(k) for k in wd.NAN_KINDS], :] == 0).all() and (le_len[:, list(nan_lists)] == 0).all()
    if not weighted:
        return
    # B = 0: the zero-weight kind under the observed placement of every list scores as the unweighted walk; the one-gene kind
    # meets a zero weight under some null placements and a positive one under others
    ones = er.gsea_scored_ref(stat, np.ones_like(w), Gp, Gi, P)[er.STD]
    z, o = wd.GSEA_KINDS.index("zero_w"), wd.GSEA_KINDS.index("one")
    mem = Gi[Gp[o]:Gp[o + 1]]
    for l in range(ncol):
        if l in nan_lists:
            continue
        assert want[er.STD][0][z, 0, l] == ones[0][z, 0, l]
        Wpos = ref.walk_weights(ref.observed_placement(stat[:, l]), w[:, l])
        nul = np.array([Wpos[P[mem, b]].sum() for b in range(B)])
        assert ((nul == 0).any() and (nul > 0).any()) or B == 2, l


def test_expanding_keeps_rows_segments_and_copies():
    kinds = wd.GSEA_KINDS
    names, idx = wd.deal(kinds, 64)
    stat, w, P, Gp, Gi, want = wd.gsea_case(2, (1,), True, 2)
    out, null, le_len, le_idx = wd.expand_gsea(want[er.POS], Gp, idx)
    dGp, dGi = wd.deck_pattern(kinds, idx)
    assert out.shape == (len(names), 12, 2) and null.shape == (len(names), 2, 2) and le_idx.shape == (dGp[-1], 2)
    for j in (0, 5, 63, 64, len(names) - 1):
        i = idx[j]
        assert np.array_equal(np.delete(out[j], 3, axis=0), np.delete(want[er.POS][0][i], 3, axis=0), equal_nan=True)
        assert np.array_equal(le_idx[dGp[j]:dGp[j + 1]], want[er.POS][3][Gp[i]:Gp[i + 1]])
    assert np.array_equal(out[:, 3, 0], ref.bh(out[:, 2, 0]), equal_nan=True)
    assert len(wd.copies_differ(out[:, [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11], :], idx)) == 0
    assert len(wd.copies_differ(le_len, idx)) == 0
    spoiled = out.copy()
    spoiled[70, 0, 0] = 0.125
    assert wd.copies_differ(spoiled, idx).tolist() == [70]
