"""The host restatements of plaid.gsea's score types and leading edges (tests/helpers/gsea_edge_ref.py) against each other and
against hand-worked answers, and the new surface (header, ctypes table, hook, wrappers) without a device."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import gsea_edge_ref as er
from tests.helpers import gsea_perm_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = [er.extremes_numpy, er.extremes_literal, er.extremes_fraction]
TYPES = [er.STD, er.POS, er.NEG]


def decreasing(N):
    """a list whose walk order is the row order: pos is the identity"""
    stat = np.arange(N, 0, -1, dtype=np.float64)
    pos = ref.observed_placement(stat)
    assert np.array_equal(pos, np.arange(N))
    return pos, np.ones(N)


def all_forms(pos, mem, Wpos, st, exact=True):
    """(ES, edge) of the numpy form, on which the three forms agree.  exact: every value of the case is a dyadic rational,
    so the rational form has the very ES and the very edge.  Otherwise the two fp64 forms agree bit for bit, the rational
    ES lies within (2k + 4) 2^-53 of theirs, and the rational edge is theirs wherever no other candidate (for std: nor the
    other extreme's magnitude) lies within twice that bound of the extreme"""
    mem = np.asarray(mem, dtype=np.int64)
    got = [er.score_and_edge(pos, mem, Wpos, st, f) for f in FORMS]
    assert got[0] == got[1], (st, got[0], got[1])
    es, (esq, edgeq) = Fraction(got[0][0]), got[2]
    if exact:
        assert es == esq and got[0][1] == edgeq, (st, got[0], got[2])
        return got[0]
    bound = (2 * len(mem) + 4) * Fraction(1, 2**53)
    assert abs(es - esq) <= bound
    maxP, minP, _, _, g_top, g_bot = er.extremes_fraction(pos, mem, Wpos, gaps=True)
    b = er.branch(maxP, minP, st)
    clear = (g_top if b > 0 else g_bot) if b != 0 else Fraction(0)
    if (clear is None or clear > 2 * bound) and (st != er.STD or abs(maxP + minP) > 2 * bound):
        assert got[0][1] == edgeq, (st, got[0][1], edgeq)
    return got[0]


def test_first_and_last_of_four():
    pos, W = decreasing(4)
    es, edge = all_forms(pos, [0, 3], W, er.STD)
    assert es == 0.0 and not np.signbit(es) and edge == []          # maxP = 1/2 = -minP: the tie, no edge
    es, edge = all_forms(pos, [0, 3], W, er.POS)
    assert es == 0.5 and edge == [0]                                 # top branch, length 1
    es, edge = all_forms(pos, [0, 3], W, er.NEG)
    assert es == -0.5 and edge == [3]                                # bottom branch, length 1: the last gene


def test_odd_positions_of_8192_tie_across_lanes_and_chunks():
    N = 8192
    pos, W = decreasing(N)
    mem = er.odd_positions_set(N)
    assert len(mem) == 4096
    for form in FORMS:                                               # every after_t is 1/4096 and every before_t 0.0, exactly
        maxP, minP, t_top, t_bot = form(pos, mem, W)
        assert Fraction(maxP) == Fraction(1, 4096) and Fraction(minP) == 0 and (t_top, t_bot) == (1, 1)
    _, p = er.walk_order(pos, mem)
    t = np.arange(1, 4097)
    assert np.all(t / 4096.0 - (p - t) / 4096.0 == 1.0 / 4096.0) and np.all((t - 1) / 4096.0 - (p - t) / 4096.0 == 0.0)
    for st in (er.STD, er.POS):
        es, edge = all_forms(pos, mem, W, st)
        assert es == 1.0 / 4096.0 and edge == [0]                    # exactly one gene, the first
    es, edge = all_forms(pos, mem, W, er.NEG)
    assert es == 0.0 and edge == list(range(N - 2, -1, -2))          # all 4096 members in reverse walk order


@pytest.mark.parametrize("N", [5, 65])
def test_a_set_of_one_gene(N):
    pos, W = decreasing(N)
    mid = (N - 1) // 2
    want = {   # row: (ES, edge) for std, pos, neg
        0: [(1.0, [0]), (1.0, [0]), (0.0, [0])],
        mid: [(0.0, []), (0.5, [mid]), (-0.5, [mid])],               # miss = 1/2: the std tie
        N - 1: [(-1.0, [N - 1]), (0.0, [N - 1]), (-1.0, [N - 1])],
    }
    for row, answers in want.items():
        for st, (es, edge) in zip(TYPES, answers):
            assert all_forms(pos, [row], W, st) == (es, edge), (row, st)


def test_nan_pairs_have_no_edge():
    pos, W = decreasing(8)
    for mem in ([], list(range(8))):
        for st in TYPES:
            for f in FORMS:
                es, edge = er.score_and_edge(pos, np.asarray(mem, dtype=np.int64), W, st, f)
                assert (es is None or es != es) and edge == []


@pytest.mark.parametrize("weights", ["one", "int"])
@pytest.mark.parametrize("N", [65, 130, 1000])
def test_three_forms_agree_on_exact_weights_with_ties(N, weights):
    rng = np.random.default_rng(N + len(weights))
    stat = np.round(np.clip(rng.normal(size=N), -1, 1))              # three levels: the stable order decides
    w = np.ones(N) if weights == "one" else rng.integers(0, 2**20, size=N).astype(np.float64)
    pos = ref.observed_placement(stat)
    Wpos = ref.walk_weights(pos, w)
    Gp, Gi = ref.make_sets(N, [k for k in (1, 2, 3, 63, 64, 65, N // 2, N - 1) if k < N], seed=N)
    for j in range(len(Gp) - 1):
        mem = Gi[Gp[j]:Gp[j + 1]]
        for st in TYPES:
            es, edge = all_forms(pos, mem, Wpos, st, exact=False)
            assert set(edge) <= set(int(x) for x in mem) and len(set(edge)) == len(edge)
            if st == er.STD:
                assert es == ref.es_numpy(pos, mem.astype(np.int64), Wpos)          # std is the score already pinned
            if st == er.POS:
                assert list(pos[edge]) == sorted(pos[edge]) and len(edge) >= 1      # walk order
            if st == er.NEG:
                assert list(pos[edge]) == sorted(pos[edge], reverse=True) and len(edge) >= 1


def test_the_column_form_has_the_bits_of_the_numpy_form():
    N, B = 130, 65
    rng = np.random.default_rng(21)
    w = rng.integers(0, 1000, size=N).astype(np.float64)
    w[rng.random(size=N) < 0.5] = 0.0                                # sets of total weight 0 take the unweighted rule
    P = ref.placements(N, B, seed=22)
    Gp, Gi = ref.make_sets(N, (1, 2, 3, 64, 65, 129), seed=23)
    zero = 0
    for j in range(len(Gp) - 1):
        mem = Gi[Gp[j]:Gp[j + 1]].astype(np.int64)
        cols = er.extremes_numpy_columns(P, mem, w)
        for b in range(B):
            one = er.extremes_numpy(P[:, b], mem, w)
            assert one == (float(cols[0][b]), float(cols[1][b]), int(cols[2][b]), int(cols[3][b])), (j, b)
            zero += w[P[mem, b]].sum() == 0.0
    assert zero > 0
    assert er.extremes_numpy_columns(P, np.arange(N), w) is None and er.extremes_numpy_columns(P, np.arange(0), w) is None


def test_std_is_the_choice_between_pos_and_neg():
    N = 130
    rng = np.random.default_rng(3)
    stat, w = rng.normal(size=N), rng.integers(1, 100, size=N).astype(np.float64)
    pos = ref.observed_placement(stat)
    Wpos = ref.walk_weights(pos, w)
    Gp, Gi = ref.make_sets(N, (1, 2, 5, 64, 65, 129), seed=4)
    for j in range(len(Gp) - 1):
        mem = Gi[Gp[j]:Gp[j + 1]]
        (ep, gp), (en, gn), (es, gs) = (er.score_and_edge(pos, mem, Wpos, st) for st in (er.POS, er.NEG, er.STD))
        assert es == (ep if ep > -en else (en if ep < -en else 0.0))
        assert gs == (gp if ep > -en else (gn if ep < -en else []))


def test_whole_call_reference_keeps_std_as_pinned_and_fills_the_buffers():
    N, B, c = 65, 65, 2
    rng = np.random.default_rng(11)
    stat = np.round(np.clip(rng.normal(size=(N, c)), -1, 1))
    w = rng.integers(0, 2**20, size=(N, c)).astype(np.float64)
    Gp, Gi = ref.make_sets(N, (0, 1, 2, 33, 64, 65), seed=12)
    P = ref.placements(N, B, seed=13)
    res = er.gsea_scored_ref(stat, w, Gp, Gi, P)
    want, want_null = ref.gsea_ref(stat, w, Gp, Gi, P)
    assert np.array_equal(res[er.STD][0], want, equal_nan=True) and np.array_equal(res[er.STD][1], want_null, equal_nan=True)
    for st in TYPES:
        out, null, le_len, le_idx = res[st]
        k = np.diff(Gp)
        assert np.all(le_len[(k == 0) | (k == N), :] == 0)
        for l in range(c):
            for j in range(len(k)):
                seg = le_idx[Gp[j]:Gp[j + 1], l]
                assert np.all(seg[le_len[j, l]:] == -1) and np.all(seg[:le_len[j, l]] >= 0)
        if st == er.POS:      # one-sided columns: pval and nMoreExtreme read the upper counts alone
            ok = ~np.isnan(out[:, 0, :])
            assert np.array_equal(out[:, 4, :][ok], out[:, 6, :][ok])
            assert np.array_equal(out[:, 2, :][ok], ((1.0 + out[:, 6, :]) / (1.0 + out[:, 8, :]))[ok])
            assert np.all(out[:, 0, :][ok] >= 0.0) and np.all(null[~np.isnan(null)] >= 0.0)      # maxP >= after_k = 0
        if st == er.NEG:
            ok = ~np.isnan(out[:, 0, :])
            assert np.array_equal(out[:, 4, :][ok], out[:, 7, :][ok])
            assert np.array_equal(out[:, 2, :][ok], ((1.0 + out[:, 7, :]) / (1.0 + out[:, 9, :]))[ok])
            assert np.all(out[:, 0, :][ok] <= 0.0)


def test_the_new_surface_is_declared_everywhere():
    from plaid_amd import _lib, engine
    header = open(os.path.join(ROOT, "include", "plaidhip.h")).read()
    for name, nargs in (("plaidhip_gsea_scored", 16), ("plaidhip_gsea_scored_multi", 17)):
        assert re.search(r"\bint\s+%s\s*\(" % name, header) and len(_lib.SIGNATURES[name]) == nargs
    for name, value in (("PLAIDHIP_GSEA_STD", 0), ("PLAIDHIP_GSEA_POS", 1), ("PLAIDHIP_GSEA_NEG", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header)
    assert engine.GSEA_SCORE_TYPES == er.SCORE_TYPES
    assert re.search(r'Not offered: fgsea\'s multilevel p-values', header) and "leading edges. */" not in header
    multi = open(os.path.join(ROOT, "plaid_amd", "csrc", "multi.cpp")).read()
    assert re.search(r"\bint\s+plaidhip_debug_gsea_scored_sharded_on_one_device\s*\(", multi)
    with pytest.raises(ValueError, match="score_type"):
        engine.gsea_score_type("both")


def test_plaid_gsea_refuses_an_unknown_score_type_before_any_device_work():
    import plaid_amd
    with pytest.raises(ValueError, match="scoreType"):
        plaid_amd.plaid_gsea({"a": 1.0, "b": 2.0}, {"s": ["a"]}, scoreType="both")


def test_argument_errors_come_in_the_stated_order_without_a_device():
    """plaidhip_gsea_scored without a context: the score type, the le_len / le_idx pair, then plaidhip_gsea's own order; every
    check comes before the context is looked at, so nothing is launched and nothing is written"""
    from plaid_amd import _lib
    lib = _lib.load()
    g, c, m = 65, 3, 2
    stat = np.asfortranarray(np.random.default_rng(1).normal(size=(g, c)))
    w, wneg = np.ones((g, c), order="F"), np.ones((g, c), order="F")
    wneg[3, 2] = -1.0
    Gp, Gi = np.array([0, 2, 5], dtype=np.int32), np.array([0, 3, 1, 2, 64], dtype=np.int32)
    out = np.full((m, 12, c), -7.0, order="F")
    le_len, le_idx = np.full((m, c), -7, dtype=np.int32, order="F"), np.full((5, c), -7, dtype=np.int32, order="F")

    def call(st, ln, ix, nperm, lists, weight, fn=lib.plaidhip_gsea_scored, head=(None,)):
        rc = fn(*head, stat.ctypes.data, weight.ctypes.data, g, lists, Gp.ctypes.data, Gi.ctypes.data, m, None, nperm, 1, st,
                out.ctypes.data, None, None if ln is None else ln.ctypes.data, None if ix is None else ix.ctypes.data)
        return rc, lib.plaidhip_last_error_string()

    for st in (-1, 3):
        rc, msg = call(st, le_len, None, 0, 0, wneg)
        assert rc == _lib.EINVAL and b"score_type" in msg
    for ln, ix in ((le_len, None), (None, le_idx)):
        rc, msg = call(1, ln, ix, 0, 0, wneg)
        assert rc == _lib.EINVAL and b"le_len and le_idx" in msg
    for st in (0, 1, 2):
        for args, word in (((0, 0, wneg), b"nperm"), ((10, 0, wneg), b"ranked lists"), ((10, c, wneg), b"weight"),
                           ((10, c, w), b"null plaidhip_ctx")):
            rc, msg = call(st, le_len, le_idx, *args)
            assert rc == _lib.EINVAL and word in msg, (st, word, msg)
    dev = np.zeros(1, dtype=np.int32)
    rc, msg = call(3, le_len, None, 0, 0, wneg, fn=lib.plaidhip_gsea_scored_multi, head=(dev.ctypes.data, 1))
    assert rc == _lib.EINVAL and b"score_type" in msg
    rc, msg = call(2, None, le_idx, 0, 0, wneg, fn=lib.plaidhip_gsea_scored_multi, head=(dev.ctypes.data, 1))
    assert rc == _lib.EINVAL and b"le_len and le_idx" in msg
    assert np.all(out == -7.0) and np.all(le_len == -7) and np.all(le_idx == -7)
