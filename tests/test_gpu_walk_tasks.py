"""The bitmap-walk kernels past a workgroup's first task (`pytest -m gpu`).

Every exact walk keeps an N-bit map in LDS that "is all zero on the way in and has to be on the way out"
(plaid_amd/csrc/bitmap_walk.h), and its kernels loop over tasks on a capped grid.  The other tests of these entries pin
the arithmetic with launches in which no workgroup takes a second task (the one exception: gsva_cases._long, ordinary
sets only).  Here every launch is longer than its cap, a task is a set (N = 4,160 genes -- two scan steps --, eight
columns or lists: one tile), and the sets are a deck (tests/helpers/walk_decks.py) in which every kind of set -- empty,
full, one member, 64, 65, first scan step only, second only, both, a planted B = 0 -- follows every kind inside some
workgroup (wavefront) of the launcher's grid.  Two of the eight columns are NaN, so that one wavefront meets NaN and then
an ordinary column and another the other way round.

Every check is bit equality (integer equality for the edges) with the existing host restatements, computed on the K
distinct member lists and expanded by index; padj keeps its rtol = 1e-15 comparison.  Weights are 1 or integers below
2^20, alpha and tau are 0 or 1: every partial sum is exact.  Each test also asserts that all copies of a kind have the
same bits, and -- before the device is touched -- that its deck shows every ordered pair for the device's CU count.

Which test gives which kernel a second task (stride = tasks between two tasks of a workgroup or wavefront):

  gsea_ks_kernel<false> / <true>     32 CUs (ks_launch)            test_ssgsea_ks[0.0] / [1.0]
  gsva_ks_kernel<false> / <true>     32 CUs (ks_launch)            test_gsva_ks[0.0-*] / [1.0-*]
  sing_mad_kernel                    32 CUs (launch_sing_mad)      test_sing_mad
  gsea_obs_kernel<W,ST>              64 CUs pairs (gn_pair_launch) test_gsea_obs_and_edges: <false,std>, <true,std>, <true,pos>,
                                                                   <true,neg>; <false,pos> and <false,neg> pass their cap in
                                                                   test_gsea_null[unit-pos|neg] (8 lists: 8 m pairs), the
                                                                   pair condition not asserted there
  gsea_edge_kernel<false> / <true>   64 CUs pairs (gn_pair_launch) test_gsea_obs_and_edges[unit-*] / [int-*]
  gsea_null_kernel<W,ST>             16 CUs (launch_gsea_null)     test_gsea_null, all six; the partial block of placements
                                                                   and the short list tile after full ones:
                                                                   test_gsea_null_partial_block_and_short_tile (<true,std>)

A deck is stride + 88 sets (88 = 9 kinds squared + 7): rank_decks.deck gives the 88 workgroups (wavefronts) that take a
second task the 81 ordered pairs, and every workgroup with one task the first kind of the tuple (`both`).  A library whose task loops leave after
one trip fails every test here but the first (run once on an MI355X with 256 CUs) and none of the earlier tests of these
entries: DESIGN.md section 17.

Not covered: the multilevel kernels past their cap (they reload their map per task and carry nothing)."""
import numpy as np
import pytest

from tests.helpers import exact_ref as xr
from tests.helpers import gsea_edge_ref as er
from tests.helpers import gsea_perm_ref as ref
from tests.helpers import rank_decks as rd
from tests.helpers import walk_decks as wd

pytestmark = pytest.mark.gpu

NOT_PADJ = [q for q, nm in enumerate(ref.COLUMNS) if nm != "padj"]
_DECKS = {}


def _cu():
    """the CU count plaidhip_create keeps in ctx->num_cu (api.cpp: hipDeviceProp_t::multiProcessorCount), which every walk
    launcher multiplies its cap by"""
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _deck(kinds, stride):
    """(names, idx, Gp, Gi) of the deck for this stride, dealt once; the pair condition is asserted here, before a launch"""
    key = (kinds, stride)
    if key not in _DECKS:
        names, idx = wd.deal(kinds, stride)
        assert len(names) == stride + len(kinds) ** 2 + 7 and rd.pairs_seen(names, stride) == rd.all_pairs(kinds)
        _DECKS[key] = (names, idx) + wd.deck_pattern(kinds, idx)
        print(f"{_cu()} CUs: a deck of {len(names)} sets of {len(kinds)} kinds at stride {stride}, {len(_DECKS[key][3])} members")
    return _DECKS[key]


def _same_rows(got, want_kinds, idx, what):
    """the device's sets x columns result against the K lists' reference, and all copies of a kind against each other"""
    assert got.shape == (len(idx), want_kinds.shape[1]), what
    xr.assert_same_bits(got, wd.expand(want_kinds, idx), what)
    assert len(wd.copies_differ(got, idx)) == 0, what


# ---- restatements of the caps (see walk_decks.ks_stride / pair_stride / null_stride) ---------------------------------------------
def ks_stride():
    return 32 * _cu()        # ks_launch (kernels_ks.hip), launch_sing_mad (kernels_sing.hip): num_cu * 32 workgroups


def pair_stride():
    return 64 * _cu()        # gn_pair_launch (kernels_gsea.hip): num_cu * 16 workgroups of kGnWaves = 4 pairs


def null_stride():
    return 16 * _cu()        # launch_gsea_null (kernels_gsea.hip): num_cu * 16 workgroups


def test_the_strides_are_the_helpers(hip_ctx):
    cu = _cu()
    assert (ks_stride(), pair_stride(), null_stride()) == (wd.ks_stride(cu), wd.pair_stride(cu), wd.null_stride(cu))


# ---- gsea_ks_kernel, gsva_ks_kernel, sing_mad_kernel -------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_ssgsea_ks(hip_ctx, alpha):
    names, idx, Gp, Gi = _deck(wd.KS_KINDS, ks_stride())
    want = wd.ssgsea_ks_ref(alpha)
    assert wd.nan_only_where(want, wd.KS_KINDS, wd.NAN_KINDS, wd.NAN_COLS)
    got = hip_ctx.ssgsea_exact(wd.columns(), Gp, Gi, alpha, True, False, single=False)
    _same_rows(got, want, idx, f"ssgsea.exact(single = FALSE) alpha = {alpha}")


@pytest.mark.parametrize("max_diff", [True, False])
@pytest.mark.parametrize("tau", [0.0, 1.0])
def test_gsva_ks(hip_ctx, tau, max_diff):
    """tau = 1: the kind `centre` is the gene at q = N / 2 alone, B = 0: the map is zeroed without a walk and the score is NaN"""
    names, idx, Gp, Gi = _deck(wd.KS_KINDS, ks_stride())
    want = wd.gsva_ks_ref(tau, max_diff)
    assert wd.nan_only_where(want, wd.KS_KINDS, wd.NAN_KINDS + (("centre",) if tau == 1.0 else ()), wd.NAN_COLS)
    got = hip_ctx.gsva_exact(wd.columns(), Gp, Gi, tau, "none", max_diff)
    _same_rows(got, want, idx, f"gsva.exact tau = {tau} max_diff = {max_diff}")


def test_sing_mad(hip_ctx):
    names, idx, Gp, Gi = _deck(wd.KS_KINDS, ks_stride())
    want = wd.sing_ref()
    assert wd.nan_only_where(want["UpScore"], wd.KS_KINDS, ("empty", "full"), wd.NAN_COLS)
    assert wd.nan_only_where(want["UpDispersion"], wd.KS_KINDS, ("empty",), wd.NAN_COLS)       # k = N: an ordinary pair here
    got = hip_ctx.sing_exact(wd.columns(), Gp, Gi, None, None, True, True)
    assert sorted(got) == sorted(want) == ["UpDispersion", "UpScore"]
    for name in want:
        _same_rows(got[name], want[name], idx, f"sing.exact {name}")


# ---- plaid.gsea ------------------------------------------------------------------------------------------------------------------
def _check_gsea(ctx, stride, ncol, nan_lists, weighted, st_name, B):
    names, idx, Gp, Gi = _deck(wd.GSEA_KINDS, stride)
    stat, w, P, kGp, kGi, want = wd.gsea_case(ncol, nan_lists, weighted, B)
    k_out, k_null = want[er.SCORE_TYPES[st_name]][:2]
    assert wd.nan_only_where(k_out[:, 0, :], wd.GSEA_KINDS, wd.NAN_KINDS, nan_lists)
    assert all(wd.nan_only_where(k_null[:, b, :], wd.GSEA_KINDS, wd.NAN_KINDS, nan_lists) for b in range(B))
    w_out, w_null, w_len, w_idx = wd.expand_gsea(want[er.SCORE_TYPES[st_name]], kGp, idx)
    out, null, le_len, le_idx = ctx.gsea(stat, w, Gp, Gi, perm=P, null=True, score_type=st_name, leading_edge=True)
    what = f"{st_name} {'int' if weighted else 'unit'} c={ncol} B={B} NaN lists {nan_lists}"
    assert out.shape == w_out.shape and null.shape == w_null.shape, what
    xr.assert_same_bits(null, w_null, f"{what}: null scores")
    for q, nm in enumerate(ref.COLUMNS):
        if nm == "padj":
            np.testing.assert_allclose(out[:, q, :], w_out[:, q, :], rtol=1e-15, atol=0, equal_nan=True, err_msg=what)
        else:
            xr.assert_same_bits(out[:, q, :], w_out[:, q, :], f"{what}: {nm}")
    assert le_len.dtype == w_len.dtype == np.int32 and np.array_equal(le_len, w_len), f"{what}: le_len"
    assert le_idx.dtype == w_idx.dtype == np.int32 and le_idx.shape == w_idx.shape, f"{what}: le_idx"
    bad = np.argwhere(le_idx != w_idx)
    assert len(bad) == 0, f"{what}: le_idx differs at {len(bad)} places, first {bad[0]}"
    for arr, nm in ((out[:, NOT_PADJ, :], "out"), (null, "null"), (le_len, "le_len")):
        assert len(wd.copies_differ(arr, idx)) == 0, f"{what}: copies of a kind differ in {nm}"
    return names


@pytest.mark.parametrize("weights,st_name,nan_at", [("unit", "std", "first"), ("int", "std", "last"), ("int", "pos", "first"),
                                                    ("int", "neg", "last")])
def test_gsea_obs_and_edges(hip_ctx, weights, st_name, nan_at):
    """two lists, one NaN, B = 2 placements: m = 64 CUs + 88 sets, so a wavefront of gsea_obs_kernel / gsea_edge_kernel takes
    the pairs e, e + 64 CUs, ... of e = l m + j: every ordered pair of kinds inside the ordinary list, and a crossing from
    (into) the NaN list.  int: the kind zero_w has B = 0 under the observed placement (the unweighted walk of the same map)"""
    stride = pair_stride()
    names, _, _, _ = _deck(wd.GSEA_KINDS, stride)
    listnan = (True, False) if nan_at == "first" else (False, True)
    seen = rd.pairs_seen(wd.pair_kinds(names, listnan), stride)
    assert {(a, b) for (a, na), (b, nb) in seen if not na and not nb} == rd.all_pairs(wd.GSEA_KINDS)
    assert any((na, nb) == ((True, False) if listnan[0] else (False, True)) for (a, na), (b, nb) in seen)
    _check_gsea(hip_ctx, stride, 2, (0,) if nan_at == "first" else (1,), weights == "int", st_name, 2)


@pytest.mark.parametrize("weights,st_name,nan_lists", [("unit", "std", (0, 3)), ("unit", "pos", (0, 3)), ("unit", "neg", (0, 3)),
                                                       ("int", "std", (0, 3)), ("int", "pos", (3, 7)), ("int", "neg", (0, 3)),
                                                       ("int", "std", (3, 7))],
                         ids=lambda v: "nan" + "".join(map(str, v)) if isinstance(v, tuple) else v)
def test_gsea_null(hip_ctx, weights, st_name, nan_lists):
    """eight lists (one list tile), two of them NaN, B = 64 placements (one block): task = set, m = 16 CUs + 88.  int: a
    permutation's bits are walked once per list and the LAST list's walk clears the map -- (3, 7) has the NaN list last
    (walk_zero_map instead of a walk), (0, 3) first; the one-gene kind has B = 0 under about a quarter of the placements
    (the unweighted fallback walk clears the map).  The edges and the observed scores run on 8 m pairs beside it"""
    stride = null_stride()
    names, _, _, _ = _deck(wd.GSEA_KINDS, stride)
    blk, tile, j, nb, nl = wd.null_tasks(len(names), 8, 64, weights == "int")
    assert np.array_equal(j, np.arange(len(names))) and len(names) > stride                    # task = set, past the cap
    _check_gsea(hip_ctx, stride, 8, nan_lists, weights == "int", st_name, 64)


def test_gsea_null_partial_block_and_short_tile(hip_ctx):
    """the same deck with B = 130 placements and nine lists, weighted: three blocks of placements, the last of 2, and two list
    tiles, the last of one list: 6 m tasks.  A workgroup meets the partial block after a full one (s_es behind the
    trailing barrier holds 64 scores of the task before, 2 are this task's) and the short tile after the full one, some
    of them straight after a NaN-scoring set"""
    stride = null_stride()
    names, _, _, _ = _deck(wd.GSEA_KINDS, stride)
    got = wd.null_successions(names, 9, 130, stride)
    assert got["block"] > 0 and got["tile"] > 0 and got["from_nan"] > 0, got
    _check_gsea(hip_ctx, stride, 9, (3,), True, "std", 130)
