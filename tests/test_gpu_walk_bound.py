"""The bitmap-walk kernels of plaid.gsea at the map bound, N = 131,072 genes (engine.GSEA_KS_MAX_GENES; `pytest -m gpu`).

The other tests of plaid.gsea walk at most 8,193 genes (seams, not sizes) and refuse 131,073.  Here the map is as long as
it gets: 2,048 words, 32 scan steps, four maps in 64 KB of dynamic LDS.  Every check is bit equality (integer equality
for the edges and the traces) with the host restatements of tests/helpers/gsea_perm_ref.py, gsea_edge_ref.py and
gsea_multilevel_ref.py; weights are 1 or integers below 2^20, so every partial sum is exact; padj keeps its rtol = 1e-15.

What runs at the bound, and which test launches it:

  gsea_null_kernel<W,ST> (68 KB, PH_FULL_LDS per instance)   test_supplied_placements[unit|int - std|pos|neg]: all six
  gsea_obs_kernel<W,ST> (64 KB)                              the same six
  gsea_edge_kernel<false> / <true> (96 KB, PH_FULL_LDS)      test_supplied_placements[unit-*] / [int-*]
  gsea_check_perm_kernel (its 4,096 words, the last bit)     test_supplied_placements (good), test_a_bad_placement (refused)
  gsea_philox_keys_kernel, the min ranker at g = 2^17,       test_generated_placements
  gsea_rank_to_placement_kernel
  gsea_ml_init_kernel<W,ST>, gsea_ml_mutate_kernel<W,ST>     test_rulers: <false,std> (side 0), <true,std> (side 1), <true,pos>,
  (64 KB; 32 scan steps, ml_select over 2,048 words)         <false,neg>: four of the six instances of each

65 placements are a full block and a block of one, and at this N a slab of 64 (gsea_slab_perms): two launches of the null.
The ten sets: 0, 1, 2, 65 and 4,097 members, N - 1 and N; the 64 lowest statistics of list 0 (exactly the last map word
of its observed placement); walk positions 126,970 .. 126,981 of list 0 (astride the last scan-step boundary, 31 x 4,096 =
126,976); ten positions inside the first word.  The restatement of the rulers takes seconds at k = 1 and 7 (five slots,
one sweep): none is recorded.

Not covered at the bound: <true,neg> and <false,pos> of the two multilevel kernels (the issue's four sides), general
weights, more than two lists."""
import numpy as np
import pytest

from tests.helpers import gsea_edge_ref as er
from tests.helpers import gsea_multilevel_ref as ml
from tests.helpers import gsea_perm_ref as ref
from tests.test_gpu_gsea_edges import same, same_but_padj, same_int
from tests.test_gpu_gsea_multilevel import SIDES, TYPE_NAME, same_trace

pytestmark = pytest.mark.gpu

N = 131072
B = 65
_cache = {}


def lists_and_sets():
    """(stat N x 2 -- list 0 continuous, list 1 of three levels: the stable order decides --, Gp, Gi of the ten sets)"""
    if "sets" not in _cache:
        assert N == __import__("plaid_amd").engine.GSEA_KS_MAX_GENES
        rng = np.random.default_rng(131072)
        stat = rng.normal(size=(N, 2))
        stat[:, 1] = np.round(np.clip(stat[:, 1], -1, 1))
        Gp, Gi = ref.make_sets(N, (0, 1, 2, 65, 4097, N - 1, N), seed=17)
        row_at = np.argsort(-stat[:, 0], kind="stable")                     # the row at each walk position of list 0
        assert np.array_equal(ref.observed_placement(stat[:, 0])[row_at], np.arange(N))
        planted = [np.arange(N - 64, N),                                     # the last map word, all of it
                   np.arange(31 * 4096 - 6, 31 * 4096 + 6),                  # astride the last scan-step boundary
                   np.array([0, 1, 5, 9, 17, 31, 32, 33, 62, 63])]           # inside the first word
        lists = [Gi[Gp[j]:Gp[j + 1]] for j in range(len(Gp) - 1)] + [np.sort(row_at[p]).astype(np.int32) for p in planted]
        Gp = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int32)
        _cache["sets"] = (stat, Gp, np.concatenate(lists).astype(np.int32))
    return _cache["sets"]


def weights_of(kind):
    if kind == "unit":
        return np.ones((N, 2))
    return np.random.default_rng(7).integers(0, 2**20, size=(N, 2)).astype(np.float64)


def supplied():
    if "P" not in _cache:
        rng = np.random.default_rng(65)
        _cache["P"] = np.asfortranarray(np.stack([rng.permutation(N) for _ in range(B)], axis=1).astype(np.int32))
    return _cache["P"]


def reference(weights):
    """{score type: (out, null, le_len, le_idx)}: every walk of the restatement is taken once and serves the three types"""
    key = ("ref", weights)
    if key not in _cache:
        stat, Gp, Gi = lists_and_sets()
        _cache[key] = er.gsea_scored_ref(stat, weights_of(weights), Gp, Gi, supplied())
    return _cache[key]


# ---- 1. supplied placements: the six instances of the null and observed kernels, the two of the edge kernel -----------------------
@pytest.mark.parametrize("st_name", ["std", "pos", "neg"])
@pytest.mark.parametrize("weights", ["unit", "int"])
def test_supplied_placements(hip_ctx, weights, st_name):
    st = er.SCORE_TYPES[st_name]
    stat, Gp, Gi = lists_and_sets()
    assert len(Gp) - 1 == 10 and list(np.diff(Gp)) == [0, 1, 2, 65, 4097, N - 1, N, 64, 12, 10]
    w_out, w_null, w_len, w_idx = reference(weights)[st]
    out, null, le_len, le_idx = hip_ctx.gsea(stat, weights_of(weights), Gp, Gi, perm=supplied(), null=True, score_type=st_name,
                                             leading_edge=True)
    same(null, w_null, "null scores")
    same_but_padj(out, w_out, f"N={N} {weights} {st_name}")
    same_int(le_len, w_len, "le_len")
    same_int(le_idx, w_idx, "le_idx")
    k = np.diff(Gp)
    assert np.array_equal(out[:, 5, 0], k.astype(np.float64))
    nanset = (k == 0) | (k == N)
    assert np.isnan(out[nanset][:, [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11], :]).all() and np.isnan(null[nanset]).all()
    assert not np.isnan(null[~nanset]).any() and not np.isnan(out[~nanset][:, [0, 1, 2, 4], :]).any()
    for l in range(2):
        for j in range(len(k)):
            seg = le_idx[Gp[j]:Gp[j + 1], l]
            assert 0 <= le_len[j, l] <= k[j] and np.all(seg[le_len[j, l]:] == -1) and np.all(seg[:le_len[j, l]] >= 0)
    if st != er.STD:
        assert np.all(le_len[~nanset] >= 1)                          # a one-sided edge is never empty
    # the planted sets of list 0 are where they were put: all of the last word scores -1 at its first member (std, neg)
    if st_name != "pos" and weights == "unit":
        assert out[7, 0, 0] == -1.0 and le_len[7, 0] == 64


# ---- 2. generated placements: the Philox keys, the min ranker at g = 2^17, rank -> placement -------------------------------------
def test_generated_placements(hip_ctx):
    seed = 2**35 + 131
    stat, Gp, Gi = lists_and_sets()
    w = weights_of("int")
    P = ref.placements(N, B, seed)                 # (asserts that every column's keys r 2^17 + i are free of ties)
    assert np.array_equal(hip_ctx.gsea_permutations(N, B, seed=seed), P)
    a = hip_ctx.gsea(stat, w, Gp, Gi, perm=None, nperm=B, seed=seed, null=True, leading_edge=True)
    b = hip_ctx.gsea(stat, w, Gp, Gi, perm=P, null=True, leading_edge=True)
    for x, y, nm in zip(a, b, ("out", "null", "le_len", "le_idx")):
        assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True), nm
    assert not np.isnan(a[1][[1, 2, 3, 4, 5, 7, 8, 9]]).any()


# ---- 3. a bad placement at the bound -------------------------------------------------------------------------------------------
def test_a_bad_placement(hip_ctx):
    """the status and message of tests/test_gpu_gsea.py::test_argument_errors at N = 65: EINVAL, `column <b> of perm`.
    Column 64 is the one column of the second slab; 131,071 is the last bit of the last word of the kernel's map"""
    import plaid_amd
    from plaid_amd import _lib
    stat, Gp, Gi = lists_and_sets()
    w = weights_of("unit")
    P2 = supplied().copy(order="F")
    P2[np.flatnonzero(P2[:, 64] == 5)[0], 64] = N - 1             # 131,071 twice, 5 never
    with pytest.raises(plaid_amd.PlaidHipError, match="column 64 of perm") as e:
        hip_ctx.gsea(stat, w, Gp, Gi, perm=P2)
    assert e.value.code == _lib.EINVAL
    P2 = supplied().copy(order="F")
    P2[N - 1, 0] = N                                               # one past the map
    with pytest.raises(plaid_amd.PlaidHipError, match="column 0 of perm") as e:
        hip_ctx.gsea(stat, w, Gp, Gi, perm=P2)
    assert e.value.code == _lib.EINVAL
    # and the context still serves a good call
    out = hip_ctx.gsea(stat[:, :1], w[:, :1], Gp, Gi, perm=supplied()[:, :1])
    same(out[:, 0, :], reference("unit")[er.STD][0][:, 0, :1], "ES after the refusals")


# ---- 4. multilevel rulers ------------------------------------------------------------------------------------------------------
RULERS = [(N, (1, 7)[q % 2], st, side, ("unit", "int", "int", "unit")[q], 300 + q, 40 + q, 5, 1) for q, (st, side) in enumerate(SIDES)]


@pytest.mark.parametrize("case", RULERS, ids=ml.golden_key)
def test_rulers(hip_ctx, case):
    """the restatement runs here (seconds at k = 1 and 7 with five slots and one sweep): no trace is recorded"""
    n_, k, st, side, weights, dseed, cseed, n, sweeps = case
    stat, weight, Wpos, gamma = ml.ruler_case(N, k, st, side, weights, dseed)
    want = ml.run_ruler(Wpos, k, 1, side, st, gamma, cseed, n, sweeps, 1e-50)
    print(f"{ml.golden_key(case)}: {want['stages']} stages, status {want['status']}, gamma {gamma!r}")
    got = hip_ctx.gsea_ruler(stat, weight, k, l=1, side=side, score_type=TYPE_NAME[st], gamma=gamma, seed=cseed, sample_size=n,
                             sweeps=sweeps, eps=1e-50)
    same_trace(got, want, ml.golden_key(case))
    assert want["stages"] >= 2
