"""plaid.gsea's multilevel p-values on the device (plaidhip_gsea_multilevel, plaidhip_gsea_ruler, kernels_gsea_ml.hip;
DESIGN.md section 23) against the host restatement of tests/helpers/gsea_multilevel_ref.py.

A ruler's chain is deterministic given the seed, so where every walk has host bits -- weights of 1, integer weights below
2^20 -- the device's trace (stages, end status, every level, every count, every recorded score) must BE the restatement's.
For general weights a score lies within (2k + 4) 2^-53 of the rational value (section 17's bound), so the discrete trace
must still be the restatement's wherever the restatement never compared the scores of two different states closer than
twice that bound; the seeds below are such (the test asserts it), so no case is undecidable.  (Sets of two or three
members always meet such a pair -- after_k = 1 - miss_k does not see the weights -- so the general-weight cases start at 7.)  The sizes are the seams: N = 65 (one past a map word)
and 4097 (one past a 64-word chunk), k at both ends, n = 5 and 101, 1 and 4 sweeps, 2 and 9 lists (the list tile of 8)."""
import os

import numpy as np
import pytest

from tests.helpers import gsea_edge_ref as er
from tests.helpers import gsea_multilevel_ref as ml
from tests.helpers import gsea_perm_ref as ref

pytestmark = pytest.mark.gpu

TYPE_NAME = {er.STD: "std", er.POS: "pos", er.NEG: "neg"}
SIDES = [(er.STD, 0), (er.STD, 1), (er.POS, 0), (er.NEG, 1)]
_cache = {}


def same_trace(got, want, what):
    assert got["stages"] == want["stages"] and got["status"] == want["status"], \
        f"{what}: {got['stages']} stages ending {got['status']}, the restatement {want['stages']} ending {want['status']}"
    assert np.array_equal(got["s"], want["s"]), f"{what}: counts {got['s']} != {want['s']}"
    assert np.array_equal(got["m"], want["m"]), f"{what}: levels differ, first at stage {np.flatnonzero(got['m'] != want['m'])[0]}"
    assert np.array_equal(got["h"], want["h"]), f"{what}: scores differ, first at {np.argwhere(got['h'] != want['h'])[0]}"


def same(a, b, what=""):
    assert a.shape == b.shape
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    assert not bad.any(), f"{what}: {int(bad.sum())} differ, first at {np.argwhere(bad)[0]}: {a[bad][0]!r} != {b[bad][0]!r}"


# ---- 1. one ruler, bit for bit ------------------------------------------------------------------------------------------------------
def ruler_cases():
    cases, q = [], 0
    for k in (1, 2, 7, 62, 64):                       # N = 65: both ends of k, every side, n and sweeps alternating
        for st, side in SIDES:
            cases.append((65, k, st, side, ("unit", "int")[q % 2], 100 + q, 5 + q, (5, 101)[(q // 2) % 2], (1, 4)[(q // 3) % 2]))
            q += 1
    for k, n, sweeps in ((1, 101, 4), (2, 101, 1), (7, 5, 4)):   # N = 4097, the small sizes
        for st, side in SIDES[q % 2::2]:
            cases.append((4097, k, st, side, ("unit", "int")[q % 2], 100 + q, 5 + q, n, sweeps))
            q += 1
    return cases


@pytest.mark.parametrize("case", ruler_cases(), ids=ml.golden_key)
def test_ruler_trace_has_the_restatements_bits(hip_ctx, case):
    N, k, st, side, weights, dseed, cseed, n, sweeps = case
    stat, weight, Wpos, gamma = ml.ruler_case(N, k, st, side, weights, dseed)
    want = ml.run_ruler(Wpos, k, 3, side, st, gamma, cseed, n, sweeps, 1e-50)
    got = hip_ctx.gsea_ruler(stat, weight, k, l=3, side=side, score_type=TYPE_NAME[st], gamma=gamma, seed=cseed, sample_size=n,
                             sweeps=sweeps, eps=1e-50)
    print(f"{ml.golden_key(case)}: {want['stages']} stages, status {want['status']}, gamma {gamma!r}")
    same_trace(got, want, ml.golden_key(case))
    assert want["stages"] >= 2


@pytest.mark.parametrize("case", ml.GOLDEN_RULERS, ids=ml.golden_key)
def test_ruler_trace_next_to_n(hip_ctx, golden_dir, case):
    """k = N - 3 and N - 1 at N = 4097: the restatement's traces as recorded (it takes minutes there)"""
    N, k, st, side, weights, dseed, cseed, n, sweeps = case
    stat, weight, Wpos, gamma = ml.ruler_case(N, k, st, side, weights, dseed)
    rec, key = np.load(os.path.join(golden_dir, "gsea_ml_traces.npz")), ml.golden_key(case)
    want = {"stages": len(rec[key + "_m"]), "status": int(rec[key + "_status"][0]), "m": rec[key + "_m"], "s": rec[key + "_s"],
            "h": rec[key + "_h"]}
    got = hip_ctx.gsea_ruler(stat, weight, k, l=3, side=side, score_type=TYPE_NAME[st], gamma=gamma, seed=cseed, sample_size=n,
                             sweeps=sweeps, eps=1e-50)
    same_trace(got, want, key)


# ---- 2. termination ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps,end", [(0.0, ml.STALLED), (1e-3, ml.FLOOR)])
def test_a_target_no_set_attains(hip_ctx, eps, end):
    stat, weight, Wpos, _ = ml.ruler_case(65, 2, er.STD, 0, "int", 77)
    want = ml.run_ruler(Wpos, 2, 0, 0, er.STD, 2.0, 9, 101, 4, eps)
    got = hip_ctx.gsea_ruler(stat, weight, 2, l=0, side=0, gamma=2.0, seed=9, sample_size=101, sweeps=4, eps=eps)
    same_trace(got, want, f"eps = {eps}")
    assert got["status"] == end
    qhat, log2err, lstar, status, c = ml.read_off(got, 2.0)
    assert status == end and lstar == got["stages"] - 1 and c == 0


# ---- 3. general weights -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,k,st,side,dseed,cseed", [(65, 7, er.STD, 0, 201, 3), (65, 62, er.STD, 1, 202, 2),
                                                     (300, 17, er.NEG, 1, 204, 4), (130, 40, er.STD, 0, 205, 1)])
def test_general_weights_keep_the_discrete_trace(hip_ctx, N, k, st, side, dseed, cseed):
    stat, weight, Wpos, gamma = ml.ruler_case(N, k, st, side, "abs", dseed)
    bound = (2 * k + 4) * 2.0 ** -53
    want = ml.run_ruler(Wpos, k, 0, side, st, gamma, cseed, 21, 2, 1e-50)
    print(f"N {N} k {k}: {want['stages']} stages, smallest gap {want['gap']:.3e}, bound {bound:.3e}")
    assert want["gap"] > 2 * bound, "the restatement itself is undecided for this seed: pick another"
    got = hip_ctx.gsea_ruler(stat, weight, k, l=0, side=side, score_type=TYPE_NAME[st], gamma=gamma, seed=cseed, sample_size=21,
                             sweeps=2, eps=1e-50)
    assert got["stages"] == want["stages"] and got["status"] == want["status"]
    assert np.array_equal(got["s"], want["s"])
    print(f"largest |m - m_ref| {np.max(np.abs(got['m'] - want['m'])):.3e}, scores {np.max(np.abs(got['h'] - want['h'])):.3e}")
    assert np.all(np.abs(got["m"] - want["m"]) <= bound) and np.all(np.abs(got["h"] - want["h"]) <= bound)
    for ga in (gamma, 0.5 * gamma):   # the counts of a read-off
        if np.min(np.abs(want["h"] - ga)) > 2 * bound and np.min(np.abs(want["m"] - ga)) > 2 * bound:
            assert ml.read_off(got, ga)[2:] == ml.read_off(want, ga)[2:]


# ---- 4. the table -------------------------------------------------------------------------------------------------------------------------
NT, BT, SEEDT, NS, SW = 300, 128, 17, 21, 2


def table_case():
    """(stat 300 x 9, weight, Gp, Gi, P, (out, ml, null) of the restatement): 12 sets, three sizes four times -- one drawn from
    the top third of list 0, one from its bottom third, two at random -- integer weights, 128 generated placements"""
    if "table" not in _cache:
        rng = np.random.default_rng(4242)
        stat = rng.standard_normal((NT, 9))
        stat[:, 1] = -stat[:, 0]
        weight = np.floor(np.abs(stat) * 1000.0) + 1.0
        order = np.argsort(-stat[:, 0], kind="stable")
        Gp, Gi = [0], []
        for rep in range(4):
            for k in (5, 17, 40):
                pool = (order[:NT // 3], order[-(NT // 3):], np.arange(NT), np.arange(NT))[rep]
                Gi.extend(np.sort(rng.choice(pool, size=k, replace=False)).tolist())
                Gp.append(len(Gi))
        Gp, Gi = np.asarray(Gp, dtype=np.int32), np.asarray(Gi, dtype=np.int32)
        P = ref.placements(NT, BT, SEEDT)
        _cache["table"] = (stat, weight, Gp, Gi, P, ml.table(stat, weight, Gp, Gi, P, SEEDT, er.STD, NS, SW, 1e-50, 10))
    return _cache["table"]


def device_table(ctx, stat, weight, Gp, Gi, **kw):
    args = dict(nperm=BT, seed=SEEDT, null=True, leading_edge=True, sample_size=NS, sweeps=SW, eps=1e-50, ml_min=10)
    args.update(kw)
    return ctx.gsea_multilevel(stat, weight, Gp, Gi, **args)


def same_table(out, mlo, want_out, want_ml, what):
    for q, nm in enumerate(ref.COLUMNS):
        if nm == "padj":
            np.testing.assert_allclose(out[:, q, :], want_out[:, q, :], rtol=1e-15, atol=0, equal_nan=True, err_msg=what)
        else:
            same(out[:, q, :], want_out[:, q, :], f"{what} {nm}")
    for q, nm in enumerate(ml.ML_COLUMNS):
        same(mlo[:, q, :], want_ml[:, q, :], f"{what} {nm}")


@pytest.mark.parametrize("c", [2, 9])
def test_table_against_the_restatement(hip_ctx, c):
    stat, weight, Gp, Gi, P, (want_out, want_ml, want_null) = table_case()
    assert np.array_equal(hip_ctx.gsea_permutations(NT, BT, SEEDT), P)
    out, mlo, null, le_len, le_idx = device_table(hip_ctx, stat[:, :c], weight[:, :c], Gp, Gi)
    same(null, want_null[:, :, :c], "null")
    same_table(out, mlo, want_out[:, :, :c], want_ml[:, :, :c], f"c = {c}")
    used = out[:, 4, :] < 10
    print(f"c = {c}: {int(used.sum())} of {used.size} pairs report pvalML; smallest {np.nanmin(mlo[:, 0, :]):.3e}; "
          f"statuses {sorted(set(mlo[:, 3, :].ravel().tolist()))}")
    assert used.any() and not used.all()
    assert np.array_equal(out[:, 2, :][used], mlo[:, 0, :][used])
    assert np.nanmin(out[:, 2, :]) < 1.0 / (BT + 1)                       # below what the permutations can say
    assert np.array_equal(mlo[:, 5, :], (1.0 + np.where(out[:, 0, :] > 0, out[:, 8, :], out[:, 9, :])) / (1.0 + BT))
    # ml_min = 0: plaidhip_gsea_scored's bits, edges included
    from plaid_amd import engine
    plain = engine._gsea(hip_ctx.lib.plaidhip_gsea_scored, (hip_ctx.handle,), stat[:, :c], weight[:, :c], Gp, Gi, None, BT, SEEDT,
                         True, "std", True)
    out0, ml0, null0, len0, idx0 = device_table(hip_ctx, stat[:, :c], weight[:, :c], Gp, Gi, ml_min=0)
    for a, b, nm in zip((out0, null0, len0, idx0, le_len, le_idx), plain + plain[2:], ("out", "null", "le_len", "le_idx") * 2):
        same(a.astype(np.float64), b.astype(np.float64), f"ml_min = 0 {nm}")
    same(ml0, mlo, "ml_out whatever ml_min")


def test_a_row_does_not_know_the_other_sets(hip_ctx):
    stat, weight, Gp, Gi, P, _ = table_case()
    full = device_table(hip_ctx, stat[:, :2], weight[:, :2], Gp, Gi)
    for pick in ([11, 3, 7, 0], [4], list(range(11, -1, -1)) + [5, 5]):   # dropped and reordered; reordered with one added twice
        gp = np.concatenate([[0], np.cumsum([Gp[j + 1] - Gp[j] for j in pick])]).astype(np.int32)
        gi = np.concatenate([Gi[Gp[j]:Gp[j + 1]] for j in pick]).astype(np.int32)
        out, mlo = device_table(hip_ctx, stat[:, :2], weight[:, :2], gp, gi)[:2]
        keep = [q for q, nm in enumerate(ref.COLUMNS) if nm != "padj"]
        same(out[:, keep, :], full[0][pick][:, keep, :], f"out of the sets {pick}")
        same(mlo, full[1][pick], f"ml_out of the sets {pick}")


# ---- 5. sharding ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nshards", [1, 2, 3, 40])
def test_every_sharding_has_the_one_device_bits(hip_ctx, nshards):
    """2 lists x 2 sides x 3 sizes: at most 12 rulers, so 40 shards leave most without one; 128 permutations are 2 blocks"""
    from tests.helpers import gsea_ml_hooks
    stat, weight, Gp, Gi, P, _ = table_case()
    if "one" not in _cache:
        _cache["one"] = device_table(hip_ctx, stat[:, :2], weight[:, :2], Gp, Gi)
    status, got = gsea_ml_hooks.gsea_multilevel(nshards, stat[:, :2], weight[:, :2], Gp, Gi, nperm=BT, seed=SEEDT, sample_size=NS,
                                               sweeps=SW, eps=1e-50, ml_min=10)
    assert status == 0
    for a, b, nm in zip(got, _cache["one"], ("out", "ml_out", "null", "le_len", "le_idx")):
        same(a.astype(np.float64), b.astype(np.float64), f"{nshards} shards: {nm}")


def test_multi_with_one_device(hip_ctx):
    from plaid_amd import gsea_multilevel_multi
    stat, weight, Gp, Gi, P, _ = table_case()
    if "one" not in _cache:
        _cache["one"] = device_table(hip_ctx, stat[:, :2], weight[:, :2], Gp, Gi)
    got = gsea_multilevel_multi(stat[:, :2], weight[:, :2], Gp, Gi, nperm=BT, seed=SEEDT, null=True, devices=1, leading_edge=True,
                                sample_size=NS, sweeps=SW, eps=1e-50, ml_min=10)
    for a, b, nm in zip(got, _cache["one"], ("out", "ml_out", "null", "le_len", "le_idx")):
        same(a.astype(np.float64), b.astype(np.float64), f"_multi: {nm}")


# ---- 6. argument errors, in their order ---------------------------------------------------------------------------------------------------
def test_argument_errors_in_their_order(hip_ctx):
    import ctypes as C

    from plaid_amd import _lib
    stat, weight, Gp, Gi, P, _ = table_case()
    s, w = np.asfortranarray(stat[:, :2]), np.asfortranarray(weight[:, :2])
    out, mlo = np.zeros((12, 12, 2), order="F"), np.zeros((12, 6, 2), order="F")

    def call(sample=21, sweeps=2, eps=1e-50, ml_min=10, c=2, st=0, nperm=BT, mlp=True, ctx=hip_ctx.handle):
        rc = hip_ctx.lib.plaidhip_gsea_multilevel(ctx, s.ctypes.data, w.ctypes.data, NT, c, Gp.ctypes.data, Gi.ctypes.data, 12, None,
                                                  nperm, 1, st, sample, sweeps, eps, ml_min, out.ctypes.data, None, None, None,
                                                  mlo.ctypes.data if mlp else None)
        try:
            _lib.check(rc)
        except _lib.PlaidHipError as e:
            return e.code, str(e)
        return rc, ""

    # every call is wrong in everything that comes later in the order as well, and on no context: the first wrong argument speaks
    later = dict(nperm=0, st=7, ctx=None)
    for kw, word in [(dict(sample=20, sweeps=0, eps=1.0, ml_min=-1), "sample_size"), (dict(sample=1025, sweeps=0), "sample_size"),
                     (dict(sample=1, sweeps=33), "sample_size"), (dict(sweeps=0, eps=-0.5, ml_min=-1), "sweeps"),
                     (dict(sweeps=33, eps=1.0), "sweeps"), (dict(eps=1.0, ml_min=-1), "eps"), (dict(eps=float("nan"), ml_min=-1), "eps"),
                     (dict(ml_min=-1, c=1 << 30), "ml_min"), (dict(c=1 << 30, mlp=False), "ranked lists"), (dict(mlp=False), "ml_out"),
                     (dict(), "score_type")]:
        rc, text = call(**{**later, **kw})
        assert rc == _lib.EINVAL and word in text, (kw, text)
    rc, text = call(ctx=None)
    assert rc == _lib.EINVAL and "plaidhip_ctx" in text
    with pytest.raises(ValueError, match="sample_size"):
        hip_ctx.gsea_multilevel(s, w, Gp, Gi, nperm=0, sample_size=100)
    with pytest.raises(ValueError, match="sweeps"):
        hip_ctx.gsea_ruler(s[:, 0], w[:, 0], 5, sweeps=0, eps=2.0)
    for kw, word in [(dict(side=2, k=0), "side"), (dict(l=-1, k=0), "list number"), (dict(k=NT), "k ="), (dict(k=0), "k ="),
                     (dict(gamma=float("nan"), score_type=5), "gamma"), (dict(score_type=5), "score_type"),
                     (dict(score_type="pos", side=1), "side")]:
        with pytest.raises(_lib.PlaidHipError, match=word):
            hip_ctx.gsea_ruler(s[:, 0], w[:, 0], **{**dict(k=5), **kw})


# ---- 7. the wrapper ---------------------------------------------------------------------------------------------------------------------------
def test_plaid_gsea_multilevel_end_to_end(hip_ctx):
    import plaid_amd
    from plaid_amd.matrix import NamedMatrix
    stat, weight, Gp, Gi, P, _ = table_case()
    genes = [f"g{i}" for i in range(NT)]
    import scipy.sparse as sp
    # a membership matrix over all 300 genes in their own order: the aligned rows, and so the placements, are the direct call's
    gmt = NamedMatrix(sp.csc_matrix((np.ones(len(Gi)), Gi, Gp), shape=(NT, 12)), genes, [f"set{j}" for j in range(12)])
    kw = dict(nperm=BT, seed=SEEDT, ctx=hip_ctx, sort_by=None)
    plain = plaid_amd.plaid_gsea(dict(zip(genes, stat[:, 0])), gmt, **kw)
    tab = plaid_amd.plaid_gsea(dict(zip(genes, stat[:, 0])), gmt, multilevel=True, sampleSize=NS, sweeps=SW, **kw)
    assert tab.colnames == ["ES", "NES", "pval", "padj", "nMoreExtreme", "size", "log2err"] and tab.rownames == plain.rownames
    W = np.abs(stat[:, :1])
    out, mlo = hip_ctx.gsea_multilevel(stat[:, :1], W, Gp, Gi, nperm=BT, seed=SEEDT, sample_size=NS, sweeps=SW)
    order = [tab.rownames.index(f"set{j}") for j in range(12)]
    same(tab.values[order, :6], out[:, :6, 0], "the table")
    used = out[:, 4, 0] < 10
    assert used.any() and np.array_equal(np.isnan(tab.values[order, 6]), ~used)
    same(tab.values[order, 6][used], mlo[used, 1, 0], "log2err")
    same(tab.values[order][:, [0, 1, 4, 5]], plain.values[order][:, [0, 1, 4, 5]], "what the permutations alone decide")
    assert np.all(tab.values[order, 2][used] <= plain.values[order, 2][used]) and tab.values[order, 2][used].min() < 1.0 / (BT + 1)
    both = plaid_amd.plaid_gsea(NamedMatrix(stat[:, :2], genes, ["a", "b"]), gmt, multilevel=True, sampleSize=NS, sweeps=SW, **kw)
    assert list(both) == ["a", "b"] and both["a"].colnames[-1] == "log2err"
    same(both["a"].values, plaid_amd.plaid_gsea(NamedMatrix(stat[:, :1], genes, ["a"]), gmt, multilevel=True, sampleSize=NS,
                                                sweeps=SW, **kw)["a"].values, "column a of two")
