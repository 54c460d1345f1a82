"""plaid.gsea's score types and leading edges on the device (plaidhip_gsea_scored, gsea_edge_kernel)
against the host restatements of tests/helpers/gsea_edge_ref.py.

Where every partial sum is exact -- weights of 1, integer weights below 2^20 -- out, null_out, le_len and le_idx must have
the bits of the numpy form for std, pos and neg.  For general weights ES lies within (2k + 4) 2^-53 of the rational value
(section 17's bound: (k - 1) roundings in each of cw_t and B, one division, one in miss, one subtraction, on magnitudes
<= 1), and the edge is the rational one wherever no other candidate lies within twice that bound of the extreme.  The
sizes are the seams: N on both sides of a map word, of the 64-word chunk (4097) and across two chunks (8192), 65
permutations (a block of 64 and one more), 1 and 9 lists (the list tile of 8)."""
import os
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import gsea_edge_ref as er
from tests.helpers import gsea_perm_ref as ref

pytestmark = pytest.mark.gpu

B = 65
SEED65, SEED4097 = 31, 31
TYPES = [("std", er.STD), ("pos", er.POS), ("neg", er.NEG)]
_cache = {}


def sets_of(N, seed, extra=()):
    """sets of 1, 2, 63, 64, 65, N / 2 and N - 1 random members and the rows 0, 2, 4, ... (the odd walk positions of a
    decreasing list); extra: further sizes (0 and N for the NaN rules)"""
    Gp, Gi = ref.make_sets(N, [k for k in (1, 2, 63, 64, 65, N // 2, N - 1) if k < N] + list(extra), seed=seed)
    odd = er.odd_positions_set(N)
    return np.append(Gp, Gp[-1] + len(odd)).astype(np.int32), np.concatenate([Gi, odd]).astype(np.int32)


def case(N, weights):
    """(stat, weight, Gp, Gi, P, {score type: reference}) at 9 lists, computed once; a call on the first list alone has the
    reference's first list (the lists do not meet: padj runs over the sets of one list)"""
    key = (N, weights)
    if key not in _cache:
        rng = np.random.default_rng(7000 * N + len(weights))
        stat = np.round(np.clip(rng.normal(size=(N, 9)), -1, 1))          # three levels: the stable order decides
        stat[:, 8] = np.arange(N, 0, -1)                                    # one list in row order: the odd-positions set ties
        w = np.ones((N, 9)) if weights == "one" else rng.integers(0, 2**20, size=(N, 9)).astype(np.float64)
        Gp, Gi = sets_of(N, seed=N)
        P = np.asfortranarray(np.stack([rng.permutation(N) for _ in range(B)], axis=1).astype(np.int32))
        _cache[key] = (stat, w, Gp, Gi, P, er.gsea_scored_ref(stat, w, Gp, Gi, P))
    return _cache[key]


def same(a, b, what=""):
    assert a.shape == b.shape
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    assert not bad.any(), f"{what}: {int(bad.sum())} differ, first at {np.argwhere(bad)[0]}: {a[bad][0]!r} != {b[bad][0]!r}"


def same_but_padj(out, want, what=""):
    """bit for bit, but padj: the library's Benjamini-Hochberg against numpy's, as tests/test_gpu_gsea.py holds it"""
    for q, nm in enumerate(ref.COLUMNS):
        if nm == "padj":
            np.testing.assert_allclose(out[:, q, :], want[:, q, :], rtol=1e-15, atol=0, equal_nan=True, err_msg=what)
        else:
            same(out[:, q, :], want[:, q, :], f"{what} {nm}")


def same_int(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype == np.int32
    bad = a != b
    assert not bad.any(), f"{what}: {int(bad.sum())} differ, first at {np.argwhere(bad)[0]}: {a[bad][0]} != {b[bad][0]}"


def scored(ctx, stat, w, Gp, Gi, st, **kw):
    """(out, null, le_len, le_idx) through plaidhip_gsea_scored whatever the score type (Context.gsea keeps std without edges
    on plaidhip_gsea)"""
    from plaid_amd import engine
    return engine._gsea(ctx.lib.plaidhip_gsea_scored, (ctx.handle,), stat, w, Gp, Gi, kw.get("perm"), kw.get("nperm", B),
                        kw.get("seed", 1), True, st, True)


# ---- 1. exact weights: the bits of the numpy form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("st_name,st", TYPES)
@pytest.mark.parametrize("weights", ["one", "int"])
@pytest.mark.parametrize("N,c", [(65, 1), (65, 9), (4097, 1), (4097, 9), (8192, 1), (8192, 9)])
def test_exact_cases_have_the_bits_of_the_numpy_form(hip_ctx, N, c, weights, st_name, st):
    stat, w, Gp, Gi, P, want = case(N, weights)
    out, null, le_len, le_idx = hip_ctx.gsea(stat[:, :c], w[:, :c], Gp, Gi, perm=P, null=True, score_type=st_name,
                                             leading_edge=True)
    w_out, w_null, w_len, w_idx = want[st]
    same(null, w_null[:, :, :c], "null scores")
    same_but_padj(out, w_out[:, :, :c], f"N={N} c={c} {st_name}")
    same_int(le_len, np.asfortranarray(w_len[:, :c]), "le_len")
    same_int(le_idx, np.asfortranarray(w_idx[:, :c]), "le_idx")
    k = np.diff(Gp)
    for l in range(c):
        for j in range(len(k)):
            seg = le_idx[Gp[j]:Gp[j + 1], l]
            assert 0 <= le_len[j, l] <= k[j] and np.all(seg[le_len[j, l]:] == -1) and np.all(seg[:le_len[j, l]] >= 0)
    if st != er.STD:
        assert np.all(le_len >= 1)                                   # a one-sided edge is never empty


# ---- 2. std is the choice between pos and neg ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,weights", [(65, "int"), (4097, "int"), (8192, "one")])
def test_std_is_the_choice_between_the_pos_and_neg_results(hip_ctx, N, weights):
    stat, w, Gp, Gi, P, _ = case(N, weights)
    o, _, ln, ix = ({nm: hip_ctx.gsea(stat, w, Gp, Gi, perm=P, null=True, score_type=nm, leading_edge=True)[q] for nm, _ in TYPES}
                    for q in range(4))
    ep, en, es = o["pos"][:, 0, :], o["neg"][:, 0, :], o["std"][:, 0, :]
    top, bot = ep > -en, ep < -en
    same(es, np.where(top, ep, np.where(bot, en, 0.0)), "ES_std from ES_pos and ES_neg")
    assert top.any() and bot.any()
    same_int(ln["std"], np.where(top, ln["pos"], np.where(bot, ln["neg"], 0)).astype(np.int32), "std length")
    for l in range(stat.shape[1]):
        for j in range(len(Gp) - 1):
            seg = slice(Gp[j], Gp[j + 1])
            want = ix["pos"][seg, l] if top[j, l] else (ix["neg"][seg, l] if bot[j, l] else np.full(Gp[j + 1] - Gp[j], -1))
            assert np.array_equal(ix["std"][seg, l], want), (j, l)


# ---- 3. std through the new entry is plaidhip_gsea ------------------------------------------------------------------------------
@pytest.mark.parametrize("generated", [False, True])
def test_std_through_the_new_entry_has_the_bits_of_plaidhip_gsea(hip_ctx, generated):
    stat, w, Gp, Gi, P, _ = case(4097, "int")
    stat, w = stat[:, :3], w[:, :3]
    kw = dict(nperm=130, seed=2**40 + 5) if generated else dict(perm=P)
    old, old_null = hip_ctx.gsea(stat, w, Gp, Gi, null=True, **kw)
    new, new_null, _, _ = scored(hip_ctx, stat, w, Gp, Gi, "std", **kw)
    same(new, old, "out")
    same(new_null, old_null, "null_out")
    from plaid_amd import engine
    plain = engine._gsea(hip_ctx.lib.plaidhip_gsea_scored, (hip_ctx.handle,), stat, w, Gp, Gi, kw.get("perm"), kw.get("nperm", B),
                         kw.get("seed", 1), False, "std", False)      # no null_out, no edge buffers
    same(plain, old, "out without the optional buffers")


# ---- 4. the hand-worked cases -------------------------------------------------------------------------------------------------------
def run_decreasing(ctx, N, Gp, Gi, st_name):
    stat = np.arange(N, 0, -1, dtype=np.float64)
    out, le_len, le_idx = ctx.gsea(stat, np.ones(N), np.asarray(Gp, np.int32), np.asarray(Gi, np.int32), nperm=B, seed=3,
                                   score_type=st_name, leading_edge=True)
    return out[:, 0, 0], er.edges_of(le_len, le_idx, Gp)


def test_first_and_last_of_four_on_the_device(hip_ctx):
    for st_name, es, edge in (("std", 0.0, []), ("pos", 0.5, [0]), ("neg", -0.5, [3])):
        got_es, got = run_decreasing(hip_ctx, 4, [0, 2], [0, 3], st_name)
        assert got_es[0] == es and np.signbit(got_es[0]) == (es < 0) and got == [edge], st_name


def test_odd_positions_of_8192_tie_across_lanes_and_chunks_on_the_device(hip_ctx):
    N = 8192
    mem = er.odd_positions_set(N)
    for st_name in ("std", "pos"):
        es, edge = run_decreasing(hip_ctx, N, [0, len(mem)], mem, st_name)
        assert es[0] == 1.0 / 4096.0 and edge == [[0]], st_name       # 4096 equal values in every lane of both chunks: t = 1
    es, edge = run_decreasing(hip_ctx, N, [0, len(mem)], mem, "neg")
    assert es[0] == 0.0 and edge == [list(range(N - 2, -1, -2))]      # all 4096 members, from the end backwards


@pytest.mark.parametrize("N", [65, 4097])
def test_a_set_of_one_gene_on_the_device(hip_ctx, N):
    mid = (N - 1) // 2
    Gp, Gi = [0, 1, 2, 3], [0, mid, N - 1]
    want = {"std": ([1.0, 0.0, -1.0], [[0], [], [N - 1]]), "pos": ([1.0, 0.5, 0.0], [[0], [mid], [N - 1]]),
            "neg": ([0.0, -0.5, -1.0], [[0], [mid], [N - 1]])}
    for st_name, (es, edges) in want.items():
        got_es, got = run_decreasing(hip_ctx, N, Gp, Gi, st_name)
        assert list(got_es) == es and got == edges, st_name


# ---- 5. general weights ------------------------------------------------------------------------------------------------------------
# The seeds are those for which the rational form alone, on the host, shows that no pair is left out
# (gsea_edge_ref.edge_is_decided for every pair and score type).
@pytest.mark.parametrize("N,c,seed", [(65, 9, SEED65), (4097, 1, SEED4097)])
def test_general_weights_within_the_bound_and_the_rational_edge(hip_ctx, N, c, seed):
    rng = np.random.default_rng(seed)
    stat = rng.normal(size=(N, c))
    w = np.abs(rng.normal(size=(N, c)))
    Gp, Gi = sets_of(N, seed=seed)
    P = ref.placements(N, B, seed=seed)
    got = {st: hip_ctx.gsea(stat, w, Gp, Gi, perm=P, null=True, score_type=nm, leading_edge=True) for nm, st in TYPES}
    u = Fraction(1, 2**53)
    pairs = left_out = 0
    for l in range(c):
        pos = ref.observed_placement(stat[:, l])
        Wpos = ref.walk_weights(pos, w[:, l])
        for j in range(len(Gp) - 1):
            mem = Gi[Gp[j]:Gp[j + 1]].astype(np.int64)
            bound = (2 * len(mem) + 4) * u
            ex = er.extremes_fraction(pos, mem, Wpos, gaps=True)
            nul = [er.extremes_fraction(P[:, b], mem, Wpos) for b in range(B)]
            for st in (er.STD, er.POS, er.NEG):
                out, null, le_len, le_idx = got[st]
                assert abs(Fraction(float(out[j, 0, l])) - er.es_of(ex, st, Fraction(0))) <= bound, (st, l, j)
                for b in range(B):
                    assert abs(Fraction(float(null[j, b, l])) - er.es_of(nul[b], st, Fraction(0))) <= bound, (st, l, j, b)
                # NES, pval and nMoreExtreme are the pinned operations on the device's own ES and null scores
                want = er.null_stats(float(out[j, 0, l]), null[j, :, l], st)
                same(out[j, [1, 2, 4], l], want[[1, 2, 4]], "NES / pval / nMoreExtreme")
                pairs += 1
                if not er.edge_is_decided(ex, st, bound):
                    left_out += 1
                    continue
                edge = [int(r) for r in le_idx[Gp[j]:Gp[j] + le_len[j, l], l]]
                assert edge == er.edge_of(ex, pos, mem, st), (st, l, j)
                assert np.all(le_idx[Gp[j] + le_len[j, l]:Gp[j + 1], l] == -1)
    assert left_out == 0 and pairs == 3 * c * (len(Gp) - 1)          # (the issue allows 1 %; these seeds need none)


# ---- 6. sharding -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nshards", [1, 2, 3, 7])
def test_every_sharding_has_the_one_shard_bits(hip_ctx, nshards):
    from plaid_amd import engine
    from tests.helpers.sharded_hooks import _status, hook
    stat, w, Gp, Gi, P, _ = case(4097, "int")                         # 65 permutations: 2 blocks, so 3 and 7 shards exceed them
    stat, w = stat[:, :3], w[:, :3]
    one = hip_ctx.gsea(stat, w, Gp, Gi, perm=P, null=True, score_type="pos", leading_edge=True)
    rc, res = _status(lambda: engine._gsea(hook("gsea_scored"), (0, nshards, -1), stat, w, Gp, Gi, P, B, 1, True, "pos", True))
    assert rc == 0
    same(res[0], one[0], "the 12 columns")
    same(res[1], one[1], "null_out")
    same_int(res[2], one[2], "le_len")
    same_int(res[3], one[3], "le_idx")


# ---- 7. NaN rules ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("st_name,st", TYPES)
def test_nan_pairs_have_no_edge_and_leave_the_others_untouched(hip_ctx, st_name, st):
    N, c = 65, 3
    key = ("nan", N)
    if key not in _cache:
        rng = np.random.default_rng(77)
        stat = np.round(np.clip(rng.normal(size=(N, c)), -1, 1))
        w = rng.integers(0, 2**20, size=(N, c)).astype(np.float64)
        Gp, Gi = sets_of(N, seed=78, extra=(0, N))
        P = ref.placements(N, B, seed=79)
        _cache[key] = (stat, w, Gp, Gi, P, er.gsea_scored_ref(stat, w, Gp, Gi, P))
    stat, w, Gp, Gi, P, want = _cache[key]
    k = np.diff(Gp)
    nanset = (k == 0) | (k == N)
    assert nanset.sum() == 2
    for bad in (None, np.nan, np.inf):
        s2 = stat.copy()
        if bad is not None:
            s2[7, 1] = bad
        out, null, le_len, le_idx = hip_ctx.gsea(s2, w, Gp, Gi, perm=P, null=True, score_type=st_name, leading_edge=True)
        cols = [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11]
        assert np.isnan(out[nanset][:, cols, :]).all() and np.all(le_len[nanset, :] == 0)
        for j in np.flatnonzero(nanset):
            assert np.all(le_idx[Gp[j]:Gp[j + 1], :] == -1)
        assert np.all((le_idx >= -1) & (le_idx < N))                  # every slot was written
        if bad is not None:
            assert np.isnan(out[:, cols, 1]).all() and np.isnan(null[:, :, 1]).all()
            assert np.all(le_len[:, 1] == 0) and np.all(le_idx[:, 1] == -1)
            assert np.array_equal(out[:, 5, 1], k.astype(np.float64))
        for l in ((0, 2) if bad is not None else (0, 1, 2)):
            same_but_padj(out[:, :, l:l + 1], want[st][0][:, :, l:l + 1])
            same(null[:, :, l], want[st][1][:, :, l])
            same_int(np.ascontiguousarray(le_len[:, l]), np.ascontiguousarray(want[st][2][:, l]), "le_len")
            same_int(np.ascontiguousarray(le_idx[:, l]), np.ascontiguousarray(want[st][3][:, l]), "le_idx")


# ---- 8. argument errors, in the stated order, before any device work -------------------------------------------------------------
def test_argument_errors_come_in_the_stated_order(hip_ctx):
    import plaid_amd
    from plaid_amd import _lib
    stat, w, Gp, Gi, P, _ = case(65, "one")
    st, wt = np.asfortranarray(stat[:, :3]), np.asfortranarray(w[:, :3])
    m = len(Gp) - 1
    lib = hip_ctx.lib
    out = np.full((m, 12, 3), -7.0, order="F")
    le_len = np.full((m, 3), -7, dtype=np.int32, order="F")
    le_idx = np.full((int(Gp[-1]), 3), -7, dtype=np.int32, order="F")

    def call(score_type, ln, ix, nperm=10, c=3, weight=wt, ctx=None):
        """without a context: every argument check comes before the context is looked at, so nothing can have been launched"""
        rc = lib.plaidhip_gsea_scored(ctx, st.ctypes.data, weight.ctypes.data, 65, c, Gp.ctypes.data, Gi.ctypes.data, m, None, nperm,
                                      1, score_type, out.ctypes.data, None, None if ln is None else ln.ctypes.data,
                                      None if ix is None else ix.ctypes.data)
        return rc, lib.plaidhip_last_error_string()

    wneg = wt.copy()
    wneg[3, 2] = -1.0
    for bad_type in (-1, 3):          # 1. the score type, whatever else is wrong
        rc, msg = call(bad_type, le_len, None, nperm=0, c=0, weight=wneg)
        assert rc == _lib.EINVAL and b"score_type" in msg
    for ln, ix in ((le_len, None), (None, le_idx)):     # 2. one edge buffer without the other
        rc, msg = call(1, ln, ix, nperm=0, c=0, weight=wneg)
        assert rc == _lib.EINVAL and b"le_len and le_idx" in msg
    rc, msg = call(1, le_len, le_idx, nperm=0, c=0, weight=wneg)      # 3. then the existing order: nperm, c, the genes, a weight
    assert rc == _lib.EINVAL and b"nperm" in msg
    rc, msg = call(1, le_len, le_idx, c=0, weight=wneg)
    assert rc == _lib.EINVAL and b"ranked lists" in msg
    rc, msg = call(1, le_len, le_idx, weight=wneg)
    assert rc == _lib.EINVAL and b"weight" in msg
    rc, msg = call(2, le_len, le_idx)                                  # all arguments good: only the context is missing
    assert rc == _lib.EINVAL and b"null plaidhip_ctx" in msg
    assert np.all(out == -7.0) and np.all(le_len == -7) and np.all(le_idx == -7)          # nothing was written
    with pytest.raises(ValueError, match="score_type"):
        hip_ctx.gsea(stat, w, Gp, Gi, perm=P, score_type="both")
    with pytest.raises(plaid_amd.PlaidHipError, match="score_type") as e:
        hip_ctx.gsea(stat, w, Gp, Gi, perm=P, score_type=3)            # the library's own check, with a context
    assert e.value.code == _lib.EINVAL
    rc, _ = call(2, le_len, le_idx, ctx=hip_ctx.handle)                # and the good call runs
    assert rc == 0 and not np.any(le_len == -7) and not np.any(le_idx == -7)


# ---- 9. end to end -------------------------------------------------------------------------------------------------------------------
def test_plaid_gsea_with_leading_edges_on_the_vignette_fixture(hip_ctx, pbmc, golden_dir):
    import scipy.sparse as sp

    import plaid_amd
    d, _ = pbmc
    X = sp.csc_matrix((d["x"], d["i"], d["p"]), shape=tuple(d["dim"])).toarray()
    rn = [str(r) for r in d["rownames"]]
    y = d["celltype"] == "B"
    fc = X[:, y].mean(axis=1) - X[:, ~y].mean(axis=1)
    gmt = plaid_amd.read_gmt(os.path.join(golden_dir, "hallmarks.gmt"))
    matG = plaid_amd.gmt2mat(gmt)
    kw = dict(nperm=130, seed=4242, minSize=15, maxSize=150, ctx=hip_ctx)
    stats = plaid_amd.NamedMatrix(np.stack([fc, np.abs(fc)], axis=1), rn, ["B_vs_rest", "abs"])
    value = {nm: {g: v for g, v in reversed(list(zip(rn, stats.values[:, l])))} for l, nm in enumerate(stats.colnames)}   # first of a name
    in_x = set(rn)
    Gd = sp.csc_matrix(matG.values)
    aligned = {nm: {matG.rownames[r] for r in Gd.indices[Gd.indptr[j]:Gd.indptr[j + 1]]} & in_x
               for j, nm in enumerate(matG.colnames)}
    plain = plaid_amd.plaid_gsea(stats, matG, **kw)
    for st_name in ("std", "pos", "neg"):
        res = plaid_amd.plaid_gsea(stats, matG, scoreType=st_name, leadingEdge=True, **kw)
        assert list(res) == ["B_vs_rest", "abs"]
        for nm, (tab, edges) in res.items():
            assert tab.colnames == ["ES", "NES", "pval", "padj", "nMoreExtreme", "size"] and len(edges) == len(tab.rownames) > 0
            assert np.all(np.diff(tab.values[:, 2]) >= 0)            # the table is sorted by pval, and the edges with it
            if st_name == "std":                                      # the table is the one returned without edges
                assert tab.rownames == plain[nm].rownames and np.array_equal(tab.values, plain[nm].values, equal_nan=True)
            for row, (sname, edge) in enumerate(zip(tab.rownames, edges)):
                assert 15 <= tab.values[row, 5] <= 150                # the size filter applies
                assert set(edge) <= aligned[sname] and len(set(edge)) == len(edge) <= tab.values[row, 5]
                v = [value[nm][gname] for gname in edge]
                if st_name == "pos":
                    assert len(edge) >= 1 and all(a >= b for a, b in zip(v, v[1:]))      # decreasing statistic
                if st_name == "neg":
                    assert len(edge) >= 1 and all(a <= b for a, b in zip(v, v[1:]))
                if st_name == "std" and tab.values[row, 0] != 0.0:
                    assert len(edge) >= 1 and (all(a >= b for a, b in zip(v, v[1:])) if tab.values[row, 0] > 0
                                               else all(a <= b for a, b in zip(v, v[1:])))
    # a named vector gives one (table, edges); sorted by another column, every row still has its own set's edge
    fcv = {nm: v for nm, v in reversed(list(zip(rn, fc)))}
    by_nes, e_nes = plaid_amd.plaid_gsea(fcv, matG, scoreType="pos", leadingEdge=True, sort_by="NES", **kw)
    by_pval, e_pval = plaid_amd.plaid_gsea(fcv, matG, scoreType="pos", leadingEdge=True, **kw)
    edge_of_set = dict(zip(by_pval.rownames, e_pval))
    assert np.all(np.diff(by_nes.values[:, 1]) >= 0) and by_nes.rownames != by_pval.rownames
    assert all(edge_of_set[s] == e for s, e in zip(by_nes.rownames, e_nes))
