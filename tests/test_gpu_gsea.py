"""plaid.gsea on the device (plaidhip_gsea, kernels_gsea.hip) against the host restatements of
tests/helpers/gsea_perm_ref.py.

Where every partial sum is exact -- weights of 1, integer weights below 2^20 -- the null matrix, ES, the four counts, the
two sums, NES and pval must have the bits of the numpy form.  For general weights every score lies within (2k + 4) 2^-53 of
the rational value ((k - 1) roundings in each of cw_t and B, one division, one in miss, one subtraction, on values of
magnitude <= 1), the counts are the rational counts (the inputs are chosen so that no null score lies within twice that
bound of its ES) and the sums lie within (B + 2k + 4) 2^-53 sum |es_b|.  The shapes sit on the map-word and scan-step seams
of N, the block seams of B and the list tile."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import gsea_perm_ref as ref

pytestmark = pytest.mark.gpu

COLS = ref.COLUMNS
SHAPES = [(64, 1, 1), (65, 63, 3), (4096, 64, 1), (4097, 65, 9), (8193, 130, 3)]      # N, B, c
GENERAL = [(4097, 65, 3, 21), (8193, 130, 1, 21)]                                      # N, B, c, seed: general weights
_cache = {}


def sizes(N):
    return (0, 1, 2, 63, 64, 65, N - 1, N)


def same(a, b, what=""):
    assert a.shape == b.shape
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    assert not bad.any(), f"{what}: {int(bad.sum())} differ, first at {np.argwhere(bad)[0]}: {a[bad][0]!r} != {b[bad][0]!r}"


def same_but_padj(out, want, what=""):
    for q, nm in enumerate(COLS):
        if nm == "padj":
            np.testing.assert_allclose(out[:, q, :], want[:, q, :], rtol=1e-15, atol=0, equal_nan=True, err_msg=what)
        else:
            same(out[:, q, :], want[:, q, :], f"{what} {nm}")


def case(N, B, c, weights, ties):
    """(stat, weight, Gp, Gi, P, reference out, reference null), computed once"""
    key = (N, B, c, weights, ties)
    if key not in _cache:
        rng = np.random.default_rng(1000 * N + 10 * B + c)
        stat = rng.normal(size=(N, c))
        if ties:
            stat = np.round(np.clip(stat, -1, 1))          # three levels: the stable order decides
        if weights == "one":
            w = np.ones((N, c))
        else:
            w = rng.integers(0, 2**20, size=(N, c)).astype(np.float64)
        Gp, Gi = ref.make_sets(N, sizes(N), seed=N + B)
        P = np.asfortranarray(np.stack([rng.permutation(N) for _ in range(B)], axis=1).astype(np.int32))
        _cache[key] = (stat, w, Gp, Gi, P) + ref.gsea_ref(stat, w, Gp, Gi, P)
    return _cache[key]


@pytest.mark.parametrize("N,B,c", SHAPES)
@pytest.mark.parametrize("weights,ties", [("one", False), ("one", True), ("int", True)])
def test_exact_cases_have_the_bits_of_the_numpy_form(hip_ctx, N, B, c, weights, ties):
    stat, w, Gp, Gi, P, want, want_null = case(N, B, c, weights, ties)
    out, null = hip_ctx.gsea(stat, w, Gp, Gi, perm=P, null=True)
    same(null, want_null, "null scores")
    same_but_padj(out, want, f"N={N} B={B} c={c}")
    k = np.diff(Gp)
    assert np.array_equal(out[:, 5, 0], k.astype(np.float64))
    assert np.isnan(out[(k == 0) | (k == N)][:, [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11], :]).all()


def test_first_and_last_of_four_is_exactly_zero_and_null_ties_are_counted(hip_ctx):
    N, B = 4, 130
    stat = np.array([4.0, 3.0, 2.0, 1.0])
    w = np.ones(N)
    Gp, Gi = np.array([0, 2, 3, 5], dtype=np.int32), np.array([0, 3, 1, 1, 2], dtype=np.int32)
    P = ref.placements(N, B, seed=5)
    out, null = hip_ctx.gsea(stat, w, Gp, Gi, perm=P, null=True)
    want, want_null = ref.gsea_ref(stat, w, Gp, Gi, P)
    assert out[0, 0, 0] == 0.0 and not np.signbit(out[0, 0, 0])
    same(null, want_null)
    same_but_padj(out, want)
    for j in range(3):      # null scores that tie with ES: the >= and <= counts overlap
        ties = np.sum(null[j, :, 0] == out[j, 0, 0])
        assert ties > 0 and out[j, 6, 0] + out[j, 7, 0] == B + ties


def test_zero_weight_sets_follow_the_unweighted_rule(hip_ctx):
    """Half of every list's weights are 0 and the sets have one to three members, so B == 0 is common among the observed
    and the null pairs alike: on a list that is not the last of its tile (the map stays set) and on the last (the fallback
    walk clears it).  The weights are integers, so the numpy form is exact."""
    N, B, c = 130, 65, 3
    rng = np.random.default_rng(8)
    stat = rng.normal(size=(N, c))
    w = rng.integers(1, 1000, size=(N, c)).astype(np.float64)
    w[rng.random(size=(N, c)) < 0.5] = 0.0
    ks = [1, 2, 3] * 4
    Gp = np.concatenate([[0], np.cumsum(ks)]).astype(np.int32)
    Gi = np.concatenate([np.sort(rng.choice(N, size=k, replace=False)) for k in ks]).astype(np.int32)
    P = ref.placements(N, B, seed=9)
    # a condition on the input: every list has observed and null pairs with B == 0 and with B > 0
    for l in range(c):
        pos = ref.observed_placement(stat[:, l])
        Wpos = ref.walk_weights(pos, w[:, l])
        obs = np.array([Wpos[pos[Gi[Gp[j]:Gp[j + 1]]]].sum() for j in range(len(ks))])
        nul = np.array([[Wpos[P[Gi[Gp[j]:Gp[j + 1]], b]].sum() for b in range(B)] for j in range(len(ks))])
        assert (obs == 0).any() and (obs > 0).any(), l
        assert (nul == 0).sum() >= 20 and (nul > 0).sum() >= 20, l
        assert all((nul[j] == 0).any() and (nul[j] > 0).any() for j in range(len(ks)) if ks[j] > 1), l   # inside one block
    out, null = hip_ctx.gsea(stat, w, Gp, Gi, perm=P, null=True)
    want, want_null = ref.gsea_ref(stat, w, Gp, Gi, P)
    same(null, want_null)
    same_but_padj(out, want)
    # where B == 0 the pair is the unweighted walk of the same placement
    ones, ones_null = ref.gsea_ref(stat, np.ones((N, c)), Gp, Gi, P)
    for l in range(c):
        pos = ref.observed_placement(stat[:, l])
        Wpos = ref.walk_weights(pos, w[:, l])
        for j in range(len(ks)):
            mem = Gi[Gp[j]:Gp[j + 1]]
            if Wpos[pos[mem]].sum() == 0:
                assert out[j, 0, l] == ones[j, 0, l]
            for b in range(B):
                if Wpos[P[mem, b]].sum() == 0:
                    assert null[j, b, l] == ones_null[j, b, l]


# (a set of one gene scores 1 - miss whatever its weight: N values in all, so at N = 65 some null score always meets its ES
# and the condition below cannot hold; the family takes the two larger seams)
@pytest.mark.parametrize("N,B,c,seed", GENERAL)
def test_general_weights_within_the_rounding_bound_of_the_rational_value(hip_ctx, N, B, c, seed):
    rng = np.random.default_rng(seed)
    stat = rng.normal(size=(N, c))
    w = np.abs(rng.normal(size=(N, c)))
    Gp, Gi = ref.make_sets(N, sizes(N), seed=seed)
    P = ref.placements(N, B, seed=seed)
    out, null = hip_ctx.gsea(stat, w, Gp, Gi, perm=P, null=True)
    u = Fraction(1, 2**53)
    for l in range(c):
        pos = ref.observed_placement(stat[:, l])
        Wpos = ref.walk_weights(pos, w[:, l])
        for j in range(len(Gp) - 1):
            mem = Gi[Gp[j]:Gp[j + 1]].astype(np.int64)
            k = len(mem)
            es = ref.es_fraction(pos, mem, Wpos)
            if es is None:
                assert np.isnan(out[j, [0, 1, 2, 4], l]).all() and np.isnan(null[j, :, l]).all()
                continue
            bound = (2 * k + 4) * u
            nul = [ref.es_fraction(P[:, b], mem, Wpos) for b in range(B)]
            # a condition on the input, which holds for these seeds: no null score within twice the bound of its ES
            assert all(abs(e - es) > 2 * bound for e in nul), (l, j)
            assert abs(Fraction(float(out[j, 0, l])) - es) <= bound, (l, j)
            for b in range(B):
                assert abs(Fraction(float(null[j, b, l])) - nul[b]) <= bound, (l, j, b)
            counts = [sum(e >= es for e in nul), sum(e <= es for e in nul), sum(e >= 0 for e in nul), sum(e <= 0 for e in nul)]
            assert list(out[j, 6:10, l]) == [float(x) for x in counts], (l, j)
            tot = sum(abs(e) for e in nul)
            sbound = (B + 2 * k + 4) * u * tot
            assert abs(Fraction(float(out[j, 10, l])) - sum(e for e in nul if e > 0)) <= sbound
            assert abs(Fraction(float(out[j, 11, l])) - sum(e for e in nul if e < 0)) <= sbound
            # NES, pval and nMoreExtreme are the pinned operations on the device's own partials
            want = ref.null_stats(float(out[j, 0, l]), null[j, :, l])
            same(out[j, [1, 2, 4], l], want[[1, 2, 4]], "NES / pval / nMoreExtreme")


@pytest.mark.parametrize("g", [65, 4097, 20353])
def test_generated_placements_are_the_restated_ones(hip_ctx, g):
    B = 65
    P = hip_ctx.gsea_permutations(g, B, seed=2**35 + 11)
    assert np.array_equal(P, ref.placements(g, B, seed=2**35 + 11))


def test_perm_null_equals_the_entry_fed_its_own_placements(hip_ctx):
    N, B, c = 4097, 130, 3
    stat, w, Gp, Gi, _, _, _ = case(N, 65, 9, "int", True)
    stat, w = stat[:, :c], w[:, :c]
    seed = 2**63 + 12345
    P = hip_ctx.gsea_permutations(N, B, seed=seed)
    a, na = hip_ctx.gsea(stat, w, Gp, Gi, nperm=B, seed=seed, null=True)
    b, nb = hip_ctx.gsea(stat, w, Gp, Gi, perm=P, null=True)
    same(a, b)
    same(na, nb)
    assert np.array_equal(a, hip_ctx.gsea(stat, w, Gp, Gi, nperm=B, seed=seed), equal_nan=True)       # without null_out
    assert not np.array_equal(na, hip_ctx.gsea(stat, w, Gp, Gi, nperm=B, seed=seed + 1, null=True)[1], equal_nan=True)


@pytest.mark.parametrize("nshards", [1, 2, 3, 7, 9])
@pytest.mark.parametrize("generated", [False, True])
def test_every_sharding_has_the_one_shard_bits(hip_ctx, nshards, generated):
    from tests.helpers.gsea_hooks import gsea
    N, B, c = 4097, 130 if generated else 65, 3       # 3 blocks of permutations, or 2: 7 and 9 shards are more than blocks
    stat, w, Gp, Gi, P, _, _ = case(4097, 65, 9, "int", True)
    stat, w = stat[:, :c], w[:, :c]
    kw = dict(nperm=B, seed=77) if generated else dict(perm=P)
    one, one_null = hip_ctx.gsea(stat, w, Gp, Gi, null=True, **kw)
    rc, res = gsea(nshards, stat, w, Gp, Gi, **kw)
    assert rc == 0
    same(res[0], one, "the 12 columns")
    same(res[1], one_null, "null_out")


def test_a_failing_shard_returns_an_error(hip_ctx):
    from tests.helpers.gsea_hooks import gsea
    stat, w, Gp, Gi, P, _, _ = case(65, 63, 3, "one", False)
    rc, res = gsea(2, stat, w, Gp, Gi, perm=P, fail=1)
    assert rc != 0 and res is None


def test_nan_list_is_nan_and_leaves_the_others_untouched(hip_ctx):
    stat, w, Gp, Gi, P, want, want_null = case(65, 63, 3, "int", True)
    for bad in (np.nan, np.inf):
        s2 = stat.copy()
        s2[7, 1] = bad
        out, null = hip_ctx.gsea(s2, w, Gp, Gi, perm=P, null=True)
        assert np.isnan(out[:, [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11], 1]).all() and np.isnan(null[:, :, 1]).all()
        assert np.array_equal(out[:, 5, 1], np.diff(Gp).astype(np.float64))
        for l in (0, 2):
            same_but_padj(out[:, :, l:l + 1], want[:, :, l:l + 1])
            same(null[:, :, l], want_null[:, :, l])


def test_argument_errors(hip_ctx):
    import plaid_amd
    from plaid_amd import _lib
    stat, w, Gp, Gi, P, _, _ = case(65, 63, 3, "one", False)
    P2 = P.copy()
    P2[5, 40] = P2[6, 40]                                   # a duplicate in one column
    with pytest.raises(plaid_amd.PlaidHipError, match="column 40 of perm") as e:
        hip_ctx.gsea(stat, w, Gp, Gi, perm=P2)
    assert e.value.code == _lib.EINVAL
    P2 = P.copy()
    P2[0, 0] = 65
    with pytest.raises(plaid_amd.PlaidHipError, match="column 0 of perm"):
        hip_ctx.gsea(stat, w, Gp, Gi, perm=P2)
    # the library's own checks, past the wrapper's: a negative weight, nperm < 1, c < 1, then the map bound
    lib = hip_ctx.lib
    out = np.zeros((len(Gp) - 1, 12, 3), order="F")

    def call(stat, w, g, c, nperm):
        return lib.plaidhip_gsea(hip_ctx.handle, stat.ctypes.data, w.ctypes.data, g, c, Gp.ctypes.data, Gi.ctypes.data, len(Gp) - 1,
                                 None, nperm, 1, out.ctypes.data, None)

    wneg = np.asfortranarray(w.copy())
    wneg[3, 2] = -1.0
    st = np.asfortranarray(stat)
    assert call(st, wneg, 65, 3, 10) == _lib.EINVAL and b"weight" in lib.plaidhip_last_error_string()
    assert call(st, np.asfortranarray(w), 65, 3, 0) == _lib.EINVAL
    assert call(st, np.asfortranarray(w), 65, 0, 10) == _lib.EINVAL
    big = np.zeros((131073, 1), order="F")
    assert call(big, big + 1.0, 131073, 1, 10) == _lib.EUNSUPPORTED
    assert lib.plaidhip_gsea(None, big.ctypes.data, big.ctypes.data, 131073, 1, Gp.ctypes.data, Gi.ctypes.data, len(Gp) - 1, None,
                             10, 1, out.ctypes.data, None) == _lib.EUNSUPPORTED      # before the context is looked at


def test_plaid_gsea_end_to_end_on_the_vignette_fixture(hip_ctx, pbmc, golden_dir):
    import scipy.sparse as sp

    import plaid_amd
    d, _ = pbmc
    X = sp.csc_matrix((d["x"], d["i"], d["p"]), shape=tuple(d["dim"])).toarray()
    rn = [str(r) for r in d["rownames"]]
    y = d["celltype"] == "B"
    fc = X[:, y].mean(axis=1) - X[:, ~y].mean(axis=1)
    gmt = plaid_amd.read_gmt(os.path.join(golden_dir, "hallmarks.gmt"))
    matG = plaid_amd.gmt2mat(gmt)
    B, seed = 130, 4242
    stats = plaid_amd.NamedMatrix(np.stack([fc, -fc], axis=1), rn, ["B_vs_rest", "rest_vs_B"])
    res = plaid_amd.plaid_gsea(stats, matG, nperm=B, seed=seed, minSize=15, maxSize=150, ctx=hip_ctx)
    assert list(res) == ["B_vs_rest", "rest_vs_B"]
    # the alignment by name and the size filter, restated
    posx = {nm: k for k, nm in reversed(list(enumerate(rn)))}
    gg = [nm for nm in dict.fromkeys(matG.rownames) if nm in posx]
    xrow = np.array([posx[nm] for nm in gg])
    col = {nm: k for k, nm in enumerate(gg)}
    Gd = sp.csc_matrix(matG.values)
    sets, Gp, Gi = [], [0], []
    for j, nm in enumerate(matG.colnames):
        rows = Gd.indices[Gd.indptr[j]:Gd.indptr[j + 1]]
        mem = sorted(col[matG.rownames[r]] for r in rows if matG.rownames[r] in col)
        if 15 <= len(mem) <= 150:
            sets.append(nm)
            Gi.extend(mem)
            Gp.append(len(Gi))
    assert 0 < len(sets) < matG.shape[1]                         # some sets are dropped
    N = len(gg)
    P = ref.placements(N, B, seed)
    for l, nm in enumerate(res):
        tab = res[nm]
        assert tab.colnames == ["ES", "NES", "pval", "padj", "nMoreExtreme", "size"]
        assert sorted(tab.rownames) == sorted(sets)
        assert np.all(np.diff(tab.values[:, 2]) >= 0)            # sorted by pval
        st = stats.values[xrow, l]
        want, _ = ref.gsea_ref(st, np.abs(st), np.array(Gp), np.array(Gi), P)
        o = [sets.index(s) for s in tab.rownames]
        got = tab.values
        assert np.array_equal(got[:, 5], want[o, 5, 0]) and np.array_equal(got[:, 4], want[o, 4, 0])
        np.testing.assert_allclose(got[:, 0], want[o, 0, 0], rtol=0, atol=2 * (2 * 150 + 4) * 2.0**-53)   # each within the bound of the rational
        assert np.array_equal(got[:, 2], want[o, 2, 0])          # the counts, hence pval, are those of the numpy form
        assert np.array_equal(got[:, 3], ref.bh(got[:, 2]))      # padj is a numpy BH of the table's own p-values
        np.testing.assert_allclose(got[:, 1], want[o, 1, 0], rtol=1e-12)
    # one list; sort_by another column
    one = plaid_amd.plaid_gsea(plaid_amd.NamedMatrix(fc, rn, ["fc"]), matG, nperm=B, seed=seed, minSize=15, maxSize=150,
                               sort_by="NES", ctx=hip_ctx)
    assert list(one) == ["fc"] and np.all(np.diff(one["fc"].values[:, 1]) >= 0)
    assert sorted(one["fc"].rownames) == sorted(sets)
