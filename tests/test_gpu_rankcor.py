"""plaid.rankcor on the device (plaidhip_rankcor, kernels_rankcor.hip) against the host restatements of
tests/helpers/rankcor_ref.py.

Rank mode is exact integers up to one pinned fp64 epilogue: size is equal, rho and t have the bits of rankcor_form on
scipy's ranks, p the bits of the library's own pnorm_upper at that t, for all three ties methods; q is within rtol 1e-15 of
the Benjamini-Hochberg restatement.  Value mode lies within the derived forward bound (ValueList.bound) of exact rational
arithmetic; its t and p are the pinned operations on the call's own rho.  The shapes sit on the 64-member pass of the gather
kernel and its unrolled pair (sets of 0, 1, 63, 64, 65, 129, g - 1 and g members of g = 1,500 genes: six workgroups of the pack
kernel), on the list tile of 8 and its remainders (c = 1, 7, 8, 9, 17), and one case lies past the LDS-resident rank kernel
(g = 20,480).  The lists: tie-free, five-valued, constant and holding +-Inf; without NaN, with 10 % NaN, all but two NaN and
all NaN."""
import math
import os

import mpmath
import numpy as np
import pytest

from plaid_amd import _lib, engine
from tests.helpers import rankcor_ref as ref
from tests.helpers.sharded_hooks import _status, hook

pytestmark = pytest.mark.gpu

G = 1500
LISTS = (1, 7, 8, 9, 17)
# (values, missing) of column l % 13: every kind of list with every kind of missingness that means something for it
KINDS = [("free", "none"), ("five", "tenth"), ("const", "none"), ("inf", "none"), ("free", "tenth"), ("five", "but2"),
         ("free", "all"), ("five", "none"), ("inf", "tenth"), ("const", "tenth"), ("free", "but2"), ("offset", "tenth"),
         ("five", "but2same")]
_cache = {}


def same(a, b, what=""):
    assert a.shape == b.shape
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    assert not bad.any(), f"{what}: {int(bad.sum())} differ, first at {np.argwhere(bad)[0]}: {a[bad][0]!r} != {b[bad][0]!r}"


def make_list(g, kind, missing, rng):
    if kind == "free":
        x = rng.permutation(g).astype(np.float64) * 0.37 - 11.0
    elif kind == "five":
        x = rng.integers(-2, 3, size=g).astype(np.float64)       # (0 among them: -0.0 is planted below)
        x[np.flatnonzero(x == 0)[::2]] = -0.0
    elif kind == "const":
        x = np.full(g, 2.5)
    elif kind == "offset":
        x = 1000.0 + rng.normal(size=g)
    else:
        x = rng.normal(size=g)
        x[rng.choice(g, size=6, replace=False)] = [np.inf, np.inf, -np.inf, np.inf, -np.inf, -np.inf]
    if missing == "tenth":
        x[rng.random(g) < 0.1] = np.nan
    elif missing in ("but2", "but2same"):
        keep = rng.choice(g, size=2, replace=False)
        y = np.full(g, np.nan)
        y[keep] = x[keep] if missing == "but2" else 1.0
        if missing == "but2" and y[keep[0]] == y[keep[1]]:
            y[keep[0]] += 1.0
        x = y
    elif missing == "all":
        x = np.full(g, np.nan)
    return x


def case(g, c):
    """(stat, kinds, Gp, Gi), computed once: column l is of kind KINDS[(l + c) % 13]; the members of a set are in drawn
    (unsorted) order; the set of all but one gene and the set of 63 leave out / hold the two genes of a "but2" list often
    enough by chance to matter little: k = 0, 1 and 2 of n = 2 all occur over the sets of sizes 0, 1, ..., g"""
    if (g, c) not in _cache:
        rng = np.random.default_rng(100 * g + c)
        kinds = [KINDS[(l + c) % len(KINDS)] for l in range(c)]
        stat = np.asfortranarray(np.column_stack([make_list(g, k, mi, rng) for k, mi in kinds]))
        Gp, Gi = ref.make_sets(g, (0, 1, 63, 64, 65, 129, g - 1, g), seed=g + c)
        Gi = Gi.copy()
        for j in range(len(Gp) - 1):
            rng.shuffle(Gi[Gp[j]:Gp[j + 1]])
        _cache[(g, c)] = (stat, kinds, Gp, Gi)
    return _cache[(g, c)]


def rank_reference(g, c, ties):
    key = (g, c, ties)
    if key not in _cache:
        stat, _, Gp, Gi = case(g, c)
        _cache[key] = ref.rankcor_ref(stat, Gp, Gi, ties, ref.library_pnorm_upper())
    return _cache[key]


def check_rank_result(got, want, what):
    (out, tot), (wout, wtot) = got, want
    assert np.array_equal(tot, wtot), what
    for q, nm in enumerate(ref.COLUMNS):
        if nm == "q.value":
            np.testing.assert_allclose(out[:, q, :], wout[:, q, :], rtol=1e-15, atol=0, equal_nan=True, err_msg=f"{what} {nm}")
        else:
            same(out[:, q, :], wout[:, q, :], f"{what} {nm}")


@pytest.mark.parametrize("ties", ["average", "min", "max"])
@pytest.mark.parametrize("c", LISTS)
def test_rank_mode_has_the_bits_of_the_pinned_form(hip_ctx, c, ties):
    stat, kinds, Gp, Gi = case(G, c)
    got = hip_ctx.rankcor(stat, Gp, Gi, use_rank=True, ties=ties)
    check_rank_result(got, rank_reference(G, c, ties), f"c={c} {ties}")
    out, tot = got
    for l, (kind, missing) in enumerate(kinds):                  # the NaN rules, restated
        n = int(tot[l])
        assert n == int((~np.isnan(stat[:, l])).sum())
        k = out[:, 0, l]
        dead = (k == 0) | (k == n) | (kind == "const") | (n <= 1) | (missing == "but2same")
        assert np.isnan(out[dead, 1:, l]).all(), (l, kind, missing)
        assert not np.isnan(out[~dead, 1, l]).any(), (l, kind, missing)
        if n <= 2:
            assert np.isnan(out[:, 2:, l]).all()
        else:
            assert not np.isnan(out[~dead, 2:, l]).any()
        if kind == "inf" and missing == "none":                 # an infinity is an ordinary value to a rank
            assert not np.isnan(out[1:-1, 1:, l]).any()


@pytest.mark.parametrize("c", LISTS)
def test_value_mode_is_within_the_derived_bound_of_exact_arithmetic(hip_ctx, c):
    stat, kinds, Gp, Gi = case(G, c)
    out, tot = hip_ctx.rankcor(stat, Gp, Gi, use_rank=False)
    pn = ref.library_pnorm_upper()
    m = len(Gp) - 1
    checked, worst = 0, 0.0
    for l, (kind, missing) in enumerate(kinds):
        x = stat[:, l]
        ok = ~np.isnan(x)
        n = int(ok.sum())
        assert tot[l] == n
        for j in range(m):
            assert out[j, 0, l] == int(ok[Gi[Gp[j]:Gp[j + 1]]].sum())     # size is the members in V, NaN list or not
        if kind in ("inf", "const") or missing == "but2same" or n <= 1:
            assert np.isnan(out[:, 1:, l]).all(), (l, kind, missing)
            continue
        L = ref.ValueList(x)
        for j in range(m):
            rho, t, p = (float(v) for v in out[j, 1:4, l])
            exact, k = L.exact(Gi[Gp[j]:Gp[j + 1]])
            if exact is None:
                assert rho != rho and t != t and p != p, (l, j, kind, missing)
                continue
            bound, rel = L.bound(Gi[Gp[j]:Gp[j + 1]])
            assert rel < 2.0**-20
            with mpmath.workdps(50):
                err = float(abs(mpmath.mpf(rho) - exact))
            assert err <= float(bound), (l, j, kind, missing, rho, err, float(bound))
            worst = max(worst, err / float(bound))
            want_t = ref.value_form_t(rho, n)                      # t and p: the pinned operations on the call's own rho
            assert (t == want_t) or (t != t and want_t != want_t), (l, j, t, want_t)
            want_p = 2.0 * pn(abs(t)) if t == t else ref.NAN
            assert (p == want_p) or (p != p and want_p != want_p), (l, j, p, want_p)
            checked += 1
        np.testing.assert_allclose(out[:, 4, l], ref.bh(out[:, 3, l]), rtol=1e-15, atol=0, equal_nan=True)
    print(f"c={c}: {checked} correlations, worst error / bound = {worst:.3g}")
    assert checked >= (5 if c > 1 else 0)


def test_value_mode_agrees_with_numpy_on_plain_lists(hip_ctx):
    stat, kinds, Gp, Gi = case(G, 17)
    out, tot = hip_ctx.rankcor(stat, Gp, Gi, use_rank=False)
    want, wtot = ref.rankcor_scipy(stat, Gp, Gi, use_rank=False)
    assert np.array_equal(tot, wtot) and np.array_equal(out[:, 0, :], want[:, 0, :])
    for l, (kind, missing) in enumerate(kinds):
        if kind in ("inf", "const") or missing in ("but2", "but2same", "all"):
            continue
        np.testing.assert_allclose(out[:, 1:4, l], want[:, 1:4, l], rtol=1e-9, atol=1e-300, equal_nan=True, err_msg=str(kinds[l]))


def test_past_the_lds_resident_rank_kernel(hip_ctx):
    """g = 20,480: the ranks come from the partitioned ranker; both modes, two lists (one with NaN and ties)"""
    g = 20480
    rng = np.random.default_rng(9)
    stat = np.asfortranarray(np.column_stack([make_list(g, "free", "none", rng), make_list(g, "five", "tenth", rng)]))
    Gp, Gi = ref.make_sets(g, (1, 65, 4000, g - 1), seed=2)
    got = hip_ctx.rankcor(stat, Gp, Gi, use_rank=True)
    check_rank_result(got, ref.rankcor_ref(stat, Gp, Gi, "average", ref.library_pnorm_upper()), "g=20480")
    assert not np.isnan(got[0][:, :, 0]).any()
    out, tot = hip_ctx.rankcor(stat, Gp, Gi, use_rank=False)
    for l in range(2):
        L = ref.ValueList(stat[:, l])
        for j in range(len(Gp) - 1):
            exact, k = L.exact(Gi[Gp[j]:Gp[j + 1]])
            bound, rel = L.bound(Gi[Gp[j]:Gp[j + 1]])
            with mpmath.workdps(50):
                assert out[j, 0, l] == k and rel < 2.0**-20 and float(abs(mpmath.mpf(float(out[j, 1, l])) - exact)) <= float(bound)


def on_hook(nshards, stat, Gp, Gi, use_rank, fail=-1):
    return _status(lambda: engine._rankcor(hook("rankcor"), (0, nshards, fail), stat, Gp, Gi, use_rank, "average"))


@pytest.mark.parametrize("use_rank", [True, False])
@pytest.mark.parametrize("c,nshards", [(7, 1), (7, 2), (7, 3), (7, 5), (7, 9), (17, 2), (17, 5), (1, 3), (9, 9)])
def test_every_sharding_returns_the_one_context_bits(hip_ctx, c, nshards, use_rank):
    stat, _, Gp, Gi = case(G, c)
    one = hip_ctx.rankcor(stat, Gp, Gi, use_rank=use_rank)
    status, got = on_hook(nshards, stat, Gp, Gi, use_rank)
    assert status == _lib.OK
    for a, b, nm in zip(got, one, ("out", "tot_out")):
        assert a.tobytes() == b.tobytes(), nm


@pytest.mark.parametrize("c,nshards,fail", [(7, 2, 1), (7, 3, 0), (1, 3, 2)])
def test_a_failing_shard_returns_its_status(hip_ctx, c, nshards, fail):
    stat, _, Gp, Gi = case(G, c)
    status, got = on_hook(nshards, stat, Gp, Gi, True, fail=fail)
    assert status == _lib.EHIP and got is None
    assert "injected failure" in _lib.load().plaidhip_last_error_string().decode()


def test_rankcor_multi_on_the_first_device(hip_ctx):
    stat, _, Gp, Gi = case(G, 9)
    check_rank_result(engine.rankcor_multi(stat, Gp, Gi, ties="min", devices=[0]), rank_reference(G, 9, "min"), "multi")
    engine.multi_finalize()


def test_plaid_rankcor_end_to_end_on_the_hallmark_sets(hip_ctx, golden_dir):
    import scipy.sparse as sp

    import plaid_amd
    gmt = plaid_amd.read_gmt(os.path.join(golden_dir, "hallmarks.gmt"))
    matG = plaid_amd.gmt2mat(gmt)
    rng = np.random.default_rng(11)
    in_sets = list(dict.fromkeys(matG.rownames))
    kept = [in_sets[q] for q in rng.permutation(len(in_sets))[:int(0.9 * len(in_sets))]]     # a tenth of the genes is not measured
    names = kept + [f"NOSET{q}" for q in range(500)]
    names = [names[q] for q in rng.permutation(len(names))]
    vals = rng.normal(size=(len(names), 3))
    vals[rng.random(len(names)) < 0.1, 1] = np.nan                                          # list b: genes filtered out
    vals[:, 2] = np.round(vals[:, 2], 1)                                                     # list c: ties
    stat = plaid_amd.NamedMatrix(vals, names, ["a", "b", "c"])
    lo_size, hi_size = 20, 150
    # the alignment by name and the size filter, restated: the universe is the genes in both, in G's row order
    posx = {nm: q for q, nm in enumerate(names)}
    gg = [nm for nm in in_sets if nm in posx]
    xrow = np.array([posx[nm] for nm in gg])
    col = {nm: q for q, nm in enumerate(gg)}
    Gd = sp.csc_matrix(matG.values)
    sets, Gp, Gi = [], [0], []
    for j, nm in enumerate(matG.colnames):
        rows = Gd.indices[Gd.indptr[j]:Gd.indptr[j + 1]]
        mem = sorted(col[matG.rownames[r]] for r in rows if matG.rownames[r] in col)
        if lo_size <= len(mem) <= hi_size:
            sets.append(nm)
            Gi.extend(mem)
            Gp.append(len(Gi))
    assert 0 < len(sets) < matG.shape[1]
    Gp, Gi = np.array(Gp, dtype=np.int32), np.array(Gi, dtype=np.int32)
    for use_rank in (True, False):
        res = plaid_amd.plaid_rankcor(stat, matG, use_rank=use_rank, minSize=lo_size, maxSize=hi_size, ctx=hip_ctx)
        assert list(res) == ["a", "b", "c"]
        want, _ = ref.rankcor_scipy(vals[xrow, :], Gp, Gi, use_rank=use_rank)
        for l, nm in enumerate(res):
            tab = res[nm]
            assert tab.colnames == list(ref.COLUMNS) and sorted(tab.rownames) == sorted(sets)
            assert np.all(np.diff(tab.values[:, 3]) >= 0)                                   # sorted by p.value
            o = [sets.index(s) for s in tab.rownames]
            assert np.array_equal(tab.values[:, 0], want[o, 0, l])
            np.testing.assert_allclose(tab.values[:, 1:], want[o, 1:, l], rtol=1e-9, atol=1e-300)
    # a named vector returns one table, a one-column matrix a dict; sort_by another column, or none; no p-values
    one = plaid_amd.plaid_rankcor(dict(zip(names, vals[:, 0].tolist())), matG, minSize=lo_size, maxSize=hi_size, ctx=hip_ctx)
    full = plaid_amd.plaid_rankcor(stat, matG, minSize=lo_size, maxSize=hi_size, ctx=hip_ctx)
    assert isinstance(one, plaid_amd.NamedMatrix) and one.rownames == full["a"].rownames
    same(one.values, full["a"].values)
    d = plaid_amd.plaid_rankcor(plaid_amd.NamedMatrix(vals[:, :1], names, ["a"]), matG, minSize=lo_size, maxSize=hi_size,
                                sort_by="rho", compute_p=False, ctx=hip_ctx)
    assert list(d) == ["a"] and d["a"].colnames == ["size", "rho"] and np.all(np.diff(np.abs(d["a"].values[:, 1])) <= 0)
    unsorted = plaid_amd.plaid_rankcor(stat, matG, minSize=lo_size, maxSize=hi_size, sort_by=None, ctx=hip_ctx)
    assert unsorted["b"].rownames == sets
    with pytest.raises(ValueError, match="ties must be one of"):
        plaid_amd.plaid_rankcor(stat, matG, ties="random", ctx=hip_ctx)
