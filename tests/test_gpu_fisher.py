"""plaid.fisher on the device (plaidhip_fisher, kernels_fisher.hip) against the host restatements of
tests/helpers/fisher_ref.py.

The counts (size, ovUp, ovDn, nUp, nDn, the overlap lists) are integers and must be equal.  The three p columns and the
three odds ratios are the pinned form of include/plaidhip.h, which the device runs operation for operation: they must have
the bits of fisher_ref (tail_form), NaN positions included.  padj is within rtol 1e-15 of the Benjamini-Hochberg
restatement (the host routine multiplies and divides in another order), as plaid.gsea's is.  Against exact rational
arithmetic every p of a set of size 1, 2, 63, 64, 65 or N - 1 lies within (4 n + 2) 2^-53, n = hi - lo + 1, wherever the
exact p >= 2^-900.  The shapes sit on the 64-member pass of the count kernel, on the list tile of 8 and its remainder, and
on more than one workgroup of the pack kernel."""
import os
from fractions import Fraction

import numpy as np
import pytest

from plaid_amd import _lib, engine
from tests.helpers import fisher_ref as ref
from tests.helpers.sharded_hooks import _status, hook

pytestmark = pytest.mark.gpu

COLS = ref.COLUMNS
SHAPES = [(64, 1), (65, 7), (4096, 8), (4097, 9), (8193, 65)]      # N, c
_cache, _exact = {}, {}


def sizes(N):
    return (0, 1, 2, 63, 64, 65, N - 1, N)


def same(a, b, what=""):
    assert a.shape == b.shape
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    assert not bad.any(), f"{what}: {int(bad.sum())} differ, first at {np.argwhere(bad)[0]}: {a[bad][0]!r} != {b[bad][0]!r}"


def make_sig(N, c, seed):
    """columns seeded at 5 % and 30 % density in turn (half up, half down); with four columns or more the last three are
    all zero, all +1 and all -1"""
    rng = np.random.default_rng(seed)
    sig = np.zeros((N, c), dtype=np.int8, order="F")
    for l in range(c):
        dens = (0.05, 0.30)[l % 2]
        u = rng.random(N)
        sig[u < dens / 2, l] = 1
        sig[(u >= dens / 2) & (u < dens), l] = -1
    if c >= 4:
        sig[:, c - 3], sig[:, c - 2], sig[:, c - 1] = 0, 1, -1
    return sig


def case(N, c):
    """(sig, Gp, Gi, reference out, tot, ov_len, ov_idx), computed once; the members of a set are in drawn (unsorted) order
    so that the overlap lists show the set's own order"""
    if (N, c) not in _cache:
        sig = make_sig(N, c, 100 * N + c)
        Gp, Gi = ref.make_sets(N, sizes(N), seed=N + c)
        rng = np.random.default_rng(N)
        Gi = Gi.copy()
        for j in range(len(Gp) - 1):
            rng.shuffle(Gi[Gp[j]:Gp[j + 1]])
        _cache[(N, c)] = (sig, Gp, Gi) + ref.fisher_ref(sig, Gp, Gi)
    return _cache[(N, c)]


def same_results(got, want, what=""):
    out, tot, ov_len, ov_idx = got
    wout, wtot, wlen, widx = want
    for q, nm in enumerate(COLS):
        if nm.startswith("padj"):
            np.testing.assert_allclose(out[:, q, :], wout[:, q, :], rtol=1e-15, atol=0, equal_nan=True, err_msg=f"{what} {nm}")
        else:
            same(out[:, q, :], wout[:, q, :], f"{what} {nm}")
    assert np.array_equal(tot, wtot), what
    assert ov_len.dtype == np.int32 and np.array_equal(ov_len, wlen), what
    assert ov_idx.dtype == np.int32 and np.array_equal(ov_idx, widx), what


@pytest.mark.parametrize("N,c", SHAPES)
def test_counts_are_equal_and_tails_have_the_bits_of_the_pinned_form(hip_ctx, N, c):
    sig, Gp, Gi, *want = case(N, c)
    got = hip_ctx.fisher(sig, Gp, Gi, overlap=True)
    same_results(got, want, f"N={N} c={c}")
    out, tot = got[0], got[1]
    k = np.diff(Gp)
    for l in range(c):   # the integers, restated
        assert np.array_equal(out[:, 0, l], k.astype(np.float64))
        assert tot[0, l] == np.sum(sig[:, l] == 1) and tot[1, l] == np.sum(sig[:, l] == -1)
        for j in range(len(k)):
            mem = Gi[Gp[j]:Gp[j + 1]]
            assert out[j, 1, l] == np.sum(sig[mem, l] == 1) and out[j, 2, l] == np.sum(sig[mem, l] == -1)
    none = (k == 0) | (k == N)
    assert none.sum() >= 2 and np.isnan(out[none][:, 3:, :]).all()
    assert not np.isnan(out[~none][:, 3:9, :]).any()
    # without the overlap lists: the same out and tot
    out2, tot2 = hip_ctx.fisher(sig, Gp, Gi)
    same(out2, out)
    assert np.array_equal(tot2, tot)


@pytest.mark.parametrize("N,c", SHAPES)
def test_tails_are_within_the_derived_bound_of_exact_arithmetic(hip_ctx, N, c):
    sig, Gp, Gi, *_ = case(N, c)
    out, tot = hip_ctx.fisher(sig, Gp, Gi)
    k = np.diff(Gp)
    checked, worst = 0, Fraction(0)
    chosen = np.flatnonzero(np.isin(k, (1, 2, 63, 64, 65, N - 1)) & (k < N))
    for j in chosen:
        for l in range(c):
            nU, nD, oU, oD = int(tot[0, l]), int(tot[1, l]), int(out[j, 1, l]), int(out[j, 2, l])
            for d, (K, x) in enumerate(((nU, oU), (nD, oD), (nU + nD, oU + oD))):
                tab = (N, K, int(k[j]), x)
                if tab not in _exact:
                    _exact[tab] = ref.tail_exact(*tab)
                e, p = _exact[tab], float(out[j, 3 + d, l])
                if e >= ref.P_FLOOR:
                    err = abs(Fraction(p) - e) / e
                    assert err <= ref.tail_bound(N, K, int(k[j])), (tab, p, float(err))
                    worst = max(worst, err / ref.tail_bound(N, K, int(k[j])))
                else:
                    assert 0.0 <= p <= ref.P_SMALL, (tab, p)
                checked += 1
    print(f"N={N} c={c}: {checked} tails, worst error / bound = {float(worst):.3g}")
    assert len(chosen) >= 4 and checked == 3 * c * len(chosen)


def test_only_one_overlap_buffer_is_refused(hip_ctx):
    sig, Gp, Gi, *_ = case(65, 7)
    m, c = len(Gp) - 1, sig.shape[1]
    out, tot = np.full((m, 12, c), -7.0, order="F"), np.full((2, c), -7.0, order="F")
    ov_len, ov_idx = np.full((m, c), -7, dtype=np.int32, order="F"), np.full((int(Gp[-1]), c), -7, dtype=np.int32, order="F")
    lib = _lib.load()
    for a, b in ((ov_len.ctypes.data, None), (None, ov_idx.ctypes.data)):
        rc = lib.plaidhip_fisher(hip_ctx.handle, sig.ctypes.data, 65, c, Gp.ctypes.data, Gi.ctypes.data, m, out.ctypes.data,
                                 tot.ctypes.data, a, b)
        assert rc == _lib.EINVAL and "both or neither" in lib.plaidhip_last_error_string().decode()
    assert (out == -7).all() and (tot == -7).all() and (ov_len == -7).all() and (ov_idx == -7).all()


def on_hook(nshards, sig, Gp, Gi, fail=-1):
    return _status(lambda: engine._fisher(hook("fisher"), (0, nshards, fail), sig, Gp, Gi, overlap=True))


@pytest.mark.parametrize("N,c,nshards", [(65, 7, 1), (65, 7, 2), (65, 7, 3), (65, 7, 5), (4097, 9, 2), (4097, 9, 5), (64, 1, 3),
                                         (65, 7, 9)])
def test_every_sharding_returns_the_one_context_bits(hip_ctx, N, c, nshards):
    sig, Gp, Gi, *_ = case(N, c)
    one = hip_ctx.fisher(sig, Gp, Gi, overlap=True)
    status, got = on_hook(nshards, sig, Gp, Gi)
    assert status == _lib.OK
    for a, b, nm in zip(got, one, ("out", "tot_out", "ov_len", "ov_idx")):
        assert a.tobytes() == b.tobytes(), nm


@pytest.mark.parametrize("c,nshards,fail", [(7, 2, 1), (7, 3, 0), (1, 3, 2)])
def test_a_failing_shard_returns_its_status(hip_ctx, c, nshards, fail):
    sig, Gp, Gi, *_ = case(65 if c == 7 else 64, c)
    status, got = on_hook(nshards, sig, Gp, Gi, fail=fail)
    assert status == _lib.EHIP and got is None
    assert "injected failure" in _lib.load().plaidhip_last_error_string().decode()


def test_fisher_multi_on_the_first_device(hip_ctx):
    sig, Gp, Gi, *want = case(4097, 9)
    same_results(engine.fisher_multi(sig, Gp, Gi, overlap=True, devices=[0]), want)
    engine.multi_finalize()


def test_many_lists_and_sets_adjust_on_several_host_threads(hip_ctx):
    """3,000 sets x 40 lists: 360,000 p-values, enough for the Benjamini-Hochberg columns to be dealt to several host
    threads (shard_lists.cpp: kFisherBhWork).  padj against the restatement applied to the call's own p columns, the counts
    against a sparse product, and two shards against one."""
    import scipy.sparse as sp
    N, m, c = 300, 3000, 40
    rng = np.random.default_rng(5)
    ks = rng.integers(1, 12, size=m)
    Gp = np.concatenate([[0], np.cumsum(ks)]).astype(np.int32)
    Gi = np.concatenate([rng.choice(N, size=k, replace=False) for k in ks]).astype(np.int32)
    sig = make_sig(N, c, 77)
    out, tot = hip_ctx.fisher(sig, Gp, Gi)
    G = sp.csc_matrix((np.ones(len(Gi)), Gi, Gp), shape=(N, m))
    assert np.array_equal(out[:, 1, :], G.T @ (sig == 1).astype(np.float64))
    assert np.array_equal(out[:, 2, :], G.T @ (sig == -1).astype(np.float64))
    assert not np.isnan(out[:, 3:9, :]).any()
    for l in range(c):
        for d in range(3):
            np.testing.assert_allclose(out[:, 6 + d, l], ref.bh(out[:, 3 + d, l]), rtol=1e-15, atol=0)
    for j, l, d in ((0, 0, 0), (17, 1, 2), (2999, 38, 1), (1500, 20, 0)):       # a few tails against the pinned form
        K = (tot[0, l], tot[1, l], tot[0, l] + tot[1, l])[d]
        x = (out[j, 1, l], out[j, 2, l], out[j, 1, l] + out[j, 2, l])[d]
        assert out[j, 3 + d, l] == ref.tail_form(N, int(K), int(ks[j]), int(x))
    status, got = _status(lambda: engine._fisher(hook("fisher"), (0, 2, -1), sig, Gp, Gi))
    assert status == _lib.OK and got[0].tobytes() == out.tobytes() and got[1].tobytes() == tot.tobytes()


def test_plaid_fisher_end_to_end_on_the_hallmark_sets(hip_ctx, golden_dir):
    import scipy.sparse as sp

    import plaid_amd
    gmt = plaid_amd.read_gmt(os.path.join(golden_dir, "hallmarks.gmt"))
    matG = plaid_amd.gmt2mat(gmt)
    rng = np.random.default_rng(11)
    in_sets = list(dict.fromkeys(matG.rownames))
    kept = [in_sets[q] for q in rng.permutation(len(in_sets))[:int(0.9 * len(in_sets))]]     # a tenth of the genes is not measured
    names = kept + [f"NOSET{q}" for q in range(500)]
    names = [names[q] for q in rng.permutation(len(names))]
    vals = rng.choice(np.array([-1, 0, 1]), size=(len(names), 3), p=[0.1, 0.75, 0.15])
    sig = plaid_amd.NamedMatrix(vals.astype(np.float64), names, ["a", "b", "c"])
    lo_size, hi_size = 20, 150
    res = plaid_amd.plaid_fisher(sig, matG, minSize=lo_size, maxSize=hi_size, overlap=True, ctx=hip_ctx)
    assert list(res) == ["a", "b", "c"]
    # the alignment by name and the size filter, restated: the universe is the genes in both, in G's row order
    posx = {nm: q for q, nm in enumerate(names)}
    gg = [nm for nm in in_sets if nm in posx]
    assert len(gg) == len(kept)                                  # the 500 genes in no set are not in the universe
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
    assert 0 < len(sets) < matG.shape[1]                         # some sets are dropped
    Gp, Gi = np.array(Gp, dtype=np.int32), np.array(Gi, dtype=np.int32)
    want, _, wlen, widx = ref.fisher_ref(vals[xrow, :], Gp, Gi)
    for l, nm in enumerate(res):
        tab, genes = res[nm]
        assert tab.colnames == list(COLS)
        assert sorted(tab.rownames) == sorted(sets) and len(genes) == len(sets)
        p_any = tab.values[:, 5]
        assert np.all(np.diff(p_any) >= 0)                       # sorted by pAny
        o = [sets.index(s) for s in tab.rownames]
        for q, cn in enumerate(COLS):
            if cn.startswith("padj"):
                np.testing.assert_allclose(tab.values[:, q], want[o, q, l], rtol=1e-15, atol=0)
            else:
                same(tab.values[:, q], want[o, q, l], cn)
        for row, j in enumerate(o):
            hit = widx[Gp[j]:Gp[j] + wlen[j, l], l]
            assert genes[row] == [(gg[r], int(vals[xrow[r], l])) for r in hit]
            assert all(s in (-1, 1) for _, s in genes[row]) and len(genes[row]) == tab.values[row, 1] + tab.values[row, 2]
    # a named vector returns one table, a one-column matrix a dict; sort_by another column, or none
    one = plaid_amd.plaid_fisher(dict(zip(names, vals[:, 0].tolist())), matG, minSize=lo_size, maxSize=hi_size, ctx=hip_ctx)
    assert isinstance(one, plaid_amd.NamedMatrix) and one.rownames == res["a"][0].rownames
    same(one.values, res["a"][0].values)
    d = plaid_amd.plaid_fisher(plaid_amd.NamedMatrix(vals[:, :1].astype(np.float64), names, ["a"]), matG, minSize=lo_size,
                               maxSize=hi_size, sort_by="pUp", ctx=hip_ctx)
    assert list(d) == ["a"] and np.all(np.diff(d["a"].values[:, 3]) >= 0)
    assert sorted(d["a"].rownames) == sorted(sets)
    unsorted = plaid_amd.plaid_fisher(sig, matG, minSize=lo_size, maxSize=hi_size, sort_by=None, ctx=hip_ctx)
    assert unsorted["b"].rownames == sets
    # the default sizes: every set with an aligned member but those that hold every gene
    full = plaid_amd.plaid_fisher(sig, matG, ctx=hip_ctx)
    assert len(full["a"].rownames) == matG.shape[1] and not np.isnan(full["a"].values[:, :9]).any()
