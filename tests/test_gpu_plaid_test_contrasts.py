"""plaid.test.contrasts on the device -- `pytest -m gpu`.

  1. the device entries dev_row_contrast_sums / dev_row_contrast_ssd at the kernels' seams (512 rows per workgroup, 128
     columns per partial, the contrast tile T, ld > rows, odd rows: the narrow load path), sentinels around every buffer:
     per contrast against the exact moments of the contrast's own samples at sum_bound / mean_bound / ssd_bound, and for
     EVERY contrast bit for bit what dev_row_group_sums / _ssd give for that label column (a contrast without NA is the
     one the issue asks for; the one-label kernels add +0.0 for any label that is neither 0 nor 1, so the contrasts with NA
     are held to them as well)
  2. Context.plaid_test_contrasts / _csc against one Context.plaid_test / _csc call per contrast, bit for bit
  3. contrasts that leave samples out, against the exact references on the subset (interval checks; no set may be
     "not separable": tests/test_plaid_test_contrasts_ref.py asserts that from the reference alone), and excluded columns
     overwritten with NaN / Inf / 1e300
  4. every sharding through the hook bit for bit the one-shard call
  5. the hook's failure path
  6. the oracle's plaid_test (R/plaid.R:392-474) on the subsets of the pbmc3k50 fixture
"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import contrast_hooks as ch
from tests.helpers import exact_ref as er
from tests.helpers import exact_stats as xs

pytestmark = pytest.mark.gpu
NA = ch.NA


def _tile():
    from plaid_amd import engine
    return engine.contrast_tile()


# ------------------------------------------------------------------------------------------------ 1. the seams
# (rows, n, which C of [1, T - 1, T, T + 1, 2 T + 1], padding of ld): every rows / n / C value at least twice; ld = rows
# with even rows is the 16-byte path, rows + 2 the same with padding, rows + 3 and every odd `rows` the narrow one
SEAMS = [(1, 1, 0, 0), (1, 1000, 3, 3), (2, 128, 1, 0), (2, 257, 4, 2), (255, 127, 2, 0), (255, 129, 3, 3),
         (256, 128, 2, 0), (256, 1000, 4, 2), (256, 129, 0, 3), (257, 257, 1, 0), (257, 1, 4, 3), (513, 127, 3, 0),
         (513, 1000, 1, 3), (5001, 129, 2, 0), (5001, 257, 4, 3), (5001, 1000, 0, 2)]


def _seam_labels(n, C, rng):
    """column kinds in turn: no NA, ~30 % NA, all 0, a single 1 (rest 0), group 1 inside the first 128 columns with NA, a
    duplicate of column 0"""
    Y = np.zeros((n, C), dtype=np.int32)
    for j in range(C):
        kind = j % 6
        if kind == 0:
            Y[:, j] = ch.random_contrasts(n, 1, rng)[:, 0]
        elif kind == 1:
            Y[:, j] = ch.random_contrasts(n, 1, rng, na=0.3)[:, 0]
        elif kind == 3:
            Y[int(rng.integers(n)), j] = 1
        elif kind == 4:
            Y[rng.random(n) < 0.3, j] = NA
            w = min(n, 128)
            Y[rng.choice(w, max(1, w // 3), replace=False), j] = 1
        elif kind == 5:
            Y[:, j] = Y[:, 0]
    return Y


@pytest.mark.parametrize("rows,n,ci,pad", SEAMS)
def test_device_entries_at_the_seams(hip_ctx, rows, n, ci, pad):
    import torch
    T = _tile()
    C = [1, T - 1, T, T + 1, 2 * T + 1][ci]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(100000 * ci + 1000 * rows + n)
    ld = rows + pad
    Y = _seam_labels(n, C, rng)
    check_rows = np.unique(np.concatenate([np.linspace(0, rows - 1, min(rows, 24)).astype(int),
                                           [r for r in (0, 1, 254, 255, 256, 257, 510, 511, 512, 513, rows - 2, rows - 1)
                                            if 0 <= r < rows]]))
    for kind in ("gamma", "cancel"):
        A = rng.gamma(2.0, 1.0, size=(rows, n)) + 0.25 if kind == "gamma" else 1e6 + rng.normal(size=(rows, n))
        Ad = torch.full((n, ld), 777.0, dtype=torch.float64, device=dev)
        Ad[:, :rows] = torch.from_numpy(np.ascontiguousarray(A.T)).to(dev)
        Yd = torch.from_numpy(np.ascontiguousarray(Y.T)).to(dev)              # C x n row-major = n x C column-major
        size = 2 * rows * C
        sums = torch.full((size + 5,), -7.0, dtype=torch.float64, device=dev)
        ssd = torch.full((size + 5,), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        hip_ctx.dev_row_contrast_sums(Ad.data_ptr(), ld, rows, n, Yd.data_ptr(), C, sums.data_ptr())
        hip_ctx.synchronize()
        s = sums.cpu().numpy()
        assert np.all(s[size:] == -7.0)
        s = s[:size].reshape(C, 2, rows)
        cnt = np.stack([(Y == 0).sum(axis=0), (Y == 1).sum(axis=0)], axis=1).astype(np.float64)      # C x 2
        with np.errstate(all="ignore"):
            inv = np.where(cnt > 0, 1.0 / np.maximum(cnt, 1.0), np.nan)      # the library's own scale: fl(1 / n_k), or NaN
            mean = s * inv[:, :, None]
        md = torch.from_numpy(np.ascontiguousarray(mean)).to(dev)
        torch.cuda.synchronize()
        hip_ctx.dev_row_contrast_ssd(Ad.data_ptr(), ld, rows, n, Yd.data_ptr(), C, md.data_ptr(), ssd.data_ptr())
        hip_ctx.synchronize()
        q = ssd.cpu().numpy()
        assert np.all(q[size:] == -7.0)
        q = q[:size].reshape(C, 2, rows)
        assert np.all(Ad.cpu().numpy()[:, rows:] == 777.0)
        one_s = torch.empty((2 * rows,), dtype=torch.float64, device=dev)
        one_q = torch.empty((2 * rows,), dtype=torch.float64, device=dev)
        for j in range(C):
            what = f"rows={rows} n={n} ld={ld} C={C} contrast {j} {kind}"
            # the one-label entries with this label column: the same bits
            hip_ctx.dev_row_group_sums(Ad.data_ptr(), ld, rows, n, Yd[j].data_ptr(), one_s.data_ptr())
            hip_ctx.dev_row_group_ssd(Ad.data_ptr(), ld, rows, n, Yd[j].data_ptr(), md[j].data_ptr(), one_q.data_ptr())
            hip_ctx.synchronize()
            er.assert_same_bits(s[j], one_s.cpu().numpy().reshape(2, rows), what + " sums vs dev_row_group_sums")
            er.assert_same_bits(q[j], one_q.cpu().numpy().reshape(2, rows), what + " ssd vs dev_row_group_ssd")
            if j % 6 == 5:
                er.assert_same_bits(s[j], s[0], what + " duplicate")
                er.assert_same_bits(q[j], q[0], what + " duplicate")
                continue
            # the exact moments of the contrast's own samples
            sel, y = ch.subset(Y, j)
            ref = xs.group_moments(A[np.ix_(check_rows, sel)], y)
            nk = ref["n"][:, None].astype(np.float64)
            er.assert_within(s[j][:, check_rows], ref["sum"], xs.sum_bound(ref["mag"], nk), what + " sums")
            mb = xs.mean_bound(ref["mag"], nk)
            er.assert_within(mean[j][:, check_rows], ref["mean"], mb, what + " means")
            er.assert_within(q[j][:, check_rows], ref["ssd"], xs.ssd_bound(ref["ssd"], nk, mb), what + " ssd")


# ------------------------------------------------------------------------------------------------ 2. bit identity
def _no_na_contrasts(n, C, rng):
    """C label columns without NA: at random, and among them all zero, a single 1, and a duplicate of column 0"""
    Y = ch.random_contrasts(n, C, rng)
    Y[:, 1] = 0
    Y[:, 2] = 0
    Y[int(rng.integers(n)), 2] = 1
    Y[:, C - 1] = Y[:, 0]
    return Y


BIT_N = [7, 129, 263, 1000]


@pytest.mark.parametrize("m", [1, 2, 121, 513])
def test_contrasts_without_na_have_the_bits_of_plaid_test(hip_ctx, m):
    from plaid_amd import synth
    T = _tile()
    C = T + 1
    g = 600
    Gp, Gi = synth.geneset_csc(g, m, kmin=3, kmax=60, seed=m)
    rng = np.random.default_rng(17 * m)
    k0 = [1, 2, 121, 513].index(m)
    for i in range(2):
        n = BIT_N[(k0 + 2 * i) % 4]
        X = rng.gamma(2.0, 1.0, size=(g, n))
        X[rng.random(X.shape) < 0.3] = 0.0
        Xs = sp.csc_matrix(X)
        Xs.sort_indices()
        Y = _no_na_contrasts(n, C, rng)
        S = rng.gamma(2.0, 1.0, size=(m, n)) + 0.25 if i == 0 else 1e6 + rng.normal(size=(m, n))
        for tests in (1, 3, 4, 7):
            for metap in ((0, 1) if tests in (3, 7) else (i,)):
                for gx in (None, S):
                    what = f"m={m} n={n} tests={tests} metap={metap} gsetX={'given' if gx is not None else 'NULL'}"
                    got = hip_ctx.plaid_test_contrasts(X, Y, Gp, Gi, gx, tests, metap)
                    gots = hip_ctx.plaid_test_contrasts_csc(Xs.indptr, Xs.indices, Xs.data, g, Y, Gp, Gi, gx, tests, metap)
                    assert got.shape == (m, 6, C) and gots.shape == (m, 6, C)
                    for j in range(C):
                        y = np.ascontiguousarray(Y[:, j])
                        er.assert_same_bits(got[:, :, j], hip_ctx.plaid_test(X, y, Gp, Gi, gx, tests, metap),
                                            f"{what} dense contrast {j}")
                        er.assert_same_bits(gots[:, :, j],
                                            hip_ctx.plaid_test_csc(Xs.indptr, Xs.indices, Xs.data, g, y, Gp, Gi, gx, tests, metap),
                                            f"{what} csc contrast {j}")
                    er.assert_same_bits(got[:, :, C - 1], got[:, :, 0], what + " duplicated contrast")
                    er.assert_same_bits(gots[:, :, C - 1], gots[:, :, 0], what + " duplicated contrast (csc)")


def test_empty_results(hip_ctx):
    """C = 0: an empty result; m = 0: as plaid.test, nothing to write"""
    rng = np.random.default_rng(0)
    X = rng.gamma(2.0, 1.0, size=(16, 9))
    Gp, Gi = np.arange(5, dtype=np.int32), np.arange(4, dtype=np.int32)
    assert hip_ctx.plaid_test_contrasts(X, np.zeros((9, 0), dtype=np.int32), Gp, Gi).shape == (4, 6, 0)
    Y = ch.random_contrasts(9, 3, rng, na=0.3)
    assert hip_ctx.plaid_test_contrasts(X, Y, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32)).shape == (0, 6, 3)


# ------------------------------------------------------------------------------------------------ 3. exclusions
def _check_contrast(out, X, S_all, Y, j, Gp, Gi, what):
    """contrast j of a tests = 7 result against the exact references on its own samples; returns the number of sets that
    were not separable (the caller asserts 0)"""
    sel, y = ch.subset(Y, j)
    ivs = xs.crossprod_intervals(X[:, sel], y, Gp, Gi)
    fc, fb, wiv = ch.welch_intervals(S_all[:, sel], y)
    nsep = 0
    for k, (one, two) in enumerate(ivs):
        if one is None or two is None or wiv[k] is None:
            nsep += 1
            continue
        assert xs.in_interval(out[k, 1], one), ("p.one", what, k, out[k, 1], one)
        assert xs.in_interval(out[k, 2], two), ("p.two", what, k, out[k, 2], two)
        if isinstance(wiv[k], str):
            assert out[k, 3] == xs.P_HI, ("p.lm", what, k, out[k, 3])
        else:
            assert xs.in_interval(out[k, 3], wiv[k]), ("p.lm", what, k, out[k, 3], wiv[k])
        # gsetFC = rowMeans(meanx, diff, m1 - m0)
        lo = (one[2] + two[2] + fc[k] - fb[k]) / 3.0
        hi = (one[3] + two[3] + fc[k] + fb[k]) / 3.0
        slack = 8 * xs.U * (abs(one[2]) + abs(two[2]) + abs(fc[k]) + abs(lo) + abs(hi))
        assert lo - slack <= out[k, 0] <= hi + slack, ("gsetFC", what, k, out[k, 0], lo, hi)
    return nsep


@pytest.mark.parametrize("case", ch.EXCLUSION_CASES)
def test_contrasts_with_excluded_samples_against_the_subset(hip_ctx, case):
    X, Y, Gp, Gi, S = ch.exclusion_case(*case)
    assert np.all(np.abs((Y == NA).mean(axis=0) - 0.3) < 0.1)
    assert not (Y[128:, 1] == 1).any() and (Y[:, 2] == 1).sum() == 1
    S_dev = hip_ctx.plaid_dense(X, Gp, Gi, "mean", True)                    # gsetX = NULL: plaid(X, G) over ALL samples
    for gx, S_all in ((S, S), (None, S_dev)):
        out = hip_ctx.plaid_test_contrasts(X, Y, Gp, Gi, gx, 7, 0)
        for j in range(3):
            what = f"case={case} contrast {j} gsetX={'given' if gx is not None else 'NULL'}"
            assert _check_contrast(out[:, :, j], X, S_all, Y, j, Gp, Gi, what) == 0, what
        assert np.all(out[:, 3, 2] == xs.P_HI)                              # a group of one
    # what an excluded sample holds does not reach its contrast
    ref = hip_ctx.plaid_test_contrasts(X, Y, Gp, Gi, S, 7, 0)
    for j in range(3):
        excl = np.flatnonzero(Y[:, j] == NA)
        for poison in (np.nan, np.inf, 1e300):
            Xp, Sp = X.copy(), S.copy()
            Xp[:, excl] = poison
            Sp[:, excl] = poison
            got = hip_ctx.plaid_test_contrasts(Xp, Y, Gp, Gi, Sp, 7, 0)
            er.assert_same_bits(got[:, :, j], ref[:, :, j], f"case={case} contrast {j} excluded columns = {poison}")


# ------------------------------------------------------------------------------------------------ 4. / 5. shardings
SHARD_N = [1, 129, 392, 521, 1000]


@pytest.mark.parametrize("nshards", [1, 2, 3, 4])
def test_every_sharding_has_the_bits_of_the_one_shard_call(hip_ctx, nshards):
    from plaid_amd import synth
    T = _tile()
    g, m, C = 300, 121, T + 1
    Gp, Gi = synth.geneset_csc(g, m, kmin=3, kmax=60, seed=3)
    rng = np.random.default_rng(nshards)
    for n in SHARD_N:
        X = rng.gamma(2.0, 1.0, size=(g, n))
        X[rng.random(X.shape) < 0.3] = 0.0
        S = rng.gamma(2.0, 1.0, size=(m, n)) + 0.25
        for na in (0.0, 0.3):
            Y = ch.random_contrasts(n, C, rng, na=na)
            for gx in (None, S):
                what = f"n={n} nshards={nshards} na={na} gsetX={'given' if gx is not None else 'NULL'}"
                exp = hip_ctx.plaid_test_contrasts(X, Y, Gp, Gi, gx, 7, 0)
                rc, got = ch.run(nshards, X, Y, Gp, Gi, gx, 7, 0)
                assert rc == 0, what
                er.assert_same_bits(got, exp, what)


@pytest.mark.parametrize("nshards,fail", [(1, 0), (3, 1), (4, 3)])
def test_a_failing_shard_returns_the_status_and_leaves_out_untouched(nshards, fail):
    from plaid_amd import _lib, synth
    g, m, n = 200, 30, 521
    Gp, Gi = synth.geneset_csc(g, m, kmin=3, kmax=40, seed=1)
    rng = np.random.default_rng(2)
    X = rng.gamma(2.0, 1.0, size=(g, n))
    Y = ch.random_contrasts(n, 3, rng, na=0.3)
    rc, out = ch.run(nshards, X, Y, Gp, Gi, None, 7, 0, fail=fail)
    assert rc == _lib.EHIP
    assert np.all(out == -7.0)
    msg = _lib.load().plaidhip_last_error_string().decode()
    assert "injected failure" in msg


# ------------------------------------------------------------------------------------------------ 6. the oracle
def test_subsetting_agrees_with_the_oracle_on_the_pbmc_fixture(pbmc, golden_dir):
    """the definition itself: contrast j is the reference's plaid.test on X[, sel], Y[sel, j] with gsetX = S_all[, sel],
    S_all = plaid(X, G) over all samples -- the oracle's plaid_test (R/plaid.R:392-474), to the tolerance
    tests/test_gpu_parity.py holds plaid.test to on this fixture"""
    import plaid_amd
    from oracle import plaid_oracle as po
    d, _ = pbmc
    Xs = sp.csc_matrix((d["x"], d["i"], d["p"]), shape=tuple(d["dim"]))
    Xn = plaid_amd.NamedMatrix(Xs, d["rownames"], d["colnames"])
    matG = plaid_amd.gmt2mat(plaid_amd.read_gmt(os.path.join(golden_dir, "hallmarks.gmt")))
    n = Xs.shape[1]
    rng = np.random.default_rng(2024)
    Y = ch.random_contrasts(n, 3, rng, na=0.3).astype(np.float64)
    Y[Y == NA] = np.nan
    Yn = plaid_amd.NamedMatrix(Y, d["colnames"], ["a", "b", "c"])
    rn = list(d["rownames"])
    G = sp.csc_matrix(matG.values)
    S_all = plaid_amd.plaid(Xn, matG)
    Xd = np.asarray(Xs.todense())
    for gx in (None, S_all):
        res = plaid_amd.plaid_test_contrasts(Xn, Yn, matG, gsetX=gx, sort_by=None)
        assert list(res) == ["a", "b", "c"]
        for j, nm in enumerate(res):
            sel = np.flatnonzero(~np.isnan(Y[:, j]))
            exp = po.plaid_test(Xd[:, sel], rn, Y[sel, j].astype(int), G, matG.rownames, S_all.values[:, sel],
                                metap_method="fisher", tests=("one", "two", "lm"))
            r = res[nm]
            assert r.colnames == ["gsetFC", "p.one", "p.two", "p.lm", "p.meta", "q.meta"] and r.rownames == matG.colnames
            for k, col in enumerate(r.colnames):
                np.testing.assert_allclose(r.values[:, k], exp[col], rtol=1e-7, atol=1e-300, err_msg=f"{nm} {col}")
