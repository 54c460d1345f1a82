"""plaid.test's device moments against exact references at derived fp64 bounds -- `pytest -m gpu`.

References and bounds: tests/helpers/exact_stats.py (group_moments, sum_bound, mean_bound, ssd_bound, welch_interval).
  a. the dense device entries dev_row_group_sums / dev_row_group_ssd at the kernels' seams (256 rows per workgroup, 128
     columns per partial, ld > rows, one row, one column), with sentinels around every buffer
  b. the Welch route of the context entry (the sharded engine with one shard): gsetFC = m1 - m0 at the means' bound, p.lm
     by the interval check, the degenerate cases pinned exactly
  c. the gene fold changes through one-gene sets (tests = 1: gsetFC[j] = fc_j / (1 + 1e-8)), dense and dgCMatrix,
     including a row longer than kLongRow (the 256-thread CSR row path) and two identical rows with identical bits
  d. p.one and p.two from the device crossprod (tests = 3) by the interval check; no set may be "not separable"
     (tests/test_exact_stats_ref.py asserts that from the reference alone, for the same seeds and shapes)
  e. the sharded engine at odd numbers of sets -- the first cases that run row_group_shifted_partials_kernel<*, false> and
     its lone last row: every sharding bit-identical to the one-shard run (the context entry), and within the exact bounds
     when gsetX is given
In (a) the device entry returns SUMS (reduce_blocks_kernel with scale 1); the means are formed by the test as
sums * fl(1 / n_k), the expression plaid_amd/sharded.py uses on these entries, and fed back to dev_row_group_ssd.  The
kernel's own scale0 / scale1 path (the c = 3 of mean_bound) runs in (b), (c) and (e), through plaid_test's gsetFC.
An empty group's sum of squared deviations is asserted as the empty sum, 0.0.  The reference has no such quantity: its
variance of no samples is NA and p.lm becomes 1 - 1e-99, which (b) pins; 0 / (0 - 1) / 0 is NaN on the host as well.
"""
import numpy as np
import pytest

from tests.helpers import exact_ref as er
from tests.helpers import exact_stats as xs
from tests.helpers.plaid_test_sharded import run

pytestmark = pytest.mark.gpu

# every rows value with at least two n, every n with at least two rows
SHAPES = [(1, 1), (1, 128), (1, 1000), (2, 2), (2, 129), (2, 257), (255, 127), (255, 128), (255, 255), (256, 129),
          (256, 255), (257, 1), (257, 256), (513, 2), (513, 256), (513, 257), (5001, 127), (5001, 1000)]
# (labels, data, padded ld)
COMBOS = [("random", "gamma", False), ("random", "gamma", True), ("random", "cancel", True), ("random", "nonfinite", False),
          ("all0", "gamma", True), ("one1", "cancel", False), ("first128", "gamma", False), ("first128", "cancel", True)]


def _labels(n, kind, rng):
    y = np.zeros(n, dtype=np.int32)
    if kind == "random":
        y = (rng.random(n) < 0.4).astype(np.int32)
    elif kind == "one1":
        y[int(rng.integers(n))] = 1
    elif kind == "first128":
        w = min(n, 128)
        y[rng.choice(w, max(1, w // 3), replace=False)] = 1
    return y


def _data(rows, n, kind, y, rng):
    if kind == "gamma":
        return rng.gamma(2.0, 1.0, size=(rows, n)) + 0.25
    A = 1e6 + rng.normal(size=(rows, n))
    if kind == "nonfinite":
        A = rng.gamma(2.0, 1.0, size=(rows, n)) + 0.25
        c0, c1 = np.flatnonzero(y == 0), np.flatnonzero(y == 1)
        if len(c0):
            A[0, c0[len(c0) // 2]] = np.nan                 # row 0: a NaN in group 0 only
        if len(c1):
            A[rows - 1, c1[0]] = np.inf                     # the last row: +Inf in group 1 only (rows == 1: the same row)
    return A


def _check_moments(got_sum, got_ssd, mean_used, A, y, what):
    """sums at sum_bound, the means the test formed from them at mean_bound (c = 3), ssd about those means at ssd_bound"""
    ref = xs.group_moments(A, y)
    nk = ref["n"][:, None].astype(np.float64)
    er.assert_within(got_sum, ref["sum"], xs.sum_bound(ref["mag"], nk), what + " sums")
    mb = xs.mean_bound(ref["mag"], nk)
    er.assert_within(mean_used, ref["mean"], mb, what + " means")
    er.assert_within(got_ssd, ref["ssd"], xs.ssd_bound(ref["ssd"], nk, mb), what + " ssd")
    return ref


@pytest.mark.parametrize("rows,n", SHAPES)
def test_dense_device_entries_at_the_seams(hip_ctx, rows, n):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1000 * rows + n)
    for lab, kind, padded in COMBOS:
        y = _labels(n, lab, rng)
        A = _data(rows, n, kind, y, rng)
        ld = rows + 3 if padded else rows
        Ad = torch.full((n, ld), 777.0, dtype=torch.float64, device=dev)
        Ad[:, :rows] = torch.from_numpy(np.ascontiguousarray(A.T)).to(dev)
        yd = torch.from_numpy(y).to(dev)
        sums = torch.full((2 * rows + 5,), -7.0, dtype=torch.float64, device=dev)
        ssd = torch.full((2 * rows + 5,), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        hip_ctx.dev_row_group_sums(Ad.data_ptr(), ld, rows, n, yd.data_ptr(), sums.data_ptr())
        hip_ctx.synchronize()
        s = sums.cpu().numpy()
        assert np.all(s[2 * rows:] == -7.0)
        s = s[:2 * rows].reshape(2, rows)
        cnt = np.array([np.sum(y == 0), np.sum(y == 1)], dtype=np.float64)
        with np.errstate(all="ignore"):
            inv = np.where(cnt > 0, 1.0 / np.maximum(cnt, 1.0), np.nan)      # the library's own scale: fl(1 / n_k), or NaN
            mean = s * inv[:, None]
        md = torch.from_numpy(np.ascontiguousarray(mean)).to(dev)
        torch.cuda.synchronize()
        hip_ctx.dev_row_group_ssd(Ad.data_ptr(), ld, rows, n, yd.data_ptr(), md.data_ptr(), ssd.data_ptr())
        hip_ctx.synchronize()
        q = ssd.cpu().numpy()
        assert np.all(q[2 * rows:] == -7.0)
        assert np.all(Ad.cpu().numpy()[:, rows:] == 777.0)
        what = f"rows={rows} n={n} ld={ld} {lab} {kind}"
        ref = _check_moments(s, q[:2 * rows].reshape(2, rows), mean, A, y, what)
        if lab == "all0":
            assert np.isnan(mean[1]).all() and np.all(q[rows:2 * rows] == 0.0)
        if kind == "nonfinite":                            # only the poisoned (row, group) pairs are not finite
            bad = np.zeros((2, rows), dtype=bool)
            bad[0, 0] = cnt[0] > 0
            bad[1, rows - 1] = cnt[1] > 0
            ok = ~bad & (cnt[:, None] > 0)
            assert np.isfinite(mean[ok]).all() and np.isfinite(ref["mean"][ok]).all()
            assert not np.isfinite(mean[bad]).any()


def _one_gene_sets(m, g=16):
    Gp = np.arange(m + 1, dtype=np.int32)
    Gi = (np.arange(m) % g).astype(np.int32)
    return Gp, Gi


def _check_welch(out, S, y, what, max_p=48):
    """gsetFC (tests = 4) = m1 - m0 within the two means' bounds plus the subtraction's rounding; p.lm inside the interval
    of the exact moments and their bounds, on up to max_p evenly spread sets (the 50-digit evaluation is slow); the number
    of sets that are not separable is returned"""
    ref = xs.group_moments(S, y)
    n0, n1 = (int(v) for v in ref["n"])
    nk = ref["n"][:, None].astype(np.float64)
    mb = xs.mean_bound(ref["mag"], nk)
    qb = xs.ssd_bound(ref["ssd"], nk, mb)
    with np.errstate(all="ignore"):
        fc = ref["mean"][1] - ref["mean"][0]
        er.assert_within(out[:, 0], fc, mb[0] + mb[1] + 2 * xs.U * np.abs(fc), what + " gsetFC")
    m = S.shape[0]
    nsep = 0
    if n0 < 2 or n1 < 2:                                                 # a variance of 0 / 0 (or of nothing): NaN -> 1
        assert np.all(out[:, 3] == xs.P_HI), what
        return 0
    seams = [j for j in (0, 1, 254, 255, 256, 257, 510, 511, 512, m - 2, m - 1) if 0 <= j < m]    # 256 rows a workgroup,
    for j in np.unique(np.concatenate([np.linspace(0, m - 1, min(m, max_p)).astype(int), seams])):   # 512 in the sharded one
        if not (np.isfinite(ref["ssd"][:, j]).all() and np.isfinite(fc[j])):
            assert out[j, 3] == xs.P_HI, (what, j)                       # NaN -> 1 -> 1 - 1e-99
            continue
        iv = xs.welch_interval(ref["mean"][0, j], mb[0, j], ref["mean"][1, j], mb[1, j], ref["ssd"][0, j], qb[0, j],
                               ref["ssd"][1, j], qb[1, j], n0, n1)
        if iv is None:
            nsep += 1
            continue
        assert xs.in_interval(out[j, 3], iv), (what, j, out[j, 3], iv)
    return nsep


@pytest.mark.parametrize("m,n", [(1, 2), (1, 257), (2, 129), (2, 1000), (255, 127), (255, 256), (256, 128), (256, 255),
                                 (257, 129), (257, 1000)])
def test_welch_route_of_the_context_entry(hip_ctx, m, n):
    rng = np.random.default_rng(7 * m + n)
    Gp, Gi = _one_gene_sets(m)
    X = rng.gamma(2.0, 1.0, size=(16, n))
    for kind in ("gamma", "cancel"):
        y = _labels(n, "random", rng)
        if n >= 4:
            y[:4] = [0, 1, 0, 1]                                          # both groups have two samples
        S = _data(m, n, kind, y, rng)
        if kind == "gamma":
            S = S + 0.3 * rng.normal(size=(m, 1)) * y[None, :]            # a group effect per set
        for metap in (0, 1):
            out = hip_ctx.plaid_test(X, y, Gp, Gi, S, 4, metap)
            nsep = _check_welch(out, S, y, f"m={m} n={n} {kind}")
            assert nsep == 0 or n < 4
            assert np.array_equal(out[:, 4], out[:, 3])


def test_welch_degenerate_cases_are_pinned(hip_ctx):
    """a group of one sample: its variance is 0 / 0 -> p.lm = 1 - 1e-99 for every set; a constant row: both variances 0 and
    m1 - m0 = 0, so t = 0 / 0 -> NaN -> 1 - 1e-99, as the reference's formula gives -- pinned for a row of zeros and for a
    nonzero constant whose means are exact (2.5 with group sizes 16 and 32: n_k c and fl(1 / n_k) are exact); for other
    constants whether fl(n_k c * fl(1 / n_k)) == c decides between 0 / 0 and x / 0, which no formula pins;
    a NaN score: 1 - 1e-99 for that set only"""
    rng = np.random.default_rng(4)
    m, n = 6, 40
    Gp, Gi = _one_gene_sets(m)
    X = rng.gamma(2.0, 1.0, size=(16, n))
    S = rng.normal(size=(m, n))
    for one in (0, 1):
        y = np.full(n, 1 - one, dtype=np.int32)
        y[17] = one
        out = hip_ctx.plaid_test(X, y, Gp, Gi, S, 4, 0)
        assert np.all(out[:, 3] == xs.P_HI)
    y = (rng.random(n) < 0.5).astype(np.int32)
    S2 = S.copy()
    S2[1, :] = 0.0
    S2[4, 9] = np.nan
    out = hip_ctx.plaid_test(X, y, Gp, Gi, S2, 4, 0)
    assert out[1, 3] == xs.P_HI and out[1, 0] == 0.0
    assert out[4, 3] == xs.P_HI and np.isnan(out[4, 0])
    keep = [0, 2, 3, 5]
    assert np.all(out[keep, 3] < 1.0) and _check_welch(out[keep], S2[keep], y, "finite sets") == 0
    n = 48
    y = np.zeros(n, dtype=np.int32)
    y[rng.choice(n, 32, replace=False)] = 1                               # n0 = 16, n1 = 32
    X = rng.gamma(2.0, 1.0, size=(16, n))
    S3 = rng.normal(size=(m, n))
    S3[2, :] = 2.5
    out = hip_ctx.plaid_test(X, y, Gp, Gi, S3, 4, 0)
    assert out[2, 3] == xs.P_HI and out[2, 0] == 0.0
    assert np.all(np.delete(out[:, 3], 2) < 1.0)


# column counts whose shards (cut at 128-column blocks) leave 0, 1, 7, 8, 9 and 127 columns modulo 128 and modulo 8,
# n < 128 * nshards (empty shards) included
SHARD_N = [1, 7, 129, 255, 263, 392, 512, 521, 1000]


@pytest.mark.parametrize("nshards", [1, 2, 3, 4])
@pytest.mark.parametrize("m", [1, 2, 119, 120, 121, 513])
def test_sharded_engine_at_odd_widths(hip_ctx, m, nshards):
    from plaid_amd import synth
    g = 600
    Gp, Gi = synth.geneset_csc(g, m, kmin=3, kmax=60, seed=m)
    rng = np.random.default_rng(31 * m + nshards)
    k0 = [1, 2, 119, 120, 121, 513].index(m)
    for i in range(3):
        n = SHARD_N[(3 * k0 + i + nshards) % len(SHARD_N)]
        X = rng.gamma(2.0, 1.0, size=(g, n))
        X[rng.random(X.shape) < 0.3] = 0.0
        y = _labels(n, "random", rng)
        if n >= 4:
            y[:4] = [0, 1, 0, 1]
        S = _data(m, n, "cancel" if i == 1 else "gamma", y, rng)
        for tests in (4, 7):
            for gx in (None, S):
                what = f"m={m} n={n} nshards={nshards} tests={tests} gsetX={'given' if gx is not None else 'NULL'}"
                exp = hip_ctx.plaid_test(X, y, Gp, Gi, gx, tests, 0)
                rc, got = run(nshards, X, y, Gp, Gi, gx, tests, 0)
                assert rc == 0, what
                er.assert_same_bits(got, exp, what)
                if gx is not None and tests == 4 and n >= 4:
                    assert _check_welch(got, S, y, what, max_p=16) == 0


# ------------------------------------------------------------------------------------------------ c. fold changes
def _singletons(g):
    return np.arange(g + 1, dtype=np.int32), np.arange(g, dtype=np.int32)


def _check_singleton_fc(out, X, y, c, what):
    fc, err = xs.fold_changes(X, y, c)
    er.assert_within(out[:, 0], fc / (1.0 + xs.GUARD), xs.singleton_fc_bound(fc, err), what + " gsetFC")


@pytest.mark.parametrize("g,n", [(257, 129), (257, 1000), (4097, 129), (4097, 1000)])
def test_gene_fold_changes_dense(hip_ctx, g, n):
    """row_group_sums_kernel on X, reduce_blocks_kernel's scales and fold_change_kernel, observable per gene"""
    rng = np.random.default_rng(g + n)
    Gp, Gi = _singletons(g)
    y = _labels(n, "random", rng)
    y[:2] = [0, 1]
    for kind in ("gamma", "cancel"):
        X = _data(g, n, kind, y, rng)
        X[7, :] = X[8, :]
        out = hip_ctx.plaid_test(X, y, Gp, Gi, None, 1, 0)
        _check_singleton_fc(out, X, y, xs.MEAN_C_DENSE, f"dense g={g} n={n} {kind}")
        er.assert_same_bits(out[7], out[8], "identical rows")


def _k_long_row():
    import os
    import re
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "plaid_amd", "csrc", "kernels_csr.hip")
    return int(re.search(r"constexpr int kLongRow = (\d+);", open(src).read()).group(1))


@pytest.mark.parametrize("dens", [0.02, 0.6])
def test_gene_fold_changes_csc(hip_ctx, dens):
    """csr_row_moments_kernel through plaid_test_csc: a gene with no stored value, one stored in group 1 only, a sample
    with no stored value, rows longer than kLongRow (one workgroup per row) next to short ones (one wavefront), and two
    pairs of identical rows -- one pair short, one long -- that must give identical bits"""
    import scipy.sparse as sp
    klong = _k_long_row()
    g, n = 300, klong + 205
    rng = np.random.default_rng(int(dens * 100))
    y = _labels(n, "random", rng)
    for kind in ("gamma", "cancel"):
        X = _data(g, n, kind, y, rng)
        X[rng.random(X.shape) >= dens] = 0.0
        full = _data(3, n, kind, y, rng)
        X[7], X[40], X[41] = full[0], full[1], full[1]                    # stored everywhere: longer than kLongRow
        X[3, :] = 0.0
        X[5, y == 0] = 0.0
        X[20, :] = X[21, :]
        X[:, 11] = 0.0
        assert np.count_nonzero(X[7]) > klong and np.count_nonzero(X[20]) <= klong
        Xs = sp.csc_matrix(X)
        Xs.sort_indices()
        Gp, Gi = _singletons(g)
        out = hip_ctx.plaid_test_csc(Xs.indptr, Xs.indices, Xs.data, g, y, Gp, Gi, None, 1, 0)
        _check_singleton_fc(out, X, y, xs.MEAN_C_CSR, f"csc dens={dens} {kind}")
        assert out[3, 0] == 0.0
        er.assert_same_bits(out[20], out[21], "identical short rows")
        er.assert_same_bits(out[40], out[41], "identical long rows")


# ------------------------------------------------------------------------------------------------ d. p.one / p.two
@pytest.mark.parametrize("case", xs.CROSSPROD_CASES)
def test_one_and_two_sample_p_values_from_the_device_crossprod(hip_ctx, case):
    X, y, Gp, Gi = xs.crossprod_case(*case)
    ivs = xs.crossprod_intervals(X, y, Gp, Gi)
    nsep = 0
    for metap in (0, 1):
        out = hip_ctx.plaid_test(X, y, Gp, Gi, None, 3, metap)
        for j, (one, two) in enumerate(ivs):
            if one is None or two is None:
                nsep += 1
                continue
            assert xs.in_interval(out[j, 1], one), ("p.one", case, j, out[j, 1], one)
            assert xs.in_interval(out[j, 2], two), ("p.two", case, j, out[j, 2], two)
            lo, hi = 0.5 * (one[2] + two[2]), 0.5 * (one[3] + two[3])     # gsetFC = rowMeans(meanx, diff)
            slack = 8 * xs.U * (abs(lo) + abs(hi) + abs(one[2]) + abs(two[2]))
            assert lo - slack <= out[j, 0] <= hi + slack, ("gsetFC", case, j, out[j, 0], lo, hi)
            assert np.isnan(out[j, 3])
    assert nsep == 0
