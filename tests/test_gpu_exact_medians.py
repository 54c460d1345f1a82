"""Column medians bit for bit against an independent reference (R's median.default with normalize_medians' ignore.zero
rule, tests/helpers/exact_ref.py) -- `pytest -m gpu`.

Every kernel size class, the streaming kernel's many-columns shape, columns built so that the streaming kernel's sampled
bracket misses the middle rank or its candidate list overflows (both recomputed on the host from the kernel's own
sample, so the paths are provably taken), NaN / +-0 / +-Inf / DBL_MAX columns, and the medians the sparse crossprod
selects itself (fused_medians = on)."""
import numpy as np
import pytest

from tests.helpers import exact_ref as er

pytestmark = pytest.mark.gpu


def _check_shift(S, got, med, what):
    """got == (S - med) + add bit for bit, add within the sum bound of the exact mean of the non-NaN medians"""
    from fractions import Fraction
    ok = ~np.isnan(med)
    if not ok.any():
        return
    at = (S == med[None, :]) & np.isfinite(S)                 # where S - med == 0: got is add itself
    adds = got[at]
    if adds.size:
        add = adds[0]
        assert np.all(er.bits(adds) == er.bits(add)), what
    else:                                                      # no such element: the add that reproduces got
        with np.errstate(all="ignore"):
            d = S - med[None, :]
            fin = np.isfinite(d) & np.isfinite(got)
            add = (got - d)[fin][0]
            for _ in range(16):
                if np.array_equal(er.bits((d + add)[fin]), er.bits(got[fin])):
                    break
                add = np.nextafter(add, np.inf if (d + add)[fin][0] < got[fin][0] else -np.inf)
    fm = med[ok]
    if np.isfinite(fm).all():
        exact = float(sum((Fraction(float(v)) for v in fm), Fraction(0)) / len(fm))
        # a sum of cnt medians (cnt - 1 roundings), the division, the reference's rounding: (cnt + 2) u mean|med|
        assert abs(add - exact) <= (len(fm) + 2) * er.U * np.abs(fm).mean() + 2.0 ** -1074, (what, add, exact)
    with np.errstate(all="ignore"):
        exp = (S - med[None, :]) + add
    er.assert_same_bits(got, exp, what + " shifted matrix")


@pytest.mark.parametrize("m", [1, 2, 3, 64, 65, 1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097, 5000, 5120, 5121, 6144,
                               6145, 16384, 20000, 33000, 50000, 65536, 65537, 70000])
def test_medians_every_size_class_bit_exact(hip_ctx, m):
    """the data of test_medians_every_kernel_size_class (ties, zeros, an all-masked column, tied middle values, both
    parities), ignore.zero TRUE / FALSE / auto: the medians bit for bit, the shifted matrix exactly (S - med) + add"""
    rng = np.random.default_rng(m)
    n = 5
    S = np.round(rng.normal(size=(m, n)), 2)
    S[rng.random(S.shape) < 0.15] = 0.0
    S[:, 1] = np.abs(S[:, 1])
    if m > 3:
        S[:, 2] = 0.0
        S[: m // 2, 3] = 7.25
        S[m // 2:, 3] = -1.5
    for iz in (True, False, None):
        got, med = hip_ctx.normalize_medians(S, iz)
        er.assert_same_bits(med, er.col_medians(S, iz), f"m={m} iz={iz}")
        _check_shift(S, got, med, f"m={m} iz={iz}")
    Sp = np.abs(S)                                             # min(x) == 0: auto means ignore.zero
    Sp[0, 0] = -0.0
    got, med = hip_ctx.normalize_medians(Sp, None)
    er.assert_same_bits(med, er.col_medians(Sp, True), f"m={m} auto -0.0")


def test_streaming_medians_many_columns_bit_exact(hip_ctx):
    """the shape of test_streaming_medians_many_columns_per_wavefront (6,400 x 20,480: every wavefront walks several
    columns and reuses its candidate list): every median bit for bit"""
    rng = np.random.default_rng(5)
    m, n = 6400, 20480
    S = rng.normal(size=(m, n)) + np.linspace(-3.0, 3.0, n)[None, :]
    S[:, 1::7] = np.round(S[:, 1::7], 1)
    got, med = hip_ctx.normalize_medians(S, False)
    er.assert_same_bits(med, er.col_medians(S, False), "6400 x 20480")
    del got


# ---------------------------------------------------------------- the streaming kernel's rare paths
def _keys(v):
    u = er.bits(v + 0.0)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


def _bracket(col, iz):
    """restatement of the sampled start of col_medians_stream_kernel (kernels_medians.hip): None when the sample is not used,
    else (hit, keys inside [qa, qb], ccap)"""
    m = len(col)
    K = 16 if m > 32768 else 8
    idx = np.array([min(u * m // K + lane, m - 1) for u in range(K) for lane in range(64)])
    smp = col[idx]
    valid = ~np.isnan(smp) & ~((smp == 0.0) if iz else np.zeros(len(smp), dtype=bool))
    sk = np.sort(_keys(smp[valid]))
    ns = len(sk)
    mid = (ns - 1) >> 1 if ns > 0 else 0
    w = int(np.float32(4.0) * np.float32(0.5) * np.sqrt(np.float32(ns))) + 2
    if not (ns >= 256 and mid > w and mid + 1 + w < ns - 1):
        return None
    qa, qb = sk[mid - w], sk[mid + 1 + w]
    ok = ~np.isnan(col) & ~((col == 0.0) if iz else np.zeros(m, dtype=bool))
    ck = _keys(col[ok])
    cnt = len(ck)
    below = int(np.count_nonzero(ck < qa))
    inside = int(np.count_nonzero((ck >= qa) & (ck <= qb)))
    k_lo = (cnt - 1) >> 1
    hit = below <= k_lo and k_lo - below < inside
    ccap = ((m // 4 + 63) & ~63) if m > 4096 else 0
    return hit, inside, ccap


def _adversarial(m, seed):
    """about 40 columns of length m: (matrix, column kinds)"""
    rng = np.random.default_rng(seed)
    K = 16 if m > 32768 else 8
    sidx = np.unique(np.array([min(u * m // K + lane, m - 1) for u in range(K) for lane in range(64)]))
    cols, kinds = [], []

    def add(c, kind):
        cols.append(np.asarray(c, dtype=np.float64))
        kinds.append(kind)

    for r in range(3):                                         # the sample sits far above / below the rest: bracket misses
        c = rng.normal(size=m)
        c[sidx] = (100.0 if r != 1 else -100.0) + rng.normal(size=len(sidx))
        add(c, "miss")
    c = np.round(rng.normal(size=m), 1)
    c[sidx] = 5.0                                              # a tied sample: qa == qb, far from the middle
    add(c, "miss")
    for r in range(3):                                         # > m/4 values tied at the median: the list overflows
        c = rng.normal(size=m)
        tie = rng.choice(m, size=m // 3 + 7 * r, replace=False)
        c[tie] = 0.25 if r != 2 else 0.0
        add(c, "overflow")
    c = np.empty(m)                                            # ties end exactly at the lower middle: upper middle above
    nb = (m - 1) // 2 - m // 3
    order = rng.permutation(m)
    c[order[:nb]] = -rng.random(nb) - 1.0
    c[order[nb:nb + m // 3 + 1]] = 0.5
    c[order[nb + m // 3 + 1:]] = 2.0 + rng.random(m - nb - m // 3 - 1)
    if m % 2:
        c[order[-1]] = np.nan                                  # even valid count
    add(c, "overflow")
    add(np.where(np.arange(m) == m // 3, 4.5, np.nan), "one")
    add(np.full(m, np.nan), "nan")
    for r in range(2):
        c = rng.normal(size=m)
        c[rng.random(m) < 0.3 + 0.1 * r] = np.nan
        c[: 1 + r] = np.nan                                    # both parities of the valid count
        add(c, "nan")
    for r in range(3):                                         # +-0 at the median
        c = rng.normal(size=m)
        z = rng.choice(m, size=m // 5, replace=False)
        c[z] = np.where(rng.random(len(z)) < 0.5, 0.0, -0.0)
        if r == 1:
            c[0] = np.nan
        if r == 2:
            c[:2] = -0.0
        add(c, "zero")
    for r in range(4):                                         # +-Inf, some at the middle
        c = rng.normal(size=m)
        k = m // 2 + (1 if r % 2 else -1) * (r // 2)
        c[rng.choice(m, size=k, replace=False)] = np.inf if r < 2 else -np.inf
        add(c, "inf")
    c = rng.normal(size=m)
    c[: m // 2] = np.inf
    c[m // 2:] = -np.inf
    add(c, "inf")
    big = np.finfo(np.float64).max
    for r in range(3):                                         # two different middle values near DBL_MAX
        c = np.empty(m)
        lo_n = m // 2
        c[:lo_n] = big * (0.5 + 0.4 * rng.random(lo_n))
        c[lo_n - 1] = big * 0.9375
        c[lo_n:] = big
        if r == 1:
            c[lo_n:] = -big
            c[:lo_n] = -big * (0.5 + 0.4 * rng.random(lo_n))
            c[lo_n - 1] = -big * 0.9375
        if m % 2:
            c[-1] = np.nan
        if r == 2:
            c = -c
        add(rng.permutation(c), "dblmax")
    for r in range(17):                                        # plain columns with ties, both parities
        c = np.round(rng.normal(8.0, 0.2, size=m), 2)
        c[: r % 2] = np.nan
        add(c, "plain")
    return np.stack(cols, axis=1), kinds


@pytest.mark.parametrize("m", [6145, 20000, 32768, 32769, 50000])
def test_streaming_medians_adversarial_columns_bit_exact(hip_ctx, m):
    """bracket misses and candidate-list overflows (asserted on the host to happen), a single valid value, all-NaN and
    NaN-riddled columns, +-0 / +-Inf at the median, both parities, middle values near DBL_MAX: every median bit for
    bit, ignore.zero TRUE and FALSE"""
    S, kinds = _adversarial(m, m)
    n = S.shape[1]
    assert 38 <= n <= 45
    for j, kind in enumerate(kinds):
        if kind in ("miss", "overflow"):
            b = _bracket(S[:, j], False)
            assert b is not None, (j, kind)
            hit, inside, ccap = b
            if kind == "miss":
                assert not hit, (j, "the sampled bracket holds the middle rank")
            else:
                assert inside > ccap, (j, inside, ccap, "the candidate list does not overflow")
    for iz in (False, True):
        with np.errstate(all="ignore"):
            _, med = hip_ctx.normalize_medians(S, iz)
        exp = er.col_medians(S, iz)
        er.assert_same_bits(med, exp, f"m={m} iz={iz}")
    big_cols = [j for j, k in enumerate(kinds) if k == "dblmax"]
    assert np.isfinite(exp[big_cols]).all() and (np.abs(exp[big_cols]) > 1e308).all()


def test_fused_medians_equal_the_reference():
    """the medians the sparse crossprod selects itself (fused_medians = on, C3-like: 20,000 genes, 50,000 sets, rank
    weights, 1,100 samples) against the reference median of the very matrix it wrote -- not only against the
    standalone kernel"""
    import ctypes as C
    import torch
    import plaid_amd
    from plaid_amd import synth as sy
    g, m, n = 20000, 50000, 1100                               # (the launch calibrates on 256 columns: n >= 1,024)
    Gp, Gi = sy.geneset_csc(g, m)
    Xp, Xi, Xx = sy.sparse_columns(g, 0, n)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    ctx = plaid_amd.Context(0, stream.cuda_stream)
    gs = None
    try:
        ctx.set_option("spmm_sparse_kernel", "scatter")
        ctx.set_option("fused_medians", "on")
        gs = ctx.geneset(g, Gp, Gi)
        with torch.cuda.stream(stream):
            dp, di, dx = (torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                          for a in (Xp.astype(np.int32), Xi.astype(np.int32), Xx))
            vals = torch.empty_like(dx)
            colmax = torch.zeros(n, dtype=torch.float64, device=dev)
            gm = torch.zeros(1, dtype=torch.float64, device=dev)
            ctx.dev_colranks_csc(dp.data_ptr(), dx.data_ptr(), n, int(np.diff(Xp).max()), vals.data_ptr(), "average", False,
                                 1.25, colmax.data_ptr())
            ctx.dev_max(colmax.data_ptr(), n, gm.data_ptr())
            S = torch.empty((n, m), dtype=torch.float64, device=dev)
            fl = torch.zeros(4, dtype=torch.int32, device=dev)
            med = torch.full((n,), 12345.0, dtype=torch.float64, device=dev)
            ctx.dev_spmm_csc_fused(gs, dp.data_ptr(), di.data_ptr(), vals.data_ptr(), n, S.data_ptr(), m, "mean", 1.0, -0.5,
                                   fl.data_ptr(), None, gm.data_ptr(), nnz=len(Xx))
            ctx.dev_col_medians_resume(S.data_ptr(), m, m, n, None, med.data_ptr(), fl.data_ptr())
        torch.cuda.synchronize()
        nf, p_status, _, pending = ctx.dev_fused_medians_info()
        status = np.zeros(max(nf, 1), dtype=np.int32)
        if nf:
            ctx.lib.plaidhip_memcpy_d2h(ctx.handle, status.ctypes.data_as(C.c_void_p), C.c_void_p(p_status),
                                        C.c_size_t(4 * nf))
        Sh = S.cpu().numpy().T                                 # m x n
        mh = med.cpu().numpy()
    finally:
        if gs is not None:
            gs.close()
        ctx.close()
    assert not pending
    assert nf == n and status[:nf].sum() > 0, "no column's median came out of the crossprod launch"
    er.assert_same_bits(mh, er.col_medians(Sh, None), "fused")


@pytest.mark.parametrize("m", [2, 64, 1000, 4097, 6144, 6145, 70000])
def test_two_middle_values_near_dbl_max_give_the_finite_midpoint(hip_ctx, m):
    """a + b overflows for the two middle values: every kernel class returns (a + b) / 2 rounded once, as R does --
    0.5 * (a + b) was +-Inf"""
    big = np.finfo(np.float64).max
    rng = np.random.default_rng(m)
    cols = []
    for sign in (1.0, -1.0):
        c = np.empty(m)
        c[: m // 2] = big * (0.25 + 0.5 * rng.random(m // 2))
        c[m // 2 - 1] = big * 0.8125
        c[m // 2:] = big
        if m % 2:
            c[-1] = np.nan                                     # an even count of valid values
        cols.append(sign * rng.permutation(c))
    S = np.stack(cols, axis=1)
    _, med = hip_ctx.normalize_medians(S, False)
    exp = er.col_medians(S, False)
    assert np.array_equal(exp, [0.90625 * big, -0.90625 * big])
    er.assert_same_bits(med, exp, f"m={m}")
