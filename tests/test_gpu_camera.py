"""plaid.camera on the device (kernels_camera.hip, shard_limma.cpp: limma_worker with kCamera) -- `pytest -m gpu`.

Integer-valued X in -8 .. 8.  What is checked, and against what:
  1. Z of plaidhip_dev_camera_residuals is equal bit for bit to plaidhip_camera_residual_row (the same inline functions, on
     the host) on the device's own effects and residual sums of squares; a sample a fit leaves out and a gene that is not ok
     hold +0.0, the padding of Z past `rows` is untouched.
  2. plaidhip_dev_camera_sumsq against exact rational arithmetic (Fraction) on the device's own Z: T = G'Z exactly, the
     crossprod's per-element bound delta_c = (k + 1) 2^-53 sum |z| (tests/test_gpu_exact_sums.py), and the forward bound of
     camera_ref.sumsq_bound.  A seed of the first block continued over the rest has the bits of one call.
  3. End to end against limma's literal form at 50 digits (camera_ref.camera_mp: a complete QR, U = Q2'x) on the cases
     camera_ref.e2e_case (n_f >= p + 4, every s2 above 1e-3).  plaid.limma's own end-to-end bounds are measured ones and do
     not compose into a bound on VIF and t, so the allowance is 8 x the largest relative deviation of the plain numpy fp64
     restatement in the same pinned order (camera_ref.camera_np) from the 50-digit form over the same cases, measured on the
     host (tests/test_multi_camera_host.py re-measures it): VIF 4.25e-16, t 4.27e-15, Correlation 4.16e-16 (relative to
     max(|cor|, 1 / (m - 1))).  The order is fixed, so rounding, not scatter, is what is allowed for; nothing was measured
     on the device.  Down, Up and PValue are held to the t tail's own asserted accuracy at the device's T and df.camera.
  4. The fixed correlation is equal bit for bit to plaidhip_camera_finish fed from plaidhip_limma's own output and the
     crossprod of [t | ok].
  5. plaidhip_camera_multi's engine with 1, 2 and 3 shards, and with more shards than samples: the one-device bits; a
     failing shard's message.
  6. plaid_camera_contrasts column j equals plaid_camera on that contrast's design, bit for bit.

Shapes: n = 6, 127, 128, 130, 257 (no full block, one block less one, one block, a block and a tail, two blocks and a tail);
g = 1, 2 (one thread's row pair, the 16-byte path), 3, 301 (an odd last row, the 8-byte path) and 600 (the 16-byte path past
one workgroup of 512 rows); p = 1, 2, 4; nfit = 1 and 3 with different `use` columns and a NaN / Inf in a sample a fit leaves
out; sets of 0, 1, 2, 64, 65 and g members; a constant gene (s2 below the 1e-8 floor) and a gene with a NaN in a used sample.
For item 1 alone also P_CASES: p = 5 and 8, 9 and 16, 17 and 32 (both ends of the residual kernel's 8-, 16- and 32-register
instances) on g = 3 and 4 at n = 40 and 70.  For plaidhip_dev_camera_sumsq alone a planted T of integers in -8 .. 8 with m =
257 and 513 sets (past one and two workgroups of 256 sets), n = 130, leading dimension m + 3: the integer sum exactly."""
import numpy as np
import pytest

import plaid_amd
from plaid_amd import _lib, engine
from tests.helpers import camera_ref as cr
from tests.helpers import exact_stats as xs
from tests.helpers import limma_ref as lr

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
MEASURED = {"VIF": 4.25e-16, "t": 4.27e-15, "Correlation": 4.16e-16}   # camera_np against camera_mp, on the host
FACTOR = 8
BOUND = {k: FACTOR * v for k, v in MEASURED.items()}

# g, n, p, nfit
CASES = [(301, 130, 2, 3), (301, 257, 4, 1), (3, 6, 1, 1), (2, 127, 2, 1), (1, 128, 1, 1), (301, 127, 1, 3), (600, 130, 2, 1)]
IDS = ["x".join(str(v) for v in c) for c in CASES]
# every register count of the residual kernel past p = 4 (p <= 8, 16, 32, both ends of each), on three genes (the 8-byte path)
# and four (the 16-byte path): for test_z_is_the_host_entry_bit_for_bit alone
P_CASES = [(3, 40, 5, 1), (4, 40, 8, 2), (3, 40, 9, 1), (4, 70, 16, 1), (3, 70, 17, 2), (4, 70, 32, 1)]
P_IDS = ["x".join(str(v) for v in c) for c in P_CASES]


def make_case(g, n, p, nfit):
    """X, D (n x p x nfit), use (n x nfit or None), the sets: fit 0 uses every sample, the others leave about a quarter
    out; the samples fit 1 leaves out hold a NaN and an Inf; gene 0 is constant, the last gene has a NaN in a sample every fit
    uses (sample 0)"""
    rng = np.random.default_rng(1000 * g + 10 * n + p + nfit)
    X = cr.int_matrix(g, n, rng)
    D = np.stack([cr.make_design(n, p, rng) for _ in range(nfit)], axis=2)
    use = None
    if nfit > 1:
        use = np.ones((n, nfit), dtype=np.int8, order="F")
        for f in range(1, nfit):
            use[rng.random(n) < 0.25, f] = 0
            use[:p + 4, f] = 1
        out = np.flatnonzero(use[:, 1] == 0)
        X[rng.integers(0, g), out[0]] = np.nan
        X[rng.integers(0, g), out[-1]] = np.inf
    if g >= 3:
        X[0, :] = 5.0
        X[g - 1, 0] = np.nan
    sets = cr.make_sets(g, (0, 1, 2, 64, 65, g), rng)
    return X, np.asfortranarray(D), use, sets


def device_passes(ctx, X, D, use, sets, pad=0):
    """(E [W][rows], rss [nfit][rows], Z per fit (rows x n), ss per fit (m), T per fit (m x n), Q, nf) from the device entries, the
    matrices with leading dimension rows + (rows & 1) + pad and a canary past `rows`"""
    import torch
    dev = torch.device("cuda", 0)
    rows, n = X.shape
    p, nfit = D.shape[1], D.shape[2]
    W = nfit * (p + 1)
    ld = rows + (rows & 1) + pad
    Q = np.empty((n, p, nfit), order="F")
    nf = []
    for f in range(nfit):
        des = engine.limma_design(D[:, :, f], None if use is None else use[:, f], fit=f + 1)
        Q[:, :, f] = des["Q"]
        nf.append(des["nf"])
    nf = np.array(nf, dtype=np.int64)
    Gp, Gi = cr.pattern(sets)
    m = len(sets)
    Ad = torch.full((n, ld), 777.0, dtype=torch.float64, device=dev)
    Ad[:, :rows] = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
    Qd = torch.from_numpy(np.ascontiguousarray(Q.transpose(2, 1, 0))).to(dev)
    Ud = None if use is None else torch.from_numpy(np.ascontiguousarray(use.T)).to(dev)
    inv = torch.from_numpy(1.0 / nf.astype(np.float64)).to(dev)
    E = torch.full((W * rows + 5,), -7.0, dtype=torch.float64, device=dev)
    R = torch.full((nfit * rows + 5,), -7.0, dtype=torch.float64, device=dev)
    Zd = torch.full((n, ld), -7.0, dtype=torch.float64, device=dev)
    Td = torch.full((n, m + 3), -7.0, dtype=torch.float64, device=dev)
    ssd = torch.full((m + 5,), -7.0, dtype=torch.float64, device=dev)
    half = torch.full((m + 5,), -7.0, dtype=torch.float64, device=dev)
    fl = torch.zeros(4, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    uptr = None if Ud is None else Ud.data_ptr()
    ctx.dev_row_design_effects(Ad.data_ptr(), ld, rows, n, Qd.data_ptr(), uptr, inv.data_ptr(), p, nfit, None, E.data_ptr())
    ctx.dev_row_design_rss(Ad.data_ptr(), ld, rows, n, Qd.data_ptr(), uptr, p, nfit, E.data_ptr(), None, R.data_ptr())
    ctx.synchronize()
    gs = ctx.geneset(rows, Gp, Gi)
    Zs, Ts, sss, chained = [], [], [], []
    try:
        for f in range(nfit):
            ctx.dev_camera_residuals(Ad.data_ptr(), ld, rows, n, Qd.data_ptr(), uptr, p, nfit, f, E.data_ptr(), R.data_ptr(),
                                     float(nf[f] - p), Zd.data_ptr(), ld)
            ctx.dev_spmm_dense(gs, Zd.data_ptr(), ld, n, Td.data_ptr(), m + 3, "sum", 1.0, 0.0, fl.data_ptr())
            ctx.dev_camera_sumsq(Td.data_ptr(), m + 3, m, n, None, ssd.data_ptr())
            ctx.synchronize()
            Zall = Zd.cpu().numpy()
            assert (Zall[:, rows:] == -7.0).all()               # the padding of Z is not written
            Zs.append(np.ascontiguousarray(Zall[:, :rows].T))
            Tall = Td.cpu().numpy()
            assert (Tall[:, m:] == -7.0).all()
            Ts.append(np.ascontiguousarray(Tall[:, :m].T))
            sall = ssd.cpu().numpy()
            assert (sall[m:] == -7.0).all()
            sss.append(sall[:m].copy())
            # the first block alone, then the rest from that seed
            n0 = min(n, 128)
            ctx.dev_camera_sumsq(Td.data_ptr(), m + 3, m, n0, None, half.data_ptr())
            if n > n0:
                ctx.dev_camera_sumsq(Td.data_ptr() + 8 * (m + 3) * n0, m + 3, m, n - n0, half.data_ptr(), half.data_ptr())
            ctx.synchronize()
            chained.append(half.cpu().numpy()[:m].copy())
    finally:
        gs.close()
    Eh, Rh = E.cpu().numpy(), R.cpu().numpy()
    assert (Eh[W * rows:] == -7.0).all() and (Rh[nfit * rows:] == -7.0).all()
    return {"E": Eh[:W * rows].reshape(W, rows), "rss": Rh[:nfit * rows].reshape(nfit, rows), "Z": Zs, "T": Ts, "ss": sss,
            "chained": chained, "Q": Q, "nf": nf}


@pytest.fixture(scope="module")
def passes(hip_ctx):
    cache = {}

    def get(case):
        if case not in cache:
            X, D, use, sets = make_case(*case)
            cache[case] = (X, D, use, sets, device_passes(hip_ctx, X, D, use, sets, pad=2 if case[0] == 600 else 0))
        return cache[case]
    return get


@pytest.mark.parametrize("case", CASES + P_CASES, ids=IDS + P_IDS)
def test_z_is_the_host_entry_bit_for_bit(passes, case):
    X, D, use, sets, dv = passes(case)
    g, n, p, nfit = case
    for f in range(nfit):
        uf = None if use is None else use[:, f]
        d = float(dv["nf"][f] - p)
        want = np.stack([engine.camera_residual_row(X[r], dv["Q"][:, :, f], uf, dv["E"][f * (p + 1):f * (p + 1) + p, r],
                                                    dv["rss"][f, r], d) for r in range(g)])
        got = dv["Z"][f]
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), (f, np.argwhere(got != want)[:5])
        if uf is not None:
            assert (got[:, uf == 0] == 0.0).all()
        ok = np.isfinite(dv["rss"][f])
        assert (got[~ok] == 0.0).all() and not np.signbit(got[~ok]).any()
        if g >= 3:
            assert not ok[g - 1] and ok[0]                      # the NaN gene leaves; the constant gene stays, under the floor
            assert dv["rss"][f, 0] / d < 1e-8 and np.isfinite(got[0]).all()
        assert np.isfinite(got).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sum_of_squares_against_exact_rationals(passes, case):
    X, D, use, sets, dv = passes(case)
    g, n, p, nfit = case
    worst = 0.0
    for f in range(nfit):
        Z, T, ss = dv["Z"][f], dv["T"][f], dv["ss"][f]
        assert np.array_equal(dv["chained"][f].view(np.int64), ss.view(np.int64))     # the seed continues the one-call sum
        Tex = cr.exact_T(Z, sets)
        for s, members in enumerate(sets):
            k = len(members)
            mag = np.abs(Z[members]).sum(axis=0) if k else np.zeros(n)
            delta = (k + 1) * U * mag
            tex = np.array([float(t) for t in Tex[s]])
            assert (np.abs(T[s] - tex) <= delta + U * np.abs(tex)).all(), (f, s)        # the crossprod's own bound
            exact, bound = cr.sumsq_bound(Tex[s], delta)
            err = abs(float(cr.Fraction(float(ss[s])) - exact))
            assert err <= bound, (f, s, err, bound)
            if k == 0:
                assert ss[s] == 0.0
            worst = max(worst, err / bound if bound > 0 else 0.0)
    print(f"[measure] sum of T^2 {case}: worst error / bound {worst:.3g}")


@pytest.mark.parametrize("m", [257, 513])
def test_sum_of_squares_of_a_planted_t_past_one_workgroup_of_sets(hip_ctx, m):
    """plaidhip_dev_camera_sumsq alone: integers in -8 .. 8, so every square and every partial sum is an integer far below
    2^53 and the result is numpy's integer sum exactly; m = 257 and 513 sets (a second and a third workgroup of 256, the last
    holding one set), n = 130 (a column block and a tail of two), leading dimension m + 3"""
    import torch
    dev = torch.device("cuda", 0)
    n, ldt = 130, m + 3
    rng = np.random.default_rng(m)
    Ti = rng.integers(-8, 9, size=(m, n))
    Td = torch.full((n, ldt), -7.0, dtype=torch.float64, device=dev)
    Td[:, :m] = torch.from_numpy(np.ascontiguousarray(Ti.T.astype(np.float64))).to(dev)
    ssd = torch.full((m + 5,), -7.0, dtype=torch.float64, device=dev)
    half = torch.full((m + 5,), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    hip_ctx.dev_camera_sumsq(Td.data_ptr(), ldt, m, n, None, ssd.data_ptr())
    hip_ctx.dev_camera_sumsq(Td.data_ptr(), ldt, m, 128, None, half.data_ptr())           # the first block alone ...
    hip_ctx.dev_camera_sumsq(Td.data_ptr() + 8 * ldt * 128, ldt, m, n - 128, half.data_ptr(), half.data_ptr())   # ... then the rest
    hip_ctx.synchronize()
    ss, chained = ssd.cpu().numpy(), half.cpu().numpy()
    assert (ss[m:] == -7.0).all() and (chained[m:] == -7.0).all()                    # nothing past the last set is written
    assert np.array_equal(ss[:m], (Ti * Ti).sum(axis=1).astype(np.float64))
    assert np.array_equal(chained[:m].view(np.int64), ss[:m].view(np.int64))
    assert (Td.cpu().numpy()[:, m:] == -7.0).all()


@pytest.fixture(scope="module")
def e2e(hip_ctx):
    cache = {}

    def get(name, mode):
        if (name, mode) not in cache:
            X, D, use, K, sets = cr.e2e_case(name)
            Gp, Gi = cr.pattern(sets)
            cache[(name, mode)] = hip_ctx.camera(X, D, Gp, Gi, use, K, mode[0], mode[1])
        return cache[(name, mode)]
    return get


@pytest.mark.parametrize("mode", cr.E2E_MODES, ids=["estimated", "allow_neg", "fixed"])
@pytest.mark.parametrize("name", cr.E2E_CASES)
def test_end_to_end_against_limma_at_50_digits(e2e, name, mode):
    """camera_np against camera_mp over these cases, measured on the host: VIF 4.25e-16, t 4.27e-15, Correlation 4.16e-16;
    asserted: 8 x that (3.4e-15, 3.4e-14, 3.3e-15)"""
    out, hyper = e2e(name, mode)
    X, D, use, K, sets = cr.e2e_case(name)
    ref = cr.e2e_reference(name, mode, "mp")
    worst = {k: 0.0 for k in BOUND}
    for f in range(D.shape[2]):
        heavy = cr._e2e_heavy(name)[f]
        G = int(heavy[1][1].sum())
        assert hyper[f, 4] == G == hyper[f, 3]
        d0 = float(heavy[0]["df_prior"])
        dfc = min(hyper[f, 0] + d0, G - 2.0)
        assert abs(hyper[f, 5] - dfc) <= 1e-12 * dfc               # (df.prior is plaid.limma's, held there)
        for j, want in enumerate(ref[f]):
            got = out[:, :, j, f]
            dev = cr.deviation(got, want)
            for k in worst:
                worst[k] = max(worst[k], dev[k])
            acc = xs.ASSERTED_ACC["pt"]
            for s in np.flatnonzero(~np.isnan(got[:, 3])):
                half = float(xs.two_pt(got[s, 3], hyper[f, 5])) / 2
                lo, hi = (got[s, 4], got[s, 5]) if got[s, 3] < 0 else (got[s, 5], got[s, 4])
                assert abs(lo - half) <= acc * half and abs(hi - (1 - half)) <= acc * half + U, (f, j, s)
                assert got[s, 6] == 2 * min(got[s, 4], got[s, 5])
            fdr = lr.bh(got[:, 6])
            assert np.allclose(got[:, 7], fdr, rtol=4 * U, atol=0, equal_nan=True)
    print(f"[measure] end to end {name} {mode}: " + ", ".join(f"{k} {v:.3g} (bound {BOUND[k]:.3g})" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= BOUND[k], (k, v, BOUND[k])


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[6]], ids=[IDS[0], IDS[2], IDS[6]])
def test_fixed_correlation_is_the_host_finish_on_limmas_output(hip_ctx, case):
    X, D, use, sets = make_case(*case)
    g, n, p, nfit = case
    Gp, Gi = cr.pattern(sets)
    K = np.zeros((p, min(p, 2)))
    K[p - 1, 0] = 1.0
    if p > 1:
        K[0, 1], K[1, 1] = 0.5, -1.0
    q = K.shape[1]
    for rho in (0.01, -0.3):
        out, hyper = hip_ctx.camera(X, D, Gp, Gi, use, K, rho, False)
        lo, lh = hip_ctx.limma(X, D, use, K)
        assert np.array_equal(hyper[:, :4], lh, equal_nan=True)
        ok = ~np.isnan(lo[:, 5, 0, :])                              # genes x nfit
        t = lo[:, 2, :, :]                                          # genes x q x nfit
        B = np.concatenate([np.where(ok[:, None, :], t, 0.0).reshape((g, q * nfit), order="F"), ok.astype(np.float64)], axis=1)
        S = hip_ctx.plaid_dense(np.asfortranarray(B), Gp, Gi, "sum", False)
        sumt = S[:, :q * nfit].reshape((len(sets), q, nfit), order="F")
        cnt = S[:, q * nfit:]
        assert np.array_equal(cnt, np.array([[ok[s_, f].sum() for f in range(nfit)] for s_ in sets]))   # the counts are exact
        want, gdf = engine.camera_finish(t, ok, sumt, cnt, None, lh[:, 0], lh[:, 1], rho, False)
        assert np.array_equal(out.view(np.int64), want.view(np.int64))
        assert np.array_equal(hyper[:, 4:], gdf)


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[2]], ids=[IDS[0], IDS[1], IDS[2]])
def test_every_sharding_has_the_one_device_bits(hip_ctx, case):
    X, D, use, sets = make_case(*case)
    g, n, p, nfit = case
    Gp, Gi = cr.pattern(sets)
    for rho in (None, 0.01):
        out, hyper = hip_ctx.camera(X, D, Gp, Gi, use, None, rho, False)
        assert not (out == -7.0).any() and np.isnan(out[0, 1:]).all()           # the empty set's row
        for nshards in (1, 2, 3) + ((n + 3,) if n < 10 else ()):                # more shards than samples
            status, o2, h2 = cr.run_sharded(nshards, X, D, Gp, Gi, use, None, rho, False)
            assert status == _lib.OK
            assert np.array_equal(o2.view(np.int64), out.view(np.int64)), (rho, nshards)
            assert np.array_equal(h2.view(np.int64), hyper.view(np.int64)), (rho, nshards)


def test_a_failing_shard_reports_and_writes_nothing(hip_ctx):
    X, D, use, sets = make_case(*CASES[0])
    Gp, Gi = cr.pattern(sets)
    status, out, hyper = cr.run_sharded(3, X, D, Gp, Gi, use, None, None, False, fail=1)
    assert status == _lib.EHIP
    assert "injected failure" in _lib.load().plaidhip_last_error_string().decode()
    assert (out == -7.0).all() and (hyper == -7.0).all()


def test_contrasts_column_is_the_single_call_bit_for_bit(hip_ctx):
    rng = np.random.default_rng(77)
    g, n = 120, 40
    genes = [f"g{i}" for i in range(g)]
    X = plaid_amd.NamedMatrix(cr.int_matrix(g, n, rng), genes, [f"s{i}" for i in range(n)])
    Y = np.column_stack([rng.permutation(np.arange(n) % 2).astype(np.float64) for _ in range(3)])
    Y[rng.choice(n, size=6, replace=False), 1] = np.nan
    Y[rng.choice(n, size=9, replace=False), 2] = np.nan
    Yn = plaid_amd.NamedMatrix(Y, X.colnames, ["a", "b", "c"])
    B = rng.normal(size=(n, 1))
    G = {f"set{k}": [genes[i] for i in rng.choice(g, size=sz, replace=False)] for k, sz in enumerate((1, 2, 7, 30, 64, 65))}
    for rho in (None, 0.01):
        tabs, hyp = plaid_amd.plaid_camera_contrasts(X, Yn, G, B=B, inter_gene_cor=rho, sort_by="none", ctx=hip_ctx)
        sorted_tabs, _ = plaid_amd.plaid_camera_contrasts(X, Yn, G, B=B, inter_gene_cor=rho, ctx=hip_ctx)
        for j, nm in enumerate(["a", "b", "c"]):
            Dj, uj = lr.contrast_design(Y, B, j)
            one, h1 = plaid_amd.plaid_camera(X, Dj, G, contrasts=np.array([0.0, 1.0, 0.0]), use=uj, inter_gene_cor=rho,
                                             sort_by="none", ctx=hip_ctx)
            assert tabs[nm].rownames == one["1"].rownames
            assert np.array_equal(tabs[nm].values.view(np.int64), one["1"].values.view(np.int64)), (rho, nm)
            assert hyp[nm] == h1
            pv = sorted_tabs[nm].values[:, 5]
            assert (np.diff(pv[~np.isnan(pv)]) >= 0).all() and not np.isnan(pv[:np.sum(~np.isnan(pv))]).any()   # NaN last
            direction = tabs[nm].values[:, 4]
            assert set(np.unique(direction[~np.isnan(direction)])) <= {-1.0, 1.0}
    ic = plaid_amd.plaid_intergenecor(X, lr.contrast_design(Y, B, 0)[0], G, ctx=hip_ctx)
    tabs, _ = plaid_amd.plaid_camera_contrasts(X, Yn, G, B=B, inter_gene_cor=None, sort_by="none", ctx=hip_ctx)
    assert ic.colnames == ["NGenes", "Correlation", "VIF"]
    assert np.array_equal(ic.values.view(np.int64), tabs["a"].values[:, :3].view(np.int64))
