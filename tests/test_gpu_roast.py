"""plaid.roast on the device (kernels_roast.hip, shard_limma.cpp: limma_worker with kRoast, roast_tail) -- `pytest -m gpu`.

What is checked, and against what (DESIGN.md section 27 has the derivations and the host measurements):
  1. roast_rotate_kernel against the 50-digit form on the device's own beta, RSS and residuals and on given W.  With
     zscore = "none", df0 = inf and s0^2 = 1 the kernel's output IS B (t = B / sqrt(1)): held within
     gamma_{n+1} (|beta r0| + sum |r_c w_c|), the bound of a chain of one product and n fma.  z (both z-scores, the fit's own
     prior and df0 = inf) within 4 x roast_ref.MEASURED["z"] of the 50-digit z, relative to max(1, |z|).  Rows 7 (the 8-byte
     path) and 8 (the 16-byte path); n = 5, 131, 260 with a `use` mask; p = 2 and 5; nrot = 1, 63, 64, 65, 130 with the
     chunk forced to 64 rotations (a second and a third launch); a constant gene, a gene outside the universe (NaN).  The
     padding of the last tile and what follows Z are not written.  Shapes past these: rows 515 (the 8-byte path) and 514
     (the 16-byte path), a second workgroup of 512 rows, with 65 rotations in chunks of 64 -- the device on all rows, the
     50-digit form on the first three rows, the last two of workgroup 0 and the rows of workgroup 1, at the same bounds.
  2. roast_stat_kernel / roast_mean50_kernel bit for bit against roast_ref.stats_np (mean50: the pinned threshold form) on
     given z: sets of 0, 1, 2, 3, 63, 64, 65, 300 members, one at the mean50 cap and one above it; two identical values
     straddling tau, all-equal z, +-0.0, z of one sign only; 70 rotations (a full and a partial tile).
  3. The counts b against numpy's on the device's own statistics, exactly; then end to end against the 50-digit reference,
     whose cases have no rotation within twice the allowance of the observed statistic (tests/test_roast_ref.py asserts
     it): b must match exactly, and the tables follow bit for bit from step 6.  One case has n_f - p + 1 = 135 > 128
     effects: PValue.Mixed is finite where plaid.fry returns NaN.
  4. 1, 2 and 3 shards on the hook: the rotation tiles are dealt to the shards, and the counts of the shards are added.  300
     rotations are five tiles (the last of 44 rotations): two shards take 2 + 3, three take 1 + 2 + 2; 64 rotations are one
     tile, so of three shards the first two have none and the tail reads shard 0's set sizes beside shard 2's counts.  All
     against the one-device call bit for bit -- and, so that the equality says something, an end-to-end case on three shards
     against the 50-digit reference's counts, and the sum of two half calls (supplied rotations 0 .. 127 and 128 .. 299)
     against the whole.  A failing shard; plaid_roast_contrasts against the single calls; generated against supplied
     rotations: bit for bit."""
import numpy as np
import pytest

import plaid_amd
from plaid_amd import _lib, engine
from tests.helpers import roast_ref as rr

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
STAT_ID = engine.ROAST_STATISTIC

# rows, n, p, masked, nrot
ROT_CASES = [(7, 5, 2, False, 1), (8, 5, 2, False, 63), (8, 131, 5, True, 64), (7, 260, 2, True, 65), (8, 260, 5, False, 130),
             (7, 131, 2, True, 130)]
ROT_IDS = ["x".join(str(int(v)) for v in c) for c in ROT_CASES]


def rot_case(rows, n, p, masked):
    rng = np.random.default_rng(100 * rows + n + p)
    X = np.round(rng.normal(size=(rows, n)) * 32) / 32 + np.outer(rng.normal(size=rows), np.arange(n) % 2)
    D = rr.make_design(n, p, rng)
    use = None
    if masked:
        use = np.ones(n, dtype=np.int8)
        use[rng.random(n) < 0.3] = 0
        use[:p + 4] = 1
        X[1, np.flatnonzero(use == 0)[0]] = np.nan             # a NaN where the fit does not look
    if n > 5:
        X[rows - 1, 0] = np.nan                                # a gene outside the universe
        X[2, :] = 3.0                                          # a constant gene: RSS = 0
    return X, D, use


def device_fit(ctx, X, D, use):
    """the device's own effects, RSS and raw residuals (rows x n) of one fit, with beta, t and the prior of the host finish"""
    import torch
    dev = torch.device("cuda", 0)
    rows, n = X.shape
    p = D.shape[1]
    ld = rows + (rows & 1)
    des = engine.limma_design(D, use, contrasts=np.eye(p)[:, 1], fit=1)
    nf = np.array([des["nf"]], dtype=np.int64)
    Ad = torch.full((n, ld), 777.0, dtype=torch.float64, device=dev)
    Ad[:, :rows] = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
    Qd = torch.from_numpy(np.ascontiguousarray(des["Q"].T)).to(dev)
    Ud = None if use is None else torch.from_numpy(np.ascontiguousarray(use)).to(dev)
    inv = torch.from_numpy(1.0 / nf.astype(np.float64)).to(dev)
    E = torch.full(((p + 1) * rows,), -7.0, dtype=torch.float64, device=dev)
    R = torch.full((rows,), -7.0, dtype=torch.float64, device=dev)
    Zd = torch.full((n, ld), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    uptr = None if Ud is None else Ud.data_ptr()
    ctx.dev_row_design_effects(Ad.data_ptr(), ld, rows, n, Qd.data_ptr(), uptr, inv.data_ptr(), p, 1, None, E.data_ptr())
    ctx.dev_row_design_rss(Ad.data_ptr(), ld, rows, n, Qd.data_ptr(), uptr, p, 1, E.data_ptr(), None, R.data_ptr())
    ctx.synchronize()
    Eh, Rh = E.cpu().numpy().reshape(p + 1, rows), R.cpu().numpy().reshape(1, rows)
    cg = engine.fry_divisors(Rh, nf, p, "none")                 # 1.0, or NaN outside the universe
    cgd = torch.from_numpy(cg).to(dev)
    ctx.dev_fry_residuals(Ad.data_ptr(), ld, rows, n, Qd.data_ptr(), uptr, p, 1, 0, E.data_ptr(), cgd.data_ptr(), Zd.data_ptr(), ld)
    ctx.synchronize()
    tab, hyp = engine.limma_finish(Eh, Rh, nf, des["v"][:, :, None], des["u"][:, None])
    ok = ~np.isnan(cg[0])
    beta = np.where(ok, tab[:, 0, 0, 0] / des["u"][0], np.nan)
    return {"Zd": Zd, "ld": ld, "Rz": np.ascontiguousarray(Zd.cpu().numpy()[:, :rows].T), "rss": Rh[0], "beta": beta, "ok": ok,
            "t": tab[:, 2, 0, 0], "d": float(hyp[0, 0]), "df0": float(hyp[0, 1]), "s02": float(hyp[0, 2])}


def device_rotate(ctx, fit, W, d, df0, s02, zscore, chunk):
    """z rows x nrot of plaidhip_dev_roast_rotate; asserts that nothing beside it was written"""
    import torch
    dev = torch.device("cuda", 0)
    rows, n = fit["Rz"].shape
    nrot = W.shape[1]
    ldw = (nrot + 15) // 16 * 16
    Wp = np.zeros((n + 1, ldw))
    Wp[:, :nrot] = W
    ntile = (nrot + 63) // 64
    Wd = torch.from_numpy(Wp).to(dev)
    bd = torch.from_numpy(np.ascontiguousarray(fit["beta"])).to(dev)
    rd = torch.from_numpy(np.ascontiguousarray(fit["rss"])).to(dev)
    Z = torch.full((ntile * rows * 64 + 5,), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.dev_roast_rotate(fit["Zd"].data_ptr(), fit["ld"], rows, n, bd.data_ptr(), rd.data_ptr(), Wd.data_ptr(), ldw, nrot, d, df0,
                         s02, engine.ROAST_ZSCORE[zscore], chunk, Z.data_ptr())
    ctx.synchronize()
    Zh = Z.cpu().numpy()
    assert (Zh[ntile * rows * 64:] == -7.0).all()
    T = Zh[:ntile * rows * 64].reshape(ntile, rows, 64)
    z = T.transpose(1, 0, 2).reshape(rows, ntile * 64)
    assert (z[:, nrot:] == -7.0).all()                          # the padding of the last tile is not written
    return z[:, :nrot]


@pytest.mark.parametrize("case", ROT_CASES, ids=ROT_IDS)
def test_rotate_kernel_against_the_50_digit_form(hip_ctx, case):
    rows, n, p, masked, nrot = case
    X, D, use = rot_case(rows, n, p, masked)
    fit = device_fit(hip_ctx, X, D, use)
    W = engine.roast_rotations(D, use, 0, nrot, seed=case[1])
    cols = sorted({k for k in (0, 1, 15, 16, 62, 63, 64, 65, 127, 128, 129) if k < nrot})
    chunk = 64 if nrot > 64 else 0
    gam = (n + 1) * U / (1 - (n + 1) * U)
    # B itself: zscore none, df0 = inf, s0^2 = 1
    got = device_rotate(hip_ctx, fit, W, fit["d"], np.inf, 1.0, "none", chunk)
    Bm, _, Ba = rr.rotate_mp(fit["beta"], fit["rss"], fit["Rz"], W[:, cols], fit["d"], np.inf, 1.0, "none")
    ok = fit["ok"]
    assert np.isnan(got[~ok]).all() and np.isfinite(got[ok]).all()
    err = np.abs(got[ok][:, cols] - Bm[ok])
    print(f"[rotate] {case}: worst |B - exact| / bound = {np.max(err / np.maximum(gam * Ba[ok], 1e-300)):.3g}")
    assert (err <= gam * Ba[ok]).all()
    if use is not None:                                         # the samples left out do not count: their weights are 0.0
        assert (fit["Rz"][:, use == 0] == 0.0).all()
    worst = 0.0
    for zscore in ("hill", "none"):
        for df0, s02 in ((fit["df0"], fit["s02"]), (np.inf, 0.75)):
            got = device_rotate(hip_ctx, fit, W, fit["d"], df0, s02, zscore, chunk)
            _, zm, _ = rr.rotate_mp(fit["beta"], fit["rss"], fit["Rz"], W[:, cols], fit["d"], df0, s02, zscore)
            assert np.isnan(got[~ok]).all()
            dev = rr.rel_dev(got[ok][:, cols], zm[ok])
            worst = max(worst, dev)
            assert dev <= rr.FACTOR * rr.MEASURED["z"], (zscore, df0, dev)
            assert np.isfinite(got[ok]).all() == np.isfinite(zm[ok]).all()
            whole = device_rotate(hip_ctx, fit, W, fit["d"], df0, s02, zscore, 0)       # the chunking changes no bit
            assert np.array_equal(whole.view(np.int64), got.view(np.int64))
    print(f"[rotate] {case}: worst z deviation {worst:.3g} (allowed {rr.FACTOR * rr.MEASURED['z']:.3g})")


# a second workgroup of 512 rows, holding three rows (the 8-byte path) and two (the 16-byte path); 65 rotations in chunks of 64
BLOCK_CASES = [(515, 131, 2, True, 65), (514, 131, 5, False, 65)]
BLOCK_IDS = ["x".join(str(int(v)) for v in c) for c in BLOCK_CASES]


@pytest.mark.parametrize("case", BLOCK_CASES, ids=BLOCK_IDS)
def test_rotate_kernel_past_one_workgroup_of_rows(hip_ctx, case):
    """the test above with the device on all rows and the 50-digit form on the first three rows, the last two of workgroup 0
    and the rows of workgroup 1 (rows are independent: beta, the RSS and the residuals are sliced), at the same bounds.
    Over the whole array: NaN exactly outside the universe, the last tile's padding and what follows Z unwritten
    (device_rotate), and the chunked call bit for bit the whole one."""
    rows, n, p, masked, nrot = case
    X, D, use = rot_case(rows, n, p, masked)
    fit = device_fit(hip_ctx, X, D, use)
    W = engine.roast_rotations(D, use, 0, nrot, seed=case[1])
    cols = sorted({k for k in (0, 1, 15, 16, 62, 63, 64) if k < nrot})
    pick = sorted({0, 1, 2, 510, 511, 512, 513, rows - 1})
    gam = (n + 1) * U / (1 - (n + 1) * U)
    ok = fit["ok"]
    okp = ok[pick]
    assert not ok[rows - 1] and ok[2] and ok[510:rows - 1].all()                  # the NaN gene is the last row of workgroup 1
    beta, rss, Rz = fit["beta"][pick], fit["rss"][pick], fit["Rz"][pick]
    got = device_rotate(hip_ctx, fit, W, fit["d"], np.inf, 1.0, "none", 64)
    Bm, _, Ba = rr.rotate_mp(beta, rss, Rz, W[:, cols], fit["d"], np.inf, 1.0, "none")
    assert np.isnan(got[~ok]).all() and np.isfinite(got[ok]).all()
    err = np.abs(got[pick][okp][:, cols] - Bm[okp])
    print(f"[measure] rotate {case}: worst |B - exact| / bound = {np.max(err / np.maximum(gam * Ba[okp], 1e-300)):.3g}")
    assert (err <= gam * Ba[okp]).all()
    if use is not None:
        assert (fit["Rz"][:, use == 0] == 0.0).all()
    worst = 0.0
    for zscore in ("hill", "none"):
        for df0, s02 in ((fit["df0"], fit["s02"]), (np.inf, 0.75)):
            got = device_rotate(hip_ctx, fit, W, fit["d"], df0, s02, zscore, 64)
            _, zm, _ = rr.rotate_mp(beta, rss, Rz, W[:, cols], fit["d"], df0, s02, zscore)
            assert np.isnan(got[~ok]).all()
            dev = rr.rel_dev(got[pick][okp][:, cols], zm[okp])
            worst = max(worst, dev)
            assert dev <= rr.FACTOR * rr.MEASURED["z"], (zscore, df0, dev)
            assert np.isfinite(got[pick][okp]).all() == np.isfinite(zm[okp]).all()
            whole = device_rotate(hip_ctx, fit, W, fit["d"], df0, s02, zscore, 0)       # the chunking changes no bit
            assert np.array_equal(whole.view(np.int64), got.view(np.int64))
    print(f"[measure] rotate {case}: worst z deviation {worst:.3g} (allowed {rr.FACTOR * rr.MEASURED['z']:.3g})")


# ---- the set statistics --------------------------------------------------------------------------------------------------------------
SIZES = [0, 1, 2, 3, 63, 64, 65, 300, engine.ROAST_MEAN50_MAX, engine.ROAST_MEAN50_MAX + 1]
_STAT = {}


def stat_case():
    """z (rows x 70) with the special columns, the sets, and the device's statistics of every kind -- made once"""
    if "z" not in _STAT:
        rng = np.random.default_rng(21)
        rows, nrot = engine.ROAST_MEAN50_MAX + 40, 70
        z = rng.normal(size=(rows, nrot))
        z[:, 1] = np.round(z[:, 1] * 2) / 2                      # many ties, and both zeros
        z[:, 1] = np.where((z[:, 1] == 0) & (np.arange(rows) % 2 == 1), -0.0, z[:, 1])
        z[:, 2] = 1.25                                           # all equal
        z[:, 3] = np.abs(z[:, 3])                                # one sign only
        z[:, 4] = -np.abs(z[:, 4])
        z[:, 69] = np.where(np.arange(rows) % 2, 0.0, -0.0)
        sets = [list(rng.choice(rows, size=k, replace=False)) for k in SIZES]
        for s in sets[4:8]:                                      # two identical genes straddling tau in every column
            srt = np.sort(z[s], axis=0)[::-1]
            z[s[0]] = z[s[-1]] = srt[len(s) // 2]
        _STAT.update(z=z, sets=sets, rows=rows, nrot=nrot)
    return _STAT


def tiles(z):
    rows, nrot = z.shape
    ntile = (nrot + 63) // 64
    T = np.full((ntile, rows, 64), -7.0)
    for t in range(ntile):
        w = min(64, nrot - 64 * t)
        T[t, :, :w] = z[:, 64 * t:64 * t + w]
    return T


def device_stats(ctx, z, sets, stat, obs=None):
    """(stat m x nrot x 4, cnt m x 4 or None)"""
    import torch
    dev = torch.device("cuda", 0)
    rows, nrot = z.shape
    Gp, Gi = rr.pattern(sets)
    m = len(sets)
    Zd = torch.from_numpy(tiles(z)).to(dev)
    Gpd, Gid = torch.from_numpy(Gp).to(dev), torch.from_numpy(np.concatenate([Gi, [0]]).astype(np.int32)).to(dev)
    S = torch.full((m * nrot * 4 + 3,), -7.0, dtype=torch.float64, device=dev)
    od = cd = None
    if obs is not None:
        od = torch.from_numpy(np.ascontiguousarray(obs)).to(dev)
        cd = torch.zeros((m * 4 + 2,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.dev_roast_stats(Zd.data_ptr(), rows, Gpd.data_ptr(), Gid.data_ptr(), m, STAT_ID[stat], nrot, S.data_ptr(),
                        None if od is None else od.data_ptr(), None if cd is None else cd.data_ptr())
    ctx.synchronize()
    Sh = S.cpu().numpy()
    assert (Sh[m * nrot * 4:] == -7.0).all()
    ch = None
    if cd is not None:
        ch = cd.cpu().numpy()
        assert (ch[m * 4:] == 0).all()
        ch = ch[:m * 4].reshape(m, 4)
    return Sh[:m * nrot * 4].reshape(m, nrot, 4), ch


@pytest.mark.parametrize("stat", rr.STATS)
def test_set_statistics_bit_for_bit_and_the_counts_exactly(hip_ctx, stat):
    c = stat_case()
    z, sets = c["z"], c["sets"]
    got, _ = device_stats(hip_ctx, z, sets, stat)
    for s, mem in enumerate(sets):
        want = rr.stats_np(z[mem], stat)
        if stat == "mean50" and len(mem) > engine.ROAST_MEAN50_MAX:
            want = np.full_like(want, np.nan)                    # above the cap
        same = np.array_equal(got[s].view(np.int64), want.view(np.int64)) or (
            np.isnan(want).all() and np.isnan(got[s]).all())
        assert same, (stat, len(mem), np.argwhere(got[s] != want)[:5], got[s][:3], want[:3])
    assert np.isnan(got[0]).all()                                # no member
    if stat == "mean50":
        assert not np.signbit(got[4:8, 69]).any()                # -0.0 never comes out of the keys
    # the observed column through the same kernel, then the counts
    obs, _ = device_stats(hip_ctx, z[:, :1].copy(), sets, stat)
    assert np.array_equal(obs[:, 0].view(np.int64), got[:, 0].view(np.int64))
    _, cnt = device_stats(hip_ctx, z, sets, stat, obs=obs[:, 0])
    with np.errstate(invalid="ignore"):
        want = (got >= obs[:, :1, :]).sum(axis=1)
    assert np.array_equal(cnt, want), (stat, cnt, want)
    assert (cnt[1:8] >= 1).all()                                 # rotation 0 is the observed column itself


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stat", rr.STATS)
@pytest.mark.parametrize("name", rr.E2E_CASES)
def test_end_to_end_counts_match_the_50_digit_reference(hip_ctx, name, stat):
    X, D, use, K, sets, W = rr.e2e_case(name)
    Gp, Gi = rr.pattern(sets)
    ref = rr.e2e_reference(name, stat)[0]
    for midp in (True, False):
        out, hyper = hip_ctx.roast(X, D, Gp, Gi, use, K, stat, zscore="hill", midp=midp, rotations=W)
        want = rr.finish_np(ref["cnt"], ref["msize"], ref["ndown"], ref["nup"], W.shape[1], stat, midp)
        got = out[:, :, 0, 0]
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), (name, stat, got, want)
    assert hyper[0, 4] == X.shape[0] - 1 and hyper[0, 5] == W.shape[1] and hyper[0, 6] == 0.0
    assert np.isnan(got[5, 1:]).all() and got[5, 0] == 0           # the empty set
    assert np.isnan(got[6, 1:]).all() and got[6, 0] == 0           # its only gene is outside the universe
    if name == "wide":                                             # 135 effects: above plaid.fry's cap of 128
        fry, fh = hip_ctx.fry(X, D, Gp, Gi, use, K)
        assert fh[0, 6] == 0.0 and np.isnan(fry[:, 5, 0, 0]).all()
        assert np.isfinite(got[[0, 1, 2, 3, 4, 7], 6]).all() and np.isfinite(got[[0, 1, 2, 3, 4, 7], 7]).all()


def test_generated_rotations_are_the_supplied_ones(hip_ctx):
    X, D, use, K, sets, _ = rr.e2e_case("b")
    Gp, Gi = rr.pattern(sets)
    W = engine.roast_rotations(D, use, 0, 130, seed=5)
    a, ha = hip_ctx.roast(X, D, Gp, Gi, use, K, "mean50", nrot=130, seed=5)
    b, hb = hip_ctx.roast(X, D, Gp, Gi, use, K, "mean50", rotations=W)
    assert np.array_equal(a.view(np.int64), b.view(np.int64)) and np.array_equal(ha.view(np.int64), hb.view(np.int64))
    c, _ = hip_ctx.roast(X, D, Gp, Gi, use, K, "mean50", nrot=130, seed=6)
    assert not np.array_equal(a[:, 4:], c[:, 4:], equal_nan=True)


# ---- sharding and the wrappers -----------------------------------------------------------------------------------------------------------
def shard_case():
    rng = np.random.default_rng(31)
    g, n, p = 40, 300, 2
    X = rng.normal(size=(g, n)) + 0.5 * np.outer(rng.normal(size=g), np.arange(n) % 2)
    X[g - 1, 299] = np.nan
    D = np.asfortranarray(np.stack([rr.make_design(n, p, rng), rr.make_design(n, p, rng)], axis=2))
    use = np.ones((n, 2), dtype=np.int8, order="F")
    use[rng.random(n) < 0.4, 1] = 0
    K = np.array([[0.0, 1.0, 1.0], [1.0, 0.0, -1.0]])
    sets = [list(rng.choice(g, size=k, replace=False)) for k in (1, 5, 17, 40)] + [[]]
    return X, D, use, K, sets


def counts_of(out, nrot):
    """b of the upordown and the mixed side from the p-values: p = (b + 1) / (nrot + 1)"""
    return np.rint(out[:, [4, 6]] * (nrot + 1) - 1)


@pytest.mark.parametrize("nrot", [300, 64])
@pytest.mark.parametrize("stat", ["mean50", "msq"])
def test_every_sharding_has_the_one_device_bits(hip_ctx, stat, nrot):
    X, D, use, K, sets = shard_case()
    Gp, Gi = rr.pattern(sets)
    out, hyper = hip_ctx.roast(X, D, Gp, Gi, use, K, stat, nrot=nrot, seed=2)
    assert out.shape == (5, 8, 3, 2) and np.isfinite(out[:4]).all() and np.isnan(out[4, 1:]).all()
    for nshards in (1, 2, 3):
        status, o2, h2 = rr.run_sharded(nshards, X, D, Gp, Gi, use, K, set_statistic=stat, nrot=nrot, seed=2)
        assert status == _lib.OK
        assert np.array_equal(o2.view(np.int64), out.view(np.int64)), nshards
        assert np.array_equal(h2.view(np.int64), hyper.view(np.int64)), nshards
    m1, _ = engine.roast_multi(X, D, Gp, Gi, use, K, stat, nrot=nrot, seed=2, devices=1)
    assert np.array_equal(m1.view(np.int64), out.view(np.int64))
    if nrot == 300:
        # the whole is the sum of its parts: the counts of rotations 0 .. 127 and of 128 .. 299, each a call of its own on
        # supplied rotations, add up to the counts of the call that three shards made together
        W = np.stack([engine.roast_rotations(D[:, :, f], use[:, f], f, nrot, seed=2) for f in range(2)], axis=2)
        a, _ = hip_ctx.roast(X, D, Gp, Gi, use, K, stat, rotations=W[:, :128])
        b, _ = hip_ctx.roast(X, D, Gp, Gi, use, K, stat, rotations=W[:, 128:])
        assert np.array_equal(counts_of(a[:4], 128) + counts_of(b[:4], 172), counts_of(out[:4], 300))
        assert (counts_of(a[:4], 128) + counts_of(b[:4], 172)).max() > 0


@pytest.mark.parametrize("stat", ["mean50", "floormean"])
def test_three_shards_match_the_50_digit_reference(hip_ctx, stat):
    """nrot = 40 is one tile: shard 2 counts, shards 0 and 1 add nothing, shard 0 brings the sizes and the proportions"""
    X, D, use, K, sets, W = rr.e2e_case("b")
    Gp, Gi = rr.pattern(sets)
    ref = rr.e2e_reference("b", stat)[0]
    status, out, hyper = rr.run_sharded(3, X, D, Gp, Gi, use, K, set_statistic=stat, rotations=W)
    assert status == _lib.OK
    want = rr.finish_np(ref["cnt"], ref["msize"], ref["ndown"], ref["nup"], W.shape[1], stat, True)
    assert np.array_equal(out[:, :, 0, 0].view(np.int64), want.view(np.int64))


def test_a_failing_shard_reports_and_writes_nothing(hip_ctx):
    X, D, use, K, sets = shard_case()
    Gp, Gi = rr.pattern(sets)
    status, out, hyper = rr.run_sharded(3, X, D, Gp, Gi, use, K, fail=1, nrot=64)
    assert status == _lib.EHIP
    assert (out == -7.0).all() and (hyper == -7.0).all()


def test_contrasts_wrapper_is_the_single_calls(hip_ctx):
    from tests.helpers import limma_ref as lr
    rng = np.random.default_rng(41)
    g, n = 30, 24
    X = plaid_amd.NamedMatrix(rng.normal(size=(g, n)), [f"g{i}" for i in range(g)], [f"s{i}" for i in range(n)])
    Y = rng.integers(0, 2, size=(n, 3)).astype(np.float64)
    Y[rng.random((n, 3)) < 0.15] = np.nan
    Y[:4] = [[0, 0, 0], [1, 1, 1], [0, 1, 0], [1, 0, 1]]
    Yn = plaid_amd.NamedMatrix(Y, X.colnames, ["a", "b", "c"])
    B = rng.normal(size=(n, 1))
    G = {f"set{k}": [f"g{i}" for i in rng.choice(g, size=5 + k, replace=False)] for k in range(6)}
    Ws = []
    for j in range(3):
        Dj, uj = lr.contrast_design(Y, B, j)
        Ws.append(engine.roast_rotations(Dj, uj, j, 99, seed=4))
    tabs, hyp = plaid_amd.plaid_roast_contrasts(X, Yn, G, B=B, nrot=99, seed=4, sort_by="none", ctx=hip_ctx)
    given, _ = plaid_amd.plaid_roast_contrasts(X, Yn, G, B=B, rotations=np.stack(Ws, axis=2), sort_by="none", ctx=hip_ctx)
    by_mixed, _ = plaid_amd.plaid_roast_contrasts(X, Yn, G, B=B, nrot=99, seed=4, sort_by="mixed", ctx=hip_ctx)
    for j, nm in enumerate(["a", "b", "c"]):
        Dj, uj = lr.contrast_design(Y, B, j)
        one, h1 = plaid_amd.plaid_roast(X, Dj, G, contrasts=np.array([0.0, 1.0, 0.0]), use=uj, rotations=Ws[j], sort_by="none",
                                        ctx=hip_ctx)
        assert tabs[nm].rownames == one["1"].rownames and tabs[nm].colnames == list(engine.ROAST_COLUMNS)
        assert np.array_equal(tabs[nm].values.view(np.int64), one["1"].values.view(np.int64)), nm
        assert np.array_equal(given[nm].values.view(np.int64), one["1"].values.view(np.int64)), nm
        assert hyp[nm] == h1
        assert (np.diff(by_mixed[nm].values[:, 6]) >= 0).all()
