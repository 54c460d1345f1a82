"""plaid.limma with weights on the device (include/plaidhip.h: plaidhip_limma_w).

  1. every row against the 50-digit weighted least squares from the original design: logFC, u, sigma2 and AveExpr within the
     derived forward bound (tests/helpers/limma_w_ref.units); dfres, n.ok, df.pooled and which rows are NaN exactly
  2. t and P.Value end to end, composed as test_gpu_limma_na.test_end_to_end_against_50_digits composes them
  3. the device follows the header to the bit: H, b, M' and the counts of the device entry are the emulation's, and logFC and
     t are those of plaidhip_limma_w_solve on them
  4. the old paths: no weights -> the old entries' bits; weights of 0 and 1 against na = "fit"; array weights against the same
     values as a matrix; all weights times 4; all weights 1 against plaidhip_limma
  5. every sharding has the one-device bits; a failing shard writes nothing

Shapes: wr.CASES -- (rows, n, p, nfit) = (515, 300, 3, 3), (130, 131, 10, 2), (3, 130, 1, 1), (40, 7, 2, 1) -- and, for items
1 and 3, wr.P_CASES: (12, 131, 5, 1), (11, 131, 8, 2) and (12, 131, 9, 1) for the 8-register instance of the residual kernel
and the first p past it; (12, 40, 2, 9) and (11, 40, 1, 17) for a second and a third tile of 8 fits in the counts kernel, 9
and 17 fits in the solve, and weight-column tiles that straddle fits (Wc = 3, W = 51).  12 rows hold every designated row, 11
are odd (the 8-byte loads); (11, 131, 9, 1) for the residual kernel past p = 8 on the 8-byte loads.  Item 3 runs on ALL rows
and fits of P_CASES, item 1 on the first three of them;
tests/test_limma_w_ref.py establishes what both presume of these inputs without a device.
"""
import numpy as np
import pytest

import plaid_amd
from plaid_amd import _lib, engine
from tests.helpers import exact_ref as er
from tests.helpers import exact_stats as xs
from tests.helpers import limma_na_ref as nr
from tests.helpers import limma_ref as lr
from tests.helpers import limma_w_ref as wr

pytestmark = pytest.mark.gpu

U = lr.U
CASES, IDS = wr.CASES, wr.IDS
P_CASES, P_IDS = wr.P_CASES, wr.P_IDS
_CACHE = {}


def case_results(ctx, case):
    """the inputs of a case and the device's answer with both kinds of weights at once, computed once"""
    if case not in _CACHE:
        c = wr.make_case(case)
        c["w"] = ctx.limma(c["A"], c["D"], c["use"], c["K"], na="fit", max_na=0.2, weights=(c["Wt"], c["aw"]))
        c["des"] = [engine.limma_design(c["D"][:, :, f], wr.fit_use(c, f), c["K"], fit=f + 1) for f in range(case[3])]
        _CACHE[case] = c
    return _CACHE[case]


def _post(s2, d, hyper_f):
    d0, s0 = hyper_f[1], hyper_f[2]
    return s0 if np.isinf(d0) else s2 if d0 == 0 else (d * s2 + d0 * s0) / (d + d0)


def row_units(c, f, r, ref, eta):
    """the bound of section 28 for row r in fit f (ref: its mp_wls result)"""
    des = c["des"][f]
    uf = wr.fit_use(c, f)
    sel = np.arange(c["A"].shape[1]) if uf is None else np.flatnonzero(uf != 0)
    om = wr.omega(c["Wt"][r], c["aw"])
    hinv, Hn = wr.exact_H(des["Q"], om, ref["live"])
    return wr.units(c["A"][r], om, des["Q"], list(sel), des["v"], ref, hinv, Hn, eta[0], eta[1]), sel


designated = wr.designated
assert_other_rows_are_far_from_the_rule = wr.assert_other_rows_are_far_from_the_rule      # (tests/test_limma_w_ref.py runs it too)


@pytest.mark.parametrize("case", CASES + P_CASES[:3], ids=IDS + P_IDS[:3])
def test_rows_against_the_exact_reference(hip_ctx, case):
    c = case_results(hip_ctx, case)
    rows, n, p, nfit = case
    out, hyper, dfres = c["w"]
    q = c["K"].shape[1]
    assert_other_rows_are_far_from_the_rule(c, case)
    worst = dict(logFC=0.0, u=0.0, s2=0.0, ave=0.0)
    # the 50-digit reference of every row; of the 515-row case the designated rows and every fourth (the integers of all rows)
    check = sorted(designated(c) | set(range(0, rows, 4 if rows > 200 else 1)))
    for f in range(nfit):
        Df, uf = c["D"][:, :, f], wr.fit_use(c, f)
        okall, dall = wr.expected_integers(c["A"], c["Wt"], c["aw"], c["des"][f]["Q"], uf, 0.2)
        assert np.array_equal(~np.isnan(out[:, 0, 0, f]), okall), np.flatnonzero(~np.isnan(out[:, 0, 0, f]) != okall)
        assert np.array_equal(np.isnan(dfres[:, f]), ~okall) and np.array_equal(dfres[okall, f], dall[okall])
        assert np.isnan(out[~okall][:, :, :, f]).all()
        assert hyper[f, 3] == okall.sum() and hyper[f, 4] == dall[okall].sum()
        refs = dict(zip(check, wr.limma_w_mp(c["A"][check], c["Wt"][check], c["aw"], Df, uf, c["K"], max_na=0.2, tail=False)))
        assert [refs[r] is not None for r in check] == list(okall[check])
        eta = wr.basis_error(Df, uf, c["K"], c["des"][f])
        for r in [r for r in check if okall[r]]:
            ref = refs[r]
            assert dfres[r, f] == ref["d"]
            unit, sel = row_units(c, f, r, ref, eta)
            d = ref["d"]
            s2 = float(ref["rss"]) / d
            dev = abs(out[r, 5, 0, f] - s2) / (unit["rss"] / d + U * s2)
            worst["s2"] = max(worst["s2"], dev)
            assert dev <= 1.0, (r, f, out[r, 5, 0, f], s2)
            seen = c["A"][r][sel]
            seen = seen[~np.isnan(seen)]
            dev = abs(out[r, 1, 0, f] - float(ref["M"])) / ((len(sel) + 8) * U * np.abs(seen).mean())
            worst["ave"] = max(worst["ave"], dev)
            assert dev <= 1.0, (r, f, out[r, 1, 0, f], float(ref["M"]))
            for j in range(q):
                fc = float(ref["logFC"][j])
                dev = abs(out[r, 0, j, f] - fc) / (unit["logFC"][j] + U * abs(fc))
                worst["logFC"] = max(worst["logFC"], dev)
                assert dev <= 1.0, (r, f, j, out[r, 0, j, f], fc, unit["logFC"][j])
                uref = float(ref["u"][j])
                u_dev = out[r, 0, j, f] / (out[r, 2, j, f] * np.sqrt(_post(out[r, 5, j, f], float(d), hyper[f])))
                dev = abs(u_dev - uref) / (unit["u"][j] + 4 * U * uref)        # (u comes back through t: three more roundings)
                worst["u"] = max(worst["u"], dev)
                assert dev <= 1.0, (r, f, j, u_dev, uref, unit["u"][j])
    print(f"[measure] exact reference {case}: worst share of the bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    role = c["role"]
    for key in ("w_zero", "w_neg", "w_nan", "w_inf", "nan_beside"):
        if key in role and (key != "nan_beside" or n > 20):        # (two NaN of seven values are above max_na)
            assert np.isfinite(out[role[key]]).all(), key
    for key in ("group", "p_left", "inf_live"):
        if key in role and (key != "group" or p > 1):
            assert np.isnan(out[role[key], :, :, 0]).all() and np.isnan(dfres[role[key], 0]), key
    if "above" in role and n > 20:
        assert np.isnan(out[role["above"]]).all()


@pytest.mark.parametrize("case", CASES[1:], ids=IDS[1:])
def test_t_and_p_end_to_end_against_50_digits(hip_ctx, case):
    """fit by fit against limma_w_mp with the eBayes tail of limma_na_ref.mp_finish_na: df.prior and s2.prior at the bounds of
    tests/test_gpu_limma.BOUND; t at dfc / se + |t| (du / u + ds2 / s2 + e), e the share of the eBayes tail; P.Value through
    lr.dev_p against the 50-digit tail of the t that came back and, with t, over all rows at that test's bounds"""
    from tests.test_gpu_limma import BOUND
    c = case_results(hip_ctx, case)
    rows, n, p, nfit = case
    out, hyper, dfres = c["w"]
    q = c["K"].shape[1]
    mp = lr._mp()
    e_tail = 0.5 * (BOUND["df_prior"] + BOUND["s2_prior"]) + 4 * U
    worst = dict(df_prior=0.0, s2_prior=0.0, t_share=0.0, t=0.0, p=0.0, p_tail=0.0)
    for f in range(nfit):
        Df, uf = c["D"][:, :, f], wr.fit_use(c, f)
        ref = wr.limma_w_mp(c["A"], c["Wt"], c["aw"], Df, uf, c["K"], max_na=0.2)
        okref = np.array([row is not None for row in ref["rows"]])
        assert np.array_equal(~np.isnan(out[:, 0, 0, f]), okref)
        assert hyper[f, 3] == ref["nok"] and hyper[f, 4] == float(ref["df_pooled"])
        worst["df_prior"] = max(worst["df_prior"], lr.dev_rel(hyper[f, 1], float(ref["df_prior"])))
        worst["s2_prior"] = max(worst["s2_prior"], lr.dev_rel(hyper[f, 2], float(ref["s2_prior"])))
        eta = wr.basis_error(Df, uf, c["K"], c["des"][f])
        t_ref, p_ref, p_tail = (np.full((rows, q), np.nan) for _ in range(3))
        for r in np.flatnonzero(okref):
            row = ref["rows"][r]
            unit, _ = row_units(c, f, r, row["wls"], eta)
            d_s2 = unit["rss"] / row["d"]
            for j in range(q):
                tref, se = float(row["t"][j]), float(row["se"][j])
                d_t = unit["logFC"][j] / se + abs(tref) * (unit["u"][j] / float(row["u"][j]) + d_s2 / float(row["s2"]) + e_tail)
                worst["t_share"] = max(worst["t_share"], abs(out[r, 2, j, f] - tref) / d_t)
                assert abs(out[r, 2, j, f] - tref) <= d_t, (r, f, j, out[r, 2, j, f], tref, d_t)
                t_ref[r, j], p_ref[r, j] = tref, float(row["p"][j])
                with mp.workdps(lr.DPS):
                    p_tail[r, j] = float(xs.two_pt(mp.mpf(float(out[r, 2, j, f])), row["df_total"]))
        for j in range(q):
            worst["t"] = max(worst["t"], lr.dev_t(out[:, 2, j, f], t_ref[:, j]))
            np.testing.assert_array_equal(out[:, 4, j, f], lr.bh(out[:, 3, j, f]))
        worst["p"] = max(worst["p"], lr.dev_p(out[:, 3, :, f], p_ref))
        worst["p_tail"] = max(worst["p_tail"], lr.dev_p(out[:, 3, :, f], p_tail))
    print(f"[measure] end to end, weights {case}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert worst["df_prior"] <= BOUND["df_prior"] and worst["s2_prior"] <= BOUND["s2_prior"], worst
    assert worst["p_tail"] <= BOUND["p"], worst
    assert worst["t"] <= BOUND["t"] and worst["p"] <= BOUND["p"], worst


def device_sums(ctx, A, Wt, aw, Q, use, nf):
    """(S [nfit Wc][rows], cnt [2 nfit + 1][rows]) of plaidhip_dev_limma_w_sums on A and Wt (rows x n); sentinels are checked"""
    import torch
    dev = torch.device("cuda", 0)
    rows, n = A.shape
    _, p, nfit = Q.shape
    ld = rows + (rows & 1)
    W, C = nfit * (p * (p + 1) // 2 + p + 1), 2 * nfit + 1
    Ad = torch.full((n, ld), 777.0, dtype=torch.float64, device=dev)
    Ad[:, :rows] = torch.from_numpy(np.ascontiguousarray(A.T)).to(dev)
    Wd = torch.full((n, ld), 777.0, dtype=torch.float64, device=dev)
    Wd[:, :rows] = torch.from_numpy(np.ascontiguousarray(Wt.T)).to(dev)
    awd = torch.from_numpy(np.ascontiguousarray(aw)).to(dev)
    Qd = torch.from_numpy(np.ascontiguousarray(Q.transpose(2, 1, 0))).to(dev)
    Ud = None if use is None else torch.from_numpy(np.ascontiguousarray(use.T)).to(dev)
    inv = torch.from_numpy(1.0 / nf.astype(np.float64)).to(dev)
    S = torch.full((W * rows + 5,), -7.0, dtype=torch.float64, device=dev)
    Cn = torch.full((C * rows + 5,), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.dev_limma_w_sums(Ad.data_ptr(), Wd.data_ptr(), awd.data_ptr(), ld, rows, n, Qd.data_ptr(),
                         None if Ud is None else Ud.data_ptr(), inv.data_ptr(), p, nfit, None, S.data_ptr(), None, Cn.data_ptr())
    ctx.synchronize()
    s, k = S.cpu().numpy(), Cn.cpu().numpy()
    assert np.all(s[W * rows:] == -7.0) and np.all(k[C * rows:] == -7.0)
    return s[:W * rows].reshape(W, rows), k[:C * rows].reshape(C, rows)


def device_rss(ctx, A, Wt, aw, Q, use, G):
    """rss [nfit][rows] of plaidhip_dev_limma_w_rss at G [nfit (p + 1)][rows]"""
    import torch
    dev = torch.device("cuda", 0)
    rows, n = A.shape
    _, p, nfit = Q.shape
    ld = rows + (rows & 1)
    Ad = torch.full((n, ld), 777.0, dtype=torch.float64, device=dev)
    Ad[:, :rows] = torch.from_numpy(np.ascontiguousarray(A.T)).to(dev)
    Wd = torch.full((n, ld), 777.0, dtype=torch.float64, device=dev)
    Wd[:, :rows] = torch.from_numpy(np.ascontiguousarray(Wt.T)).to(dev)
    awd = torch.from_numpy(np.ascontiguousarray(aw)).to(dev)
    Qd = torch.from_numpy(np.ascontiguousarray(Q.transpose(2, 1, 0))).to(dev)
    Ud = None if use is None else torch.from_numpy(np.ascontiguousarray(use.T)).to(dev)
    Gd = torch.from_numpy(np.ascontiguousarray(G)).to(dev)
    R = torch.full((nfit * rows + 5,), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.dev_limma_w_rss(Ad.data_ptr(), Wd.data_ptr(), awd.data_ptr(), ld, rows, n, Qd.data_ptr(),
                        None if Ud is None else Ud.data_ptr(), p, nfit, Gd.data_ptr(), None, R.data_ptr())
    ctx.synchronize()
    r = R.cpu().numpy()
    assert np.all(r[nfit * rows:] == -7.0)
    return r[:nfit * rows].reshape(nfit, rows)


def test_the_device_follows_the_header_to_the_bit(hip_ctx):
    """a dozen rows of case (515, 300, 3, 3), the designated ones among them, in every fit: the device entry's H, b, M' and
    counts are the emulation's chains (three of the rows: the emulation is slow), and the device's logFC is the fma chain v .
    gamma of plaidhip_limma_w_solve's gamma on those sums, its t logFC / (u sqrt(s2.post)) of that entry's u, bit for bit;
    what is not estimable is not ok on both sides.  Then the residual entry at those gamma: sigma2 is its RSS / d_r, and the
    RSS is the emulation's chain, bit for bit"""
    case = CASES[0]
    c = case_results(hip_ctx, case)
    rows, n, p, nfit = case
    out, hyper, dfres = c["w"]
    pick = sorted(designated(c) - {c["role"]["above"]}) + [0, 1, 2, 20]
    assert len(pick) == 12
    Q = np.stack([d["Q"] for d in c["des"]], axis=2)
    nf = np.array([d["nf"] for d in c["des"]], dtype=np.int64)
    S, cnt = device_sums(hip_ctx, np.asfortranarray(c["A"][pick]), np.asfortranarray(c["Wt"][pick]), c["aw"], Q, c["use"], nf)
    T, Wc = p * (p + 1) // 2, p * (p + 1) // 2 + p + 1
    G = np.full((nfit * (p + 1), len(pick)), np.nan)
    seen_not_ok = 0
    for f in range(nfit):
        des = c["des"][f]
        sel = np.flatnonzero(c["use"][:, f] != 0)
        for i, r in enumerate(pick):
            Htri, b, Mp = S[f * Wc:f * Wc + T, i], S[f * Wc + T:f * Wc + T + p, i], S[f * Wc + T + p, i]
            om = wr.omega(c["Wt"][r], c["aw"])
            assert cnt[2 * f, i] == wr.live_mask(c["A"][r], om, c["use"][:, f]).sum()
            assert cnt[2 * f + 1, i] == (~np.isnan(c["A"][r][sel])).sum() and cnt[2 * nfit, i] == np.isnan(c["A"][r]).sum()
            if i in (0, 2, 11):
                eH, eb, eM, _, _ = wr.emulate_sums(c["A"][r], om, des["Q"], sel)
                assert np.array_equal(Htri, np.array(eH)) and np.array_equal(b, np.array(eb)) and Mp == eM, (r, f)
            got = engine.limma_w_solve(Htri, b, int(cnt[2 * f, i]), des["v"])
            if not got["ok"] or not np.isfinite(b).all():
                seen_not_ok += 1
                assert np.isnan(out[r, :, :, f]).all() and np.isnan(dfres[r, f]), (r, f)
                continue
            d = cnt[2 * f, i] - p
            assert dfres[r, f] == d
            assert out[r, 1, 0, f] == (Mp * len(sel)) / cnt[2 * f + 1, i]
            G[f * (p + 1):f * (p + 1) + p, i] = got["gamma"]
            fc = nr.emulate_logfc(des["v"], [float(t) for t in got["gamma"]])
            for j in range(2):
                assert out[r, 0, j, f] == fc[j], (r, f, j)
                t = fc[j] / (got["u"][j] * np.sqrt(_post(out[r, 5, j, f], float(d), hyper[f])))
                assert out[r, 2, j, f] == t, (r, f, j, out[r, 2, j, f], t)
    assert seen_not_ok >= 3          # the group, |live| = p and the live Inf in fit 1 (the Inf: in every fit that uses its sample)
    rss = device_rss(hip_ctx, np.asfortranarray(c["A"][pick]), np.asfortranarray(c["Wt"][pick]), c["aw"], Q, c["use"], G)
    checked = 0
    for f in range(nfit):
        sel = np.flatnonzero(c["use"][:, f] != 0)
        for i, r in enumerate(pick):
            if np.isnan(G[f * (p + 1), i]):
                continue
            assert out[r, 5, 0, f] == rss[f, i] / dfres[r, f], (r, f)
            if i in (0, 2, 11):
                om = wr.omega(c["Wt"][r], c["aw"])
                assert rss[f, i] == wr.emulate_w_rss(c["A"][r], om, c["des"][f]["Q"], sel, [float(t) for t in G[f * (p + 1):f * (p + 1) + p, i]])
                checked += 1
    assert checked == 9


@pytest.mark.parametrize("case", P_CASES, ids=P_IDS)
def test_every_p_instance_and_fit_tile_follows_the_header_to_the_bit(hip_ctx, case):
    """the test above on ALL rows and fits of wr.P_CASES: the 8-register residual kernel (p = 5, 8), the first p past it (9),
    and a second and a third tile of fits in the counts kernel (nfit = 9, 17).  H, b and M' of the device entry are the
    emulation's chains and the counts are numpy's; the call's logFC is the fma chain v . gamma of plaidhip_limma_w_solve's
    gamma on those sums and its t follows from that entry's u; dfres = |live| - p; sigma2 is the residual entry's RSS / d_r
    and that RSS is the emulation's chain.  A row above max_na, and a pair that is not estimable, is NaN on both sides."""
    c = case_results(hip_ctx, case)
    rows, n, p, nfit = case
    out, hyper, dfres = c["w"]
    q = c["K"].shape[1]
    Q = np.stack([d["Q"] for d in c["des"]], axis=2)
    nf = np.array([d["nf"] for d in c["des"]], dtype=np.int64)
    S, cnt = device_sums(hip_ctx, c["A"], c["Wt"], c["aw"], Q, c["use"], nf)
    T, Wc = p * (p + 1) // 2, p * (p + 1) // 2 + p + 1
    G = np.full((nfit * (p + 1), rows), np.nan)
    fitted = np.isnan(c["A"]).sum(axis=1) / n <= 0.2
    assert np.array_equal(cnt[2 * nfit], np.isnan(c["A"]).sum(axis=1))
    seen_not_ok = 0
    for f in range(nfit):
        des, uf = c["des"][f], wr.fit_use(c, f)
        sel = np.arange(n) if uf is None else np.flatnonzero(uf != 0)
        for r in range(rows):
            Htri, b, Mp = S[f * Wc:f * Wc + T, r], S[f * Wc + T:f * Wc + T + p, r], S[f * Wc + T + p, r]
            om = wr.omega(c["Wt"][r], c["aw"])
            assert cnt[2 * f, r] == wr.live_mask(c["A"][r], om, uf).sum(), (r, f)
            assert cnt[2 * f + 1, r] == (~np.isnan(c["A"][r][sel])).sum(), (r, f)
            eH, eb, eM, _, _ = wr.emulate_sums(c["A"][r], om, des["Q"], sel)
            er.assert_same_bits(Htri, eH, f"H of row {r}, fit {f}")
            er.assert_same_bits(b, eb, f"b of row {r}, fit {f}")
            assert Mp == eM, (r, f)
            got = engine.limma_w_solve(Htri, b, int(cnt[2 * f, r]), des["v"])
            if not fitted[r] or not got["ok"] or not np.isfinite(b).all():
                seen_not_ok += 1
                assert np.isnan(out[r, :, :, f]).all() and np.isnan(dfres[r, f]), (r, f)
                continue
            d = cnt[2 * f, r] - p
            assert dfres[r, f] == d
            assert out[r, 1, 0, f] == (Mp * len(sel)) / cnt[2 * f + 1, r]
            G[f * (p + 1):f * (p + 1) + p, r] = got["gamma"]
            fc = nr.emulate_logfc(des["v"], [float(t) for t in got["gamma"]])
            for j in range(q):
                assert out[r, 0, j, f] == fc[j], (r, f, j)
                t = fc[j] / (got["u"][j] * np.sqrt(_post(out[r, 5, j, f], float(d), hyper[f])))
                assert out[r, 2, j, f] == t, (r, f, j, out[r, 2, j, f], t)
    # fit 1 at least: |live| = p, the live Inf, the group without weight (p > 1), the row above max_na (12 rows)
    assert seen_not_ok >= 2 + (p > 1) + (rows > wr.ROLE["above"])
    rss = device_rss(hip_ctx, c["A"], c["Wt"], c["aw"], Q, c["use"], G)
    checked = 0
    for f in range(nfit):
        uf = wr.fit_use(c, f)
        sel = np.arange(n) if uf is None else np.flatnonzero(uf != 0)
        for r in range(rows):
            if np.isnan(G[f * (p + 1), r]):
                continue
            assert out[r, 5, 0, f] == rss[f, r] / dfres[r, f], (r, f)
            om = wr.omega(c["Wt"][r], c["aw"])
            gam = [float(t) for t in G[f * (p + 1):f * (p + 1) + p, r]]
            assert rss[f, r] == wr.emulate_w_rss(c["A"][r], om, c["des"][f]["Q"], sel, gam), (r, f)
            checked += 1
    assert checked == nfit * rows - seen_not_ok


def test_no_weights_is_the_old_entries_bits(hip_ctx):
    """weights = None through the wrappers runs plaidhip_limma / plaidhip_limma_na as before: their bits, called directly"""
    c = case_results(hip_ctx, CASES[1])
    lib = _lib.load()
    A = c["A"].copy(order="F")
    D, use = c["D"][:, :, 0], c["use"][:, 0]
    A[5, np.flatnonzero(use != 0)[3]] = np.nan            # (a sample that fit 1 uses)
    S = plaid_amd.NamedMatrix(A, [f"r{i}" for i in range(A.shape[0])], [f"s{i}" for i in range(A.shape[1])])
    o0, h0 = engine._limma(lib.plaidhip_limma, (hip_ctx.handle,), A, D, use, c["K"])
    o1, h1, d1 = engine._limma_na(lib.plaidhip_limma_na, (hip_ctx.handle,), A, D, use, c["K"], 0.2)
    tabs, hyper = plaid_amd.plaid_limma(S, D, contrasts=c["K"], use=use, ctx=hip_ctx, weights=None)
    tabf, hyperf = plaid_amd.plaid_limma(S, D, contrasts=c["K"], use=use, ctx=hip_ctx, na="fit", weights=None)
    for j, nm in enumerate(("1", "2")):
        er.assert_same_bits(tabs[nm].values, o0[:, :, j, 0], "propagate")
        er.assert_same_bits(tabf[nm].values[:, :6], o1[:, :, j, 0], "fit")
    assert hyper["df.prior"] == h0[0, 1] and hyperf["df.pooled"] == h1[0, 4]
    assert np.isnan(tabs["1"].values[5]).all() and np.isfinite(tabf["1"].values[5]).all()
    got = hip_ctx.limma(A, c["D"], c["use"], c["K"], na="fit", weights=None)
    ref = engine._limma_na(lib.plaidhip_limma_na, (hip_ctx.handle,), A, c["D"], c["use"], c["K"], 0.2)
    for a, b in zip(got, ref):
        er.assert_same_bits(a, b, "Context.limma without weights")


def test_weights_of_zero_and_one_against_na_fit(hip_ctx):
    """NaN at the zeros: the same live sets, so equal dfres everywhere; a dozen rows within the sum of both allowances (section
    28's bound and section 24's allowance, each against the 50-digit refit)"""
    case = CASES[0]
    c = case_results(hip_ctx, case)
    rows, n, p, nfit = case
    rng = np.random.default_rng(24)
    W01 = np.asfortranarray((rng.random((rows, n)) > 0.06).astype(np.float64))
    A = np.asfortranarray(np.nan_to_num(c["A"], nan=0.0, posinf=1.0))
    An = np.asfortranarray(np.where(W01 == 1.0, A, np.nan))
    ow, hw, dw = hip_ctx.limma(A, c["D"], c["use"], c["K"], na="fit", max_na=1.0, weights=W01)
    on, hn, dn = hip_ctx.limma(An, c["D"], c["use"], c["K"], na="fit", max_na=1.0)
    assert np.array_equal(dw, dn) and np.isfinite(dw).all()
    assert np.array_equal(hw[:, [0, 3, 4]], hn[:, [0, 3, 4]])
    worst = 0.0
    for r in range(12):
        f = r % nfit
        des, uf = c["des"][f], c["use"][:, f]
        sel = np.flatnonzero(uf != 0)
        ref = wr.mp_wls(A[r], W01[r], c["D"][:, :, f], uf, c["K"])
        eta = wr.basis_error(c["D"][:, :, f], uf, c["K"], des)
        hinv, Hn = wr.exact_H(des["Q"], W01[r], ref["live"])
        uw = wr.units(A[r], W01[r], des["Q"], list(sel), des["v"], ref, hinv, Hn, eta[0], eta[1])
        mis = [int(t) for t in sel if W01[r, t] == 0.0]
        un = nr.units(np.nan_to_num(An[r]), des["Q"], list(sel), mis, des["v"], {"u": [float(t) for t in ref["u"]]}, hinv)
        for j in range(2):
            allow = uw["logFC"][j] + nr.FACTOR * nr.RATIO_SEEN["logFC"] * un["logFC"][j]
            worst = max(worst, abs(ow[r, 0, j, f] - on[r, 0, j, f]) / allow)
            assert abs(ow[r, 0, j, f] - on[r, 0, j, f]) <= allow, (r, f, j)
        allow = (uw["rss"] + nr.FACTOR * nr.RATIO_SEEN["rss"] * un["rss"]) / ref["d"]
        assert abs(ow[r, 5, 0, f] - on[r, 5, 0, f]) <= allow, (r, f)
        assert ow[r, 1, 0, f] != on[r, 1, 0, f] or not mis     # AveExpr: a value under a zero weight still counts
    print(f"[measure] 0 / 1 weights against na = fit: worst share of both allowances, logFC {worst:.3g}")


def test_array_weights_scaling_and_unit_weights(hip_ctx):
    case = CASES[0]
    c = case_results(hip_ctx, case)
    rows, n, p, nfit = case
    A = np.asfortranarray(np.nan_to_num(c["A"], nan=0.0, posinf=1.0))
    # a vector of array weights against the same values as a full matrix: the same bits
    va = hip_ctx.limma(A, c["D"], c["use"], c["K"], na="fit", weights=c["aw"])
    vm = hip_ctx.limma(A, c["D"], c["use"], c["K"], na="fit", weights=np.broadcast_to(c["aw"], (rows, n)).copy(order="F"))
    for a, b in zip(va, vm):
        er.assert_same_bits(a, b, "array weights as a matrix")
    # all weights times 4: the same logFC, AveExpr and dfres to the bit, sigma2 times 4 exactly
    Wt = np.asfortranarray(np.where(np.isfinite(c["Wt"]), c["Wt"], 0.0))
    w1 = hip_ctx.limma(A, c["D"], c["use"], c["K"], na="fit", weights=(Wt, c["aw"]))
    w4 = hip_ctx.limma(A, c["D"], c["use"], c["K"], na="fit", weights=(Wt * 4.0, c["aw"]))
    er.assert_same_bits(w4[0][:, :2], w1[0][:, :2], "weights x 4: logFC and AveExpr")
    er.assert_same_bits(w4[0][:, 5], w1[0][:, 5] * 4.0, "weights x 4: sigma2")
    er.assert_same_bits(w4[2], w1[2], "weights x 4: dfres")
    assert np.array_equal(np.isnan(w1[0][:, 0, 0, 0]), np.isnan(w4[0][:, 0, 0, 0])) and np.isnan(w1[0][c["role"]["group"], 0, 0, 0])
    # all weights 1 and no NaN: not the bits of plaidhip_limma, but its integers, and its values within the bound
    o1, h1, d1 = hip_ctx.limma(A, c["D"], c["use"], c["K"], na="fit", weights=np.ones(n))
    o0, h0 = hip_ctx.limma(A, c["D"], c["use"], c["K"])
    nf = (c["use"] != 0).sum(axis=0)
    assert np.array_equal(d1, np.broadcast_to((nf - p).astype(np.float64), d1.shape))
    assert np.array_equal(h1[:, [0, 3]], h0[:, [0, 3]]) and np.array_equal(h1[:, 4], h0[:, 3] * h0[:, 0])
    one = np.ones(n)
    for r in range(12):
        f = r % nfit
        des, uf = c["des"][f], c["use"][:, f]
        sel = np.flatnonzero(uf != 0)
        ref = wr.mp_wls(A[r], one, c["D"][:, :, f], uf, c["K"])
        eta = wr.basis_error(c["D"][:, :, f], uf, c["K"], des)
        hinv, Hn = wr.exact_H(des["Q"], one, ref["live"])
        uw = wr.units(A[r], one, des["Q"], list(sel), des["v"], ref, hinv, Hn, eta[0], eta[1])
        mag = np.abs(A[r][sel]) @ np.abs(des["Q"][sel])
        for j in range(2):
            allow = uw["logFC"][j] + float(np.abs(des["v"][:, j]) @ lr.effects_bound(mag, len(sel)))
            assert abs(o1[r, 0, j, f] - o0[r, 0, j, f]) <= allow, (r, f, j)
        assert abs(o1[r, 5, 0, f] - o0[r, 5, 0, f]) <= 2 * uw["rss"] / ref["d"]


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[3]], ids=[IDS[0], IDS[1], IDS[3]])
def test_every_sharding_has_the_one_device_bits(hip_ctx, case):
    c = case_results(hip_ctx, case)
    one = c["w"]
    if case == CASES[3]:
        assert np.isfinite(one[0]).any()
    for nshards in ((2, 9) if case[1] == 7 else (1, 2, 3, 5)):       # (n = 7: more shards than samples)
        status, out, hyper, dfres = wr.run_sharded(nshards, c["A"], (c["Wt"], c["aw"]), c["D"], c["use"], c["K"], max_na=0.2)
        assert status == _lib.OK
        er.assert_same_bits(out, one[0], f"{nshards} shards")
        er.assert_same_bits(hyper, one[1], f"{nshards} shards, hyper")
        er.assert_same_bits(dfres, one[2], f"{nshards} shards, dfres")


def test_a_failing_shard_reports_and_writes_nothing(hip_ctx):
    c = case_results(hip_ctx, CASES[0])
    status, out, hyper, dfres = wr.run_sharded(3, c["A"], (c["Wt"], c["aw"]), c["D"], c["use"], c["K"], fail=1)
    text = _lib.load().plaidhip_last_error_string().decode()
    assert status == _lib.EHIP and "injected failure" in text, (status, text)
    assert (out == -7).all() and (hyper == -7).all() and (dfres == -7).all()
