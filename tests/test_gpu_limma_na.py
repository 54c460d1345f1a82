"""plaid.limma with na = "fit" on the device (include/plaidhip.h: plaidhip_limma_na).

  1. no missing value anywhere: every bit of na = "propagate"
  2. complete rows beside incomplete ones keep the bits of "propagate"; NaN / Inf in samples no fit uses change nothing
  3. incomplete rows against the parent path: today's plaid_limma on that row alone with use = sel \\ mis
  4. end to end against limma_na_mp at 50 digits, dfres / df.pooled / df.prior / s2.prior included
  5. the rows that must be NaN (above max_na, not estimable, no residual df, a used Inf); max_na = 0 and 1
  6. every sharding has the one-device bits; a failing shard writes nothing
  7. plaid_limma_contrasts on the 50-cell fixture with 5 % NaN: every contrast is its own plaid_limma(na = "fit")
  8. the device's gamma and u are those of plaidhip_limma_na_solve on the same Q rows and E', bit for bit

Shapes: CASES -- (rows, n, p, nfit) = (515, 300, 3, 3), (130, 131, 8, 2), (130, 300, 2, 3) -- and, for items 1, 2 and 5,
P_CASES = (60, 131, 10, 1), (61, 131, 9, 2): p = 9 and 10 run the 16-register instance of the residual kernel with the NaN
select, which no case with p <= 8 launches, and (61, 131, 8, 1): its 8-register instance on an odd number of rows (the 8-byte
loads); 60 rows are the fewest that hold ROLE, SINGLES and SPREAD.
"""
import numpy as np
import pytest

import plaid_amd
from plaid_amd import _lib, engine
from tests.helpers import exact_ref as er
from tests.helpers import exact_stats as xs
from tests.helpers import limma_na_ref as nr
from tests.helpers import limma_ref as lr

pytestmark = pytest.mark.gpu

U = lr.U
# rows, n, p, nfit: past a 64-lane tile, odd (the narrow loads) and even (the wide ones); ragged past one and two blocks of 128
CASES = [(515, 300, 3, 3), (130, 131, 8, 2), (130, 300, 2, 3)]
IDS = [f"rows{c[0]}-n{c[1]}-p{c[2]}-nfit{c[3]}" for c in CASES]
# past eight coefficients (p = 9, 10: the 16-register instance of the residual kernel with the NaN select), at the fewest rows that
# hold ROLE, SINGLES and SPREAD; even and odd.  Held to na = "propagate", whose p = 9 is held to exact sums in test_gpu_limma.py
P_CASES = [(60, 131, 10, 1), (61, 131, 9, 2)]
# (appended) the 8-register instance with the NaN select on the 8-byte loads (5 <= p <= 8, odd rows), which no case above launches;
# 131 columns: the walk crosses one block boundary and ends in a tail of 3
P_CASES += [(61, 131, 8, 1)]
P_IDS = [f"rows{c[0]}-n{c[1]}-p{c[2]}-nfit{c[3]}" for c in P_CASES]
ROLE = {"c0": 0, "c127": 1, "c128": 2, "clast": 3, "four": 4, "group": 5, "all": 6, "unused": 7, "inf_used_nan": 8,
        "inf_unused": 9, "inf_used": 10, "above": 11, "p_left": 12}
SINGLES = range(20, 40)       # one NaN per row, anywhere
SPREAD = range(40, 60)        # 3 - 12 % NaN
_CACHE = {}


def make_case(case):
    """designs [1, group, covariates], use (every fit leaves samples out; the columns in `never` are used by no fit), the
    complete matrix A0 and A with the NaN and Inf of ROLE / SINGLES / SPREAD; K: two contrasts"""
    rows, n, p, nfit = case
    rng = np.random.default_rng(list(case))
    D = np.empty((n, p, nfit), order="F")
    use = np.ones((n, nfit), dtype=np.int8, order="F")
    never = [5, n - 2]
    for f in range(nfit):
        D[:, 0, f] = 1.0
        D[:, 1, f] = rng.permutation(np.arange(n) % 2)
        D[:, 2:, f] = rng.normal(size=(n, p - 2))
        use[rng.random(n) < 0.2, f] = 0
        use[[0, 10, 127, 128, n - 1], f] = 1
        use[never, f] = 0
    A0 = rng.normal(size=(rows, n)) * np.exp(0.5 * rng.normal(size=(rows, 1))) + rng.normal(size=(rows, 1))
    A = A0.copy()
    A[ROLE["c0"], 0] = A[ROLE["c127"], 127] = A[ROLE["c128"], 128] = A[ROLE["clast"], n - 1] = np.nan
    A[ROLE["four"], [0, 127, 128, n - 1]] = np.nan
    A[ROLE["group"], np.flatnonzero((D[:, 1, 0] == 1) & (use[:, 0] != 0))] = np.nan      # fit 1 loses its group column
    A[ROLE["all"], :] = np.nan
    A[ROLE["unused"], never] = np.nan
    A[ROLE["inf_used_nan"], 10], A[ROLE["inf_used_nan"], 0] = np.inf, np.nan
    A[ROLE["inf_unused"], never[0]] = -np.inf
    A[ROLE["inf_used"], 10] = np.inf
    A[ROLE["above"], rng.permutation(n)[: int(0.25 * n) + 1]] = np.nan
    A[ROLE["p_left"], rng.permutation(np.flatnonzero(use[:, 0] != 0))[p:]] = np.nan           # fit 1 keeps p samples
    for r in SINGLES:
        A[r, rng.integers(n)] = np.nan
    for r in SPREAD:
        A[r, rng.permutation(n)[: rng.integers(int(0.03 * n), int(0.12 * n))]] = np.nan
    K = np.zeros((p, 2), order="F")
    K[1, 0], K[1, 1], K[0, 1] = 1.0, 1.0, -0.5
    return dict(D=D, use=use, A0=np.asfortranarray(A0), A=np.asfortranarray(A), K=K, never=never)


def case_results(ctx, case):
    """the inputs and the device's answers of a case, computed once: "propagate" and "fit" (max_na 0.2 and 1) on A"""
    if case not in _CACHE:
        c = make_case(case)
        c["prop"] = ctx.limma(c["A"], c["D"], c["use"], c["K"])
        c["fit"] = ctx.limma(c["A"], c["D"], c["use"], c["K"], na="fit", max_na=0.2)
        c["fit1"] = ctx.limma(c["A"], c["D"], c["use"], c["K"], na="fit", max_na=1.0)
        _CACHE[case] = c
    return _CACHE[case]


def pair_state(c, r, f, max_na):
    """(fitted by max_na, the missing samples inside the fit's sel, sel)"""
    x = c["A"][r]
    sel = np.flatnonzero(c["use"][:, f] != 0)
    return np.isnan(x).sum() / len(x) <= max_na, [int(t) for t in sel[np.isnan(x[sel])]], sel


@pytest.mark.parametrize("case", CASES + P_CASES, ids=IDS + P_IDS)
def test_without_missing_values_fit_is_propagate(hip_ctx, case):
    c = case_results(hip_ctx, case)
    out0, hyper0 = hip_ctx.limma(c["A0"], c["D"], c["use"], c["K"])
    out1, hyper1, dfres = hip_ctx.limma(c["A0"], c["D"], c["use"], c["K"], na="fit")
    er.assert_same_bits(out1, out0, "out")
    er.assert_same_bits(hyper1[:, :4], hyper0, "hyper")
    nf = (c["use"] != 0).sum(axis=0)
    assert np.array_equal(dfres, np.broadcast_to((nf - case[2]).astype(np.float64), dfres.shape))
    assert np.array_equal(hyper1[:, 4], hyper0[:, 3] * hyper0[:, 0])


@pytest.mark.parametrize("case", CASES + P_CASES, ids=IDS + P_IDS)
def test_complete_rows_keep_the_bits_of_propagate(hip_ctx, case):
    c = case_results(hip_ctx, case)
    rows, n, p, nfit = case
    (outp, _), (outf, hyper, dfres) = c["prop"], c["fit"]
    seen = 0
    for f in range(nfit):
        for r in range(rows):
            fitted, mis, sel = pair_state(c, r, f, 0.2)
            if fitted and not mis:
                seen += 1
                for col in (0, 1, 5):                      # logFC, AveExpr, sigma2
                    er.assert_same_bits(outf[r, col, :, f], outp[r, col, :, f], f"row {r} fit {f} column {col}")
                if np.isfinite(outp[r, 5, 0, f]):
                    assert dfres[r, f] == len(sel) - p
                else:                                      # (a used Inf)
                    assert np.isnan(dfres[r, f])
    assert seen > nfit * (rows - 60)
    # NaN / Inf only in samples that no fit uses: nothing changes at all
    B = c["A"].copy(order="F")
    B[ROLE["unused"], c["never"]] = 1.0
    B[ROLE["inf_unused"], c["never"][0]] = 1.0
    out2, hyper2, dfres2 = hip_ctx.limma(B, c["D"], c["use"], c["K"], na="fit", max_na=0.2)
    er.assert_same_bits(out2, outf, "values in unused samples")
    er.assert_same_bits(hyper2, hyper, "values in unused samples, hyper")
    er.assert_same_bits(dfres2, dfres, "values in unused samples, dfres")
    assert np.isfinite(outf[ROLE["unused"]]).all() and np.isfinite(outf[ROLE["inf_unused"]]).all()


def _post(s2, d, hyper_f):
    d0, s0 = hyper_f[1], hyper_f[2]
    return s0 if np.isinf(d0) else s2 if d0 == 0 else (d * s2 + d0 * s0) / (d + d0)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_incomplete_rows_against_the_parent_path(hip_ctx, case):
    """a dozen incomplete (row, fit) pairs: plaid_limma as it stands (the per-fit QR route) on that row alone with use =
    sel \\ mis.  logFC, u, sigma2 and AveExpr agree within the section 24 allowance of the refit (FACTOR x RATIO_SEEN x
    nr.units) plus that route's own lr.effects_bound and lr.rss_bound.  u of the refit is recovered from t = logFC / (u
    sqrt(s2.post)) and held to the section 24 allowance alone."""
    c = case_results(hip_ctx, case)
    rows, n, p, nfit = case
    outf, hyper, dfres = c["fit1"]
    pairs = [(ROLE[k], 0) for k in ("c0", "c127", "c128", "clast", "four")] + [(ROLE["group"], 1), (ROLE["above"], nfit - 1)]
    for r in [t for two in zip(SINGLES, SPREAD) for t in two]:   # up to a dozen: the first fit in which the row misses a used sample
        hit = [f for f in range(nfit) if pair_state(c, r, (f + r) % nfit, 1.0)[1]]
        if hit and len(pairs) < 12:
            pairs.append((r, (hit[0] + r) % nfit))
    assert len(pairs) == 12
    worst = dict(logFC=0.0, u=0.0, s2=0.0)
    for r, f in pairs:
        fitted, mis, sel = pair_state(c, r, f, 1.0)
        assert fitted and mis and np.isfinite(outf[r, :, :, f]).all(), (r, f)
        x = c["A"][r]
        obs = np.zeros(n, dtype=np.int8)
        obs[[t for t in sel if t not in set(mis)]] = 1
        Df = c["D"][:, :, f]
        one, h1 = hip_ctx.limma(x[None, :], Df, obs, c["K"])
        des, red = engine.limma_design(Df, c["use"][:, f], c["K"]), engine.limma_design(Df, obs, c["K"])
        _, hinv, _ = nr.mp_H(des["Q"], mis)
        oi = np.flatnonzero(obs)
        ref = {"u": red["u"]}
        unit = nr.units(x, des["Q"], list(sel), mis, des["v"], ref, hinv)
        d = len(oi) - p
        assert dfres[r, f] == d == h1[0, 0]
        mag = np.abs(x[oi]) @ np.abs(red["Q"][oi])
        E = red["Q"][oi].T @ x[oi]
        res = x[oi] - red["Q"][oi] @ E
        rho = np.abs(x[oi]) + np.abs(red["Q"][oi]) @ np.abs(E)
        rssb = float(lr.rss_bound(res[None, :], rho[None, :], np.array([one[0, 5, 0, 0] * d]), len(oi), p)[0])
        for j in range(2):
            allow = nr.FACTOR * nr.RATIO_SEEN["logFC"] * unit["logFC"][j] + \
                float(np.abs(red["v"][:, j]) @ lr.effects_bound(mag, len(oi)))
            dev = abs(outf[r, 0, j, f] - one[0, 0, j, 0])
            worst["logFC"] = max(worst["logFC"], dev / allow)
            assert dev <= allow, (r, f, j, dev, allow)
            u_na = outf[r, 0, j, f] / (outf[r, 2, j, f] * np.sqrt(_post(outf[r, 5, j, f], d, hyper[f])))
            allow_u = nr.FACTOR * nr.RATIO_SEEN["u"] * unit["u"][j]
            worst["u"] = max(worst["u"], abs(u_na - red["u"][j]) / allow_u)
            assert abs(u_na - red["u"][j]) <= allow_u, (r, f, j, u_na, red["u"][j])
        allow_s = (nr.FACTOR * nr.RATIO_SEEN["rss"] * unit["rss"] + rssb) / d
        worst["s2"] = max(worst["s2"], abs(outf[r, 5, 0, f] - one[0, 5, 0, 0]) / allow_s)
        assert abs(outf[r, 5, 0, f] - one[0, 5, 0, 0]) <= allow_s
        assert abs(outf[r, 1, 0, f] - one[0, 1, 0, 0]) <= 2 * (len(sel) + 3) * U * np.abs(x[oi]).mean()
    print(f"[measure] parent path {case}: worst share of the allowance " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_end_to_end_against_50_digits(hip_ctx):
    """case (130, 131, 8, 2) against limma_na_mp, fit by fit.  The integers (dfres, df.pooled, n.ok, which rows are NaN) are
    exact.  df.prior and s2.prior are held to the bounds of test_end_to_end_against_limma_np (tests/test_gpu_limma.BOUND).
    Per row: logFC, u and sigma2 carry the section 24 allowance, which scales with |H^-1| (complete rows: the same form
    without missing samples), so t is held to dfc / se + |t| (du / u + ds2 / s2 + e), e the share of the eBayes tail:
    s2.post = (d s2 + d0 s0) / (d + d0) moves by at most the relative deviations of d0 and s0, half of it reaches t.
    P.Value goes through lr.dev_p against the 50-digit tail of the t that came back, at the reference's df.total, with
    that test's bound; the relative deviations of t and P.Value over all rows (lr.dev_t, lr.dev_p) are printed and held to
    that test's bounds as well."""
    from tests.test_gpu_limma import BOUND
    case = CASES[1]
    c = case_results(hip_ctx, case)
    rows, n, p, nfit = case
    out, hyper, dfres = c["fit"]
    mp = lr._mp()
    e_tail = 0.5 * (BOUND["df_prior"] + BOUND["s2_prior"]) + 4 * U
    worst = dict(df_prior=0.0, s2_prior=0.0, t_share=0.0, t=0.0, p=0.0, p_tail=0.0)
    for f in range(nfit):
        Df, uf = c["D"][:, :, f], c["use"][:, f]
        ref = nr.limma_na_mp(c["A"], Df, uf, c["K"], max_na=0.2)
        des = engine.limma_design(Df, uf, c["K"])
        sel = np.flatnonzero(uf != 0)
        okref = np.array([row is not None for row in ref["rows"]])
        assert np.array_equal(~np.isnan(out[:, 0, 0, f]), okref)
        assert np.array_equal(np.isnan(dfres[:, f]), ~okref)
        assert hyper[f, 3] == ref["nok"] and hyper[f, 4] == float(ref["df_pooled"]) and hyper[f, 0] == len(sel) - p
        worst["df_prior"] = max(worst["df_prior"], lr.dev_rel(hyper[f, 1], float(ref["df_prior"])))
        worst["s2_prior"] = max(worst["s2_prior"], lr.dev_rel(hyper[f, 2], float(ref["s2_prior"])))
        t_ref, p_ref, p_tail = (np.full((rows, 2), np.nan) for _ in range(3))
        for r in np.flatnonzero(okref):
            row = ref["rows"][r]
            x = c["A"][r]
            mis = [int(t) for t in sel[np.isnan(x[sel])]]
            assert dfres[r, f] == row["d"] == len(sel) - len(mis) - p
            hinv = nr.mp_H(des["Q"], mis)[1] if mis else 1.0
            unit = nr.units(x, des["Q"], list(sel), mis, des["v"], {"u": [float(t) for t in row["u"]]}, hinv)
            d_s2 = nr.FACTOR * nr.RATIO_SEEN["rss"] * unit["rss"] / row["d"]
            assert abs(out[r, 5, 0, f] - float(row["s2"])) <= d_s2 + U * float(row["s2"])
            obs = [t for t in sel if t not in set(mis)]
            assert abs(out[r, 1, 0, f] - float(row["M"])) <= (len(sel) + 4) * U * np.abs(x[obs]).mean()
            for j in range(2):
                d_fc = nr.FACTOR * nr.RATIO_SEEN["logFC"] * unit["logFC"][j]
                assert abs(out[r, 0, j, f] - float(row["logFC"][j])) <= d_fc + U * abs(float(row["logFC"][j]))
                tref, se = float(row["t"][j]), float(row["se"][j])
                d_t = d_fc / se + abs(tref) * (nr.FACTOR * nr.RATIO_SEEN["u"] * unit["u"][j] / float(row["u"][j]) +
                                               d_s2 / float(row["s2"]) + e_tail)
                worst["t_share"] = max(worst["t_share"], abs(out[r, 2, j, f] - tref) / d_t)
                assert abs(out[r, 2, j, f] - tref) <= d_t, (r, f, j, out[r, 2, j, f], tref, d_t)
                t_ref[r, j], p_ref[r, j] = tref, float(row["p"][j])
                with mp.workdps(lr.DPS):
                    p_tail[r, j] = float(xs.two_pt(mp.mpf(float(out[r, 2, j, f])), row["df_total"]))
        for j in range(2):
            worst["t"] = max(worst["t"], lr.dev_t(out[:, 2, j, f], t_ref[:, j]))
            np.testing.assert_array_equal(out[:, 4, j, f], lr.bh(out[:, 3, j, f]))
        worst["p"] = max(worst["p"], lr.dev_p(out[:, 3, :, f], p_ref))
        worst["p_tail"] = max(worst["p_tail"], lr.dev_p(out[:, 3, :, f], p_tail))
    print("[measure] end to end, na = fit: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert worst["df_prior"] <= BOUND["df_prior"] and worst["s2_prior"] <= BOUND["s2_prior"], worst
    assert worst["p_tail"] <= BOUND["p"], worst
    assert worst["t"] <= BOUND["t"] and worst["p"] <= BOUND["p"], worst          # and as that test holds them, over all rows


def test_the_device_follows_the_header_to_the_bit(hip_ctx):
    """a dozen incomplete pairs of case (515, 300, 3, 3): E' from the effects entry on the row with its NaN set to 0.0 (an
    fma with a zero product leaves the chain's bits), plaidhip_limma_na_solve on the missing samples' rows of the same Q:
    the device's logFC is the fma chain v . gamma of the host's gamma, its t is logFC / (u sqrt(s2.post)) of the host's u,
    bit for bit; the pair that is not estimable is not ok on both sides"""
    from tests.test_gpu_limma import device_passes, fit_Q
    case = CASES[0]
    c = case_results(hip_ctx, case)
    rows, n, p, nfit = case
    out, hyper, dfres = c["fit1"]
    Q, nf = fit_Q(c["D"], c["use"])
    pairs = [(ROLE[k], 0) for k in ("c0", "c127", "c128", "clast", "four", "group")] + [(ROLE["group"], 1), (ROLE["above"], 2)]
    pairs += [(r, f) for r in (40, 41, 42, 43) for f in (r % nfit,) if pair_state(c, r, f, 1.0)[1]]
    A0 = np.asfortranarray(np.nan_to_num(c["A"][[r for r, _ in pairs]], nan=0.0, posinf=0.0, neginf=0.0))
    E, _ = device_passes(hip_ctx, A0, A0.shape[0], Q, c["use"], nf)
    seen_not_ok = 0
    for i, (r, f) in enumerate(pairs):
        _, mis, sel = pair_state(c, r, f, 1.0)
        assert mis
        des = engine.limma_design(c["D"][:, :, f], c["use"][:, f], c["K"], fit=f + 1)
        assert np.array_equal(des["Q"], Q[:, :, f])
        got = engine.limma_na_solve(des["Q"][mis], E[f * (p + 1):f * (p + 1) + p, i], len(sel) - len(mis), des["v"])
        if not got["ok"]:
            seen_not_ok += 1
            assert np.isnan(out[r, :, :, f]).all() and np.isnan(dfres[r, f])
            continue
        d = len(sel) - len(mis) - p
        assert dfres[r, f] == d
        fc = nr.emulate_logfc(des["v"], [float(t) for t in got["gamma"]])
        for j in range(2):
            assert out[r, 0, j, f] == fc[j], (r, f, j)
            t = fc[j] / (got["u"][j] * np.sqrt(_post(out[r, 5, j, f], float(d), hyper[f])))
            assert out[r, 2, j, f] == t, (r, f, j, out[r, 2, j, f], t)
    assert seen_not_ok == 1 and len(pairs) >= 10


@pytest.mark.parametrize("case", CASES + P_CASES, ids=IDS + P_IDS)
def test_rows_that_must_be_nan(hip_ctx, case):
    c = case_results(hip_ctx, case)
    rows, n, p, nfit = case
    (outf, hyper, dfres), (out1, hyper1, dfres1) = c["fit"], c["fit1"]
    for key in ("above", "group", "all", "p_left", "inf_used", "inf_used_nan"):       # max_na = 0.2: above it, or an Inf
        assert np.isnan(outf[ROLE[key]]).all() and np.isnan(dfres[ROLE[key]]).all(), key
    for f in range(nfit):
        assert hyper[f, 3] == (~np.isnan(outf[:, 0, 0, f])).sum() == (~np.isnan(dfres[:, f])).sum()
        assert hyper[f, 4] == np.nansum(dfres[:, f])
        assert hyper1[f, 3] == (~np.isnan(out1[:, 0, 0, f])).sum() and hyper1[f, 4] == np.nansum(dfres1[:, f])
    # max_na = 1 keeps all that are estimable
    assert np.isnan(out1[ROLE["group"], :, :, 0]).all() and np.isnan(dfres1[ROLE["group"], 0])     # not estimable in fit 1
    assert np.isfinite(out1[ROLE["group"], :, :, 1:]).all()                                         # the other fits' groups differ
    assert np.isnan(out1[ROLE["p_left"], :, :, 0]).all()                                            # |obs| = p
    assert np.isnan(out1[ROLE["all"]]).all() and np.isnan(out1[ROLE["inf_used"]]).all() and np.isnan(out1[ROLE["inf_used_nan"]]).all()
    assert np.isfinite(out1[ROLE["above"]]).all() and np.isfinite(out1[list(SPREAD)]).all()
    # max_na = 0 refuses every row with a NaN, in every fit: the ok rows are the complete ones without a used Inf
    out0, hyper0, dfres0 = hip_ctx.limma(c["A"], c["D"], c["use"], c["K"], na="fit", max_na=0.0)
    complete = ~np.isnan(c["A"]).any(axis=1)
    complete[ROLE["inf_used"]] = False
    for f in range(nfit):
        assert np.array_equal(~np.isnan(out0[:, 0, 0, f]), complete)
        assert hyper0[f, 3] == complete.sum()
    er.assert_same_bits(out0[complete][:, [0, 1, 5]], c["prop"][0][complete][:, [0, 1, 5]], "max_na = 0, the complete rows")


@pytest.mark.parametrize("case", CASES[:2] + [(40, 7, 2, 1)], ids=IDS[:2] + ["rows40-n7-p2-nfit1"])
def test_every_sharding_has_the_one_device_bits(hip_ctx, case):
    if case in CASES:
        c = case_results(hip_ctx, case)
        A, D, use, K, one = c["A"], c["D"], c["use"], c["K"], c["fit"]
        shards = (1, 2, 3, 5)
    else:                                                   # more shards than samples
        rng = np.random.default_rng(7)
        rows, n, p, _ = case
        D = np.column_stack([np.ones(n), np.arange(n) % 2])[:, :, None]
        A = rng.normal(size=(rows, n))
        A[np.arange(0, rows, 3), rng.integers(n, size=len(range(0, rows, 3)))] = np.nan
        use, K = None, None
        one = hip_ctx.limma(A, D, use, K, na="fit", max_na=0.2)
        assert np.isfinite(one[0]).any() and np.isfinite(one[0][np.isnan(A).any(axis=1)]).any()
        shards = (2, 9)
    for nshards in shards:
        status, out, hyper, dfres = nr.run_sharded(nshards, A, D, use, K, max_na=0.2)
        assert status == _lib.OK
        er.assert_same_bits(out, one[0], f"{nshards} shards")
        er.assert_same_bits(hyper, one[1], f"{nshards} shards, hyper")
        er.assert_same_bits(dfres, one[2], f"{nshards} shards, dfres")


def test_a_failing_shard_reports_and_writes_nothing(hip_ctx):
    c = case_results(hip_ctx, CASES[0])
    status, out, hyper, dfres = nr.run_sharded(3, c["A"], c["D"], c["use"], c["K"], fail=1)
    text = _lib.load().plaidhip_last_error_string().decode()
    assert status == _lib.EHIP and "injected failure" in text, (status, text)
    assert (out == -7).all() and (hyper == -7).all() and (dfres == -7).all()


def test_contrasts_on_the_fixture_with_missing_values(hip_ctx, pbmc):
    import scipy.sparse as sp
    d, _ = pbmc
    X = sp.csc_matrix((d["x"], d["i"], d["p"]), shape=tuple(d["dim"])).toarray()
    rng = np.random.default_rng(50)
    X[rng.random(X.shape) < 0.05] = np.nan
    S = plaid_amd.NamedMatrix(np.asfortranarray(X), d["rownames"], d["colnames"])
    types, counts = np.unique(d["celltype"], return_counts=True)
    top = types[np.argsort(-counts)][:2]
    Y = np.full((50, 2), np.nan)
    Y[:, 0] = d["celltype"] == top[0]
    Y[d["celltype"] == top[0], 1], Y[d["celltype"] == top[1], 1] = 1.0, 0.0      # the rest take no part: an NA column
    Yn = plaid_amd.NamedMatrix(Y, d["colnames"], ["vs_rest", "vs_second"])
    tabs, hyper = plaid_amd.plaid_limma_contrasts(S, Yn, ctx=hip_ctx, na="fit")
    tabp, _ = plaid_amd.plaid_limma_contrasts(S, Yn, ctx=hip_ctx)
    cols = ["logFC", "AveExpr", "t", "P.Value", "adj.P.Val", "sigma2", "df.residual"]
    for j, nm in enumerate(Yn.colnames):
        assert tabs[nm].colnames == cols and tabs[nm].shape == (X.shape[0], 7) and tabp[nm].shape == (X.shape[0], 6)
        assert set(hyper[nm]) == {"df.residual", "df.prior", "s2.prior", "n.ok", "df.pooled"}
        D, use = lr.contrast_design(Y, np.zeros((50, 0)), j)
        own, h = plaid_amd.plaid_limma(S, D, contrasts=[0.0, 1.0], use=use, ctx=hip_ctx, na="fit")
        er.assert_same_bits(tabs[nm].values, own["1"].values, nm)
        np.testing.assert_equal(h, hyper[nm])
        ok = ~np.isnan(tabs[nm].values[:, 0])
        assert ok.sum() > np.isfinite(tabp[nm].values[:, 0]).sum() and hyper[nm]["n.ok"] == ok.sum()
        assert np.array_equal(np.isnan(tabs[nm].values[:, 6]), ~ok)
        assert hyper[nm]["df.pooled"] == tabs[nm].values[ok, 6].sum()
