"""plaid.limma with weights on the host (include/plaidhip.h: plaidhip_limma_w), without a GPU.

  1. the 50-digit reference (weighted normal equations from the original design) against numpy's lstsq on sqrt(omega)-scaled
     rows, and against limma_na_ref.mp_refit for weights of 0 and 1
  2. plaidhip_limma_w_solve against the Python emulation of the pinned chains, bit for bit: gamma, u, the pivots, ok
  3. the estimability rule: a group without weight, |live| = p, |live| = p + 1; it is relative -- all weights times a power
     of two change no bit of gamma and no decision
  4. the emulation of the whole pinned order lies within the forward bound of section 28 of the 50-digit reference
  5. na = "fit" keeps its absolute rule: plaidhip_limma_na_solve against limma_na_ref's emulation on a pivot between the rules
  6. limma_w_ref.P_CASES meet what tests/test_gpu_limma_w.py presumes of them: pivot ratios, the designated rows, the bound's
     own condition
"""
import numpy as np
import pytest

from plaid_amd import engine
from tests.helpers import limma_na_ref as nr
from tests.helpers import limma_ref as lr
from tests.helpers import limma_w_ref as wr

PS = (1, 2, 3, 8, 10)


def deck(p, n=37, seed=5, kind="plain"):
    """one row: design (limma_na_ref.solve_design), x, omega log-uniform in [0.25, 4] with the zeros of `kind`, K"""
    rng = np.random.default_rng([seed, p])
    D, g = nr.solve_design(p, n, seed)
    x = rng.normal(size=n) * 2.0 + 1.0
    om = np.exp(rng.uniform(np.log(0.25), np.log(4.0), size=n))
    one = np.flatnonzero(g == 1)
    if kind == "zeros":
        om[[0, 5, n - 1]] = [0.0, -2.0, np.nan]
    elif kind == "half":
        om[one[: len(one) // 2]] = 0.0
    elif kind == "group":
        om[one] = 0.0
    elif kind == "p_left":
        om[rng.permutation(n)[p:]] = 0.0
    elif kind == "p_plus_one":
        om[rng.permutation(n)[p + 1:]] = 0.0
    K = np.eye(p)[:, : min(p, 2)].copy()
    if p > 1:
        K[0, 1] = -0.5
    return D, x, om, K


@pytest.mark.parametrize("p", PS)
def test_reference_against_lstsq_and_against_the_refit(p):
    D, x, om, K = deck(p, kind="zeros")
    ref, alt = wr.mp_wls(x, om, D, None, K), wr.np_wls(x, om, D, None, K)
    assert ref["d"] == alt["d"] == 37 - 3 - p
    for j in range(K.shape[1]):
        assert abs(float(ref["logFC"][j]) - alt["logFC"][j]) <= 1e-11 * (1 + abs(alt["logFC"][j]))
        assert abs(float(ref["u"][j]) - alt["u"][j]) <= 1e-11 * alt["u"][j]
    assert abs(float(ref["rss"]) - alt["rss"]) <= 1e-11 * alt["rss"]
    # weights of 0 and 1 are missing values: the refit of na = "fit" on the observed samples, at 50 digits
    w01 = np.where(wr.live_mask(x, om), 1.0, 0.0)
    xn = np.where(w01 == 1.0, x, np.nan)
    a, b = wr.mp_wls(x, w01, D, None, K), nr.mp_refit(xn, D, None, K)
    assert a["d"] == b["d"]
    for j in range(K.shape[1]):
        assert abs(a["logFC"][j] - b["logFC"][j]) < 1e-40 and abs(a["u"][j] - b["u"][j]) < 1e-40
    assert abs(a["rss"] - b["rss"]) < 1e-40
    assert abs(a["M"] - np.mean(x)) < 1e-12            # AveExpr ignores the weights: every value that is not NaN counts


def sums(D, x, om, K):
    des = engine.limma_design(D, None, K)
    sel = np.arange(D.shape[0])
    return des, sel, wr.emulate_sums(x, om, des["Q"], sel)


@pytest.mark.parametrize("kind", ["plain", "zeros", "half"])
@pytest.mark.parametrize("p", PS)
def test_host_solve_follows_the_pinned_chains_to_the_bit(p, kind):
    D, x, om, K = deck(p, kind=kind)
    des, sel, (Htri, b, _, nlive, _) = sums(D, x, om, K)
    got = engine.limma_w_solve(Htri, b, nlive, des["v"])
    ok, g, us, piv = wr.emulate_w_solve(Htri, b, nlive, des["v"])
    assert ok and got["ok"]
    assert np.array_equal(got["gamma"], np.array(g)) and np.array_equal(got["u"], np.array(us))
    assert np.array_equal(got["pivots"], np.array(piv))
    assert wr.pivot_ratios(Htri, p).min() > 1e-3       # (no case sits near the rule)


@pytest.mark.parametrize("p", PS)
def test_estimability_is_the_relative_rule(p):
    for kind, want in (("group", p == 1), ("p_left", False), ("p_plus_one", True)):
        D, x, om, K = deck(p, kind=kind)
        if kind == "group" and p == 1:
            continue                                     # (the intercept alone has no group column to lose)
        des, sel, (Htri, b, _, nlive, _) = sums(D, x, om, K)
        got = engine.limma_w_solve(Htri, b, nlive, des["v"])
        ok, g, us, piv = wr.emulate_w_solve(Htri, b, nlive, des["v"])
        assert got["ok"] == ok == want, (kind, p, got["pivots"])
        k = len(piv)
        assert np.array_equal(got["pivots"][:k], np.array(piv)) and np.isnan(got["pivots"][k:]).all()
        if not want:
            assert np.isnan(got["gamma"]).all() and np.isnan(got["u"]).all()
            assert (wr.mp_wls(x, om, D, None, K) is None) or kind == "group"
        else:
            assert np.array_equal(got["gamma"], np.array(g)) and nlive - p == 1
    # scaling every weight by a power of two commutes with every rounding: the same gamma, the same decisions
    D, x, om, K = deck(p, kind="half")
    des, sel, (Htri, b, _, nlive, _) = sums(D, x, om, K)
    base = engine.limma_w_solve(Htri, b, nlive, des["v"])
    for e in (2, -40, 300):
        s = 2.0 ** e
        Hs, bs, _, _, _ = wr.emulate_sums(x, om * s, des["Q"], sel)
        assert np.array_equal(np.array(Hs), np.array(Htri) * s) and np.array_equal(np.array(bs), np.array(b) * s)
        got = engine.limma_w_solve(Hs, bs, nlive, des["v"])
        assert got["ok"] and np.array_equal(got["gamma"], base["gamma"])
        assert np.array_equal(got["pivots"], base["pivots"] * s)
    D, x, om, K = deck(max(p, 2), kind="group")           # ... and a deficient row stays deficient at any scale
    des, sel, (Htri, b, _, nlive, _) = sums(D, x, om, K)
    for e in (0, -40, 300):
        assert not engine.limma_w_solve(np.array(Htri) * 2.0 ** e, np.array(b) * 2.0 ** e, nlive, des["v"])["ok"]


@pytest.mark.parametrize("kind", ["plain", "zeros", "half"])
@pytest.mark.parametrize("p", PS)
def test_the_pinned_order_lies_within_the_derived_bound(p, kind):
    D, x, om, K = deck(p, kind=kind)
    des, sel, (Htri, b, Mp, nlive, nseen) = sums(D, x, om, K)
    ok, g, us, _ = wr.emulate_w_solve(Htri, b, nlive, des["v"])
    ref = wr.mp_wls(x, om, D, None, K)
    assert ok and ref is not None and ref["d"] == nlive - p
    hinv, Hn = wr.exact_H(des["Q"], om, ref["live"])
    eta_q, eta_v = wr.basis_error(D, None, K, des)
    unit = wr.units(x, om, des["Q"], list(sel), des["v"], ref, hinv, Hn, eta_q, eta_v)
    fc = nr.emulate_logfc(des["v"], g)
    rss = wr.emulate_w_rss(x, om, des["Q"], sel, g)
    dev = nr.deviations(fc, us, rss, ref, unit)
    print(f"[measure] p {p} {kind}: share of the bound " + ", ".join(f"{k} {v:.3g}" for k, v in dev.items()),
          f"|H^-1| Hn {hinv * Hn:.3g}")
    assert all(v <= 1.0 for v in dev.values()), dev
    ave = (Mp * len(sel)) / nseen
    assert abs(ave - float(ref["M"])) <= (len(sel) + 4) * lr.U * np.abs(x).mean()


@pytest.mark.parametrize("case", wr.P_CASES, ids=wr.P_IDS)
def test_the_p_cases_meet_what_the_device_tests_presume(case):
    """wr.P_CASES, on the inputs and the references alone, so that tests/test_gpu_limma_w.py can only fail on the device's
    numbers: every row that is not designated is far from the estimability rule; the designated rows behave as planted (a
    weight that is not positive and finite only removes its observation; the group without weight, |live| = p and the live
    Inf are not fitted in fit 1; the row above max_na in none); the integers of the plain-numpy rules agree with the
    50-digit reference on which rows are fitted; the bound's own condition (wr.units asserts it) holds on every fitted row;
    and the emulation of the pinned order lies within that bound"""
    rows, n, p, nfit = case
    c = wr.make_case(case)
    c["des"] = wr.case_designs(c, case)
    role = c["role"]
    assert set(role) == {k for k, r in wr.ROLE.items() if r < rows} and (rows < 12 or len(role) == len(wr.ROLE))
    wr.assert_other_rows_are_far_from_the_rule(c, case)
    worst = {}
    for f in range(nfit):
        Df, uf, des = c["D"][:, :, f], wr.fit_use(c, f), c["des"][f]
        sel = np.arange(n) if uf is None else np.flatnonzero(uf != 0)
        okall, dall = wr.expected_integers(c["A"], c["Wt"], c["aw"], des["Q"], uf, 0.2)
        refs = wr.limma_w_mp(c["A"], c["Wt"], c["aw"], Df, uf, c["K"], max_na=0.2, tail=False)
        assert [ref is not None for ref in refs] == list(okall)
        assert okall.sum() >= rows - len(role) and okall.sum() >= 3
        for key in ("w_zero", "w_neg", "w_nan", "w_inf", "nan_beside"):
            assert okall[role[key]], (key, f)
        if f == 0:
            assert not okall[role["p_left"]] and dall[role["p_left"]] == 0 and not okall[role["inf_live"]]
            assert p == 1 or not okall[role["group"]]
        if "above" in role:
            assert not okall[role["above"]]
        if case not in wr.P_CASES[:3]:
            continue
        eta = wr.basis_error(Df, uf, c["K"], des)
        for r in np.flatnonzero(okall):
            om = wr.omega(c["Wt"][r], c["aw"])
            hinv, Hn = wr.exact_H(des["Q"], om, refs[r]["live"])
            unit = wr.units(c["A"][r], om, des["Q"], list(sel), des["v"], refs[r], hinv, Hn, eta[0], eta[1])
            Htri, b, _, nlive, _ = wr.emulate_sums(c["A"][r], om, des["Q"], sel)
            ok, g, us, _ = wr.emulate_w_solve(Htri, b, nlive, des["v"])
            assert ok and refs[r]["d"] == nlive - p == dall[r]
            dev = nr.deviations(nr.emulate_logfc(des["v"], g), us, wr.emulate_w_rss(c["A"][r], om, des["Q"], sel, g), refs[r], unit)
            assert all(v <= 1.0 for v in dev.values()), (r, f, dev)
            worst = {k: max(v, worst.get(k, 0.0)) for k, v in dev.items()}
    if worst:
        print(f"[measure] {case}: the emulation's worst share of the bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_na_fit_keeps_its_absolute_rule():
    """a row whose pivot lies between the two rules -- above 1e-10 in absolute terms, below 1e-10 of nothing relative that
    matters: na = "fit" decides by the absolute threshold as before, and its bits are limma_na_ref's emulation"""
    for p in (2, 3, 8):
        D, g = nr.solve_design(p)
        des = engine.limma_design(D)
        for kind in nr.MISSING_KINDS:
            mis = nr.solve_missing(g, kind)
            x = np.random.default_rng(p).normal(size=len(g))
            x[mis] = np.nan
            Ep = nr.emulate_effects(x, des["Q"], np.arange(len(g)))
            got = engine.limma_na_solve(des["Q"][mis], Ep, len(g) - len(mis), des["v"])
            ok, gam, us, piv = nr.emulate_solve(des["Q"][mis], Ep, des["v"])
            assert got["ok"] == ok
            if ok:
                assert np.array_equal(got["gamma"], np.array(gam)) and np.array_equal(got["u"], np.array(us))
                assert np.array_equal(got["pivots"], np.array(piv))
    # H = diag(1, 5e-11): the absolute rule refuses it; the same triangle is estimable under the relative rule
    qmis = np.array([[0.0, np.sqrt(1.0 - 5e-11)]])
    got = engine.limma_na_solve(qmis, np.array([1.0, 1.0]), 5, np.eye(2))
    assert not got["ok"] and 0 < got["pivots"][1] <= 1e-10
    assert engine.limma_w_solve([1.0, 0.0, got["pivots"][1]], [1.0, 1.0], 5, np.eye(2))["ok"]
