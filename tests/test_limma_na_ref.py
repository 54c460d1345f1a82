"""plaid.limma with na = "fit" on the host, no device: the shared solve (csrc/lmfit_na.h behind plaidhip_limma_na_solve)
against a 50-digit refit that does not use the downdate, the estimability rule, and plaidhip_limma_finish_na against the
header's unequal-df eBayes at 50 digits.  DESIGN.md section 24."""
import numpy as np
import pytest

from plaid_amd import engine
from tests.helpers import limma_na_ref as nr
from tests.helpers import limma_ref as lr

pytest.importorskip("mpmath")

N = 37
# plaidhip_limma_finish_na against mp_finish_na: the worst relative deviation measured over the five branch cases, and what is
# asserted: 8 times it, for libm differences between hosts
FINISH_MEASURED = {"df_prior": 9.8e-16, "s2_prior": 1.6e-15, "t": 5.9e-15, "p": 1.9e-14}
FINISH_FACTOR = 8
FINISH_BOUND = {k: FINISH_FACTOR * v for k, v in FINISH_MEASURED.items()}
P_CASES = (1, 2, 3, 8, engine.LIMMA_NA_MAX_COEF)


def _case(p, kind):
    D, g = nr.solve_design(p, N)
    mis = nr.solve_missing(g, kind)
    rng = np.random.default_rng(100 * p + nr.MISSING_KINDS.index(kind))
    x = D @ rng.normal(size=p) + rng.normal(size=N)
    x[mis] = np.nan
    return D, x, sorted(int(c) for c in mis)


def _library_row(D, x, mis):
    """the library's row: E' in the pinned order, then plaidhip_limma_na_solve; logFC and the RSS as the later passes take them"""
    des = engine.limma_design(D)
    Q, v = des["Q"], des["v"]
    sel = np.arange(len(x))
    Ep = nr.emulate_effects(x, Q, sel)
    got = engine.limma_na_solve(Q[mis], Ep, len(x) - len(mis), v)
    return des, Ep, got


@pytest.mark.parametrize("kind", nr.MISSING_KINDS)
@pytest.mark.parametrize("p", P_CASES)
def test_solve_against_50_digits(p, kind):
    """logFC, stdev.unscaled and the RSS of a row with missing samples: the library's solve against lr.mp_design / mp_fit on
    the row's observed samples.  The allowance is FACTOR x the largest ratio the fp64 emulation of the pinned order
    (tests/helpers/limma_na_ref.emulate_*) showed on these cases, in the units of nr.units; the emulation is held to the
    recorded ratio here, so the allowance never follows the library.  The library follows the pinned order to the bit."""
    D, x, mis = _case(p, kind)
    des, Ep, got = _library_row(D, x, mis)
    Q, v = des["Q"], des["v"]
    sel = np.arange(N)
    ref = nr.mp_refit(x, D)
    assert ref is not None and got["ok"]
    _, hinv, piv = nr.mp_H(Q, mis)
    assert all(float(d) > 1e-6 for d in piv), "an estimable case sits near the rule"
    unit = nr.units(x, Q, sel, mis, v, ref, hinv)
    ok, g_em, u_em, piv_em = nr.emulate_solve(Q[mis], Ep, v)
    assert ok
    dev_em = nr.deviations(nr.emulate_logfc(v, g_em), u_em, nr.emulate_rss(x, Q, sel, g_em), ref, unit)
    gam = [float(t) for t in got["gamma"]]
    dev = nr.deviations(nr.emulate_logfc(v, gam), list(got["u"]), nr.emulate_rss(x, Q, sel, gam), ref, unit)
    print(f"p={p} {kind}: |mis|={len(mis)} |H^-1|={float(hinv):.3g} emulation {dev_em} library {dev}")
    for key in dev:
        assert dev_em[key] <= nr.RATIO_SEEN[key], (key, dev_em[key])
        assert dev[key] <= nr.FACTOR * nr.RATIO_SEEN[key], (key, dev[key])
    # the pinned order, to the bit
    assert np.array_equal(got["gamma"], np.array(g_em)) and np.array_equal(got["u"], np.array(u_em))
    assert np.array_equal(got["pivots"], np.array(piv_em))
    assert abs(ref["d"] - (N - len(mis) - p)) == 0


def test_estimability_rule():
    """a group entirely missing, |obs| = p and |obs| = p + 1: not ok, not ok, ok with d = 1; a group with one sample left is
    estimable with a pivot far from the rule.  The 50-digit pivots of the estimable cases are > 1e-6, a deficient case has a
    pivot that is exactly 0 (from the exact Q of the design), so no case sits near 1e-10."""
    p = 3
    D, g = nr.solve_design(p, N)
    des = engine.limma_design(D)
    Q, v = des["Q"], des["v"]
    rng = np.random.default_rng(3)
    x0 = D @ rng.normal(size=p) + rng.normal(size=N)

    def run(mis):
        x = x0.copy()
        x[mis] = np.nan
        Ep = nr.emulate_effects(x, Q, np.arange(N))
        return x, engine.limma_na_solve(Q[mis], Ep, N - len(mis), v)

    # a whole group
    mis = [int(c) for c in np.flatnonzero(g == 1)]
    x, got = run(mis)
    assert not got["ok"] and np.isnan(got["gamma"]).all() and np.isnan(got["u"]).all()
    piv = nr.mp_pivots_exact(D, None, mis)
    assert min(abs(t) for t in piv) < 1e-60, "the deficient case has an exact zero pivot"
    assert nr.mp_refit(x, D) is None
    # all but one of the group: estimable, far from the rule
    x, got = run(mis[:-1])
    assert got["ok"] and np.isfinite(got["gamma"]).all()
    assert min(float(t) for t in nr.mp_pivots_exact(D, None, mis[:-1])) > 1e-6
    assert min(got["pivots"]) > 1e-6
    # |obs| = p: no residual degree of freedom; |obs| = p + 1: d = 1
    keep = [0, 1, 2, 5]   # two of each group, a batch value each: a full-rank 4 x 3 design
    mis_p1 = [c for c in range(N) if c not in keep]
    mis_p = [c for c in range(N) if c not in keep[:3]]
    x, got = run(mis_p)
    assert not got["ok"] and np.isnan(got["gamma"]).all()
    assert nr.mp_refit(x, D) is None
    x, got = run(mis_p1)
    ref = nr.mp_refit(x, D)
    assert got["ok"] and ref is not None and ref["d"] == 1
    assert min(float(t) for t in nr.mp_pivots_exact(D, None, mis_p1)) > 1e-6
    fc = nr.emulate_logfc(v, [float(t) for t in got["gamma"]])
    _, hinv, _ = nr.mp_H(Q, mis_p1)
    unit = nr.units(x, Q, np.arange(N), mis_p1, v, ref, hinv)
    for j in range(p):
        assert abs(fc[j] - ref["logFC"][j]) <= nr.FACTOR * nr.RATIO_SEEN["logFC"] * unit["logFC"][j]


def _finish_inputs(name, dvals, seed=0):
    """E, rss of branch case `name` for the fit [1, Y[, 0], B] from the 50-digit fit, rounded once, and per-row d drawn from
    dvals (the RSS scaled so that s2 = rss / d keeps the case's s2, which is what steers the branch)"""
    X, Y, B = lr.branch_case(name)
    D, use = lr.contrast_design(Y, B, 0)
    des = lr.mp_design(D, use)
    fits = lr.mp_fit(X, des)
    rows, p = X.shape[0], 3
    rng = np.random.default_rng(seed)
    d = rng.choice(dvals, size=rows)
    d0 = des["nf"] - p
    E = np.full((p + 1, rows), np.nan)
    rss = np.full(rows, np.nan)
    for r, f in enumerate(fits):
        if f is not None:
            E[:p, r] = [float(t) for t in f[0]]
            E[p, r] = float(f[1])
            rss[r] = float(f[2]) * d[r] / d0
    return des, E, rss, d, lr.flat_rows(X, use)


@pytest.mark.parametrize("name", lr.BRANCH_CASES)
def test_finish_na_against_50_digits(name):
    """plaidhip_limma_finish_na on the five branch cases with d_r drawn from three values, against the unequal-df text at 50
    digits, as tests/test_limma_ref.py holds plaidhip_limma_finish: relative deviations through lr.dev_t (the constant rows
    against the size of the terms that cancel) and lr.dev_p, 8 x the worst value measured"""
    mp = lr._mp()
    des, E, rss, d, flat = _finish_inputs(name, (5, 8, 11))
    rows, p = E.shape[1], 3
    v = np.array([[float(t) for t in vj] for vj in des["v"]]).T      # p x q
    q = v.shape[1]
    rng = np.random.default_rng(1)
    urow = np.abs(rng.normal(size=(q, rows))) + 0.5
    out, hyper = engine.limma_finish_na(E, rss, [des["nf"]], v, d.astype(np.float64)[None, :], urow)
    with mp.workdps(lr.DPS + 20):
        fits = [None if np.isnan(rss[r]) else ([mp.mpf(float(t)) for t in E[:p, r]], mp.mpf(float(E[p, r])), mp.mpf(float(rss[r])))
                for r in range(rows)]
        vm = [[mp.mpf(float(v[k, j])) for k in range(p)] for j in range(q)]
        um = [[mp.mpf(float(urow[j, r])) for j in range(q)] for r in range(rows)]
    ref = nr.mp_finish_na(fits, [int(t) for t in d], vm, um)
    assert ref["branch"] == lr.EXPECTED_BRANCH[name]
    assert hyper.shape == (1, 5) and hyper[0, 3] == ref["nok"] and hyper[0, 0] == des["nf"] - p
    assert hyper[0, 4] == float(ref["df_pooled"])
    okrows = [r for r in range(rows) if ref["rows"][r] is not None]
    assert np.array_equal(np.flatnonzero(~np.isnan(out[:, 0, 0, 0])), np.array(okrows))
    dev = {"df_prior": lr.dev_rel(hyper[0, 1], float(ref["df_prior"])), "s2_prior": lr.dev_rel(hyper[0, 2], float(ref["s2_prior"]))}
    t_ref, p_ref = np.full((rows, q), np.nan), np.full((rows, q), np.nan)
    for r in okrows:
        t_ref[r], p_ref[r] = [float(x) for x in ref["rows"][r]["t"]], [float(x) for x in ref["rows"][r]["p"]]
    dev["t"] = 0.0
    for j in range(q):
        scale = np.array([float(ref["rows"][r]["mag"][j] / ref["rows"][r]["se"][j]) if ref["rows"][r] is not None else 0.0
                          for r in range(rows)])
        dev["t"] = max(dev["t"], lr.dev_t(out[:, 2, j, 0], t_ref[:, j], flat, scale))
    dev["p"] = lr.dev_p(out[:, 3, :, 0], p_ref)
    print(f"[measure] limma_finish_na {name} ({ref['branch']}): " + ", ".join(f"{k} {x:.3g}" for k, x in dev.items()))
    for k, x in dev.items():
        assert x <= FINISH_BOUND[k], (k, x)
    for j in range(q):
        np.testing.assert_array_equal(out[:, 4, j, 0], lr.bh(out[:, 3, j, 0]))
        np.testing.assert_array_equal(out[okrows, 5, j, 0], rss[okrows] / d[okrows])
        np.testing.assert_array_equal(out[okrows, 1, j, 0], E[p, okrows])


@pytest.mark.parametrize("name", lr.BRANCH_CASES)
def test_finish_na_with_equal_df_has_the_bits_of_finish(name):
    des, E, rss, _, _ = _finish_inputs(name, (11,))
    rows, p = E.shape[1], 3
    d0 = des["nf"] - p
    rss = rss * d0 / 11        # (undo the scaling: the fit's own d)
    v = np.array([[float(t) for t in vj] for vj in des["v"]]).T
    u = np.array([float(t) for t in des["u"]])
    out0, hyper0 = engine.limma_finish(E, rss, [des["nf"]], v, u)
    drow = np.full((1, rows), float(d0))
    out1, hyper1 = engine.limma_finish_na(E, rss, [des["nf"]], v, drow, np.repeat(u[:, None], rows, axis=1))
    assert np.array_equal(out0, out1, equal_nan=True)
    assert np.array_equal(hyper0, hyper1[:, :4], equal_nan=True)
    assert hyper1[0, 4] == hyper0[0, 3] * d0
    # a row that is not fitted (d = NaN) takes no part and is NaN
    assert not np.isnan(out0[1, 0, 0, 0])
    drow[0, 1] = np.nan
    out2, hyper2 = engine.limma_finish_na(E, rss, [des["nf"]], v, drow, np.repeat(u[:, None], rows, axis=1))
    assert np.isnan(out2[1]).all() and hyper2[0, 3] == hyper0[0, 3] - 1
