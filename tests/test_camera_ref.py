"""plaid.camera on the host, no device: the sample-space identity behind the variance inflation factor proved against limma's
literal form (tests/helpers/camera_ref.camera_mp: a complete QR, U = Q2'x), and the two host entries held to it.

  1. identity: vif = || sum of the members' z ||^2 / (m d) in sample space, at 50 digits from the thin Q, equals
     m * mean(colMeans(U[set, ])^2) of the complete QR to 1e-40 -- with `use`, p = 1, 2, 4, sets of 1, 2, many and all genes.
  2. plaidhip_camera_residual_row against the 50-digit z.  Bound, per element: the chain of p fma from x_c carries
     gamma_{p + 1} (|x_c| + sum_k |Q_ck E_k|), the effects it is fed are exact here up to their own rounding u |E_k|, the
     division and the square root are correctly rounded and s2 is fed rounded (u each, 1/2 u through the root); the
     library's Householder Q is orthonormal to n_f p u in norm, which moves the projection by 2 (n_f p + p) u ||x||_2:
     |dz| <= ((p + 3) u rho_c + 2 (n_f p + p) u ||x|| + 3 u |r_c|) / sigma, asserted with a factor 2 for the higher orders.
  3. plaidhip_camera_finish against step 5 at 50 digits, fed the 50-digit t, member sums and sums of squares rounded once.
     First-order forward bound (u = 2^-53): the two means carry (G + 1) u mean|t| each and the inputs u |t|, so
     |d delta| <= (G / m2) 2 (G + 3) u max|t|; var (two passes) and the subtraction in pooled carry (2 G + 8) u (G - 1) var /
     (G - 2) plus 2 |delta d delta| m m2 / (G (G - 2)); T = delta / sqrt(pooled k) then has
     |dT| <= |d delta| / sqrt(pooled k) + |T| (|d pooled| / (2 pooled) + 4 u).  Asserted with a factor 4 for what first
     order leaves out.  The tails are held to exact_stats.ASSERTED_ACC["pt"] at the library's own T and df.
  4. the edge rows: m = 0, m = 1, m = G, G = 2, and a set whose ok members are fewer than its members."""
import numpy as np
import pytest

from plaid_amd import engine
from tests.helpers import camera_ref as cr
from tests.helpers import exact_stats as xs
from tests.helpers import limma_ref as lr

mpmath = pytest.importorskip("mpmath")
U = 2.0 ** -53


def _case(seed, g, n, p, masked):
    rng = np.random.default_rng(seed)
    X = cr.int_matrix(g, n, rng)
    D = cr.make_design(n, p, rng)
    use = None
    if masked:
        use = np.ones(n, dtype=np.int8)
        use[rng.choice(n, size=3, replace=False)] = 0
        X[1, np.flatnonzero(use == 0)[0]] = np.nan          # an unused NaN reaches nothing
    sets = cr.make_sets(g, (1, 2, 5, g // 2, g), rng)
    return X, D, use, sets


def _sample_space(X, D, use, sets):
    """(vif per set, z genes x n_f, s2) at 50 digits from the thin Q: the form the library computes"""
    mp = mpmath
    des = lr.mp_design(D, use)
    fits = lr.mp_fit(X, des)
    d = des["nf"] - des["p"]
    with mp.workdps(cr.DPS + 20):
        z, s2 = {}, {}
        for g, f in enumerate(fits):
            if f is None:
                continue
            xm = [mp.mpf(float(v)) for v in X[g, des["sel"]]]
            r = [a - mp.fsum(q[c] * e for q, e in zip(des["Q"], f[0])) for c, a in enumerate(xm)]
            s2[g] = f[2] / d
            sg = mp.sqrt(max(s2[g], mp.mpf("1e-8")))
            z[g] = [v / sg for v in r]
        vif = []
        for members in sets:
            mem = [g for g in members if g in z]
            if len(mem) < 2:
                vif.append(None)
                continue
            T = [mp.fsum(z[g][c] for g in mem) for c in range(des["nf"])]
            vif.append(mp.fsum(t * t for t in T) / (len(mem) * d))
    return vif, z, s2, des, fits


@pytest.mark.parametrize("seed,g,n,p,masked", [(1, 12, 9, 1, False), (2, 14, 11, 2, True), (3, 10, 12, 4, False)])
def test_sample_space_identity(seed, g, n, p, masked):
    X, D, use, sets = _case(seed, g, n, p, masked)
    ref, ok = cr.mp_vif(X, D, use, sets)
    vif, *_ = _sample_space(X, D, use, sets)
    assert ok.all()
    for (m, v, cor), mine in zip(ref, vif):
        if m < 2:
            assert mine is None
            continue
        assert abs(mine - v) <= mpmath.mpf(10) ** -40 * abs(v), (m, mine, v)


@pytest.mark.parametrize("seed,g,n,p,masked", [(4, 8, 10, 1, False), (5, 9, 13, 2, True), (6, 7, 12, 4, True)])
def test_residual_row_against_50_digits(seed, g, n, p, masked):
    X, D, use, sets = _case(seed, g, n, p, masked)
    X[0, :] = 3.0                                              # s2 = 0 with an intercept: the 1e-8 floor
    _, z, s2, des, fits = _sample_space(X, D, use, sets)
    Q = engine.limma_design(D, use)["Q"]
    d = des["nf"] - p
    sel = des["sel"]
    unused = np.setdiff1d(np.arange(n), sel)
    for gi in range(g):
        # the effects on the library's own Q (its columns' signs are Householder's), exact and rounded once
        E = np.array([float(mpmath.fsum(mpmath.mpf(float(Q[c, k])) * mpmath.mpf(float(X[gi, c])) for c in sel)) for k in range(p)])
        rss = float(fits[gi][2])
        got = engine.camera_residual_row(X[gi], Q, use, E, rss, d)
        assert (got[unused] == 0.0).all() and not np.signbit(got[unused]).any()
        sigma = np.sqrt(max(float(s2[gi]), 1e-8))
        rho = np.abs(X[gi, sel]) + np.abs(Q[sel]) @ np.abs(E)
        ref = np.array([float(v) for v in z[gi]])
        bound = 2 * ((p + 3) * U * rho + 2 * (des["nf"] * p + p) * U * np.linalg.norm(X[gi, sel]) + 3 * U * np.abs(ref) * sigma) / sigma
        assert (np.abs(got[sel] - ref) <= bound + 1e-300).all(), (gi, np.max(np.abs(got[sel] - ref) / (bound + 1e-300)))
        print(f"[measure] residual_row gene {gi}: worst |dz| / bound {np.max(np.abs(got[sel] - ref) / (bound + 1e-300)):.3g}")
    # a gene that is not ok: every z is 0.0
    assert (engine.camera_residual_row(X[1], Q, use, np.zeros(p), np.nan, d) == 0.0).all()
    assert (engine.camera_residual_row(X[1], Q, use, np.zeros(p), np.inf, d) == 0.0).all()


def _finish_inputs(t, ok, sets, vifs, d):
    """t (mp or None per gene), the sets, mp vifs -> the fp64 operands of plaidhip_camera_finish, every value rounded once"""
    mp = mpmath
    g = len(t)
    tf = np.array([np.nan if v is None else float(v) for v in t]).reshape(g, 1, 1)
    cnt = np.array([[float(sum(1 for i in s if ok[i]))] for s in sets])
    with mp.workdps(cr.DPS + 20):
        sumt = np.array([float(mp.fsum(t[i] for i in s if ok[i])) for s in sets]).reshape(len(sets), 1, 1)
        ss = np.array([[0.0 if v[1] is None or v[0] < 2 else float(v[1] * v[0] * d)] for v in vifs])
    return tf, cnt, sumt, ss


@pytest.mark.parametrize("rho,allow_neg", [(None, False), (None, True), (0.01, False), (-0.02, False)])
def test_finish_against_50_digits(rho, allow_neg):
    mp = mpmath
    X, D, use, sets = _case(7, 24, 12, 2, True)
    X[3, np.flatnonzero(use)[1]] = np.nan                      # a gene that leaves the universe
    sets = sets + [[3, 4, 5], [3], []]                          # fewer ok members than members; no ok member; empty
    ref = cr.camera_mp(X, D, use, np.array([0.0, 1.0]), sets, rho, allow_neg)
    fit = lr.limma_mp(X, D, use, np.array([0.0, 1.0]))
    vifs, ok = cr.mp_vif(X, D, use, sets)
    t = [None if r is None else r["t"][0] for r in fit["rows"]]
    d = float(int(np.sum(use)) - 2)
    tf, cnt, sumt, ss = _finish_inputs(t, ok, sets, vifs, d)
    out, gdf = engine.camera_finish(tf, ok, sumt, cnt, None if rho is not None else ss, [d], [float(fit["df_prior"])], rho,
                                    allow_neg)
    got, want = out[:, :, 0, 0], cr.table_float(ref["tables"][0])
    assert gdf[0, 0] == ref["G"] == 23 and abs(gdf[0, 1] - float(ref["dfc"])) <= 4 * U * gdf[0, 1]
    assert np.array_equal(got[:, 0], want[:, 0])
    assert np.array_equal(np.isnan(got[:, :7]), np.isnan(want))
    G = float(ref["G"])
    tk = np.abs(tf[ok, 0, 0])
    var = float(np.var(tf[ok, 0, 0], ddof=1))
    for s, row in enumerate(ref["tables"][0]):
        m = got[s, 0]
        if row["VIF"] is not None:
            assert abs(got[s, 2] - want[s, 2]) <= 4 * U * abs(want[s, 2]), (s, got[s, 2], want[s, 2])
        if row["Correlation"] is not None:
            assert abs(got[s, 1] - want[s, 1]) <= 6 * U * max(abs(want[s, 1]), 1.0 / max(m - 1, 1)), (s, got[s, 1], want[s, 1])
        if row["t"] is None:
            continue
        m2 = G - m
        used = want[s, 2] if (rho is not None or allow_neg) else max(want[s, 2], 1.0)
        T = want[s, 3]
        k = used / m + 1.0 / m2
        # pooled from the reference's own T: T = delta / sqrt(pooled k)
        dl = (G / m2) * (float(sumt[s, 0, 0]) / m - float(np.mean(tf[ok, 0, 0])))
        pooled = (dl / T) ** 2 / k if T != 0 else ((G - 1) * var) / (G - 2)
        d_delta = (G / m2) * 2 * (G + 3) * U * tk.max()
        d_pooled = (2 * G + 8) * U * (G - 1) * var / (G - 2) + 2 * abs(dl) * d_delta * m * m2 / (G * (G - 2))
        bound = 4 * (d_delta / np.sqrt(pooled * k) + abs(T) * (d_pooled / (2 * pooled) + 4 * U))
        assert abs(got[s, 3] - T) <= bound, (s, got[s, 3], T, bound)
        # the tails at the library's own T and df
        half = float(xs.two_pt(got[s, 3], gdf[0, 1])) / 2
        acc = xs.ASSERTED_ACC["pt"]
        lo, hi = (got[s, 4], got[s, 5]) if got[s, 3] < 0 else (got[s, 5], got[s, 4])
        assert abs(lo - half) <= acc * half and abs(hi - (1 - half)) <= acc * half + U
        assert got[s, 6] == 2 * min(got[s, 4], got[s, 5])
    assert np.array_equal(out[:, 7, 0, 0], lr.bh(out[:, 6, 0, 0]), equal_nan=True) or \
        np.allclose(out[:, 7, 0, 0], lr.bh(out[:, 6, 0, 0]), rtol=4 * U, atol=0, equal_nan=True)


def test_finish_edge_rows():
    """m = 0, m = 1, m = G (m2 = 0), fewer ok members than members; G = 2 makes every test NaN; a negative fixed rho on a large
    set (vif / m + 1 / m2 <= 0) is NaN in the test alone"""
    rng = np.random.default_rng(8)
    g = 12
    t = rng.normal(size=(g, 1, 1))
    ok = np.ones((g, 1), dtype=np.int8)
    ok[[2, 7]] = 0
    t[[2, 7]] = np.nan
    okb = ok[:, 0] != 0
    sets = [[], [0], list(range(g)), [1, 2, 3], [2], [0, 1, 3, 4, 5]]
    cnt = np.array([[float(sum(okb[i] for i in s))] for s in sets])
    sumt = np.array([sum(t[i, 0, 0] for i in s if okb[i]) for s in sets]).reshape(-1, 1, 1)
    ss = np.array([[0.0], [5.0], [30.0], [9.0], [0.0], [20.0]])
    out, gdf = engine.camera_finish(t, ok, sumt, cnt, ss, [6.0], [3.0])
    tab = out[:, :, 0, 0]
    assert gdf.tolist() == [[10.0, 8.0]]                       # df.camera = min(6 + 3, 10 - 2)
    assert tab[:, 0].tolist() == [0, 1, 10, 2, 0, 5]
    assert np.isnan(tab[0, 1:]).all() and np.isnan(tab[4, 1:]).all()          # m = 0
    assert tab[1, 2] == 1.0 and np.isnan(tab[1, 1]) and not np.isnan(tab[1, 3:7]).any()   # m = 1: vif 1, no correlation, tested
    assert tab[2, 2] == 30.0 / (10 * 6.0) and np.isnan(tab[2, 3:]).all()      # m = G: VIF reported, no test
    assert tab[3, 2] == 9.0 / (2 * 6.0) and tab[3, 1] == tab[3, 2] - 1.0      # 2 of 3 members ok
    assert tab[5, 2] == 20.0 / (5 * 6.0) and not np.isnan(tab[5, 3])
    # the estimated vif below 1 is raised to 1 in the test unless allow_neg_cor; the reported columns stay
    out2, _ = engine.camera_finish(t, ok, sumt, cnt, ss, [6.0], [3.0], None, True)
    assert np.array_equal(out2[:, 0:3, 0, 0], tab[:, 0:3], equal_nan=True)
    assert tab[3, 2] < 1 and abs(out2[3, 3, 0, 0]) > abs(tab[3, 3])
    assert tab[5, 2] < 1 and abs(out2[5, 3, 0, 0]) > abs(tab[5, 3])
    # a fixed negative rho on the set of 5 of 10: vif / m + 1 / m2 = (1 - 3.6) / 5 + 1 / 5 < 0
    out3, _ = engine.camera_finish(t, ok, sumt, cnt, None, [6.0], [3.0], -0.9, False)
    assert out3[5, 2, 0, 0] == 1.0 + 4.0 * -0.9 and np.isnan(out3[5, 3:, 0, 0]).all() and out3[5, 1, 0, 0] == -0.9
    # G = 2
    ok2 = np.zeros((g, 1), dtype=np.int8)
    ok2[[0, 1]] = 1
    out4, gdf4 = engine.camera_finish(t, ok2, sumt[:2], np.array([[0.0], [1.0]]), ss[:2], [6.0], [3.0])
    assert gdf4[0, 0] == 2 and np.isnan(out4[:, 3:, 0, 0]).all()
