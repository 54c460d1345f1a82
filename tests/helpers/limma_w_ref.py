"""plaid.limma with weights for the tests (include/plaidhip.h: plaidhip_limma_w).

mp_wls        one row's weighted least squares at 50 digits from the ORIGINAL design: the normal equations D' W D beta = D' W x
              over its live observations.  It does not go through Q.
np_wls        the same through numpy.linalg.lstsq on the rows scaled by sqrt(omega): shares no line with mp_wls.
emulate_*     the pinned order (the sums in blocks of 128, Cholesky with the relative pivot rule, the substitutions, the
              residual chain) in plain fp64 with an exact fma, from the Q that plaidhip_limma_design returns.  It shares no
              line with csrc/lmfit_na.h.
units         the forward bound of DESIGN.md section 28, from n, p, omega, x, |H^-1| and the basis' own error.
limma_w_mp    end to end for one fit at 50 digits (eBayes: limma_na_ref.mp_finish_na).
"""
from __future__ import annotations

import numpy as np

from tests.helpers import limma_na_ref as nr
from tests.helpers import limma_ref as lr

U = lr.U
PIVOT_REL = 1e-10
fma = nr.fma


def omega(wt, aw):
    """the effective weights of one row: Wt * aw in one rounded product; an operand that is None counts as 1.0"""
    if wt is None:
        return np.asarray(aw, dtype=np.float64).copy()
    wt = np.asarray(wt, dtype=np.float64)
    with np.errstate(all="ignore"):
        return wt.copy() if aw is None else wt * np.asarray(aw, dtype=np.float64)


def live_mask(x, om, use=None):
    x, om = np.asarray(x, dtype=np.float64), np.asarray(om, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        m = ~np.isnan(x) & (om > 0) & (om < np.inf)
    return m if use is None else m & (np.asarray(use) != 0)


# ---- 50 digits, from the original design ------------------------------------------------------------------------------------------
def mp_wls(x, om, D, use=None, K=None):
    """dict of logFC (q), u (q), rss, M, d = |live| - p, resid (the live residuals), live -- mp numbers -- or None: a live
    Inf value, d < 1, or a Gram matrix that is singular at 50 digits (a Cholesky pivot below 1e-40 of its diagonal entry)"""
    mp = lr._mp()
    x, om, D = np.asarray(x, dtype=np.float64), np.asarray(om, dtype=np.float64), np.asarray(D, dtype=np.float64)
    n, p = D.shape
    live = live_mask(x, om, use)
    idx = np.flatnonzero(live)
    d = len(idx) - p
    if d < 1 or not np.isfinite(x[idx]).all():
        return None
    Kc = np.eye(p) if K is None else np.asarray(K, dtype=np.float64).reshape(p, -1)
    # the Gram sums exactly, in integers (every input is a dyadic rational); then p x p work at 50 digits
    Di, sd = lr.to_ints(D[idx])
    wi, sw = lr.to_ints(om[idx])
    xi, sx = lr.to_ints(x[idx])
    WD = Di * wi[:, None]
    Gi, bi, xwx = WD.T.dot(Di), WD.T.dot(xi), int((wi * xi * xi).sum())
    with mp.workdps(lr.DPS + 20):
        G = mp.matrix(p, p)
        rhs = mp.matrix(p, 1)
        for k in range(p):
            rhs[k] = mp.ldexp(mp.mpf(int(bi[k])), -(sw + sd + sx))
            for l in range(p):
                G[k, l] = mp.ldexp(mp.mpf(int(Gi[k, l])), -(sw + 2 * sd))
        L = mp.zeros(p, p)
        for k in range(p):
            for l in range(k):
                L[k, l] = (G[k, l] - mp.fsum(L[k, m] * L[l, m] for m in range(l))) / L[l, l]
            dk = G[k, k] - mp.fsum(L[k, m] ** 2 for m in range(k))
            if not dk > mp.mpf(10) ** -40 * G[k, k]:
                return None
            L[k, k] = mp.sqrt(dk)
        y = mp.lu_solve(L, rhs)
        beta = mp.lu_solve(L.T, y)
        fc, us = [], []
        for j in range(Kc.shape[1]):
            kj = mp.matrix([mp.mpf(float(t)) for t in Kc[:, j]])
            fc.append(mp.fsum(kj[i] * beta[i] for i in range(p)))
            z = mp.lu_solve(L, kj)
            us.append(mp.sqrt(mp.fsum(t * t for t in z)))
        # RSS = x'Wx - b'beta at the exact minimiser (no cancellation that 70 digits would notice)
        rss = mp.ldexp(mp.mpf(xwx), -(sw + 2 * sx)) - mp.fsum(rhs[k] * beta[k] for k in range(p))
        seen = ~np.isnan(x) if use is None else ~np.isnan(x) & (np.asarray(use) != 0)
        M = mp.fsum(mp.mpf(float(t)) for t in x[seen]) / int(seen.sum())
        res = x[idx] - D[idx] @ np.array([float(t) for t in beta])   # (fp64: the bound takes their magnitudes only)
    return {"logFC": fc, "u": us, "rss": rss, "M": M, "d": d, "resid": res, "live": idx}


def np_wls(x, om, D, use=None, K=None):
    """the same numbers in fp64 by lstsq on the sqrt(omega)-scaled rows"""
    x, om, D = np.asarray(x, dtype=np.float64), np.asarray(om, dtype=np.float64), np.asarray(D, dtype=np.float64)
    p = D.shape[1]
    idx = np.flatnonzero(live_mask(x, om, use))
    s = np.sqrt(om[idx])
    Ds, xs = D[idx] * s[:, None], x[idx] * s
    beta = np.linalg.lstsq(Ds, xs, rcond=None)[0]
    Kc = np.eye(p) if K is None else np.asarray(K, dtype=np.float64).reshape(p, -1)
    res = xs - Ds @ beta
    return {"logFC": Kc.T @ beta, "u": np.sqrt(np.diag(Kc.T @ np.linalg.inv(Ds.T @ Ds) @ Kc)), "rss": float(res @ res),
            "d": len(idx) - p}


# ---- the pinned order in fp64 -----------------------------------------------------------------------------------------------------
def emulate_sums(x, om, Q, sel):
    """(Htri list, b list, M', |live|, the mean's count) of the header: blocks of 128 columns ascending, chains from 0.0"""
    n, p = Q.shape
    insel = np.zeros(n, dtype=bool)
    insel[sel] = True
    live = live_mask(x, om, insel)
    nf = int(insel.sum())

    def blocks(term, take):
        tot = 0.0
        for c0 in range(0, n, 128):
            acc = 0.0
            for c in range(c0, min(n, c0 + 128)):
                if take[c]:
                    acc = term(c, acc)
            tot = tot + acc
        return tot

    Htri = []
    for k in range(p):
        for l in range(k + 1):
            Htri.append(blocks(lambda c, a: fma(float(om[c]), float(Q[c, k] * Q[c, l]), a), live))
    with np.errstate(all="ignore"):
        y = om * x
    b = [blocks(lambda c, a: fma(float(y[c]), float(Q[c, k]), a), live) for k in range(p)]
    seen = insel & ~np.isnan(x)
    Mp = blocks(lambda c, a: fma(float(x[c]), 1.0 / nf, a), seen)
    return Htri, b, Mp, int(live.sum()), int(seen.sum())


def emulate_w_solve(Htri, b, nlive, v):
    """(ok, gamma, u list, pivots) of the header: Cholesky row by row with the relative pivot rule, forward, back, w = L^-1 v_j"""
    p = len(b)
    H = [[0.0] * p for _ in range(p)]
    it = iter(Htri)
    for k in range(p):
        for l in range(k + 1):
            H[k][l] = float(next(it))
    piv = []
    for k in range(p):
        for l in range(k):
            s = H[k][l]
            for m in range(l):
                s = fma(-H[k][m], H[l][m], s)
            H[k][l] = s / H[l][l]
        hkk = H[k][k]
        d = hkk
        for m in range(k):
            d = fma(-H[k][m], H[k][m], d)
        piv.append(d)
        if not d > PIVOT_REL * hkk:
            return False, None, None, piv
        H[k][k] = float(np.sqrt(d))
    if nlive - p < 1:
        return False, None, None, piv
    g = [0.0] * p
    for k in range(p):
        s = float(b[k])
        for m in range(k):
            s = fma(-H[k][m], g[m], s)
        g[k] = s / H[k][k]
    for k in range(p - 1, -1, -1):
        s = g[k]
        for m in range(k + 1, p):
            s = fma(-H[m][k], g[m], s)
        g[k] = s / H[k][k]
    v = np.asarray(v, dtype=np.float64).reshape(p, -1)
    us = []
    for j in range(v.shape[1]):
        w, s2 = [0.0] * p, 0.0
        for k in range(p):
            s = float(v[k, j])
            for m in range(k):
                s = fma(-H[k][m], w[m], s)
            w[k] = s / H[k][k]
            s2 = fma(w[k], w[k], s2)
        us.append(float(np.sqrt(s2)))
    return True, g, us, piv


def emulate_w_rss(x, om, Q, sel, gamma):
    """the weighted residual chain at gamma: r * r rounded first, then fma(omega, ., .), blocks of 128"""
    n, p = Q.shape
    insel = np.zeros(n, dtype=bool)
    insel[sel] = True
    live = live_mask(x, om, insel)
    tot = 0.0
    for c0 in range(0, n, 128):
        acc = 0.0
        for c in range(c0, min(n, c0 + 128)):
            if live[c]:
                r = float(x[c])
                for k in range(p):
                    r = fma(-float(Q[c, k]), gamma[k], r)
                acc = fma(float(om[c]), r * r, acc)
        tot = tot + acc
    return tot


def pivot_ratios(Htri, p):
    """the Cholesky pivots d_k / H_kk of a triangle in plain fp64 (the host's estimability assertion)"""
    H = np.zeros((p, p))
    H[np.tril_indices(p)] = Htri
    H = H + np.tril(H, -1).T
    try:
        L = np.linalg.cholesky(H)
    except np.linalg.LinAlgError:                       # (a pivot that is not positive)
        return np.zeros(p)
    return np.diag(L) ** 2 / np.diag(H)


def expected_integers(A, Wt, aw, Q, use, max_na):
    """(ok, d) of every row of one fit by the header's rules in plain numpy: fitted by max_na, |live| - p >= 1, no live Inf,
    every pivot ratio above the rule (the cases keep them either above 1e-3 or at rounding level)"""
    rows, n = A.shape
    p = Q.shape[1]
    ok, d = np.zeros(rows, dtype=bool), np.zeros(rows)
    for r in range(rows):
        om = omega(None if Wt is None else Wt[r], aw)
        live = live_mask(A[r], om, use)
        d[r] = live.sum() - p
        if np.isnan(A[r]).sum() / n > max_na or d[r] < 1 or not np.isfinite(A[r][live]).all():
            continue
        H = (Q[live] * om[live, None]).T @ Q[live]
        ok[r] = pivot_ratios(H[np.tril_indices(p)], p).min() > 1e-6
    return ok, d


# ---- the bound of DESIGN.md section 28 --------------------------------------------------------------------------------------------
def exact_H(Q, om, live):
    """(|H^-1|_2, Hn = sum omega |q_c|^2 >= |H|_2) of H = sum over the live c of omega_c q_c q_c', summed exactly in integers
    from the fp64 Q and rounded once; the smallest eigenvalue by numpy (the bound takes |H^-1| 1e-6 larger than that)"""
    live = np.asarray(live)
    Qi, sq = lr.to_ints(Q[live])
    wi, sw = lr.to_ints(om[live])
    H = lr.ints_to_float((Qi * wi[:, None]).T.dot(Qi), sw + 2 * sq)
    lam = float(np.linalg.eigvalsh(H).min())
    return ((1.0 + 1e-6) / lam if lam > 0 else np.inf), float(np.sum(om[live] * np.sum(Q[live] ** 2, axis=1)))


def basis_error(D, use, K, des):
    """what plaidhip_limma_design's fp64 basis `des` is away from the exact one of the original design, measured at 50 digits:
    (eta_Q = |Q - Q~ S|_F over the used rows, [|v_j - S v~_j|_2]); S = the signs of R's diagonal (the exact basis has it positive)"""
    mp = lr._mp()
    ex = lr.mp_design(D, use=use, K=K)
    p = ex["p"]
    sgn = np.sign(np.diag(des["R"]))
    with mp.workdps(lr.DPS + 20):
        eq = mp.sqrt(mp.fsum((mp.mpf(float(des["Q"][c, k])) - mp.mpf(float(sgn[k])) * ex["Q"][k][i]) ** 2
                             for k in range(p) for i, c in enumerate(ex["sel"])))
        ev = [mp.sqrt(mp.fsum((mp.mpf(float(des["v"][k, j])) - mp.mpf(float(sgn[k])) * ex["v"][j][k]) ** 2 for k in range(p)))
              for j in range(len(ex["v"]))]
    return float(eq), [float(t) for t in ev]


def units(x, om, Q, sel, v, ref, hinv, Hn, eta_q, eta_v):
    """DESIGN.md section 28, per contrast: the first-order forward bounds of logFC, u and the RSS, doubled for the orders it
    drops (the bound asserts that cnt (1 + |H^-1| Hn) stays below 2^-20, where they are far smaller)."""
    x, om = np.asarray(x, dtype=np.float64), np.asarray(om, dtype=np.float64)
    p = Q.shape[1]
    live = np.asarray(ref["live"])
    cnt = (len(sel) + 4 * p * p + 8) * U
    kap = 1.0 + hinv * Hn
    assert cnt * kap < 2.0 ** -20, (cnt, kap)
    ox = om[live] * np.abs(x[live])
    nm = float(np.linalg.norm([np.sum(ox * np.abs(Q[live, k])) for k in range(p)]))
    wmax = float(om[live].max())
    gnorm = hinv * nm                                              # |gamma| <= |H^-1| |b| <= |H^-1| |mag|
    dH = cnt * Hn + 2.0 * wmax * eta_q                             # arithmetic (sums and Cholesky's backward error) + basis
    dgam = hinv * (cnt * nm + eta_q * float(np.linalg.norm(ox)) + dH * gnorm)
    v = np.asarray(v, dtype=np.float64).reshape(p, -1)
    out = {"logFC": [], "u": []}
    for j in range(v.shape[1]):
        vn = float(np.linalg.norm(v[:, j]))
        out["logFC"].append(2.0 * (vn * dgam + (eta_v[j] + p * U * vn) * gnorm))
        uj = float(ref["u"][j])
        out["u"].append(2.0 * ((2.0 * eta_v[j] * hinv * vn + hinv * hinv * vn * vn * dH) / (2.0 * uj) + (p + 3) * U * uj))
    qn = np.linalg.norm(Q[live], axis=1)
    rho = np.abs(x[live]) + qn * gnorm
    e = eta_q * gnorm + qn * dgam + (p + 1) * U * rho
    r = np.abs(np.asarray(ref["resid"], dtype=np.float64))
    out["rss"] = 2.0 * (float(np.sum(om[live] * (2.0 * r * e + e * e))) + (len(sel) + 4) * U * float(ref["rss"]))
    return out


# ---- end to end at 50 digits ------------------------------------------------------------------------------------------------------
def limma_w_mp(X, Wt, aw, D, use=None, K=None, max_na=0.2, tail=True):
    """one fit, every row by mp_wls, rows above max_na left out, then limma_na_ref.mp_finish_na.  Rows: dict with logFC, t, p
    (q lists), s2, M, d, u, and the row's mp_wls result under "wls" -- or None.  tail = False: the list of the rows' mp_wls
    results alone (no eBayes)"""
    mp = lr._mp()
    X = np.asarray(X, dtype=np.float64)
    n, p = np.asarray(D).shape
    fits, ds, us, keep = [], [], [], []
    for r in range(X.shape[0]):
        om = omega(None if Wt is None else Wt[r], aw)
        fit = mp_wls(X[r], om, D, use, K) if np.isnan(X[r]).sum() / n <= max_na else None
        keep.append(fit)
        if fit is None:
            fits.append(None), ds.append(None), us.append(None)
        else:   # (mp_finish_na forms logFC as v . E: hand it the unit vectors and the logFC themselves)
            fits.append((fit["logFC"], fit["M"], fit["rss"])), ds.append(fit["d"]), us.append(fit["u"])
    if not tail:
        return keep
    q = p if K is None else np.asarray(K).reshape(p, -1).shape[1]
    with mp.workdps(lr.DPS + 20):
        eye = [[mp.mpf(1 if a == b else 0) for a in range(q)] for b in range(q)]
    res = nr.mp_finish_na(fits, ds, eye, us)
    for r, row in enumerate(res["rows"]):
        if row is not None:
            row["d"], row["u"], row["wls"] = ds[r], us[r], keep[r]
    return res


# ---- the sharding hook ------------------------------------------------------------------------------------------------------------
def run_sharded(nshards, A, weights, design, use=None, contrasts=None, max_na=0.2, fail=-1):
    """(status, out, hyper, dfres) of plaid.limma with weights on `nshards` contexts of one device; the results hold -7 before
    the call"""
    from plaid_amd import engine
    from tests.helpers.sharded_hooks import _status, hook
    A = np.asfortranarray(A, dtype=np.float64)
    D, _, _, q = engine.limma_operands(A.shape[1], design, use, contrasts)
    out = np.full((A.shape[0], 6, q, D.shape[2]), -7.0, order="F")
    hyper = np.full((D.shape[2], 5), -7.0)
    dfres = np.full((A.shape[0], D.shape[2]), -7.0, order="F")
    status, _ = _status(lambda: engine._limma_w(hook("limma_w"), (0, nshards, fail), A, weights, design, use, contrasts, max_na,
                                                out=out, hyper=hyper, dfres=dfres))
    return status, out, hyper, dfres


# ---- the cases the host and the GPU tests share -----------------------------------------------------------------------------------
CASES = [(515, 300, 3, 3), (130, 131, 10, 2), (3, 130, 1, 1), (40, 7, 2, 1)]
IDS = [f"rows{c[0]}-n{c[1]}-p{c[2]}-nfit{c[3]}" for c in CASES]
# the instances and tiles CASES does not reach, at a dozen rows (12: every designated row; 11: odd, the 8-byte loads): p = 5 and
# 8 (the 8-register residual kernel) and p = 9 (the first p past it); nfit = 9 (a second tile of 8 fits in the counts kernel,
# holding one fit) and nfit = 17 (three of them; Wc = 3 and W = 51, so the tiles of 8 weight columns straddle fits)
P_CASES = [(12, 131, 5, 1), (11, 131, 8, 2), (12, 131, 9, 1), (12, 40, 2, 9), (11, 40, 1, 17)]
# (appended: P_CASES[:3] keeps its meaning) p = 9 on an odd number of rows: the last instance of the residual kernel (p past 8) on
# the 8-byte loads, which no case above launches
P_CASES += [(11, 131, 9, 1)]
P_IDS = [f"rows{c[0]}-n{c[1]}-p{c[2]}-nfit{c[3]}" for c in P_CASES]
# the designated rows (a case with fewer rows has those that fit): weights that make an observation missing at columns 0, 127,
# 128 and n - 1 (zero, negative, NaN, +Inf); all weights zero within one group of fit 1 (not estimable); |live| = p in fit 1; a
# live Inf value; NaN values beside the weights
ROLE = {"w_zero": 3, "w_neg": 4, "w_nan": 5, "w_inf": 6, "group": 7, "p_left": 8, "inf_live": 9, "nan_beside": 10, "above": 11}


def make_case(case):
    """designs [1, group, covariates] (p = 1: the intercept alone), use (several fits: each leaves samples out), A, the
    observation weights Wt (log-uniform in [0.25, 4]) with the designated rows, array weights aw, and K (two contrasts, p = 1:
    one)"""
    rows, n, p, nfit = case
    rng = np.random.default_rng(list(case) + [28])
    D = np.empty((n, p, nfit), order="F")
    use = np.ones((n, nfit), dtype=np.int8, order="F") if nfit > 1 else None
    for f in range(nfit):
        D[:, 0, f] = 1.0
        if p > 1:
            D[:, 1, f] = rng.permutation(np.arange(n) % 2)
            D[:, 2:, f] = rng.normal(size=(n, p - 2))
        if use is not None:
            use[rng.random(n) < 0.2, f] = 0
            use[[0, min(127, n - 1), min(128, n - 1), n - 1], f] = 1
    A = rng.normal(size=(rows, n)) * np.exp(0.5 * rng.normal(size=(rows, 1))) + rng.normal(size=(rows, 1))
    Wt = np.exp(rng.uniform(np.log(0.25), np.log(4.0), size=(rows, n)))
    aw = np.exp(rng.uniform(np.log(0.25), np.log(4.0), size=n))
    edge = sorted({0, min(127, n - 1), min(128, n - 1), n - 1})
    sel0 = np.arange(n) if use is None else np.flatnonzero(use[:, 0] != 0)
    role = {k: r for k, r in ROLE.items() if r < rows}
    for key, bad in (("w_zero", 0.0), ("w_neg", -1.5), ("w_nan", np.nan), ("w_inf", np.inf)):
        if key in role:
            Wt[role[key], edge] = bad
    if "group" in role and p > 1:
        Wt[role["group"], sel0[D[sel0, 1, 0] == 1]] = 0.0
    if "p_left" in role:
        Wt[role["p_left"], rng.permutation(sel0)[p:]] = 0.0
    if "inf_live" in role:
        A[role["inf_live"], sel0[2]] = np.inf
    if "nan_beside" in role:
        A[role["nan_beside"], sel0[[1, 3]]] = np.nan
        Wt[role["nan_beside"], sel0[[4, 5]]] = 0.0
    if "above" in role and n > 20:
        A[role["above"], rng.permutation(n)[: int(0.25 * n) + 1]] = np.nan
    if p > 1:
        K = np.zeros((p, 2), order="F")
        K[1, 0], K[1, 1], K[0, 1] = 1.0, 1.0, -0.5
    else:
        K = np.ones((1, 1), order="F")
    return dict(D=D, use=use, A=np.asfortranarray(A), Wt=np.asfortranarray(Wt), aw=aw, K=K, role=role)


def fit_use(c, f):
    return None if c["use"] is None else c["use"][:, f]


def case_designs(c, case):
    """plaidhip_limma_design of every fit of a case (on the host)"""
    from plaid_amd import engine
    return [engine.limma_design(c["D"][:, :, f], fit_use(c, f), c["K"], fit=f + 1) for f in range(case[3])]


def designated(c):
    return set(c["role"].values())


def assert_other_rows_are_far_from_the_rule(c, case):
    """on the CPU: the smallest Cholesky pivot ratio d_k / H_kk of every row that is not designated exceeds 1e-3, so the
    estimability rule is exercised only where the case plants it"""
    rows, n, p, nfit = case
    for f in range(nfit):
        Q = c["des"][f]["Q"]
        uf = fit_use(c, f)
        for r in range(rows):
            if r in designated(c):
                continue
            om = omega(c["Wt"][r], c["aw"])
            live = live_mask(c["A"][r], om, uf)
            H = (Q[live] * om[live, None]).T @ Q[live]
            assert pivot_ratios(H[np.tril_indices(p)], p).min() > 1e-3, (r, f)
