"""plaid.limma with na = "fit" for the tests (include/plaidhip.h: plaidhip_limma_na).

mp_refit      a row refitted on the samples it has, at 50 digits, WITHOUT the downdate: tests/helpers/limma_ref.mp_design on
              the row's observed samples and mp_fit -- "limma refits the row on the rest".
emulate_*     the pinned order (E' in blocks of 128, the H chains, Cholesky, the substitutions, logFC, the residual chain) in
              plain fp64 with an exact fma, from the Q that plaidhip_limma_design returns.  It shares no line with
              csrc/lmfit_na.h.
mp_finish_na  the unequal-df eBayes of the header at 50 digits.
limma_na_mp   both, end to end for one fit of a matrix with NaN.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from tests.helpers import exact_stats as xs
from tests.helpers import limma_ref as lr

U = lr.U
PIVOT_MIN = 1e-10
# the largest |emulation - mp_refit| / units(...) seen over the solve cases (logFC, u, RSS), and the factor
# the allowance takes over it.  tests/test_limma_na_ref.py asserts that the emulation stays below RATIO_SEEN.
RATIO_SEEN = {"logFC": 0.19, "u": 0.11, "rss": 0.01}   # seen: 0.1822, 0.1054, 0.0096
FACTOR = 4.0


def fma(a, b, c):
    """the correctly rounded a * b + c"""
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


# ---- the pinned order in fp64 ---------------------------------------------------------------------------------------------------
def emulate_effects(x, Q, sel):
    """E'_k: the select `c in sel and x_c == x_c`, blocks of 128 columns ascending, fma chains from 0.0"""
    n, p = Q.shape
    insel = np.zeros(n, dtype=bool)
    insel[sel] = True
    E = [0.0] * p
    for k in range(p):
        tot = 0.0
        for c0 in range(0, n, 128):
            acc = 0.0
            for c in range(c0, min(n, c0 + 128)):
                if insel[c] and x[c] == x[c]:
                    acc = fma(float(x[c]), float(Q[c, k]), acc)
            tot = tot + acc
        E[k] = tot
    return E


def emulate_solve(qmis, Ep, v):
    """(ok, gamma, u list, pivots) of the header's words: H by chains over the missing rows, Cholesky row by row, forward,
    back, w = L^-1 v_j"""
    qmis = np.asarray(qmis, dtype=np.float64).reshape(-1, len(Ep))
    p = len(Ep)
    H = [[0.0] * p for _ in range(p)]
    for k in range(p):
        for l in range(k + 1):
            s = 0.0
            for i in range(qmis.shape[0]):
                s = fma(float(qmis[i, k]), float(qmis[i, l]), s)
            H[k][l] = (1.0 if k == l else 0.0) - s
    piv = []
    for k in range(p):
        for l in range(k):
            s = H[k][l]
            for m in range(l):
                s = fma(-H[k][m], H[l][m], s)
            H[k][l] = s / H[l][l]
        d = H[k][k]
        for m in range(k):
            d = fma(-H[k][m], H[k][m], d)
        piv.append(d)
        if not d > PIVOT_MIN:
            return False, None, None, piv
        H[k][k] = float(np.sqrt(d))
    g = [0.0] * p
    for k in range(p):
        s = float(Ep[k])
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


def emulate_logfc(v, gamma):
    v = np.asarray(v, dtype=np.float64).reshape(len(gamma), -1)
    out = []
    for j in range(v.shape[1]):
        s = 0.0
        for k in range(len(gamma)):
            s = fma(float(v[k, j]), gamma[k], s)
        out.append(s)
    return out


def emulate_rss(x, Q, sel, gamma):
    """the residual chain at gamma with the extended select, blocks of 128"""
    n, p = Q.shape
    insel = np.zeros(n, dtype=bool)
    insel[sel] = True
    tot = 0.0
    for c0 in range(0, n, 128):
        acc = 0.0
        for c in range(c0, min(n, c0 + 128)):
            r = float(x[c])
            for k in range(p):
                r = fma(-float(Q[c, k]), gamma[k], r)
            if insel[c] and x[c] == x[c]:
                acc = acc + r * r
        tot = tot + acc
    return tot


# ---- 50 digits ------------------------------------------------------------------------------------------------------------------
def obs_mask(x, use=None):
    x = np.asarray(x, dtype=np.float64)
    m = ~np.isnan(x)
    return m if use is None else m & (np.asarray(use) != 0)


def mp_refit(x, D, use=None, K=None):
    """one row on its observed samples: dict of logFC (q), u (q), rss, M, d = |obs| - p -- mp numbers -- or None when the
    reduced design is rank-deficient or has no residual degree of freedom (exactly, at 50 digits: the Gram-Schmidt norm is 0)"""
    mp = lr._mp()
    D = np.asarray(D, dtype=np.float64)
    m = obs_mask(x, use)
    d = int(m.sum()) - D.shape[1]
    if d < 1:
        return None
    try:
        des = lr.mp_design(D, use=m, K=K)
    except ZeroDivisionError:
        return None
    with mp.workdps(lr.DPS + 20):
        if any(abs(des["R"][k][k]) < mp.mpf(10) ** -40 for k in range(D.shape[1])):
            return None
    fit = lr.mp_fit(np.asarray(x, dtype=np.float64)[None, :], des)[0]
    if fit is None:
        return None
    E, M, rss = fit
    with mp.workdps(lr.DPS + 20):
        fc = [mp.fsum(a * b for a, b in zip(vj, E)) for vj in des["v"]]
    return {"logFC": fc, "u": des["u"], "rss": rss, "M": M, "d": d}


def mp_H(Q, mis):
    """(H, |H^-1|_2, its pivots) at 50 digits from the fp64 Q's rows of the missing samples"""
    mp = lr._mp()
    p = Q.shape[1]
    with mp.workdps(lr.DPS + 20):
        H = mp.eye(p)
        for c in mis:
            q = mp.matrix([mp.mpf(float(t)) for t in Q[c]])
            H -= q * q.T
        piv, L = [], mp.zeros(p, p)
        for k in range(p):
            for l in range(k):
                L[k, l] = (H[k, l] - mp.fsum(L[k, m] * L[l, m] for m in range(l))) / L[l, l] if L[l, l] != 0 else mp.mpf(0)
            dk = H[k, k] - mp.fsum(L[k, m] ** 2 for m in range(k))
            piv.append(dk)
            L[k, k] = mp.sqrt(dk) if dk > 0 else mp.mpf(0)
        ev = mp.eigsy(H, eigvals_only=True)
        lam = min(ev)
        return H, (1 / lam if lam > mp.mpf(10) ** -30 else mp.inf), piv


def mp_pivots_exact(D, use, mis):
    """the Cholesky pivots of H from the EXACT Q of D (50-digit Gram-Schmidt): a pivot that is 0 comes out below 1e-60"""
    mp = lr._mp()
    D = np.asarray(D, dtype=np.float64)
    des = lr.mp_design(D, use=use)
    sel = list(des["sel"])
    p = D.shape[1]
    with mp.workdps(lr.DPS + 20):
        H = mp.eye(p)
        for c in mis:
            i = sel.index(c)
            q = mp.matrix([des["Q"][k][i] for k in range(p)])
            H -= q * q.T
        piv, L = [], mp.zeros(p, p)
        for k in range(p):
            for l in range(k):
                L[k, l] = (H[k, l] - mp.fsum(L[k, m] * L[l, m] for m in range(l))) / L[l, l] if abs(L[l, l]) > mp.mpf(10) ** -30 else mp.mpf(0)
            dk = H[k, k] - mp.fsum(L[k, m] ** 2 for m in range(k))
            piv.append(dk)
            L[k, k] = mp.sqrt(dk) if dk > mp.mpf(10) ** -60 else mp.mpf(0)
        return piv


def units(x, Q, sel, mis, v, ref, hinv):
    """the magnitudes the allowances scale with, per contrast: for logFC (|mis| + p^2 + n_f) 2^-53 |H^-1| |v_j| |mag|, mag_k =
    sum over obs of |x_c| |Q[c, k]| (what lr.effects_bound takes); for u the same count times |H^-1| u_j; for the RSS the
    count times |H^-1| (sum over obs of (|x_c| + |q_c| |H^-1| |mag|)^2)"""
    p = Q.shape[1]
    obs = [c for c in sel if c not in set(mis)]
    cnt = (len(mis) + p * p + len(sel)) * U
    mag = np.array([np.sum(np.abs(x[obs]) * np.abs(Q[obs, k])) for k in range(p)])
    nm = float(np.linalg.norm(mag))
    v = np.asarray(v, dtype=np.float64).reshape(p, -1)
    hinv = float(hinv)
    ufc = [cnt * hinv * float(np.linalg.norm(v[:, j])) * nm for j in range(v.shape[1])]
    uu = [cnt * hinv * float(ref["u"][j]) for j in range(v.shape[1])]
    rho = np.abs(x[obs]) + np.linalg.norm(Q[obs], axis=1) * hinv * nm
    return {"logFC": ufc, "u": uu, "rss": cnt * hinv * float(np.sum(rho * rho))}


def deviations(got_fc, got_u, got_rss, ref, unit):
    """the worst |got - ref| / unit of logFC, u and the RSS"""
    out = {"logFC": 0.0, "u": 0.0, "rss": 0.0}
    for j in range(len(got_fc)):
        out["logFC"] = max(out["logFC"], float(abs(got_fc[j] - ref["logFC"][j])) / unit["logFC"][j])
        out["u"] = max(out["u"], float(abs(got_u[j] - ref["u"][j])) / unit["u"][j])
    out["rss"] = float(abs(got_rss - ref["rss"])) / unit["rss"]
    return out


# ---- the solve cases (host) -----------------------------------------------------------------------------------------------------
def solve_design(p, n=37, seed=5):
    """intercept, a two-group column, then batch covariates: n x p (p = 1: the intercept alone)"""
    rng = np.random.default_rng(seed + p)
    g = (np.arange(n) % 2).astype(np.float64)
    cols = [np.ones(n), g] + [rng.normal(size=n) for _ in range(max(0, p - 2))]
    return np.column_stack(cols[:p]), g


def solve_missing(g, kind):
    """the missing samples of a case: 1, 2, half of group 1, all but one of group 1"""
    one = np.flatnonzero(g == 1)
    return {"one": [3], "two": [0, 128 % len(g)], "half": list(one[: len(one) // 2]), "all_but_one": list(one[:-1])}[kind]


MISSING_KINDS = ("one", "two", "half", "all_but_one")


# ---- eBayes with unequal df -----------------------------------------------------------------------------------------------------
def mp_finish_na(fits, d, v, u):
    """fits: per row (E list of p, M, rss) in mp or None; d: per row int or None; v: q lists of p; u: per row list of q (mp).
    The header's unequal-df text: dict like lr.mp_finish, plus df_pooled and per row df_total"""
    mp = lr._mp()
    with mp.workdps(lr.DPS + 20):
        s2 = [None if f is None or dd is None else f[2] / dd for f, dd in zip(fits, d)]
        okr = [r for r, s in enumerate(s2) if s is not None]
        nok = len(okr)
        pooled = mp.mpf(sum(d[r] for r in okr))
        if nok < 2:
            d0, s0, branch = mp.mpf(0), mp.nan, "none"
        else:
            srt = sorted(s2[r] for r in okr)
            med = srt[nok // 2] if nok % 2 else (srt[nok // 2 - 1] + srt[nok // 2]) / 2
            if med == 0:
                med = mp.mpf(1)
            x = [max(s2[r], mp.mpf("1e-5") * med) for r in okr]
            e = [mp.log(t) - mp.psi(0, mp.mpf(d[r]) / 2) + mp.log(mp.mpf(d[r]) / 2) for t, r in zip(x, okr)]
            ebar = mp.fsum(e) / nok
            var = mp.fsum((t - ebar) ** 2 for t in e) / (nok - 1) - mp.fsum(mp.psi(1, mp.mpf(d[r]) / 2) for r in okr) / nok
            if var > 0:
                y = lr.mp_trigamma_inverse(var)
                d0, s0, branch = 2 * y, mp.exp(ebar + mp.psi(0, y) - mp.log(y)), "finite"
            else:
                d0, s0, branch = mp.inf, mp.fsum(x) / nok, "inf"
        rows = []
        for r, (f, s) in enumerate(zip(fits, s2)):
            if s is None:
                rows.append(None)
                continue
            dr = mp.mpf(d[r])
            post = s0 if d0 == mp.inf else s if d0 == 0 else (dr * s + d0 * s0) / (dr + d0)
            dft = pooled if d0 == mp.inf else min(dr + d0, pooled)
            fc = [mp.fsum(a * b for a, b in zip(vj, f[0])) for vj in v]
            t = [c / (uj * mp.sqrt(post)) if post > 0 else (mp.nan if c == 0 else mp.sign(c) * mp.inf) for c, uj in zip(fc, u[r])]
            rows.append({"logFC": fc, "t": t, "p": [xs.two_pt(tt, dft) for tt in t], "s2": s, "M": f[1], "df_total": dft,
                         "se": [uj * mp.sqrt(post) for uj in u[r]],
                         "mag": [mp.fsum(abs(a * b) for a, b in zip(vj, f[0])) for vj in v]})
        return {"df_prior": d0, "s2_prior": s0, "nok": nok, "branch": branch, "df_pooled": pooled, "rows": rows}


def limma_na_mp(X, D, use=None, K=None, max_na=0.2):
    """one fit of a matrix with NaN, end to end at 50 digits: every row refitted on the samples it has (mp_refit), rows above
    max_na or with an Inf in a used sample or not estimable left out, then mp_finish_na.  Rows: dict with logFC, t, p (q
    lists), s2, M, d, u -- or None"""
    mp = lr._mp()
    X = np.asarray(X, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64)
    n, p = D.shape
    cache, fits, ds, us, vs = {}, [], [], [], None
    for r in range(X.shape[0]):
        x = X[r]
        m = obs_mask(x, use)
        if np.isnan(x).sum() / n > max_na or not np.isfinite(x[m]).all() or int(m.sum()) - p < 1:
            fits.append(None), ds.append(None), us.append(None)
            continue
        key = m.tobytes()
        if key not in cache:
            try:
                des = lr.mp_design(D, use=m, K=K)
                with mp.workdps(lr.DPS + 20):
                    bad = any(abs(des["R"][k][k]) < mp.mpf(10) ** -40 for k in range(p))
            except ZeroDivisionError:
                des, bad = None, True
            cache[key] = None if bad else des
        des = cache[key]
        if des is None:
            fits.append(None), ds.append(None), us.append(None)
            continue
        E, M, rss = lr.mp_fit(x[None, :], des)[0]
        with mp.workdps(lr.DPS + 20):
            fc = [mp.fsum(a * b for a, b in zip(vj, E)) for vj in des["v"]]
        # (mp_finish_na forms logFC as v . E: hand it the unit vectors and the logFC themselves)
        fits.append((fc, M, rss)), ds.append(int(m.sum()) - p), us.append(des["u"])
        vs = len(fc)
    q = vs if vs is not None else (p if K is None else np.asarray(K).reshape(p, -1).shape[1])
    with mp.workdps(lr.DPS + 20):
        eye = [[mp.mpf(1 if a == b else 0) for a in range(q)] for b in range(q)]
    res = mp_finish_na(fits, ds, eye, us)
    for r, row in enumerate(res["rows"]):
        if row is not None:
            row["d"], row["u"] = ds[r], us[r]
    return res


# ---- the sharding hook ----------------------------------------------------------------------------------------------------------
def run_sharded(nshards, A, design, use=None, contrasts=None, max_na=0.2, fail=-1):
    """(status, out, hyper, dfres) of plaid.limma with na = "fit" on `nshards` contexts of one device; the results hold -7
    before the call"""
    from plaid_amd import engine
    from tests.helpers.sharded_hooks import _status, hook
    A = np.asfortranarray(A, dtype=np.float64)
    D, _, _, q = engine.limma_operands(A.shape[1], design, use, contrasts)
    out = np.full((A.shape[0], 6, q, D.shape[2]), -7.0, order="F")
    hyper = np.full((D.shape[2], 5), -7.0)
    dfres = np.full((A.shape[0], D.shape[2]), -7.0, order="F")
    status, _ = _status(lambda: engine._limma_na(hook("limma_na"), (0, nshards, fail), A, design, use, contrasts, max_na, out=out,
                                                 hyper=hyper, dfres=dfres))
    return status, out, hyper, dfres
