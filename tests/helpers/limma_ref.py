"""plaid.limma for the tests: two restatements of the statistic pinned in include/plaidhip.h (plaidhip_limma), exact integer
arithmetic for the two device passes, the branch cases that the host and the GPU tests share, and the sharding hook.

limma_mp   the header's words in mpmath at 50 digits: QR by exact Gram-Schmidt, mpmath.psi, a bracketed root for the trigamma
           inverse, the t tail by betainc (tests/helpers/exact_stats.two_pt).
limma_np   independent of that form: numpy.linalg.lstsq per fit, (X'X)^-1 for stdev.unscaled, scipy.special.digamma /
           polygamma, scipy.stats.t.sf.  It shares no line with the library or with limma_mp.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from plaid_amd import engine
from tests.helpers import exact_stats as xs
from tests.helpers.sharded_hooks import _status, hook

DPS = 50
U = 2.0 ** -53


def _mp():
    import mpmath
    return mpmath


def _sel(n, use):
    return np.arange(n) if use is None else np.flatnonzero(np.asarray(use) != 0)


# ---- limma_mp ------------------------------------------------------------------------------------------------------------------
def mp_design(D, use=None, K=None):
    """Q (nf x p, the used rows only), R (p x p), v = R^-T K (q lists of p), u (q), sel, at 50 digits: classical Gram-Schmidt
    in exact-enough arithmetic (R's diagonal positive; logFC, u and the RSS do not depend on the signs)"""
    mp = _mp()
    D = np.asarray(D, dtype=np.float64)
    n, p = D.shape
    sel = _sel(n, use)
    with mp.workdps(DPS + 20):
        a = [[mp.mpf(float(D[c, k])) for c in sel] for k in range(p)]          # columns
        Q, R = [], [[mp.mpf(0)] * p for _ in range(p)]
        for k in range(p):
            w = list(a[k])
            for l in range(k):
                R[l][k] = mp.fsum(x * y for x, y in zip(Q[l], a[k]))
                w = [x - R[l][k] * y for x, y in zip(w, Q[l])]
            R[k][k] = mp.sqrt(mp.fsum(x * x for x in w))
            Q.append([x / R[k][k] for x in w])
        Kc = np.eye(p) if K is None else np.asarray(K, dtype=np.float64).reshape(p, -1)
        v, u = [], []
        for j in range(Kc.shape[1]):
            vj = []
            for i in range(p):
                acc = mp.mpf(float(Kc[i, j])) - mp.fsum(R[l][i] * vj[l] for l in range(i))
                vj.append(acc / R[i][i])
            v.append(vj)
            u.append(mp.sqrt(mp.fsum(x * x for x in vj)))
    return {"Q": Q, "R": R, "v": v, "u": u, "sel": sel, "nf": len(sel), "p": p}


def mp_fit(X, des):
    """per row of X: (E list of p, M, RSS) at 50 digits, or None for a row with a non-finite value in a used sample"""
    mp = _mp()
    X = np.asarray(X, dtype=np.float64)
    out = []
    with mp.workdps(DPS + 20):
        for r in range(X.shape[0]):
            x = X[r, des["sel"]]
            if not np.isfinite(x).all():
                out.append(None)
                continue
            xm = [mp.mpf(float(t)) for t in x]
            E = [mp.fsum(a * b for a, b in zip(xm, q)) for q in des["Q"]]
            res = [a - mp.fsum(q[c] * e for q, e in zip(des["Q"], E)) for c, a in enumerate(xm)]
            out.append((E, mp.fsum(xm) / len(xm), mp.fsum(t * t for t in res)))
    return out


def mp_trigamma_inverse(v):
    """the root y of psi'(y) = v, v > 0: it lies in (1 / v, 1 / v + 1) because 1 / y < psi'(y) < 1 / y + 1 / y^2"""
    mp = _mp()
    return mp.findroot(lambda y: mp.psi(1, y) - v, (1 / v, 1 / v + 1), solver="anderson", tol=mp.mpf(10) ** -(DPS - 5),
                       maxsteps=200)


def mp_finish(fits, des):
    """eBayes of the header on mp_fit's rows: dict of df_prior, s2_prior (floats may be inf / nan), nok, branch ("finite",
    "inf", "none"), and per row (None for a row that is not ok) logFC, t, p lists of q and s2 -- all mp numbers; also se =
    u_j sqrt(s2.post) and mag = sum_k |v_jk E_k|, the size of the terms that logFC is the sum of"""
    mp = _mp()
    with mp.workdps(DPS + 20):
        d = mp.mpf(des["nf"] - des["p"])
        s2 = [None if f is None else f[2] / d for f in fits]
        ok = [s for s in s2 if s is not None]
        nok = len(ok)
        if nok < 2:
            d0, s0, branch = mp.mpf(0), mp.nan, "none"
        else:
            srt = sorted(ok)
            med = srt[nok // 2] if nok % 2 else (srt[nok // 2 - 1] + srt[nok // 2]) / 2
            if med == 0:
                med = mp.mpf(1)
            x = [max(s, mp.mpf("1e-5") * med) for s in ok]
            e = [mp.log(t) - mp.psi(0, d / 2) + mp.log(d / 2) for t in x]
            ebar = mp.fsum(e) / nok
            var = mp.fsum((t - ebar) ** 2 for t in e) / (nok - 1) - mp.psi(1, d / 2)
            if var > 0:
                y = mp_trigamma_inverse(var)
                d0, s0, branch = 2 * y, mp.exp(ebar + mp.psi(0, y) - mp.log(y)), "finite"
            else:
                d0, s0, branch = mp.inf, mp.fsum(x) / nok, "inf"
        dft = nok * d if d0 == mp.inf else min(d + d0, nok * d)
        rows = []
        for f, s in zip(fits, s2):
            if f is None:
                rows.append(None)
                continue
            post = s0 if d0 == mp.inf else s if d0 == 0 else (d * s + d0 * s0) / (d + d0)
            fc = [mp.fsum(a * b for a, b in zip(vj, f[0])) for vj in des["v"]]
            t = [c / (uj * mp.sqrt(post)) if post > 0 else (mp.nan if c == 0 else mp.sign(c) * mp.inf)
                 for c, uj in zip(fc, des["u"])]
            rows.append({"logFC": fc, "t": t, "p": [xs.two_pt(tt, dft) for tt in t], "s2": s, "M": f[1],
                         "se": [uj * mp.sqrt(post) for uj in des["u"]],
                         "mag": [mp.fsum(abs(a * b) for a, b in zip(vj, f[0])) for vj in des["v"]]})
    return {"df_prior": d0, "s2_prior": s0, "nok": nok, "branch": branch, "df_total": dft, "rows": rows}


def limma_mp(X, D, use=None, K=None):
    des = mp_design(D, use, K)
    return mp_finish(mp_fit(X, des), des)


# ---- limma_np ------------------------------------------------------------------------------------------------------------------
def bh(p):
    """p.adjust(p, "fdr"); NaN stay NaN and do not count"""
    p = np.asarray(p, dtype=np.float64)
    q = np.full(p.shape, np.nan)
    idx = np.flatnonzero(~np.isnan(p))
    if len(idx):
        o = idx[np.argsort(-p[idx], kind="stable")]
        k = len(o)
        q[o] = np.minimum(1.0, np.minimum.accumulate(p[o] * k / (k - np.arange(k))))
    return q


def limma_np(X, D, use=None, K=None):
    """one fit: dict of logFC, t, p, adjp, se = stdev.unscaled sqrt(s2.post) (rows x q), AveExpr, s2 (rows), df_prior, s2_prior,
    nok, df_residual, and w1 (q): sum_c |w_jc| of the weights with logFC_j = sum_c w_jc x_c"""
    import scipy.optimize as so
    import scipy.special as ss
    import scipy.stats as st
    X, D = np.asarray(X, dtype=np.float64), np.asarray(D, dtype=np.float64)
    n, p = D.shape
    sel = _sel(n, use)
    Ds, Xs = D[sel], X[:, sel]
    Kc = np.eye(p) if K is None else np.asarray(K, dtype=np.float64).reshape(p, -1)
    q, rows, d = Kc.shape[1], X.shape[0], len(sel) - p
    ok = np.isfinite(Xs).all(axis=1)
    beta = np.linalg.lstsq(Ds, Xs[ok].T, rcond=None)[0]
    res = Xs[ok].T - Ds @ beta
    s2 = np.full(rows, np.nan)
    s2[ok] = (res * res).sum(axis=0) / d
    fc = np.full((rows, q), np.nan)
    fc[ok] = (Kc.T @ beta).T
    ave = np.full(rows, np.nan)
    ave[ok] = Xs[ok].mean(axis=1)
    su = np.sqrt(np.diag(Kc.T @ np.linalg.inv(Ds.T @ Ds) @ Kc))
    nok = int(ok.sum())
    if nok < 2:
        d0, s0, post = 0.0, np.nan, s2
    else:
        med = np.median(s2[ok])
        x = np.maximum(s2[ok], 1e-5 * (med if med != 0 else 1.0))
        e = np.log(x) - ss.digamma(d / 2) + np.log(d / 2)
        var = e.var(ddof=1) - ss.polygamma(1, d / 2)
        if var > 0:
            y = so.brentq(lambda t: ss.polygamma(1, t) - var, 1 / var, 1 / var + 1, xtol=1e-300, rtol=1e-15)
            d0, s0 = 2 * y, np.exp(e.mean() + ss.digamma(y) - np.log(y))
            post = (d * s2 + d0 * s0) / (d + d0)
        else:
            d0, s0 = np.inf, x.mean()
            post = np.where(ok, s0, np.nan)
    dft = nok * d if np.isinf(d0) else min(d + d0, nok * d)
    with np.errstate(all="ignore"):
        t = fc / (su[None, :] * np.sqrt(post)[:, None])
        pv = 2 * st.t.sf(np.abs(t), dft)
    wts = np.abs(np.linalg.pinv(Ds).T @ Kc).sum(axis=0)      # logFC_j = w_j . x: the 1-norm of the samples' weights
    with np.errstate(all="ignore"):
        se = su[None, :] * np.sqrt(post)[:, None]
    return {"w1": wts, "se": se, "logFC": fc, "AveExpr": ave, "t": t, "p": pv, "adjp": np.column_stack([bh(pv[:, j]) for j in range(q)]), "s2": s2,
            "df_prior": d0, "s2_prior": s0, "nok": nok, "df_residual": d}


# ---- deviations as the tests measure them ---------------------------------------------------------------------------------------
def flat_rows(X, use=None):
    """the rows of X that are one value over the used samples: their true logFC is 0 for a design with an intercept, so no
    relative deviation of logFC or t is defined for them"""
    Xs = np.asarray(X)[:, _sel(np.asarray(X).shape[1], use)]
    with np.errstate(all="ignore"):
        return np.nan_to_num(Xs.max(axis=1) - Xs.min(axis=1), nan=1.0) == 0


def dev_t(got, ref, flat=None, scale=None):
    """the worst relative deviation |got - ref| / |ref| of t (or logFC) over the rows; where ref is 0, got must be 0.  The
    rows marked `flat` (flat_rows) are held apart: their reference is 0 up to its own rounding, and what the code returns is
    the rounding of terms of size scale (for logFC: sum_k |v_k E_k| or |c| sum_c |w_c|; for t: that over stdev.unscaled
    sqrt(s2.post)) that cancel, so their deviation is |got - ref| / scale, and with scale 0 (a row of zeros) got == ref"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    flat = np.zeros(ref.shape, dtype=bool) if flat is None else np.asarray(flat)
    worst = 0.0
    for r in np.flatnonzero(~np.isnan(ref)):
        if flat[r]:
            if scale[r] == 0:
                assert got[r] == ref[r], (r, got[r], ref[r])
            else:
                worst = max(worst, abs(got[r] - ref[r]) / scale[r])
        elif ref[r] == 0:
            assert got[r] == 0, (r, got[r])
        else:
            worst = max(worst, abs(got[r] - ref[r]) / abs(ref[r]))
    return float(worst)


def dev_p(got, ref):
    """|got - ref| / ref where ref >= 1e-300; below it got must lie in [0, 1e-290] (asserted here)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    tiny = ref < 1e-300
    assert ((got[tiny] >= 0) & (got[tiny] <= 1e-290)).all()
    m = ~np.isnan(ref) & ~tiny
    return float(np.max(np.abs(got[m] - ref[m]) / ref[m])) if m.any() else 0.0


def dev_rel(got, ref):
    got, ref = float(got), float(ref)
    if np.isnan(ref) or np.isinf(ref):
        assert (np.isnan(got) and np.isnan(ref)) or got == ref, (got, ref)
        return 0.0
    return abs(got - ref) / abs(ref) if ref != 0 else abs(got)


# ---- the branch cases (host: plaidhip_limma_finish against limma_mp; GPU: end to end against limma_np) --------------------------
BRANCH_CASES = ("finite", "inf", "clamp", "nan_rows", "one_ok")
EXPECTED_BRANCH = {"finite": "finite", "inf": "inf", "clamp": "finite", "nan_rows": "finite", "one_ok": "none"}


def branch_case(name, n=14, rows=96, seed=11):
    """X (rows x n), Y (n x 2: a contrast without NA, one with three NA samples) and B (n x 1, centred), made so that the fit
    [1, Y[, 0], B] on all samples takes the branch `name`:
      finite    row variances s0^2 d0 / chisq_d0 with d0 = 4: a finite df.prior
      inf       every row's residual is one vector up to sign, the fitted part differs: all s2 equal, df.prior = Inf
      clamp     `finite` with a tenth of the rows constant (s2 = 0): the 1e-5 median floor
      nan_rows  `finite` with a NaN or an Inf in a used sample of some rows
      one_ok    three rows, two of them with a NaN: df.prior = 0, the ordinary t"""
    rng = np.random.default_rng(seed + BRANCH_CASES.index(name))
    y = (np.arange(n) % 2).astype(np.float64)
    rng.shuffle(y)
    b = rng.normal(size=n)
    b -= b.mean()
    Y = np.column_stack([y, y])
    Y[[1, 6, n - 2], 1] = np.nan
    D = np.column_stack([np.ones(n), y, b])
    if name == "one_ok":
        rows = 3
    coef = rng.normal(size=(rows, 3)) * np.array([2.0, 0.7, 0.3])
    if name == "inf":
        z = rng.normal(size=n)
        z -= D @ np.linalg.lstsq(D, z, rcond=None)[0]
        X = coef @ D.T + rng.choice([-1.0, 1.0], size=(rows, 1)) * z[None, :]
    else:
        sd = np.sqrt(0.25 * 4.0 / rng.chisquare(4.0, size=rows))
        X = coef @ D.T + sd[:, None] * rng.normal(size=(rows, n))
    if name == "clamp":
        X[::10, :] = 0.0
        X[5::20, :] = 3.25
    if name == "nan_rows":
        X[3, 0] = np.nan
        X[17, 5] = np.inf
        X[40, n - 1] = -np.inf
    if name == "one_ok":
        X[0, 2] = np.nan
        X[2, 0] = np.nan
    return np.asfortranarray(X), Y, b[:, None]


def contrast_design(Y, B, j):
    """(D, use) of contrast j of plaid_limma_contrasts: [1, Y[, j], B] on the samples with a label"""
    y = Y[:, j]
    use = ~np.isnan(y)
    return np.column_stack([np.ones(len(y)), np.where(use, y, 0.0), B]), use


# ---- exact integer arithmetic for the device passes ----------------------------------------------------------------------------
def to_ints(a):
    """(object array of Python ints, s) with a == ints * 2^-s exactly; a finite"""
    a = np.asarray(a, dtype=np.float64)
    nz = a[a != 0]
    s = 0 if nz.size == 0 else max(0, 53 - int(np.frexp(nz)[1].min()))
    scaled = np.ldexp(a, s)
    assert np.isfinite(scaled).all() and (scaled == np.rint(scaled)).all()
    out = np.empty(a.shape, dtype=object)
    out.ravel()[:] = [int(v) for v in scaled.ravel().tolist()]
    return out, s


def ints_to_float(a, s):
    """the integers a * 2^-s rounded once to fp64"""
    den = 1 << s
    return np.array([float(Fraction(int(v), den)) for v in a.ravel()], dtype=np.float64).reshape(a.shape)


def exact_effects(X, Wm):
    """X (rows x n) and the weights Wm (n x W, zero for an excluded sample; X finite): (the exact X Wm rounded once, sum |x||w|)"""
    Xi, sx = to_ints(X)
    Wi, sw = to_ints(Wm)
    return ints_to_float(Xi.dot(Wi), sx + sw), np.abs(X) @ np.abs(Wm)


def exact_rss(X, Q, used, E):
    """the pinned expression at the effects E (rows x p) the device returned, in integers: r_c = x_c - sum_k Q[c, k] E_k and
    RSS = sum over the used c of r_c^2.  Returns (RSS rounded once, r rounded once (rows x used), rho = |x_c| + sum_k |Q E|)"""
    X, Q, E = X[:, used], Q[used, :], np.asarray(E)
    Xi, sx = to_ints(X)
    Qi, sq = to_ints(Q)
    Ei, se = to_ints(E)
    s = max(sx, sq + se)
    R = Xi * (1 << (s - sx)) - Ei.dot(Qi.T) * (1 << (s - sq - se))
    rss = ints_to_float((R * R).sum(axis=1), 2 * s)
    return rss, ints_to_float(R, s), np.abs(X) + np.abs(E) @ np.abs(Q.T)


def effects_bound(mag, nf):
    """(n_f + 1) 2^-53 sum |x||w|, with the higher orders of gamma_{n_f + 1} (a factor below 1 + 2^-40) and the subnormal floor:
    DESIGN.md section 20"""
    return (nf + 1) * U * mag * (1 + 2.0 ** -40) + (nf + 1) * 2.0 ** -1074


def rss_bound(r, rho, rss, nf, p):
    """g = gamma_{p + 1} on rho_c for r_c, then h = gamma_{n_f + 2} for the squaring and the sum, and u for
    the reference's rounding"""
    g = (p + 1) * U * (1 + 2.0 ** -40)
    h = (nf + 2) * U * (1 + 2.0 ** -40)
    per = (2 * np.abs(r) * g * rho + (g * rho) ** 2) * (1 + h) + h * r * r
    return (per.sum(axis=1) + U * rss) * (1 + 2.0 ** -30) + (nf + 2) * 2.0 ** -1074


# ---- the sharding hook ----------------------------------------------------------------------------------------------------------
def run_sharded(nshards, A, design, use=None, contrasts=None, fail=-1):
    """(status, out, hyper) of plaid.limma on `nshards` contexts of one device; the results hold -7 before the call"""
    A = np.asfortranarray(A, dtype=np.float64)
    D, _, _, q = engine.limma_operands(A.shape[1], design, use, contrasts)
    out = np.full((A.shape[0], 6, q, D.shape[2]), -7.0, order="F")
    hyper = np.full((D.shape[2], 4), -7.0)
    status, _ = _status(lambda: engine._limma(hook("limma"), (0, nshards, fail), A, design, use, contrasts, out=out, hyper=hyper))
    return status, out, hyper
