"""plaid.camera for the tests: limma's camera.default restated literally at 50 digits, a plain fp64 restatement of the pinned
form, exact rational arithmetic for the sums of squares, the cases the host and the GPU tests share, and the sharding hook.

camera_mp   camera as limma writes it: a COMPLETE QR of the design's used rows (mpmath.qr, Householder), the effects Q'x of
            every gene, U = the effects past the first p (Q2'x), sigma2 = colMeans(U^2), U / sqrt(pmax(sigma2, 1e-8)),
            vif = m * mean(colMeans(U[set, ])^2), the two-sample t of the moderated t (tests/helpers/limma_ref.mp_finish) and
            the t tail (exact_stats.two_pt).  It knows nothing of the sample-space identity the library uses.
camera_np   the header's pinned form (include/plaidhip.h: plaidhip_camera) in plain numpy fp64, in the pinned order of
            every sum -- ordinary rounded products where the library writes an fma.  What it deviates from camera_mp by is
            rounding in a fixed order: that deviation, measured on the host, is what the end-to-end GPU test allows 8 times.
"""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

from plaid_amd import engine
from tests.helpers import exact_stats as xs
from tests.helpers import limma_ref as lr
from tests.helpers.sharded_hooks import _status, hook

DPS = lr.DPS
U = 2.0 ** -53
COLS = engine.CAMERA_COLUMNS


def _mp():
    import mpmath
    return mpmath


def pattern(sets):
    """(Gp, Gi) of a list of index lists"""
    Gp = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    Gi = np.concatenate([np.asarray(s, dtype=np.int32) for s in sets] + [np.zeros(0, np.int32)]).astype(np.int32)
    return Gp, Gi


# ---- camera_mp -----------------------------------------------------------------------------------------------------------------
def mp_vif(X, D, use, sets):
    """per set (m over the ok genes, vif, correlation) as limma computes them, mp numbers (None where undefined), and the ok
    genes: effects = Q'x with the complete Q of the used rows of D, U = effects[p:], sigma2 = mean(U^2)"""
    mp = _mp()
    X, D = np.asarray(X, dtype=np.float64), np.asarray(D, dtype=np.float64)
    sel = lr._sel(D.shape[0], use)
    nf, p = len(sel), D.shape[1]
    d = nf - p
    with mp.workdps(DPS + 20):
        Q, _ = mp.qr(mp.matrix(D[sel].tolist()))           # nf x nf, nf x p
        Q2 = [[Q[c, p + k] for c in range(nf)] for k in range(d)]
        ok, Ug = [], {}
        for g in range(X.shape[0]):
            x = X[g, sel]
            if not np.isfinite(x).all():
                ok.append(False)
                continue
            xm = [mp.mpf(float(v)) for v in x]
            u = [mp.fsum(a * b for a, b in zip(q, xm)) for q in Q2]
            sigma2 = mp.fsum(v * v for v in u) / d
            s = mp.sqrt(max(sigma2, mp.mpf("1e-8")))
            Ug[g] = [v / s for v in u]
            ok.append(True)
        out = []
        for members in sets:
            mem = [g for g in members if ok[g]]
            m = len(mem)
            if m == 0:
                out.append((0, None, None))
            elif m == 1:
                out.append((1, mp.mpf(1), None))
            else:
                colmeans = [mp.fsum(Ug[g][k] for g in mem) / m for k in range(d)]
                vif = m * mp.fsum(v * v for v in colmeans) / d
                out.append((m, vif, (vif - 1) / (m - 1)))
    return out, np.array(ok)


def mp_test(t, vifs, dfc, rho=None, allow_neg=False, sets=None, ok=None):
    """step 5 at 50 digits for one (fit, contrast): t a list over the genes (None: not ok); returns per set a dict of the
    eight columns (mp numbers, None for NaN)"""
    mp = _mp()
    with mp.workdps(DPS + 20):
        tt = [v for v in t if v is not None]
        G = len(tt)
        rows = []
        if G >= 2:
            mean = mp.fsum(tt) / G
            var = mp.fsum((v - mean) ** 2 for v in tt) / (G - 1)
        for (m, vif, cor), members in zip(vifs, sets):
            if rho is not None:
                vif, cor = (1 + (m - 1) * mp.mpf(float(rho)), mp.mpf(float(rho))) if m >= 1 else (None, None)
            row = {"NGenes": m, "Correlation": cor, "VIF": vif, "t": None, "Down": None, "Up": None, "PValue": None}
            m2 = G - m
            if m >= 1 and m2 >= 1 and G >= 3:
                used = vif if (rho is not None or allow_neg) else max(vif, mp.mpf(1))
                meanset = mp.fsum(t[g] for g in members if ok[g]) / m
                delta = mp.mpf(G) / m2 * (meanset - mean)
                pooled = ((G - 1) * var - delta ** 2 * m * m2 / G) / (G - 2)
                s2 = pooled * (used / m + mp.mpf(1) / m2)
                if pooled > 0 and s2 > 0:
                    T = delta / mp.sqrt(s2)
                    half = xs.two_pt(T, dfc) / 2
                    row["t"] = T
                    row["Down"], row["Up"] = (half, 1 - half) if T < 0 else (1 - half, half)
                    row["PValue"] = 2 * min(row["Down"], row["Up"])
            rows.append(row)
    return rows


def camera_mp(X, D, use, K, sets, rho=None, allow_neg=False, heavy=None):
    """one fit: {"tables": per contrast the list of set rows, "G", "dfc", "ok"}.  heavy: (limma_mp, mp_vif) of the same
    operands where the caller has them (they do not depend on rho and allow_neg)"""
    mp = _mp()
    fit, (vifs, ok) = heavy if heavy is not None else (lr.limma_mp(X, D, use, K), mp_vif(X, D, use, sets))
    assert [r is not None for r in fit["rows"]] == list(ok)
    G = int(ok.sum())
    nf, p = len(lr._sel(np.asarray(D).shape[0], use)), np.asarray(D).shape[1]
    with mp.workdps(DPS + 20):
        d0 = fit["df_prior"]
        dfc = mp.mpf(G - 2) if d0 == mp.inf else min(mp.mpf(nf - p) + d0, mp.mpf(G - 2))
    q = np.eye(p).shape[1] if K is None else np.asarray(K).reshape(p, -1).shape[1]
    tables = []
    for j in range(q):
        t = [None if r is None else r["t"][j] for r in fit["rows"]]
        tables.append(mp_test(t, vifs, dfc, rho, allow_neg, sets, ok))
    return {"tables": tables, "G": G, "dfc": dfc, "ok": ok}


def table_float(rows):
    """sets x 7 doubles of mp_test's rows (no FDR), NaN for None"""
    return np.array([[np.nan if r[c] is None else float(r[c]) for c in COLS[:7]] for r in rows], dtype=np.float64)


# ---- camera_np: the pinned form in plain fp64 ----------------------------------------------------------------------------------
def np_design(D, use):
    """the header's Householder QR of the used rows, in numpy: (Q n x p with zero rows for the unused samples, R)"""
    D = np.asarray(D, dtype=np.float64)
    n, p = D.shape
    sel = lr._sel(n, use)
    a = D[sel].copy()
    nf = len(sel)
    vs = []
    R = np.zeros((p, p))
    for k in range(p):
        x = a[k:, k].copy()
        alpha = -np.sqrt(np.dot(x, x)) if x[0] >= 0 else np.sqrt(np.dot(x, x))
        v = x.copy()
        v[0] -= alpha
        vs.append(v)
        a[k:, k:] -= np.outer(v, 2.0 * (v @ a[k:, k:]) / np.dot(v, v))
        R[k, k:] = a[k, k:]
        R[k, k] = alpha
    q = np.eye(nf, p)
    for k in range(p - 1, -1, -1):
        v = vs[k]
        q[k:, :] -= np.outer(v, 2.0 * (v @ q[k:, :]) / np.dot(v, v))
    Q = np.zeros((n, p))
    Q[sel] = q
    return Q, R


def _block_sum(terms):
    """the pinned order: the columns of a block of 128 in ascending order from 0.0, then the blocks in ascending order;
    terms: rows x n"""
    tot = np.zeros(terms.shape[0])
    for c0 in range(0, terms.shape[1], 128):
        acc = np.zeros(terms.shape[0])
        for c in range(c0, min(c0 + 128, terms.shape[1])):
            acc = acc + terms[:, c]
        tot = tot + acc
    return tot


def camera_np(X, D, use, K, sets, rho=None, allow_neg=False):
    """one fit of the pinned form: out sets x 8 x q and (G, df.camera).  eBayes and the tail are scipy's (limma_ref.limma_np
    supplies df.prior and s2.prior); the fit, Z, T, the sums of squares and step 5 are written out here"""
    import scipy.stats as st
    X, D = np.asarray(X, dtype=np.float64), np.asarray(D, dtype=np.float64)
    g, n = X.shape
    p = D.shape[1]
    used = np.zeros(n, dtype=bool)
    used[lr._sel(n, use)] = True
    nf = int(used.sum())
    d = float(nf - p)
    Q, R = np_design(D, use)
    Kc = np.eye(p) if K is None else np.asarray(K, dtype=np.float64).reshape(p, -1)
    Xu = np.where(used[None, :], X, 0.0)
    E = np.column_stack([_block_sum(Xu * Q[None, :, k]) for k in range(p)])
    with np.errstate(all="ignore"):                            # (a NaN or an Inf in a used sample: the gene is not ok)
        res = Xu.copy()
        for k in range(p):
            res = res - Q[None, :, k] * E[:, k:k + 1]
        res = np.where(used[None, :], res, 0.0)
        s2 = _block_sum(res * res) / d
    res, E = np.nan_to_num(res, nan=0.0, posinf=0.0, neginf=0.0), np.where(np.isfinite(s2)[:, None], E, 0.0)
    ok = np.isfinite(s2)
    eb = lr.limma_np(X, D, use, K)
    d0, s0 = eb["df_prior"], eb["s2_prior"]
    post = np.where(ok, s0 if np.isinf(d0) else (d * s2 + d0 * s0) / (d + d0) if d0 > 0 else s2, np.nan)
    G = int(ok.sum())
    dfc = min(d + d0, G - 2.0)
    Z = np.where(ok[:, None] & used[None, :], res / np.sqrt(np.maximum(s2, 1e-8))[:, None], 0.0)
    q = Kc.shape[1]
    out = np.full((len(sets), 8, q), np.nan)
    for j in range(q):
        v = np.linalg.solve(R.T, Kc[:, j])
        t = (E @ v) / (np.sqrt(np.dot(v, v)) * np.sqrt(post))
        tk = t[ok]
        mean = np.add.reduce(tk) / G if G else np.nan
        var = np.add.reduce((tk - mean) ** 2) / (G - 1.0) if G > 1 else np.nan
        for s, members in enumerate(sets):
            mem = [i for i in members if ok[i]]
            m = float(len(mem))
            vif = cor = np.nan
            if rho is not None:
                if m >= 1:
                    vif, cor = 1.0 + (m - 1.0) * rho, rho
            elif m > 1:
                T = np.zeros(n)
                for i in mem:
                    T = T + Z[i]
                vif = _block_sum((T * T)[None, :])[0] / (m * d)
                cor = (vif - 1.0) / (m - 1.0)
            elif m == 1:
                vif = 1.0
            out[s, 0:3, j] = m, cor, vif
            m2 = G - m
            if m >= 1 and m2 >= 1 and G >= 3:
                usedv = vif if (rho is not None or allow_neg) else max(vif, 1.0)
                delta = (G / m2) * (np.add.reduce(t[mem]) / m - mean)
                pooled = ((G - 1.0) * var - ((delta * delta) * m * m2) / G) / (G - 2.0)
                sc = pooled * (usedv / m + 1.0 / m2)
                if pooled > 0 and sc > 0:
                    Ts = delta / np.sqrt(sc)
                    half = float(st.t.sf(abs(Ts), dfc))
                    down, up = (half, 1.0 - half) if Ts < 0 else (1.0 - half, half)
                    out[s, 3:7, j] = Ts, down, up, 2.0 * min(down, up)
        out[:, 7, j] = lr.bh(out[:, 6, j])
    return out, (G, dfc)


def deviation(got, ref):
    """the worst relative deviation of VIF, t and PValue (sets x 8 against table_float's sets x 7), the NaN patterns and NGenes
    equal; Correlation is (VIF - 1) / (m - 1), a difference that cancels near VIF = 1: it is measured relative to
    max(|cor|, 1 / (m - 1)), the size of the terms"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert np.array_equal(got[:, 0], ref[:, 0]), (got[:, 0], ref[:, 0])
    worst = {}
    for name, c in (("VIF", 2), ("t", 3), ("Down", 4), ("Up", 5), ("PValue", 6)):
        assert np.array_equal(np.isnan(got[:, c]), np.isnan(ref[:, c])), (name, got[:, c], ref[:, c])
        k = ~np.isnan(ref[:, c])
        worst[name] = float(np.max(np.abs(got[k, c] - ref[k, c]) / np.abs(ref[k, c]))) if k.any() else 0.0
    assert np.array_equal(np.isnan(got[:, 1]), np.isnan(ref[:, 1]))
    k = ~np.isnan(ref[:, 1])
    scale = np.maximum(np.abs(ref[k, 1]), 1.0 / np.maximum(ref[k, 0] - 1.0, 1.0))
    worst["Correlation"] = float(np.max(np.abs(got[k, 1] - ref[k, 1]) / scale)) if k.any() else 0.0
    return worst


# ---- exact rational arithmetic for the sums of squares ---------------------------------------------------------------------------
def exact_T(Z, sets):
    """T = G'Z in exact rationals from the device's own Z (genes x n doubles): a list over the sets of lists of Fractions"""
    Zi, s = lr.to_ints(Z)
    den = 1 << s
    return [[Fraction(int(sum(Zi[g, c] for g in members)), den) for c in range(Z.shape[1])] for members in sets]


def sumsq_bound(Tex, delta):
    """the forward bound of the device's sum of T^2 for one set: the crossprod returns T_c + e_c with
    |e_c| <= delta_c, squaring moves a term by at most 2 |T_c| delta_c + delta_c^2, and the n squares and n additions carry
    gamma_{n + 1}:
        sum_c (2 |T_c| delta_c + delta_c^2) + gamma_{n + 1} sum_c T_c^2.
    Returns (the exact sum as a Fraction, the bound as a float); the caller compares in exact rationals"""
    n = len(Tex)
    exact = sum((t * t for t in Tex), Fraction(0))
    gam = (n + 1) * U / (1 - (n + 1) * U)
    a = np.array([abs(float(t)) for t in Tex])
    dl = np.asarray(delta, dtype=np.float64)
    return exact, float(np.sum(2 * a * dl + dl * dl) + gam * float(exact))


# ---- shared cases ----------------------------------------------------------------------------------------------------------------
def int_matrix(g, n, rng):
    """integer-valued X in -8 .. 8"""
    return np.asfortranarray(rng.integers(-8, 9, size=(g, n)).astype(np.float64))


def make_design(n, p, rng):
    """[1, group, covariates ...] (n x p; p = 1: the intercept alone)"""
    D = np.empty((n, p), order="F")
    D[:, 0] = 1.0
    if p > 1:
        D[:, 1] = rng.permutation(np.arange(n) % 2)
    if p > 2:
        D[:, 2:] = rng.normal(size=(n, p - 2))
    return D


def make_sets(g, sizes, rng):
    """sets of the given sizes drawn without replacement (a size above g is cut to g; size g is every gene in order)"""
    return [sorted(rng.choice(g, size=min(k, g), replace=False).tolist()) for k in sizes]


# ---- the sharding hook ----------------------------------------------------------------------------------------------------------
def run_sharded(nshards, X, design, Gp, Gi, use=None, contrasts=None, rho=None, allow_neg=False, fail=-1):
    """(status, out, hyper) of plaid.camera on `nshards` contexts of one device; the results hold -7 before the call"""
    X = np.asfortranarray(X, dtype=np.float64)
    Dd, _, _, q = engine.limma_operands(X.shape[1], design, use, contrasts)
    out = np.full((len(Gp) - 1, 8, q, Dd.shape[2]), -7.0, order="F")
    hyper = np.full((Dd.shape[2], 6), -7.0)
    status, _ = _status(lambda: engine._camera(hook("camera"), (0, nshards, fail), X, design, Gp, Gi, use, contrasts, rho,
                                               allow_neg, out=out, hyper=hyper))
    return status, out, hyper


# ---- the end-to-end cases (n_f >= p + 4, every s2 above 1e-3: integer X in -8 .. 8) ------------------------------------------------
E2E_CASES = ("small", "block", "intercept")
E2E_MODES = ((None, False), (None, True), (0.01, False))      # (inter_gene_cor, allow_neg_cor)


def e2e_case(name):
    """X, D (n x p x nfit), use (n x nfit or None), K (p x q or None) and the sets (sizes 0, 1, 2, 5, g / 2 and g):
      small      40 genes x 20 samples, [1, group], two fits -- the second leaves five samples out, one of them holding a NaN
                 and one an Inf, so those two genes leave the universe of the fit that uses every sample -- one contrast
      block      24 genes x 130 samples (a full block of 128 columns and a tail), [1, group, two covariates], two contrasts
      intercept  30 genes x 12 samples, the intercept alone (K = NULL)"""
    rng = np.random.default_rng(40 + E2E_CASES.index(name))
    g, n, p, nfit = {"small": (40, 20, 2, 2), "block": (24, 130, 4, 1), "intercept": (30, 12, 1, 1)}[name]
    X = int_matrix(g, n, rng)
    D = np.stack([make_design(n, p, rng) for _ in range(nfit)], axis=2)
    use, K = None, None
    if name == "small":
        use = np.ones((n, nfit), dtype=np.int8, order="F")
        out = rng.choice(n, size=5, replace=False)
        use[out, 1] = 0
        X[3, out[0]] = np.nan
        X[11, out[1]] = np.inf
        K = np.array([[0.0], [1.0]])
    if name == "block":
        K = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [0.0, 0.0]])
    sets = make_sets(g, (0, 1, 2, 5, g // 2, g), rng)
    return X, np.asfortranarray(D), use, K, sets


@functools.lru_cache(maxsize=None)
def _e2e_heavy(name):
    """per fit (limma_mp, mp_vif): the 50-digit parts that the modes share"""
    X, D, use, K, sets = e2e_case(name)
    return [(lr.limma_mp(X, D[:, :, f], None if use is None else use[:, f], K),
             mp_vif(X, D[:, :, f], None if use is None else use[:, f], sets)) for f in range(D.shape[2])]


def e2e_reference(name, mode, which="mp"):
    """per fit, per contrast: sets x 7 doubles of camera_mp (or sets x 8 of camera_np) for one case and mode"""
    X, D, use, K, sets = e2e_case(name)
    rho, allow_neg = mode
    tabs = []
    for f in range(D.shape[2]):
        uf = None if use is None else use[:, f]
        if which == "mp":
            ref = camera_mp(X, D[:, :, f], uf, K, sets, rho, allow_neg, heavy=_e2e_heavy(name)[f])
            tabs.append([table_float(t) for t in ref["tables"]])
        else:
            out, _ = camera_np(X, D[:, :, f], uf, K, sets, rho, allow_neg)
            tabs.append([out[:, :, j] for j in range(out.shape[2])])
    return tabs
