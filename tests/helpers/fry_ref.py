"""plaid.fry for the tests: the header's words (include/plaidhip.h: plaidhip_fry) at 50 digits, a plain numpy fp64
restatement, the Gram kernel's summation order in numpy, the shared cases and the sharding hook.

fry_mp    the statistic from X and the design with its OWN decomposition: a complete Householder QR of the design's used rows
          (mpmath.qr), the effects Q'x of every gene, rho = the effects past the first p over c_g, the fit and eBayes of
          tests/helpers/limma_ref (Gram-Schmidt, another route again), svd(F_S)$d^2 as the eigenvalues of the smaller of
          F_S'F_S and F_S F_S' (mpmath.eigsy), the t tail of exact_stats and mpmath.betainc.  It knows nothing of the
          sample-space identity, of Q2 as reflectors, or of M's border form.
fry_np    the same in numpy fp64: lstsq, numpy.linalg.qr(mode="complete"), eigvalsh of the full M, scipy's tails.  What it
          deviates from fry_mp by is rounding: that deviation, measured on the host, is what the GPU test allows 4 times.
gram_np   C, b, a, tr M and |M|_F^2 in exactly the order of fry_gram_kernel.

Measured on the host (tests/test_multi_fry_host.py re-measures): see MEASURED, EIG_DEV and BETA_ACC below."""
from __future__ import annotations

import functools

import numpy as np

from plaid_amd import engine
from tests.helpers import camera_ref as cr
from tests.helpers import exact_stats as xs
from tests.helpers import limma_ref as lr
from tests.helpers.sharded_hooks import _status, hook

DPS = lr.DPS
U = 2.0 ** -53
COLS = engine.FRY_COLUMNS
STD = ("posterior.sd", "residual.sd", "none")

# fry_np against fry_mp over E2E_CASES x STD, the worst relative deviation (host, this file's __main__ prints them)
MEASURED = {"t": 1.22e-13, "PValue": 9.27e-15, "PValue.Mixed": 1.47e-14}
FACTOR = 4
# numpy.linalg.eigvalsh against the 50-digit spectrum over eigen_cases(), worst |lambda - exact| / lambda_1 of lambda_1 and
# lambda_D; the device is allowed max(4 x this, D 2^-53)
EIG_DEV = 1.28e-15
# plaidhip_debug_beta_upper against mpmath.betainc over the e2e triples and beta_grid(), worst relative error for tails
# >= 1e-280; asserted: 4 x
BETA_ACC = 1.84e-11


def _mp():
    import mpmath
    return mpmath


# ---- fry_mp ----------------------------------------------------------------------------------------------------------------------
def mp_mixed(a, lams, D):
    """the header's step 4 from a_j = sum e^2 and the D eigenvalues (decreasing), mp numbers: dict of Fobs, alpha, beta, Fv, p"""
    mp = _mp()
    l1, lD = lams[0], lams[D - 1]
    SA, SA2 = mp.fsum(lams), mp.fsum(v * v for v in lams)
    den = l1 - lD
    if den == 0:
        return {"p": None, "den": den, "l1": l1, "lD": lD, "SA": SA, "SA2": SA2}
    Fobs = (a - lD) / den
    bm = mp.mpf(1) / D
    bv = mp.mpf(D - 1) / (D * D) / (mp.mpf(D) / 2 + 1)
    Fm = (SA * bm - lD) / den
    Fv = (bv * SA2 - bv / (D - 1) * (SA * SA - SA2)) / (den * den)
    out = {"Fobs": Fobs, "Fv": Fv, "den": den, "l1": l1, "lD": lD, "SA": SA, "SA2": SA2, "alpha": None, "beta": None, "p": None}
    if Fv != 0:
        ab = Fm * (1 - Fm) / Fv - 1
        alpha = ab * Fm
        beta = ab - alpha
        out.update(alpha=alpha, beta=beta)
        if alpha > 0 and beta > 0:
            x = min(max(Fobs, mp.mpf(0)), mp.mpf(1))
            out["p"] = mp_beta_upper(x, alpha, beta)
    return out


def mp_beta_upper(x, a, b):
    """pbeta(x, a, b, lower.tail = FALSE) at the working precision: I_{1 - x}(b, a) from 0 (mpmath.betainc over [x, 1] forms
    1 - I_x and loses the digits of a small tail)"""
    mp = _mp()
    return mp.betainc(b, a, 0, 1 - x, regularized=True)


def fry_mp(X, D, use, K, sets, standardize="posterior.sd"):
    """one fit: {"tables": per contrast a list of per-set dicts (m, t, p, mixed: mp_mixed's dict or None), "d", "inuni",
    "z": gene -> the sample-space z (used samples), "rho": gene -> rho, "e": gene -> e_j list}"""
    mp = _mp()
    X, D = np.asarray(X, dtype=np.float64), np.asarray(D, dtype=np.float64)
    des = lr.mp_design(D, use, K)
    fits = lr.mp_fit(X, des)
    fin = lr.mp_finish(fits, des)
    sel, p, nf = des["sel"], des["p"], des["nf"]
    d = nf - p
    q = len(des["v"])
    with mp.workdps(DPS + 20):
        Qc, _ = mp.qr(mp.matrix(D[sel].tolist()))
        Q2 = [[Qc[c, p + k] for c in range(nf)] for k in range(d)]
        d0, s0 = fin["df_prior"], fin["s2_prior"]
        inuni, zs, rhos, es = [], {}, {}, {}
        for g in range(X.shape[0]):
            row = fin["rows"][g]
            if row is None:
                inuni.append(False)
                continue
            s = row["s2"]
            if standardize == "posterior.sd":
                post = s0 if d0 == mp.inf else s if d0 == 0 else (mp.mpf(d) * s + d0 * s0) / (d + d0)
                c = mp.sqrt(post)
            elif standardize == "residual.sd":
                c = mp.sqrt(s)
            else:
                c = mp.mpf(1)
            if c == 0 or not mp.isfinite(c):
                inuni.append(False)
                continue
            inuni.append(True)
            xm = [mp.mpf(float(v)) for v in X[g, sel]]
            E = fits[g][0]
            zs[g] = [(xm[i] - mp.fsum(qk[i] * e for qk, e in zip(des["Q"], E))) / c for i in range(nf)]
            rhos[g] = [mp.fsum(a * b for a, b in zip(qk, xm)) / c for qk in Q2]
            es[g] = [fc / (uj * c) for fc, uj in zip(row["logFC"], des["u"])]
        tables = []
        for j in range(q):
            rows = []
            for members in sets:
                mem = [g for g in members if inuni[g]]
                m = len(mem)
                r = {"m": m, "t": None, "p": None, "mixed": None}
                if m >= 1:
                    mean = mp.fsum(es[g][j] for g in mem) / m
                    tot = [mp.fsum(rhos[g][k] for g in mem) for k in range(d)]
                    ss = mp.fsum(v * v for v in tot)
                    den = mp.sqrt(ss / (mp.mpf(m) * m * d))
                    if den != 0:
                        r["t"] = mean / den
                        r["p"] = xs.two_pt(r["t"], d)
                    elif mean != 0:
                        r["t"] = mp.sign(mean) * mp.inf
                        r["p"] = mp.mpf(0)
                    if m == 1:
                        r["mixed"] = {"p": r["p"], "single": True}
                    else:
                        F = [[es[g][j]] + rhos[g] for g in mem]                 # m x (d + 1)
                        Dn = min(m, d + 1)
                        if m <= d + 1:
                            Gm = mp.matrix([[mp.fsum(a * b for a, b in zip(F[x], F[y])) for y in range(m)] for x in range(m)])
                        else:
                            Gm = mp.matrix([[mp.fsum(F[g_][x] * F[g_][y] for g_ in range(m)) for y in range(d + 1)]
                                            for x in range(d + 1)])
                        lam = sorted((v for v in mp.eigsy(Gm, eigvals_only=True)), reverse=True)
                        a = mp.fsum(es[g][j] ** 2 for g in mem)
                        r["mixed"] = mp_mixed(a, [lam[i] for i in range(Dn)], Dn)
                        r["mixed"]["a"] = a
                rows.append(r)
            tables.append(rows)
    return {"tables": tables, "d": d, "inuni": np.array(inuni), "z": zs, "rho": rhos, "e": es, "Q2": Q2, "fin": fin}


def table_float(rows):
    """sets x 4 doubles (NGenes, t, PValue, PValue.Mixed) of fry_mp's rows, NaN for None"""
    f = lambda v: np.nan if v is None else float(v)
    return np.array([[r["m"], f(r["t"]), f(r["p"]), f(None if r["mixed"] is None else r["mixed"]["p"])] for r in rows])


def conditioned(r):
    """the issue's rule for a mixed case: lambda_1 - lambda_D >= 1e-3 lambda_1, Fv > 0, 0.5 <= alpha, beta <= 1e4"""
    mx = r["mixed"]
    if mx is None or mx.get("single"):
        return True
    if mx.get("alpha") is None or mx.get("p") is None:
        return False
    return bool(mx["den"] >= mx["l1"] / 1000 and mx["Fv"] > 0 and 0.5 <= mx["alpha"] <= 1e4 and 0.5 <= mx["beta"] <= 1e4)


# ---- fry_np ----------------------------------------------------------------------------------------------------------------------
def fry_np(X, D, use, K, sets, standardize="posterior.sd"):
    """one fit in numpy fp64: sets x 4 x q (NGenes, t, PValue, PValue.Mixed)"""
    import scipy.stats as st
    X, D = np.asarray(X, dtype=np.float64), np.asarray(D, dtype=np.float64)
    n, p = D.shape
    sel = lr._sel(n, use)
    nf = len(sel)
    d = nf - p
    eb = lr.limma_np(X, D, use, K)
    d0, s0, s2 = eb["df_prior"], eb["s2_prior"], eb["s2"]
    ok = np.isfinite(s2)
    with np.errstate(all="ignore"):
        post = np.where(ok, s0 if np.isinf(d0) else (d * s2 + d0 * s0) / (d + d0) if d0 > 0 else s2, np.nan)
        c = {"posterior.sd": np.sqrt(post), "residual.sd": np.sqrt(s2), "none": np.where(ok, 1.0, np.nan)}[standardize]
    inuni = np.isfinite(c) & (c != 0)
    Qc, _ = np.linalg.qr(D[sel], mode="complete")
    Xs = np.where(inuni[:, None], X[:, sel], 0.0)
    cc = np.where(inuni, c, 1.0)
    rho = (Xs @ Qc[:, p:]) / cc[:, None]
    Kc = np.eye(p) if K is None else np.asarray(K, dtype=np.float64).reshape(p, -1)
    su = np.sqrt(np.diag(Kc.T @ np.linalg.inv(D[sel].T @ D[sel]) @ Kc))
    q = Kc.shape[1]
    out = np.full((len(sets), 4, q), np.nan)
    for j in range(q):
        e = np.where(inuni, eb["logFC"][:, j] / (su[j] * cc), 0.0)
        for s, members in enumerate(sets):
            mem = [g for g in members if inuni[g]]
            m = len(mem)
            out[s, 0, j] = m
            if m == 0:
                continue
            with np.errstate(all="ignore"):
                tot = rho[mem].sum(axis=0)
                t = e[mem].mean() / np.sqrt(np.dot(tot, tot) / (m * m * d))
            out[s, 1, j] = t
            out[s, 2, j] = 2 * st.t.sf(abs(t), d) if not np.isnan(t) else np.nan
            if m == 1:
                out[s, 3, j] = out[s, 2, j]
                continue
            F = np.column_stack([e[mem], rho[mem]])
            lam = np.sort(np.linalg.eigvalsh(F.T @ F))[::-1]
            Dn = min(m, d + 1)
            l1, lD = lam[0], lam[Dn - 1]
            SA, SA2 = np.trace(F.T @ F), np.sum((F.T @ F) ** 2)
            with np.errstate(all="ignore"):
                den = l1 - lD
                Fobs = (np.dot(e[mem], e[mem]) - lD) / den
                bm, bv = 1.0 / Dn, (Dn - 1.0) / (Dn * Dn) / (Dn / 2.0 + 1.0)
                Fm = (SA * bm - lD) / den
                Fv = (bv * SA2 - bv / (Dn - 1.0) * (SA * SA - SA2)) / (den * den)
                ab = Fm * (1 - Fm) / Fv - 1
                alpha, beta = ab * Fm, ab - ab * Fm
            if np.isfinite(alpha) and np.isfinite(beta) and alpha > 0 and beta > 0 and not np.isnan(Fobs):
                out[s, 3, j] = st.beta.sf(min(max(Fobs, 0.0), 1.0), alpha, beta)
    return out


def deviation(got, ref, keep=None):
    """worst relative deviation of t, PValue, PValue.Mixed (sets x 4 each; `keep`: the sets whose mixed value is compared);
    NGenes and the NaN patterns equal"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert np.array_equal(got[:, 0], ref[:, 0]), (got[:, 0], ref[:, 0])
    worst = {}
    for name, c in (("t", 1), ("PValue", 2), ("PValue.Mixed", 3)):
        k = ~np.isnan(ref[:, c])
        if c == 3 and keep is not None:
            k &= np.asarray(keep)
        else:
            assert np.array_equal(np.isnan(got[:, c]), np.isnan(ref[:, c])), (name, got[:, c], ref[:, c])
        assert not np.isnan(got[k, c]).any(), (name, got[:, c])
        with np.errstate(all="ignore"):
            r = np.abs(got[k, c] - ref[k, c]) / np.abs(ref[k, c])
        r = np.where(got[k, c] == ref[k, c], 0.0, r)
        worst[name] = float(r.max()) if k.any() else 0.0
    return worst


# ---- the Gram kernel's order -------------------------------------------------------------------------------------------------------
def gram_np(rho, e, sets):
    """rho rows x d, e rows x q (0.0 outside the universe): per set C (d x d), b (q x d), a (q), tr (q), fro (q) -- every
    entry one accumulator from 0.0 over the members in the set's order, the product rounded, then added; then
    rs_i = sum_k C_ik^2, sc = sum_i rs_i, dg = sum_i C_ii, sb_j = sum_i b_ji^2, tr_j = a_j + dg, fro_j = (a_j a_j + 2 sb_j) + sc,
    every sum ascending from 0.0"""
    rho, e = np.asarray(rho, dtype=np.float64), np.asarray(e, dtype=np.float64)
    d, q = rho.shape[1], e.shape[1]
    out = []
    for members in sets:
        C, b, a = np.zeros((d, d)), np.zeros((q, d)), np.zeros(q)
        for g in members:
            C = C + np.outer(rho[g], rho[g])
            b = b + np.outer(e[g], rho[g])
            a = a + e[g] * e[g]
        rs = np.zeros(d)
        for k in range(d):
            rs = rs + C[:, k] * C[:, k]
        sc = dg = 0.0
        sb = np.zeros(q)
        for i in range(d):
            sc = sc + rs[i]
            dg = dg + C[i, i]
            sb = sb + b[:, i] * b[:, i]
        out.append({"C": C, "b": b, "a": a, "tr": a + dg, "fro": (a * a + 2.0 * sb) + sc})
    return out


# ---- the eigen cases ----------------------------------------------------------------------------------------------------------------
EIG128_SEED = 20261020


def eig128_matrix():
    """the seeded D = 128 matrix whose 50-digit lambda_1 and lambda_128 are committed (tests/golden/fry_eig128.npz)"""
    rng = np.random.default_rng(EIG128_SEED)
    F = rng.integers(-8, 9, size=(160, 128)).astype(np.float64) / 8.0
    return F.T @ F          # (exact in fp64: integers / 64 below 2^53)


def eigen_cases():
    """name -> (M, D): D = 2, 3 (an odd pairing), 8, 33; rank-deficient (m = 5 < dim = 12); a repeated top eigenvalue; a
    diagonal matrix.  Integer-valued F / 8, so M = F'F is exact in fp64."""
    rng = np.random.default_rng(5)
    out = {}
    for dim in (2, 3, 8, 33):
        F = rng.integers(-8, 9, size=(dim + 7, dim)).astype(np.float64) / 8.0
        out[f"D{dim}"] = (F.T @ F, dim)
    F = rng.integers(-8, 9, size=(5, 12)).astype(np.float64) / 8.0
    out["rank5of12"] = (F.T @ F, 5)
    Qo = np.array([[1.0, 1.0, 1.0, 1.0], [1.0, -1.0, 1.0, -1.0], [1.0, 1.0, -1.0, -1.0], [1.0, -1.0, -1.0, 1.0]]) / 2.0
    out["repeated_top"] = (Qo @ np.diag([3.0, 3.0, 1.0, 0.5]) @ Qo.T, 4)
    out["diagonal"] = (np.diag([0.25, 7.0, 3.0, 7.0, 1.0, 0.0]), 6)
    return out


@functools.lru_cache(maxsize=None)
def eigen_exact(name):
    """(lambda_1, lambda_D) of eigen_cases()[name] at 50 digits, as floats of the mp values and the mp values themselves"""
    mp = _mp()
    M, Dn = eigen_cases()[name]
    with mp.workdps(DPS + 20):
        lam = sorted(mp.eigsy(mp.matrix(M.tolist()), eigvals_only=True), reverse=True)
        return lam[0], lam[Dn - 1]


def eig_allowance(Dn):
    return max(FACTOR * EIG_DEV, Dn * U)


def beta_grid():
    """(x, alpha, beta) over 0.5 <= alpha, beta <= 400 and x across (0, 1), and the corners with 1e4 that mpmath's series
    reaches at the working precision"""
    ab = (0.5, 0.75, 1.0, 2.5, 10.0, 63.5, 400.0)
    xq = (1e-6, 1e-3, 0.05, 0.3, 0.5, 0.7, 0.95, 0.999, 1 - 1e-6)
    far = [(0.001, 0.75, 1e4), (0.001, 1.0, 1e4), (0.001, 10.0, 1e4), (0.999, 1e4, 10.0), (0.9995, 1e4, 0.5)]
    return [(x, a, b) for a in ab for b in ab for x in xq] + far


# ---- shared cases --------------------------------------------------------------------------------------------------------------------
E2E_CASES = ("small", "intercept", "wide")


def e2e_case(name):
    """X, D (n x p x nfit), use, K, sets (n_f >= p + 4, 12 to 40 samples; integer X in -8 .. 8 plus a set-wise shift so that
    the sets are not all null):
      small      40 genes x 20 samples, [1, group], two fits (the second leaves five samples out; a NaN and an Inf gene)
      intercept  30 genes x 12 samples, the intercept alone
      wide       24 genes x 40 samples, [1, group, two covariates], two contrasts"""
    if name in ("small", "intercept"):
        X, D, use, K, sets = cr.e2e_case(name)
    else:
        rng = np.random.default_rng(91)
        g, n, p = 24, 40, 4
        X = cr.int_matrix(g, n, rng)
        D = np.asfortranarray(cr.make_design(n, p, rng)[:, :, None])
        use = None
        K = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [0.0, 0.0]])
        sets = cr.make_sets(g, (0, 1, 2, 5, g // 2, g), rng)
    X = X.copy(order="F")
    grp = D[:, min(1, D.shape[1] - 1), 0]
    for k, members in enumerate(sets):                      # a shift of alternating sign along the group column
        for i, gidx in enumerate(members[:6]):
            X[gidx, :] += (2.5 if (i + k) % 2 else -1.25) * grp
    return X, D, use, K, sets


@functools.lru_cache(maxsize=None)
def e2e_reference(name, standardize="posterior.sd"):
    """per fit: fry_mp's result"""
    X, D, use, K, sets = e2e_case(name)
    return [fry_mp(X, D[:, :, f], None if use is None else use[:, f], K, sets, standardize) for f in range(D.shape[2])]


def e2e_np(name, standardize="posterior.sd"):
    X, D, use, K, sets = e2e_case(name)
    return [fry_np(X, D[:, :, f], None if use is None else use[:, f], K, sets, standardize) for f in range(D.shape[2])]


def measure_np():
    """fry_np against fry_mp over the cases: (worst per column, conditioned pairs, all mixed pairs)"""
    worst = {k: 0.0 for k in MEASURED}
    kept = total = 0
    for name in E2E_CASES:
        for std in STD:
            for fit, got in zip(e2e_reference(name, std), e2e_np(name, std)):
                for j, rows in enumerate(fit["tables"]):
                    keep = np.array([conditioned(r) for r in rows])
                    mixed = np.array([r["mixed"] is not None and not r["mixed"].get("single") for r in rows])
                    kept += int((keep & mixed).sum())
                    total += int(mixed.sum())
                    dev = deviation(got[:, :, j], table_float(rows), keep)
                    for k in worst:
                        worst[k] = max(worst[k], dev[k])
    return worst, kept, total


# ---- the sharding hook ------------------------------------------------------------------------------------------------------------
def run_sharded(nshards, X, design, Gp, Gi, use=None, contrasts=None, standardize="posterior.sd", fail=-1):
    """(status, out, hyper) of plaid.fry on `nshards` contexts of one device; the results hold -7 before the call"""
    X = np.asfortranarray(X, dtype=np.float64)
    Dd, _, _, q = engine.limma_operands(X.shape[1], design, use, contrasts)
    out = np.full((len(Gp) - 1, 7, q, Dd.shape[2]), -7.0, order="F")
    hyper = np.full((Dd.shape[2], 7), -7.0)
    status, _ = _status(lambda: engine._fry(hook("fry"), (0, nshards, fail), X, design, Gp, Gi, use, contrasts, standardize,
                                            out=out, hyper=hyper))
    return status, out, hyper


if __name__ == "__main__":
    print(measure_np())
