"""plaid.roast restated twice from the words of include/plaidhip.h (plaidhip_roast, steps 2 to 6): at 50 digits (mpmath) and
in numpy fp64.  limma's source is not in this tree and R is not installed: the header pins the form as recalled, and these
two restatements hold the code to it.

  identity_mp      the identity the design rests on: limma's own form (the effects [beta | Q2'r] against (r0, Q2'w), row sums
                   of squares) equals the sample-space form (beta r0 + r.w, beta^2 + RSS) at 50 digits
  rotate_mp / _np  steps 3 and 4 on given beta, RSS, residuals and W
  stats_mp / _np   step 5 on given z; stats_np reproduces the device's bits (one accumulator per side in the order of Gi)
  finish_np        step 6 from counts
  roast_mp / _np   end to end from X

MEASURED: the worst deviation of the numpy restatement from the 50-digit one over CASES, per quantity, relative to
max(1, |reference|) -- measured on the host (tests/test_roast_ref.py re-measures).  The device is held to FACTOR x these."""
import numpy as np

from plaid_amd import engine
from tests.helpers import limma_ref as lr
from tests.helpers.sharded_hooks import _status, hook

DPS = 50
U = 2.0 ** -53
FACTOR = 4
STATS = ("mean", "floormean", "msq", "mean50")
SQRT_Q = 0.67448975019608171
MEASURED = {"B": 4.5e-16, "z": 7.0e-16, "mean": 3.8e-15, "floormean": 2.4e-15, "msq": 1.8e-15, "mean50": 2.4e-15}


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


# ---- steps 3 and 4 ----------------------------------------------------------------------------------------------------------------
def hill_mp(t, nu):
    mp = _mp()
    A = nu - mp.mpf(1) / 2
    C = 48 * A * A
    y = A * mp.log1p(t * t / nu)
    pol = ((mp.mpf("-0.4") * y - mp.mpf("3.3")) * y - 24) * y - mp.mpf("85.5")
    z = mp.sqrt(y) * (1 + ((y + 3) + pol / (mp.mpf("0.8") * y * y + 100 + C)) / C)
    return -z if t < 0 else z


def moderated_mp(B, beta, rss, d, df0, s02):
    mp = _mp()
    s2r = max((beta * beta + rss - B * B) / d, mp.mpf(0))
    post = s02 if df0 == mp.inf else s2r if df0 == 0 else (df0 * s02 + d * s2r) / (df0 + d)
    if post == 0:
        return mp.nan if B == 0 else mp.sign(B) * mp.inf
    return B / mp.sqrt(post)


def _nu(d, df0):
    return min(float(df0) + float(d), 1e4)


def rotate_mp(beta, rss, Rz, W, d, df0, s02, zscore="hill"):
    """(B, z, Babs) as float arrays rows x nrot from the 50-digit form; Babs = |beta r0| + sum |r_c w_c| (the size of B's
    terms); a gene with a NaN beta gives NaN"""
    mp = _mp()
    rows, n = Rz.shape
    nrot = W.shape[1]
    B = np.full((rows, nrot), np.nan)
    z = np.full((rows, nrot), np.nan)
    Ba = np.full((rows, nrot), np.nan)
    mdf0 = mp.inf if np.isinf(df0) else mp.mpf(float(df0))
    ms02 = mp.mpf(float(s02)) if np.isfinite(s02) else mp.nan
    nu = mp.mpf(_nu(d, df0))
    Wm = [[mp.mpf(float(W[i, k])) for i in range(n + 1)] for k in range(nrot)]
    for r in range(rows):
        if not np.isfinite(beta[r]):
            continue
        b, rs = mp.mpf(float(beta[r])), mp.mpf(float(rss[r]))
        res = [mp.mpf(float(x)) for x in Rz[r]]
        for k in range(nrot):
            w = Wm[k]
            terms = [b * w[0]] + [x * y for x, y in zip(res, w[1:])]
            Bm = mp.fsum(terms)
            t = moderated_mp(Bm, b, rs, mp.mpf(d), mdf0, ms02)
            zz = t if zscore == "none" or mp.isnan(t) else hill_mp(t, nu) if mp.isfinite(t) else mp.nan
            B[r, k], z[r, k], Ba[r, k] = float(Bm), float(zz), float(mp.fsum(abs(x) for x in terms))
    return B, z, Ba


def hill_np(t, nu):
    A = nu - 0.5
    C = 48.0 * A * A
    y = A * np.log1p(t * t / nu)
    pol = ((-0.4 * y - 3.3) * y - 24.0) * y - 85.5
    mag = np.sqrt(y) * (1.0 + ((y + 3.0) + pol / ((0.8 * y * y + 100.0) + C)) / C)
    return np.where(t < 0, -mag, mag)


def rotate_np(beta, rss, Rz, W, d, df0, s02, zscore="hill"):
    """(B, z) rows x nrot in numpy fp64"""
    with np.errstate(all="ignore"):
        B = beta[:, None] * W[0][None, :] + Rz @ W[1:]
        q = (beta[:, None] ** 2 + rss[:, None] - B * B) / d
        s2r = np.where(q > 0, q, 0.0)
        post = np.full_like(s2r, s02) if np.isinf(df0) else s2r if df0 == 0 else (df0 * s02 + d * s2r) / (df0 + d)
        t = B / np.sqrt(post)
        z = t if zscore == "none" else hill_np(t, _nu(d, df0))
    return B, z


# ---- step 5 ----------------------------------------------------------------------------------------------------------------------
def mean50_np(z):
    """the pinned threshold form: z members x K -> (down, up, mixed), each K"""
    m = z.shape[0]
    h = m // 2 + 1
    out = []
    for key in ((-z) + 0.0, z + 0.0, np.abs(z)):
        tau = -np.sort(-key, axis=0)[h - 1]
        acc = np.zeros(z.shape[1])
        above = np.zeros(z.shape[1])
        for i in range(m):
            gt = key[i] > tau
            acc = np.where(gt, acc + key[i], acc)
            above += gt
        val = (acc + (h - above) * tau) / h
        out.append(np.where(np.isnan(key).any(axis=0), np.nan, val))
    return out


def stats_np(z, stat):
    """z: members x K in the order of Gi -> K x 4 (down, up, upordown, mixed), every sum one accumulator from 0.0"""
    m, K = z.shape
    if m == 0:
        return np.full((K, 4), np.nan)
    with np.errstate(all="ignore"):
        if stat == "mean50":
            down, up, mixed = mean50_np(z)
        else:
            a, b, c = np.zeros(K), np.zeros(K), np.zeros(K)
            for i in range(m):
                x = z[i]
                if stat == "mean":
                    a = a + x
                    c = c + np.abs(x)
                elif stat == "floormean":
                    a = a + np.where(-x > 0, -x, 0.0)
                    b = b + np.where(x > 0, x, 0.0)
                    c = c + np.where(np.abs(x) > SQRT_Q, np.abs(x), SQRT_Q)
                else:
                    xx = x * x
                    a = a + np.where(x < 0, xx, 0.0)
                    b = b + np.where(x > 0, xx, 0.0)
                    c = c + xx
            if stat == "mean":
                up, down = a / m, -a / m
            else:
                down, up = a / m, b / m
            mixed = c / m
        return np.column_stack([down, up, np.where(up > down, up, down), mixed])


def stats_mp(z, stat):
    """z: members x K of floats (or mp numbers) -> K lists of 4 mp numbers from the header's words (mean50 by a sort)"""
    mp = _mp()
    m = len(z)
    K = len(z[0]) if m else 0
    out = []
    for k in range(K):
        col = [mp.mpf(z[i][k]) for i in range(m)]
        if stat == "mean":
            s = mp.fsum(col)
            down, up, mixed = -s / m, s / m, mp.fsum(abs(x) for x in col) / m
        elif stat == "floormean":
            down, up = mp.fsum(max(-x, 0) for x in col) / m, mp.fsum(max(x, 0) for x in col) / m
            mixed = mp.fsum(max(abs(x), mp.mpf(SQRT_Q)) for x in col) / m
        elif stat == "msq":
            down, up = mp.fsum(x * x for x in col if x < 0) / m, mp.fsum(x * x for x in col if x > 0) / m
            mixed = mp.fsum(x * x for x in col) / m
        else:
            h = m // 2 + 1
            top = lambda v: mp.fsum(sorted(v, reverse=True)[:h]) / h
            down, up, mixed = top([-x for x in col]), top(col), top([abs(x) for x in col])
        out.append([down, up, max(down, up), mixed])
    return out


# ---- step 6 ----------------------------------------------------------------------------------------------------------------------
def finish_np(cnt, msize, ndown, nup, nrot, stat="mean50", midp=True):
    """cnt sets x 4, msize / ndown / nup per set -> sets x 8"""
    cnt = np.asarray(cnt, dtype=np.float64)
    m = np.asarray(msize, dtype=np.float64)
    out = np.full((len(m), 8), np.nan)
    has = (m >= 1) & ~((stat == "mean50") & (m > engine.ROAST_MEAN50_MAX))
    p = (cnt + 1.0) / (nrot + 1.0)
    out[:, 0] = m
    with np.errstate(all="ignore"):
        out[:, 1] = np.where(m >= 1, np.asarray(ndown) / m, np.nan)
        out[:, 2] = np.where(m >= 1, np.asarray(nup) / m, np.nan)
    out[:, 3] = np.where(has, np.where(p[:, 1] < p[:, 0], 1.0, -1.0), np.nan)
    for col, side in ((4, 2), (6, 3)):
        pv = np.where(has, p[:, side], np.nan)
        out[:, col] = pv
        out[:, col + 1] = np.maximum(lr.bh(pv - 0.5 / (nrot + 1.0)), pv) if midp else lr.bh(pv)
    return out


# ---- the identity ------------------------------------------------------------------------------------------------------------------
def identity_mp(x, D, R):
    """One gene x (n_f values), its design D (n_f x p) and one unit vector R of length d + 1, all at 50 digits.  Returns
    (limma's rotated effect, the sample-space one, limma's row sum of squares, beta^2 + RSS) for the LAST coefficient:
    limma takes the full QR of the design, effects Q'x = [.. beta | rho], and rotates [beta | rho] by R."""
    mp = _mp()
    nf, p = D.shape
    A = mp.matrix(D.tolist())
    Q, _ = mp.qr(A, mode="full")
    xm = mp.matrix([mp.mpf(float(v)) for v in x])
    eff = Q.T * xm
    beta, rho = eff[p - 1], [eff[i] for i in range(p, nf)]
    Rm = [mp.mpf(v) for v in R]
    limma_B = beta * Rm[0] + mp.fsum(a * b for a, b in zip(rho, Rm[1:]))
    limma_ss = beta * beta + mp.fsum(a * a for a in rho)
    # sample space: r = x - Q1 Q1'x, w = Q2 R2
    Q1, Q2 = Q[:, :p], Q[:, p:]
    r = xm - Q1 * (Q1.T * xm)
    w = Q2 * mp.matrix(Rm[1:])
    B = beta * Rm[0] + mp.fsum(r[i] * w[i] for i in range(nf))
    ss = beta * beta + mp.fsum(r[i] * r[i] for i in range(nf))
    return limma_B, B, limma_ss, ss


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _filtered(sets, ok):
    return [[g for g in s if ok[g]] for s in sets]


def roast_mp(X, D, use, K, sets, W, stat="mean50", zscore="hill"):
    """one fit, 50 digits from X: per contrast dict(obs: sets x 4, rot: sets x nrot x 4 (floats), cnt: sets x 4, msize,
    ndown, nup, gap: the smallest |stat_k - stat_obs| / max(1, |stat_obs|) over (set, side, rotation)).  A pair that is EQUAL
    at 50 digits does not enter the gap: real-valued z make that happen only where both sides come out of the same
    operations on the same constants -- no member of that sign (0 on both), every member under floormean's floor (sqrt(q) on
    both) -- and the device repeats those operations, so it ties as well."""
    mp = _mp()
    des = lr.mp_design(D, use, K)
    fits = lr.mp_fit(X, des)
    fin = lr.mp_finish(fits, des)
    sel, d, nrot = des["sel"], des["nf"] - des["p"], W.shape[1]
    ok = [r is not None for r in fin["rows"]]
    fs = _filtered(sets, ok)
    nu = mp.mpf(_nu(d, float(fin["df_prior"])))
    Wm = [[mp.mpf(float(W[0, k]))] + [mp.mpf(float(W[c + 1, k])) for c in sel] for k in range(nrot)]
    res = {}
    for g, f in enumerate(fits):
        if f is not None:
            xm = [mp.mpf(float(t)) for t in X[g, sel]]
            res[g] = [a - mp.fsum(q[c] * e for q, e in zip(des["Q"], f[0])) for c, a in enumerate(xm)]
    zz = lambda t: t if zscore == "none" else hill_mp(t, nu)
    out = []
    for j, uj in enumerate(des["u"]):
        zobs, zrot = {}, {}
        for g, row in enumerate(fin["rows"]):
            if row is None:
                continue
            beta = row["logFC"][j] / uj
            zobs[g] = zz(row["t"][j])
            zr = []
            for k in range(nrot):
                B = beta * Wm[k][0] + mp.fsum(a * b for a, b in zip(res[g], Wm[k][1:]))
                zr.append(zz(moderated_mp(B, beta, fits[g][2], mp.mpf(d), fin["df_prior"], fin["s2_prior"])))
            zrot[g] = zr
        obs = np.full((len(sets), 4), np.nan)
        rot = np.full((len(sets), nrot, 4), np.nan)
        cnt = np.zeros((len(sets), 4), dtype=np.int64)
        gap = np.inf
        nd, nup = np.zeros(len(sets)), np.zeros(len(sets))
        for s, mem in enumerate(fs):
            if not mem:
                continue
            so = stats_mp([[zobs[g]] for g in mem], stat)[0]
            sr = stats_mp([zrot[g] for g in mem], stat)
            obs[s] = [float(v) for v in so]
            for k in range(nrot):
                rot[s, k] = [float(v) for v in sr[k]]
                for e in range(4):
                    cnt[s, e] += int(sr[k][e] >= so[e])
                    if sr[k][e] != so[e]:   # (an exact tie at 50 digits: see roast_mp's docstring)
                        gap = min(gap, float(abs(sr[k][e] - so[e]) / max(1, abs(so[e]))))
            nd[s] = sum(1 for g in mem if zobs[g] < -mp.sqrt(2))
            nup[s] = sum(1 for g in mem if zobs[g] > mp.sqrt(2))
        out.append({"obs": obs, "rot": rot, "cnt": cnt, "msize": np.array([len(v) for v in fs], dtype=np.float64), "ndown": nd,
                    "nup": nup, "gap": gap})
    return out


def roast_np(X, D, use, K, sets, W, stat="mean50", zscore="hill"):
    """one fit in numpy fp64 from X: per contrast dict(obs: sets x 4, rot: sets x nrot x 4)"""
    X, D = np.asarray(X, dtype=np.float64), np.asarray(D, dtype=np.float64)
    n, p = D.shape
    fit = lr.limma_np(X, D, use, K)
    sel = lr._sel(n, use)
    Ds, Xs = D[sel], X[:, sel]
    Kc = np.eye(p) if K is None else np.asarray(K, dtype=np.float64).reshape(p, -1)
    ok = np.isfinite(Xs).all(axis=1)
    d = len(sel) - p
    Rz = np.zeros((X.shape[0], n))
    coef = np.linalg.lstsq(Ds, Xs[ok].T, rcond=None)[0]
    Rz[np.ix_(ok, sel)] = (Xs[ok].T - Ds @ coef).T
    rss = (Rz * Rz).sum(axis=1)
    su = np.sqrt(np.diag(Kc.T @ np.linalg.inv(Ds.T @ Ds) @ Kc))
    fs = _filtered(sets, ok)
    out = []
    for j in range(Kc.shape[1]):
        beta = np.where(ok, fit["logFC"][:, j] / su[j], np.nan)
        _, z = rotate_np(np.where(ok, beta, 0.0), rss, Rz, W, d, fit["df_prior"], fit["s2_prior"], zscore)
        with np.errstate(all="ignore"):
            zo = fit["t"][:, j] if zscore == "none" else hill_np(fit["t"][:, j], _nu(d, fit["df_prior"]))
        obs = np.full((len(sets), 4), np.nan)
        rot = np.full((len(sets), W.shape[1], 4), np.nan)
        for s, mem in enumerate(fs):
            if mem:
                obs[s] = stats_np(zo[mem][:, None], stat)[0]
                rot[s] = stats_np(z[mem], stat)
        out.append({"obs": obs, "rot": rot})
    return out


def rel_dev(got, ref):
    """the worst |got - ref| / max(1, |ref|) over the entries that are finite in the reference"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    keep = np.isfinite(ref)
    if not keep.any():
        return 0.0
    return float(np.max(np.abs(got[keep] - ref[keep]) / np.maximum(1.0, np.abs(ref[keep]))))


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def make_design(n, p, rng):
    D = np.ones((n, p))
    D[:, 1] = (np.arange(n) % 2).astype(np.float64)
    for k in range(2, p):
        D[:, k] = rng.normal(size=n)
    return D


def e2e_case(name):
    """X (genes x samples), D, use, K, sets, W: small, with a NaN gene, a constant gene and an empty set"""
    spec = {"a": (36, 10, 2, 7, 33), "b": (30, 14, 3, 11, 40), "wide": (24, 136, 2, 5, 20)}[name]
    g, n, p, seed, nrot = spec
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(g, n)) + 0.8 * np.outer(rng.normal(size=g), np.arange(n) % 2)
    X = np.round(X * 64) / 64
    D = make_design(n, p, rng)
    use = None
    if name == "b":
        use = np.ones(n, dtype=np.int8)
        use[[2, 9]] = 0
        X[3, 2] = np.nan                       # a NaN where the fit does not look
    X[g - 1, 1] = np.nan                       # a gene outside the universe
    X[2, :] = 3.0                              # a constant gene
    K = np.zeros((p, 1))
    K[1, 0] = 1.0
    pool = [i for i in range(g) if i not in (2, g - 1)]   # (the constant gene is 0 at 50 digits and rounding noise on the device:
    sets = [list(rng.choice(pool, size=k, replace=False)) for k in (1, 2, 3, 7, 12)] + [[], [g - 1], list(range(g))]   # never alone)
    W = engine.roast_rotations(D, use, 0, nrot, seed)
    return X, D, use, K, sets, W


E2E_CASES = ("a", "b", "wide")
_REF = {}


def e2e_reference(name, stat, zscore="hill"):
    key = (name, stat, zscore)
    if key not in _REF:
        X, D, use, K, sets, W = e2e_case(name)
        _REF[key] = roast_mp(X, D, use, K, sets, W, stat, zscore)
    return _REF[key]


def pattern(sets):
    Gp = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    Gi = np.array([g for s in sets for g in s], dtype=np.int32)
    return Gp, Gi


def rotate_case(name):
    """beta, rss, Rz (rows x n), W, d, df0, s02 as the host makes them from an e2e case (numpy fp64)"""
    X, D, use, K, sets, W = e2e_case(name)
    n, p = D.shape
    fit = lr.limma_np(X, D, use, K)
    sel = lr._sel(n, use)
    ok = np.isfinite(X[:, sel]).all(axis=1)
    Rz = np.zeros((X.shape[0], n))
    coef = np.linalg.lstsq(D[sel], X[ok][:, sel].T, rcond=None)[0]
    Rz[np.ix_(ok, sel)] = (X[ok][:, sel].T - D[sel] @ coef).T
    su = np.sqrt(np.diag(K.T @ np.linalg.inv(D[sel].T @ D[sel]) @ K))
    beta = np.where(ok, fit["logFC"][:, 0] / su[0], np.nan)
    return beta, (Rz * Rz).sum(axis=1), Rz, W, len(sel) - p, fit["df_prior"], fit["s2_prior"]


def measure_np():
    """the numpy restatement against the 50-digit one over the cases: the worst deviation per quantity"""
    worst = {k: 0.0 for k in MEASURED}
    for name in ("a", "b"):
        beta, rss, Rz, W, d, df0, s02 = rotate_case(name)
        Bm, zm, _ = rotate_mp(beta, rss, Rz, W, d, df0, s02)
        Bn, zn = rotate_np(np.where(np.isfinite(beta), beta, 0.0), rss, Rz, W, d, df0, s02)
        worst["B"] = max(worst["B"], rel_dev(Bn, Bm))
        worst["z"] = max(worst["z"], rel_dev(zn, zm))
    for name in E2E_CASES:
        X, D, use, K, sets, W = e2e_case(name)
        for stat in STATS:
            ref = e2e_reference(name, stat)
            got = roast_np(X, D, use, K, sets, W, stat)
            for a, b in zip(got, ref):
                worst[stat] = max(worst[stat], rel_dev(a["rot"], b["rot"]), rel_dev(a["obs"], b["obs"]))
    return worst


# ---- the sharding hook ------------------------------------------------------------------------------------------------------------
def run_sharded(nshards, X, design, Gp, Gi, use=None, contrasts=None, fail=-1, **kw):
    """(status, out, hyper) of plaid.roast on `nshards` contexts of one device; the results hold -7 before the call"""
    X = np.asfortranarray(X, dtype=np.float64)
    Dd, _, _, q = engine.limma_operands(X.shape[1], design, use, contrasts)
    out = np.full((len(Gp) - 1, 8, q, Dd.shape[2]), -7.0, order="F")
    hyper = np.full((Dd.shape[2], 7), -7.0)
    status, _ = _status(lambda: engine._roast(hook("roast"), (0, nshards, fail), X, design, Gp, Gi, use, contrasts, out=out,
                                              hyper=hyper, **kw))
    return status, out, hyper


if __name__ == "__main__":
    print(measure_np())
