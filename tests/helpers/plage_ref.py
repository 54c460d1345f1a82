"""replaid.zscore and replaid.plage restated from include/plaidhip.h in numpy, the references and certificates their tests
share, and the forward bounds DESIGN.md section 22 derives.

Nothing here trusts an SVD: a row v is certified against the set's standardized block Z (recomputed in extended precision)
by mu = |Z v|^2 / |v|^2 and rho = |Z'Z v - mu v|.  trace(Z Z') = k (n - 1) exactly and Z Z' is positive semi-definite, so
lambda_2 <= trace - mu and sin angle(v, v_1) <= rho / (2 mu - trace) whenever 2 mu > trace."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
TOL = 2.0 ** -40
COLUMNS = ("size", "lambda", "explained", "iterations", "residual", "converged")


# ---- the pinned definitions, fp64 ---------------------------------------------------------------------------------------------
def moments(X):
    """(mean, sd, flag) per row in the pinned sequential order; flag 0 kept, 1 constant, 2 sd not finite"""
    X = np.asarray(X, dtype=np.float64)
    g, n = X.shape
    with np.errstate(all="ignore"):
        s = np.zeros(g)
        for j in range(n):
            s = s + X[:, j]
        mean = s / float(n)
        ss = np.zeros(g)
        for j in range(n):
            d = X[:, j] - mean
            ss = ss + d * d
        sd = np.sqrt(ss / float(n - 1))
    flag = np.where(sd == 0.0, 1, np.where(np.isfinite(sd) & (sd > 0), 0, 2)).astype(np.int32)
    return mean, sd, flag


def standardize(X):
    """(Z, flag): z of the kept rows, 0 in a constant row, NaN in a flagged one"""
    mean, sd, flag = moments(X)
    with np.errstate(all="ignore"):
        Z = (np.asarray(X, dtype=np.float64) - mean[:, None]) / sd[:, None]
    Z[flag == 1, :] = 0.0
    Z[flag == 2, :] = np.nan
    return Z, flag


def members(Gp, Gi, flag, s):
    """(kept rows of set s in G's order, their positions in the segment, whether a flagged row is among them)"""
    seg = np.asarray(Gi[Gp[s]:Gp[s + 1]], dtype=np.int64)
    keep = flag[seg] != 1
    return seg[keep], np.flatnonzero(keep), bool((flag[seg] == 2).any())


def orient(u):
    """the sign the orientation rule gives u (+1.0 or -1.0)"""
    u = np.asarray(u, dtype=np.float64)
    s, a = u.sum(), np.abs(u).sum()
    if abs(s) > a * 2.0 ** -20:
        return -1.0 if s < 0 else 1.0
    first = int(np.flatnonzero(np.abs(u) >= np.abs(u).max() / 2.0)[0])
    return -1.0 if u[first] < 0 else 1.0


def power_iteration(C, tol=TOL, maxit=1000):
    """the pinned iteration on a symmetric C: (u oriented, lambda, iterations, r / lambda, converged)"""
    C = np.asarray(C, dtype=np.float64)
    nn = (C * C).sum(axis=0)
    c0 = int(np.argmax(nn))                      # (the lowest index at a tie)
    u = C[:, c0] / np.sqrt(nn[c0])
    it, conv = 0, 0
    while True:
        it += 1
        y = C @ u
        lam = float(u @ y)
        r = float(np.linalg.norm(y - lam * u))
        if r <= tol * lam:
            conv = 1
            break
        if it == maxit:
            break
        u = y / np.linalg.norm(y)
    return u * orient(u), lam, it, r / lam, conv


def gram(Zs):
    """C = Zs Zs' summed over the samples in order from 0.0, every product rounded before it is added (no fused operation,
    whatever the BLAS behind numpy does)"""
    C = np.zeros((Zs.shape[0], Zs.shape[0]))
    for j in range(Zs.shape[1]):
        C = C + np.multiply.outer(Zs[:, j], Zs[:, j])
    return C


def plage_set(Zs, tol=TOL, maxit=1000):
    """the pinned PLAGE of one block Zs (k x n, k >= 1, finite): dict of v, u and the six statistics"""
    C = gram(Zs)
    u, lam, it, res, conv = power_iteration(C, tol, maxit)
    v = (u @ Zs) / np.sqrt(lam)
    return dict(v=v, u=u, size=Zs.shape[0], **{"lambda": lam}, explained=lam / np.trace(C), iterations=it, residual=res,
                converged=conv)


def plage(X, Gp, Gi, tol=TOL, maxit=1000):
    """(S m x n, info m x 6, loadings Gp[m]) of the restatement"""
    X = np.asarray(X, dtype=np.float64)
    Z, flag = standardize(X)
    m, n = len(Gp) - 1, X.shape[1]
    S, info, L = np.full((m, n), np.nan), np.full((m, 6), np.nan), np.zeros(int(Gp[-1]))
    for s in range(m):
        rows, pos, bad = members(Gp, Gi, flag, s)
        info[s, 0], info[s, 3], info[s, 5] = len(rows), 0, 0
        if bad:
            L[Gp[s] + pos] = np.nan
        if bad or len(rows) == 0:
            continue
        r = plage_set(Z[rows, :], tol, maxit)
        S[s, :] = r["v"]
        info[s, :] = [r[c] for c in COLUMNS]
        L[Gp[s] + pos] = r["u"]
    return S, info, L


def zscore(X, Gp, Gi):
    """(S m x n, size m) of the restatement (fp64, members summed in G's order)"""
    Z, flag = standardize(X)
    m = len(Gp) - 1
    S, size = np.full((m, Z.shape[1]), np.nan), np.zeros(m)
    for s in range(m):
        rows, _, bad = members(Gp, Gi, flag, s)
        size[s] = len(rows)
        if not bad and len(rows):
            S[s, :] = Z[rows, :].sum(axis=0) / np.sqrt(float(len(rows)))
    return S, size


def svd_row(Zs):
    """numpy's first right singular vector of Zs and its left partner, oriented by the rule: (v, u, sigma^2)"""
    Uu, sv, Vt = np.linalg.svd(np.asarray(Zs, dtype=np.float64), full_matrices=False)
    sg = orient(Uu[:, 0])
    return Vt[0, :] * sg, Uu[:, 0] * sg, float(sv[0]) ** 2


# ---- extended precision -------------------------------------------------------------------------------------------------------
def standardize_ld(X):
    """Z of finite rows in extended precision from the same fp64 inputs (constant rows: NaN; the caller leaves them out)"""
    X = np.asarray(X, dtype=np.float64).astype(LD)
    n = X.shape[1]
    mean = X.sum(axis=1) / LD(n)
    d = X - mean[:, None]
    sd = np.sqrt((d * d).sum(axis=1) / LD(n - 1))
    with np.errstate(all="ignore"):
        return d / sd[:, None]


def certify(Zs_ld, v):
    """the certificate of a row v against the block Zs_ld (extended precision): dict of mu, rho (for the normalized v),
    trace (= k (n - 1)), gap = 2 mu - trace, sin = rho / gap, norm = |v|"""
    v = np.asarray(v, dtype=np.float64).astype(LD)
    nv = np.sqrt((v * v).sum())
    w = v / nv
    zw = Zs_ld @ w
    mu = (zw * zw).sum()
    res = Zs_ld.T @ zw - mu * w
    rho = np.sqrt((res * res).sum())
    k, n = Zs_ld.shape
    trace = LD(k) * LD(n - 1)
    gap = 2 * mu - trace
    return dict(mu=mu, rho=rho, trace=trace, gap=gap, sin=rho / gap if gap > 0 else LD(np.inf), norm=nv, w=w)


def zscore_exact(X, rows):
    """sum of z over `rows` / sqrt(k) for every sample in 50-digit arithmetic on the same fp64 inputs: a list of mpf"""
    import mpmath as mp
    mp.mp.dps = 50
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[1]
    tot = [mp.mpf(0)] * n
    for i in rows:
        x = [mp.mpf(float(t)) for t in X[i, :]]
        mean = mp.fsum(x) / n
        sd = mp.sqrt(mp.fsum([(t - mean) ** 2 for t in x]) / (n - 1))
        tot = [a + (t - mean) / sd for a, t in zip(tot, x)]
    rk = mp.sqrt(mp.mpf(len(rows)))
    return [a / rk for a in tot]


# ---- the forward bounds of DESIGN.md section 22 --------------------------------------------------------------------------------
def z_error(X, rows):
    """E (len(rows) x n): a bound on |z computed - z exact| of the pinned standardization, from the input alone.
    eta = (n + 1) u mean|x| / sd bounds the computed mean's error over sd; the computed sd is off by at most
    eps_sd = (n + 7) u / 2 + 1.5 eta + eta^2 relatively; then |dz| <= |z| (eps_sd + 3 u) + eta, and 1.01 takes the products
    of these first-order terms (each below 1e-6 for the bound to be used at all)."""
    Xr = np.asarray(X, dtype=np.float64)[rows, :].astype(LD)
    n = Xr.shape[1]
    Z = standardize_ld(Xr)
    sd = np.sqrt(((Xr - Xr.mean(axis=1)[:, None]) ** 2).sum(axis=1) / LD(n - 1))
    eta = LD(n + 1) * LD(U) * np.abs(Xr).mean(axis=1) / sd
    eps_sd = LD(n + 7) * LD(U) / 2 + LD(1.5) * eta + eta * eta
    assert float(eta.max(initial=0)) < 1e-6 and float(eps_sd.max(initial=0)) < 1e-6
    return (LD(1.01) * (np.abs(Z) * (eps_sd + 3 * LD(U))[:, None] + eta[:, None])).astype(np.float64)


def zscore_bound(X, rows, terms, exact):
    """the allowance of one set's zscore row (n values): the z errors summed, (terms - 1) u sum|z| for a sum of `terms`
    addends in any order (the crossprod adds the dropped members' zeros too), over sqrt(k); then 2 u |S| for the square
    root and the division"""
    E = z_error(X, rows)
    Zabs = np.abs(standardize_ld(np.asarray(X, dtype=np.float64)[rows, :])).astype(np.float64)
    k = len(rows)
    num = E.sum(axis=0) + 1.01 * max(terms - 1, 0) * U * (Zabs + E).sum(axis=0)
    return num / np.sqrt(k) + 1.01 * 2 * U * np.abs(np.array([float(e) for e in exact]))


def plage_rounding(X, rows, lam):
    """(R, dv, dC) for one set: dC bounds |C computed - Z Z'|_F, dv bounds |v computed - Z'u / sqrt(lambda)|_2, and
    R = 3 k u trace + dC + 2 trace dv bounds what rounding adds to |Z'Z v - lambda v| beyond the iteration's own residual
    """
    k, n = len(rows), np.asarray(X).shape[1]
    ez = float(z_error(X, rows).max())
    trace = float(k * (n - 1))
    dC = 1.01 * k * ((n + 4) * U * (n - 1) + 2 * ez * n)
    dv = 1.01 * ((k + 2) * U * np.sqrt(trace) + ez * np.sqrt(n * k)) / np.sqrt(lam)
    return 3 * k * U * trace + dC + 2 * trace * dv, dv, dC


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def planted(rng, k, n, lo=0.85, hi=0.97, negative=0.25):
    """k x n rows a_i f + sqrt(1 - a_i^2) e_i with loadings a_i in [lo, hi], a share of them negative: one strong factor"""
    f = rng.normal(size=n)
    a = rng.uniform(lo, hi, size=k)
    neg = rng.permutation(k) < int(round(negative * k))
    a = np.where(neg, -a, a)
    return a[:, None] * f[None, :] + np.sqrt(1 - a * a)[:, None] * rng.normal(size=(k, n)), a


# the effective sizes the GPU tests cover.  Edges: 15 / 16 / 17 the padding of C's rows and the 16-row tile of the MFMA form
# of the Gram kernel; 31 / 32 / 33 the 32-row tile of the product's form; 33 also three 16-row tile rows, whose six tiles end
# half-way through the second workgroup of four wavefronts, as the six 32-row tiles of 65 do; 63 / 64 / 65 the wavefront of
# the compaction; 129 past its second trip; 255 / 256 / 257 the 256 threads of the eigen workgroup and of the projection's
# sample blocks
SIZES = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 255, 256, 257)
SPECIAL = 12   # rows at the end of X: 5 constant, 1 with a NaN, 1 with an infinity, 1 copy of row 10, 4 spare


SEEDS = {2: 1, 3: 3, 65: 1, 130: 1, 257: 1}   # per sample count: the first seed whose sets all pass `separated`


def build_case(n, seed, g=600, sizes=SIZES, extras=True):
    """X (g x n, one planted factor over all ordinary genes: loadings in [0.85, 0.97], a quarter negative, row offsets) and
    the sets (Gp, Gi, names): one of every size in `sizes` drawn from the ordinary genes in unsorted order, then the named
    special sets.  Returns a dict."""
    rng = np.random.default_rng(seed)
    pool = g - SPECIAL
    X = np.zeros((g, n))
    core, a = planted(rng, pool, n)
    X[:pool] = core + rng.normal(size=(pool, 1)) * 3.0
    const = np.arange(pool, pool + 5)
    X[const] = np.array([2.5, -1.0, 0.0, 7.0, 0.125])[:, None]   # (values whose sums are exact: mean == x, sd == 0)
    r_nan, r_inf, r_copy = pool + 5, pool + 6, pool + 7
    X[pool + 5:] = rng.normal(size=(SPECIAL - 5, n))
    X[r_nan, n // 2] = np.nan
    X[r_inf, 0] = np.inf
    X[r_copy] = X[10]
    posg, negg = np.flatnonzero(a > 0), np.flatnonzero(a < 0)
    sets, names = [], []
    for k in sizes:
        sets.append(rng.permutation(pool)[:k])
        names.append(f"k{k}")
    p1, p2 = rng.permutation(pool), rng.permutation(pool)   # (no member twice in a set)
    extra = {
        "empty": np.zeros(0, dtype=np.int64),
        "constants": const[[3, 0, 4]],
        "one_constant": np.concatenate([p1[:9], const[[1]], p1[9:16]]),
        "nan_row": np.concatenate([p2[:5], [r_nan], p2[5:8]]),
        "inf_row": np.concatenate([[r_inf], rng.permutation(pool)[:6]]),
        "identical": np.concatenate([rng.permutation(np.setdiff1d(np.arange(pool), [10]))[:4], [r_copy, 10]]),
        "positive_pair": posg[rng.permutation(len(posg))[:2]],
        "negative_pair": np.array([posg[rng.integers(len(posg))], negg[rng.integers(len(negg))]]),
    }
    for nm, members_ in (extra.items() if extras else ()):
        sets.append(np.asarray(members_, dtype=np.int64))
        names.append(nm)
    Gp = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    Gi = np.concatenate(sets).astype(np.int32)
    return dict(X=np.asfortranarray(X), Gp=Gp, Gi=Gi, names=names, loadings=a, n=n, g=g)


def separated(case):
    """per set with kept members and no flagged one: the certificate of numpy's oriented svd row and whether
    2 mu - trace >= trace / 4, from the reference alone.  dict name -> (rows, pos, certificate, v_np, u_np, ok)"""
    Z, flag = standardize(case["X"])
    out = {}
    for s, nm in enumerate(case["names"]):
        rows, pos, bad = members(case["Gp"], case["Gi"], flag, s)
        if bad or len(rows) == 0:
            continue
        Zl = standardize_ld(case["X"][rows, :])
        v_np, u_np, _ = svd_row(Z[rows, :])
        c = certify(Zl, v_np)
        out[nm] = dict(s=s, rows=rows, pos=pos, Zl=Zl, cert=c, v_np=v_np, u_np=u_np, ok=bool(c["gap"] >= c["trace"] / 4))
    return out
