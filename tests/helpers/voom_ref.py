"""plaid.voom for the tests (include/plaidhip.h: plaidhip_voom, plaidhip_lowess).

lowess_walk    the header's lowess in plain Python, anchor walk and all: shares no line with csrc/lowess.h
lowess_direct  delta = 0 said differently: every point gets its own local regression over a window found from scratch
emulate_weights the pinned chain, bisection and interpolation of the weights pass in numpy / Python floats
voom_np        the same pins end to end: correctly rounded log2-CPM (mpmath), numpy least squares, lowess_walk, the weights
make_counts    negative-binomial-like integer counts with all-zero rows and a zero-heavy column
"""
from __future__ import annotations

import math

import numpy as np

from tests.helpers.limma_na_ref import fma


# ---- lowess ---------------------------------------------------------------------------------------------------------------------
def _local_fit(x, y, xs, nleft, nright, rw):
    """(ok, ys) of the header's local fit; rw None in the first pass"""
    n = len(x)
    h = max(xs - x[nleft], x[nright] - xs)
    w = {}
    tot = 0.0
    j = nleft
    while j < n:
        r = abs(x[j] - xs)
        if r <= 0.999 * h:
            if r <= 0.001 * h:
                wj = 1.0
            else:
                t = r / h
                u = 1.0 - (t * t) * t
                wj = (u * u) * u
            if rw is not None:
                wj = wj * rw[j]
            w[j] = wj
            tot = tot + wj
        elif x[j] > xs:
            break
        else:
            w[j] = 0.0
        j += 1
    if not tot > 0.0:
        return False, None
    idx = sorted(w)
    w = {j: w[j] / tot for j in idx}
    if h > 0.0:
        a = 0.0
        for j in idx:
            a = a + w[j] * x[j]
        c = 0.0
        for j in idx:
            c = c + w[j] * ((x[j] - a) * (x[j] - a))
        if math.sqrt(c) > 0.001 * (x[n - 1] - x[0]):
            b = (xs - a) / c
            w = {j: w[j] * (b * (x[j] - a) + 1.0) for j in idx}
    s = 0.0
    for j in idx:
        s = s + w[j] * y[j]
    return True, s


def _window(x, i, ns, nleft=0):
    """the header's window for point i, slid from nleft"""
    n = len(x)
    nright = nleft + ns - 1
    while nright < n - 1 and x[i] - x[nleft] > x[nright + 1] - x[i]:
        nleft += 1
        nright += 1
    return nleft, nright


def _robustness(y, ys):
    """the header's update: None when cmad < 1e-7 mean|res| (the passes stop)"""
    n = len(y)
    res = [abs(y[j] - ys[j]) for j in range(n)]
    sc = 0.0
    for r in res:
        sc = sc + r
    sc = sc / n
    srt = sorted(res)
    med = srt[n // 2] if n % 2 else (srt[n // 2 - 1] + srt[n // 2]) / 2.0
    cmad = 6.0 * med
    if cmad < 1e-7 * sc:
        return None
    out = []
    for r in res:
        if r <= 0.001 * cmad:
            out.append(1.0)
        elif r <= 0.999 * cmad:
            t = r / cmad
            u = 1.0 - t * t
            out.append(u * u)
        else:
            out.append(0.0)
    return out


def lowess_walk(x, y, f, iters=3, delta=0.0):
    """(ys, anchor flags of the last pass) by the header's anchor walk"""
    x, y = [float(t) for t in x], [float(t) for t in y]
    n = len(x)
    if n < 2:
        return np.array(y), np.ones(n, dtype=bool)
    ns = max(2, min(n, int(math.floor(f * n + 1e-7))))
    rw, ys, anchor = None, [0.0] * n, [False] * n
    for it in range(iters + 1):
        anchor = [False] * n
        i, last, nleft = 0, -1, 0
        while True:
            nleft, nright = _window(x, i, ns, nleft)
            ok, v = _local_fit(x, y, x[i], nleft, nright, rw)
            ys[i] = v if ok else y[i]
            anchor[i] = True
            for j in range(last + 1, i):
                alpha = (x[j] - x[last]) / (x[i] - x[last])
                ys[j] = alpha * ys[i] + (1.0 - alpha) * ys[last]
            last = i
            cut = x[last] + delta
            stop = n
            for j in range(last + 1, n):
                if x[j] > cut:
                    stop = j
                    break
                if x[j] == x[last]:
                    ys[j] = ys[last]
                    anchor[j] = True
                    last = j
            i = max(last + 1, stop - 1)
            if last >= n - 1:
                break
        if it == iters:
            break
        rw = _robustness(y, ys)
        if rw is None:
            break
    return np.array(ys), np.array(anchor)


def lowess_direct(x, y, f, iters=3):
    """delta = 0: a local regression at every point, each window found from scratch"""
    x, y = [float(t) for t in x], [float(t) for t in y]
    n = len(x)
    ns = max(2, min(n, int(math.floor(f * n + 1e-7))))
    rw, ys = None, [0.0] * n
    for it in range(iters + 1):
        for i in range(n):
            ok, v = _local_fit(x, y, x[i], *_window(x, i, ns), rw)
            ys[i] = v if ok else y[i]
        if it == iters:
            break
        rw = _robustness(y, ys)
        if rw is None:
            break
    return np.array(ys)


def knots_of(x, ys, anchor):
    """the anchors at distinct x (the first of each) with their fitted values"""
    kx, ky = [], []
    for i in np.flatnonzero(anchor):
        if not kx or x[i] != kx[-1]:
            kx.append(float(x[i]))
            ky.append(float(ys[i]))
    return np.array(kx), np.array(ky)


# ---- the weights pass -----------------------------------------------------------------------------------------------------------
def trend(kx, ky, lam):
    """f(lambda) of the header: the end values outside, bisection, linear interpolation"""
    nk = len(kx)
    if not lam > kx[0]:
        return float(ky[0])
    if lam >= kx[nk - 1]:
        return float(ky[nk - 1])
    lo, hi = 0, nk - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if kx[mid] <= lam:
            lo = mid
        else:
            hi = mid
    return float(ky[lo] + (ky[lo + 1] - ky[lo]) * ((lam - kx[lo]) / (kx[lo + 1] - kx[lo])))


def emulate_weights(Q, offset, Eff, kx, ky):
    """(lambda, w), rows x n, from the effects Eff (p x rows): the fma chain in ascending k from 0.0, + offset, the trend,
    1 / ((f f) (f f)); f <= 0: NaN"""
    n, p = Q.shape
    rows = Eff.shape[1]
    lam, w = np.empty((rows, n)), np.empty((rows, n))
    for r in range(rows):
        for c in range(n):
            mu = 0.0
            for k in range(p):
                mu = fma(float(Q[c, k]), float(Eff[k, r]), mu)
            lam[r, c] = mu + float(offset[c])
            fv = trend(kx, ky, lam[r, c])
            f2 = fv * fv
            w[r, c] = 1.0 / (f2 * f2) if fv > 0.0 else np.nan
    return lam, w


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def log2_cr(v):
    """the correctly rounded log2 of a positive double"""
    import mpmath
    with mpmath.workdps(40):
        return float(mpmath.log(mpmath.mpf(float(v)), 2))


def logcpm_cr(counts, lib):
    """E with the two divisions and the product as pinned (fp64) and a correctly rounded log2"""
    arg = ((np.asarray(counts, dtype=np.float64) + 0.5) / (np.asarray(lib, dtype=np.float64)[None, :] + 1.0)) * 1e6
    return np.vectorize(log2_cr)(arg)


def ulps(got, ref):
    """|got - ref| in units of the last place of ref"""
    return np.abs(got - ref) / np.spacing(np.abs(ref))


def voom_np(counts, D, lib_size=None, span=0.5):
    """the pins in numpy: dict like engine._voom's, with M, s2, sx, sy and the rows the trend took"""
    counts, D = np.asarray(counts, dtype=np.float64), np.asarray(D, dtype=np.float64)
    rows, n = counts.shape
    p = D.shape[1]
    lib = counts.sum(axis=0) if lib_size is None else np.asarray(lib_size, dtype=np.float64)
    E = logcpm_cr(counts, lib)
    beta = np.linalg.lstsq(D, E.T, rcond=None)[0]
    fitted = (D @ beta).T
    s2 = ((E - fitted) ** 2).sum(axis=1) / (n - p)
    M = E.mean(axis=1)
    l1 = np.log2(lib + 1.0)
    take = (counts.sum(axis=1) != 0) & np.isfinite(s2)
    sx, sy = (M + (l1.mean() - np.log2(1e6)))[take], np.sqrt(np.sqrt(s2[take]))
    o = np.argsort(sx, kind="stable")
    x, y = sx[o], sy[o]
    ys, anchor = lowess_walk(x, y, span, 3, 0.01 * (x[-1] - x[0]))
    kx, ky = knots_of(x, ys, anchor)
    offset = l1 - np.log2(1e6)
    lam = fitted + offset[None, :]
    f = np.array([[trend(kx, ky, v) for v in row] for row in lam])
    return {"E": E, "weights": 1.0 / f ** 4, "lib_size": lib, "offset": offset, "knots_x": kx, "knots_y": ky, "M": M, "s2": s2,
            "x": x, "y": y, "lambda": lam, "take": take}


def make_counts(rows, n, p, seed):
    """(counts, design): negative-binomial-like integers (a gamma-mixed Poisson around per-gene means spanning four decades,
    a group effect on a fifth of the genes), rows 2, 9 and rows - 1 all zero, column 1 zero-heavy; design [1, group, covariates]"""
    rng = np.random.default_rng([rows, n, p, seed])
    D = np.column_stack([np.ones(n), rng.permutation(np.arange(n) % 2)] + [rng.normal(size=n) for _ in range(p - 2)])[:, :p]
    mu = np.exp(rng.uniform(np.log(0.5), np.log(5000.0), size=rows))
    depth = np.exp(rng.normal(0.0, 0.3, size=n))
    fold = np.where(rng.random(rows) < 0.2, np.exp(rng.normal(0.0, 1.0, size=rows)), 1.0)
    mean = mu[:, None] * depth[None, :] * np.where(D[:, 1][None, :] == 1, fold[:, None], 1.0)
    lam = mean * rng.gamma(5.0, 1.0 / 5.0, size=(rows, n))
    counts = rng.poisson(lam).astype(np.float64)
    counts[[2, 9, rows - 1], :] = 0.0
    counts[rng.random(rows) < 0.7, 1] = 0.0
    return np.asfortranarray(counts), D
