"""plaid.romer as include/plaidhip.h pins it (plaidhip_romer), restated twice:

  * at 50 digits (mpmath) from the original design and expression: the fit (limma_ref), the shrink (shrink_mp), the rotated
    moderated t (roast_ref.moderated_mp), then keys, 2 rank, integer sides, counts -- romer_mp;
  * in numpy / scipy.stats.rankdata from given t: keys_np -> rank2_np -> sides_np -> counts -> finish_np.

The statistic is a function of the ORDER of the keys only, so a device that holds every t within its allowance reproduces the
counts exactly wherever the order is decided.  romer_mp asserts that on the CPU for its own cases: under every rotation, and
in the observed column, the key intervals [key(t - A), key(t + A)] of any two universe genes are disjoint, or both are the
same single point by construction (an all-zero row gives exact zeros on every path; max(x, 0) of two negative t; the floor
1), or the genes are duplicated rows (the same operations on the same inputs).  The allowance on a rotated t is
    A = 2 (FACTOR roast_ref.MEASURED["z"] max(1, |t|) + |t(beta' (1 + eps_c)) - t(beta')|)
-- roast's allowance on the rotated statistic (derived and measured there; romer takes z = t), plus the first-order effect of
the shrink factor's own error eps_c = FACTOR MEASURED["shrink"] + (FACTOR roast_ref.MEASURED["z"] / 2^-53) s, where s is the
change of c when the observed t are rounded to fp64 (the sensitivity of the shrink to one unit roundoff in its inputs); the
observed column has roast's part alone.  The shrink's one discontinuity, ntarget = ceil(pi / 2 U), is asserted to be
1e-6 away from a step.

MEASURED["shrink"]: the worst relative deviation of plaidhip_romer_shrink from shrink_mp over SHRINK_CASES, measured on the
host (tests/test_romer_ref.py re-measures and allows FACTOR x).  It is what the t tail's own error (exact_stats.MEASURED_ACC
["pt"] = 2.9e-13 relative, which enters p, ptarget and through the bisection q_r) and libm's log / exp leave after the
conditioning of the formulas -- not a guess."""
import numpy as np

from plaid_amd import engine
from tests.helpers import exact_stats as xs
from tests.helpers import limma_ref as lr
from tests.helpers import roast_ref as rr
from tests.helpers.sharded_hooks import _status, hook

DPS = 50
U = 2.0 ** -53
FACTOR = 4
STATS = ("mean", "floormean", "mean50")
MEASURED = {"shrink": 4.1e-14}
MEAN50_MAX = 16384


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


# ---- the shrink ---------------------------------------------------------------------------------------------------------------
def _normal(nu):
    return not np.isfinite(float(nu)) or float(nu) > 1e6


def two_sided_mp(t, nu):
    mp = _mp()
    if mp.mpf(t) == 0:
        return mp.mpf(1)
    if _normal(nu):
        return mp.erfc(abs(mp.mpf(t)) / mp.sqrt(2))
    return xs.two_pt(t, nu)


def upper_quantile_mp(p, nu):
    """q >= 0 with 2 P(T_nu > q) = p at 50 digits: bisection from a doubled bracket"""
    mp = _mp()
    lo, hi = mp.mpf(0), mp.mpf(1)
    while two_sided_mp(hi, nu) > p:
        lo, hi = hi, hi * 2
    for _ in range(180):
        mid = (lo + hi) / 2
        if two_sided_mp(mid, nu) > p:
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2


def shrink_mp(t, u, s02, nu, info=None):
    """(c list, pi, margin of ntarget's ceil) at 50 digits from the header's words; t: mp numbers or floats.  info (a dict)
    takes ntarget and how many v0_r met the lower and the upper clamp"""
    mp = _mp()
    t = [mp.mpf(0) if mp.isnan(mp.mpf(x)) else mp.mpf(x) for x in t]
    n = len(t)
    u2 = mp.mpf(u) ** 2
    nu_m = mp.inf if _normal(nu) else mp.mpf(nu)
    p = sorted((two_sided_mp(x, nu) for x in t), reverse=True)
    acc = mp.fsum((n - j) * min(mp.mpf(n) / (n - j) * p[j], 1) for j in range(n))
    pi = 1 - 2 * acc / (n * (n + 1))
    if not pi > 0:
        return [mp.mpf(1)] * n, pi, 1.0
    raw = pi / 2 * n
    nt = int(min(max(mp.ceil(raw), 1), n))
    margin = float(min(abs(raw - mp.floor(raw)), abs(mp.ceil(raw) - raw))) if raw > 1 else float(1 - raw)
    P = max(mp.mpf(nt) / n, pi)
    at = sorted((abs(x) for x in t), reverse=True)[:nt]
    s02 = mp.mpf(s02)
    vlo, vhi = mp.mpf("0.01") / s02, 16 / s02
    vs = []
    for r, a in enumerate(at):
        p0 = two_sided_mp(a, nu)
        pt = ((r + mp.mpf("0.5")) / n - (1 - P) * p0) / P
        v = mp.mpf(0)
        if pt > p0:
            v = u2 * ((a / upper_quantile_mp(pt, nu)) ** 2 - 1)
        vs.append(min(max(v, vlo), vhi))
        if info is not None:
            info["low"] = info.get("low", 0) + int(v < vlo)
            info["high"] = info.get("high", 0) + int(v > vhi)
            info["ntarget"] = nt
    v0 = mp.fsum(vs) / nt
    r = (u2 + v0) / u2
    c = []
    for x in t:
        if pi >= 1:
            pde = mp.mpf(1)
        else:
            t2 = x * x
            if mp.isinf(t2):
                pde = mp.mpf(1)
            else:
                kern = t2 * (1 - 1 / r) / 2 if nu_m == mp.inf else (1 + nu_m) / 2 * mp.log((t2 + nu_m) / (t2 / r + nu_m))
                pde = 1 / (1 + mp.exp(-(mp.log(pi / (1 - pi)) - mp.log(r) / 2 + kern)))
        c.append(mp.sqrt(u2 / (u2 + v0 * pde)))
    return c, pi, margin


def shrink_case(name):
    """(t, u, s02, nu) of the shrink's own cases: pi = 0, pi tiny (ntarget = 1), pi near 1, df0 = inf and df0 = 0 (nu = d),
    the clamp hit below and above"""
    rng = np.random.default_rng({"null": 1, "tiny": 2, "most": 3, "inf": 4, "nodf0": 5, "clamp_lo": 6, "clamp_hi": 7,
                                 "mixed": 8}[name])
    n = 60
    if name == "null":        # p-values above the uniform grid: every q is 1, pi0 = 1 and pi = 0 exactly
        import scipy.stats as st
        sign = np.where(np.arange(n) % 3 == 0, -1.0, 1.0)
        t = st.t.isf(np.minimum(1.0, 1.3 * np.arange(1, n + 1) / n) / 2, 9.0)
        t[np.abs(t) < 1e-12] = 0.0            # (p = 1: t is 0 itself, not isf's rounding of it)
        return sign * t, 0.6, 1.1, 9.0
    t = rng.standard_t(12, size=n)
    if name == "tiny":
        t = t * 0.55
        t[0] = 4.2
        return t, 0.5, 0.8, 16.0
    if name == "most":
        return t + np.where(np.arange(n) % 2 == 0, 9.0, -8.0) * (1 + rng.random(n)), 0.4, 1.3, 14.0
    if name == "inf":
        t[:12] += 5.0
        return t, 0.7, 0.9, np.inf
    if name == "nodf0":
        t[:9] -= 6.0
        return t, 0.45, 1.0, 4.0
    if name == "clamp_lo":    # a small prior variance: v0_r of order 1 lies below 0.01 / s0^2 = 10
        t[:15] += 3.5
        return t, 0.5, 0.001, 20.0
    if name == "clamp_hi":    # huge t and a small u: v0_r above 16 / s0^2
        t[:25] *= 400.0
        return t, 0.05, 3.0, 11.0
    t[:15] += 3.5
    return t, 0.5, 1.2, 13.5


SHRINK_CASES = ("null", "tiny", "most", "inf", "nodf0", "clamp_lo", "clamp_hi", "mixed")


def measure_shrink():
    """(worst relative deviation of c, of pi (absolute), per case) of plaidhip_romer_shrink from the 50-digit form"""
    worst = {}
    for name in SHRINK_CASES:
        t, u, s02, nu = shrink_case(name)
        got, prop = engine.romer_shrink(t, u, s02, nu)
        ref, pi, _ = shrink_mp([float(x) for x in t], u, s02, nu)
        dc = max(abs(float((a - b) / b)) for a, b in zip((_mp().mpf(float(x)) for x in got), ref))
        worst[name] = (dc, abs(prop - float(pi)))
    return worst


# ---- keys, ranks, sides, counts, tables in numpy ----------------------------------------------------------------------------------
def keys_np(t, stat):
    """t (any shape) -> (a, b, c) as the header's table; b is None unless floormean; a NaN t is keyed as 0.0"""
    x = np.where(np.isnan(t), 0.0, t) + 0.0
    if stat == "floormean":
        return np.where(x > 0, x, 0.0), np.where(-x > 0, -x, 0.0) + 0.0, np.where(np.abs(x) > 1.0, np.abs(x), 1.0)
    return x, None, np.abs(x)


def rank2_np(key):
    """key: U x K -> 2 rank (int64) of every column, ties averaged"""
    import scipy.stats as st
    if key.shape[0] == 0:
        return np.zeros(key.shape, dtype=np.int64)
    return np.rint(2.0 * st.rankdata(key, method="average", axis=0)).astype(np.int64)


def sides_np(Ra, Rb, Rc, members, stat, nuniv):
    """2 rank matrices (U x K int64) and a set's members (places in the universe) -> K x 3 int64 (Up, Down, Mixed)"""
    m = len(members)
    K = Ra.shape[1]
    a, c = Ra[members], Rc[members]
    flip = 2 * (nuniv + 1)
    if stat == "mean":
        up = a.sum(axis=0)
        return np.column_stack([up, flip * m - up, c.sum(axis=0)]).astype(np.int64)
    if stat == "floormean":
        return np.column_stack([a.sum(axis=0), Rb[members].sum(axis=0), c.sum(axis=0)]).astype(np.int64)
    h = m // 2 + 1
    srt = np.sort(a, axis=0)
    up, low = srt[m - h:].sum(axis=0), srt[:h].sum(axis=0)
    mixed = np.sort(c, axis=0)[m - h:].sum(axis=0)
    return np.column_stack([up, flip * h - low, mixed]).astype(np.int64).reshape(K, 3)


def finish_np(cnt, msize, nrot, stat="mean"):
    """cnt sets x 3, msize per set -> sets x 7"""
    cnt = np.asarray(cnt, dtype=np.float64)
    m = np.asarray(msize, dtype=np.float64)
    out = np.full((len(m), 7), np.nan)
    has = (m >= 1) & ~((stat == "mean50") & (m > MEAN50_MAX))
    out[:, 0] = m
    for e in range(3):
        pv = np.where(has, (cnt[:, e] + 1.0) / (nrot + 1.0), np.nan)
        out[:, 1 + e] = pv
        out[:, 4 + e] = lr.bh(pv)
    return out


# ---- end to end at 50 digits ---------------------------------------------------------------------------------------------------------
def _key_interval(lo, hi, which, stat):
    """the interval of key `which` (0 a, 1 b, 2 c) over t in [lo, hi]"""
    if which == 2 or stat == "floormean":
        if which == 2:
            a_lo = 0 if lo <= 0 <= hi else min(abs(lo), abs(hi))
            a_hi = max(abs(lo), abs(hi))
            return (max(a_lo, 1), max(a_hi, 1)) if stat == "floormean" else (a_lo, a_hi)
        if which == 1:
            lo, hi = -hi, -lo
        return max(lo, 0), max(hi, 0)
    return lo, hi


def _rank2_exact(vals):
    n = len(vals)
    return [2 * sum(1 for w in vals if w < v) + sum(1 for w in vals if w == v) + 1 for v in vals]


def _decidable(ts, allow, twins, stat):
    """asserts the module docstring's condition for one column: ts (mp) and allow (mp, 0 for an exact value) per universe gene;
    twins: a label per gene, equal for duplicated rows"""
    n = len(ts)
    for which in ((0, 1, 2) if stat == "floormean" else (0, 2)):
        iv = [_key_interval(t - a, t + a, which, stat) for t, a in zip(ts, allow)]
        order = sorted(range(n), key=lambda i: iv[i][0])
        reach, holder = None, None
        for i in order:
            lo, hi = iv[i]
            if reach is not None and lo <= reach:
                j = holder
                point = lo == hi and iv[j][0] == iv[j][1] == lo
                assert point or twins[i] == twins[j], f"keys of genes {j} and {i} are not decided: {iv[j]} {iv[i]}"
            if reach is None or hi > reach:
                reach, holder = hi, i
    return True


def romer_mp(X, D, use, K, sets, W, stat="mean", shrink_resid=True, shrink=None, twins=None):
    """one fit, 50 digits from X: per contrast dict(cnt sets x 3, msize, obs sets x 3, rot sets x nrot x 3 (int64), U, pi).  Asserts
    the decidability of its own case (module docstring).  shrink: given factors per gene (floats), or None"""
    mp = _mp()
    des = lr.mp_design(D, use, K)
    fits = lr.mp_fit(X, des)
    fin = lr.mp_finish(fits, des)
    sel, d, nrot = des["sel"], des["nf"] - des["p"], W.shape[1]
    univ = [g for g, r in enumerate(fin["rows"]) if r is not None]
    place = {g: i for i, g in enumerate(univ)}
    nu = len(univ)
    fs = [[place[g] for g in s if g in place] for s in sets]
    zero_row = {g for g in univ if not np.any(np.asarray(X)[g, sel] != 0.0)}
    tw = [g if twins is None or g not in twins else twins[g] for g in univ]
    Wm = [[mp.mpf(float(W[0, k]))] + [mp.mpf(float(W[c + 1, k])) for c in sel] for k in range(nrot)]
    res = {}
    for g in univ:
        xm = [mp.mpf(float(t)) for t in np.asarray(X)[g, sel]]
        res[g] = [a - mp.fsum(q[c] * e for q, e in zip(des["Q"], fits[g][0])) for c, a in enumerate(xm)]
    az = mp.mpf(FACTOR * rr.MEASURED["z"])
    df_total = mp.inf if fin["df_prior"] == mp.inf else fin["df_prior"] + d
    out = []
    for j, uj in enumerate(des["u"]):
        tobs = [fin["rows"][g]["t"][j] for g in univ]
        eps_c, pi = mp.mpf(0), 0.0
        if shrink is not None:
            cs = [mp.mpf(float(shrink[g])) for g in univ]
        elif shrink_resid and nu > 0:
            cs, pim, margin = shrink_mp(tobs, uj, fin["s2_prior"], df_total)
            assert margin > 1e-6, "ntarget = ceil(pi / 2 U) is too close to a step"
            c2, _, _ = shrink_mp([float(t) for t in tobs], uj, fin["s2_prior"], df_total)
            sens = max(abs((a - b) / b) for a, b in zip(c2, cs))
            eps_c = mp.mpf(FACTOR * MEASURED["shrink"]) + az / mp.mpf(U) * sens
            pi = float(pim)
        else:
            cs = [mp.mpf(1)] * nu
        tcols = [tobs]
        acols = [[mp.mpf(0) if g in zero_row else 2 * az * max(1, abs(t)) for g, t in zip(univ, tobs)]]
        for k in range(nrot):
            tk, ak = [], []
            for i, g in enumerate(univ):
                beta = fin["rows"][g]["logFC"][j] / uj * cs[i]
                dot = mp.fsum(a * b for a, b in zip(res[g], Wm[k][1:]))
                t = rr.moderated_mp(beta * Wm[k][0] + dot, beta, fits[g][2], mp.mpf(d), fin["df_prior"], fin["s2_prior"])
                b2 = beta * (1 + eps_c)
                t2 = rr.moderated_mp(b2 * Wm[k][0] + dot, b2, fits[g][2], mp.mpf(d), fin["df_prior"], fin["s2_prior"])
                tk.append(t)
                ak.append(mp.mpf(0) if g in zero_row else 2 * (az * max(1, abs(t)) + abs(t2 - t)))
            tcols.append(tk)
            acols.append(ak)
        sides = np.zeros((len(sets), nrot + 1, 3), dtype=np.int64)
        for k, (tk, ak) in enumerate(zip(tcols, acols)):
            assert all(mp.isfinite(t) for t in tk), "a t that is not finite"
            _decidable(tk, ak, tw, stat)
            x = [t + 0 for t in tk]
            if stat == "floormean":
                ka, kb, kc = [max(v, 0) for v in x], [max(-v, 0) for v in x], [max(abs(v), 1) for v in x]
            else:
                ka, kb, kc = x, x, [abs(v) for v in x]
            Ra, Rb, Rc = (np.array(_rank2_exact(v), dtype=np.int64)[:, None] for v in (ka, kb, kc))
            for s, mem in enumerate(fs):
                if mem:
                    sides[s, k] = sides_np(Ra, Rb, Rc, mem, stat, nu)[0]
        cnt = (sides[:, 1:, :] >= sides[:, :1, :]).sum(axis=1)
        msize = np.array([len(v) for v in fs], dtype=np.float64)
        cnt[msize == 0] = 0
        out.append({"cnt": cnt, "msize": msize, "obs": sides[:, 0], "rot": sides[:, 1:], "U": nu, "pi": pi})
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def e2e_case(name):
    """X (genes x samples), D, use, K, sets, W, twins: small, with a NaN gene (outside the universe), an all-zero gene (exact
    zeros on every path), a duplicated gene (exact ties), the empty set and a set whose only gene is outside the universe"""
    g, n, p, seed, nrot = {"a": (40, 12, 2, 7, 70), "b": (38, 12, 5, 11, 40), "wide": (36, 135, 2, 5, 40)}[name]
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(g, n)) + 0.9 * np.outer(rng.normal(size=g) * (rng.random(g) < 0.4), np.arange(n) % 2)
    X = np.round(X * 64) / 64
    D = rr.make_design(n, p, rng)
    use = None
    if name == "b":
        use = np.ones(n, dtype=np.int8)
        use[[2, 9]] = 0
        X[3, 2] = np.nan                       # a NaN where the fit does not look
    X[g - 1, 1] = np.nan                       # a gene outside the universe
    X[2, :] = 0.0                              # a constant gene: exact zeros
    X[5, :] = X[4, :]                          # a duplicated gene
    K = np.zeros((p, 1))
    K[1, 0] = 1.0
    pool = [i for i in range(g) if i != g - 1]
    sets = [list(rng.choice(pool, size=k, replace=False)) for k in (1, 2, 3, 7, 12)] + [[], [g - 1], list(range(g)), [2, 4, 5, 9]]
    W = engine.roast_rotations(D, use, 0, nrot, seed)
    return X, D, use, K, sets, W, {5: 4}


E2E_CASES = ("a", "b", "wide")
_REF = {}


def given_shrink(name):
    """factors for the `shrink` argument of a case: one per gene, in (0.3, 1]"""
    g = e2e_case(name)[0].shape[0]
    c = 0.3 + 0.7 * np.random.default_rng(99).random(g)
    c[5] = c[4]                                # (the duplicated gene stays one)
    return c


def e2e_reference(name, stat, mode="shrunk"):
    """mode: "shrunk" (shrink.resid = TRUE), "plain" (FALSE) or "given" (given_shrink)"""
    key = (name, stat, mode)
    if key not in _REF:
        X, D, use, K, sets, W, twins = e2e_case(name)
        _REF[key] = romer_mp(X, D, use, K, sets, W, stat, shrink_resid=mode == "shrunk",
                             shrink=given_shrink(name) if mode == "given" else None, twins=twins)
    return _REF[key]


def pattern(sets):
    return rr.pattern(sets)


# ---- the sharding hook ------------------------------------------------------------------------------------------------------------
def run_sharded(nshards, X, design, Gp, Gi, use=None, contrasts=None, fail=-1, **kw):
    """(status, out, hyper) of plaid.romer on `nshards` contexts of one device; the results hold -7 before the call"""
    X = np.asfortranarray(X, dtype=np.float64)
    Dd, _, _, q = engine.limma_operands(X.shape[1], design, use, contrasts)
    out = np.full((len(Gp) - 1, 7, q, Dd.shape[2]), -7.0, order="F")
    hyper = np.full((Dd.shape[2], 8 + q), -7.0)
    status, _ = _status(lambda: engine._romer(hook("romer"), (0, nshards, fail), X, design, Gp, Gi, use, contrasts, out=out,
                                              hyper=hyper, **kw))
    return status, out, hyper


if __name__ == "__main__":
    print(measure_shrink())
