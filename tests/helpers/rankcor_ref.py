"""Host restatements of plaid.rankcor (include/plaidhip.h: plaidhip_rankcor).

rankcor_exact is the rank-mode definition on Python ints, rho and t evaluated by mpmath at 50 digits; rankcor_form is the
pinned epilogue, operation for operation, on Python ints and floats (int -> float is correctly rounded, ties to even;
math.sqrt and / are IEEE); rankcor_ref is the whole call on numpy and scipy.stats.rankdata(nan_policy = "omit");
rankcor_scipy is the statistic as a user would write it; ValueList is value mode in exact rational arithmetic with its
derived forward bound."""
import math
from fractions import Fraction

import mpmath
import numpy as np
from scipy.stats import rankdata

from .gsea_perm_ref import bh, make_sets  # noqa: F401  (make_sets: re-exported for the tests)

COLUMNS = ("size", "rho", "t", "p.value", "q.value")
TIES = {"average": 0, "min": 1, "max": 2}
EPS = Fraction(1, 2**53)
NAN = float("nan")


def library_pnorm_upper():
    """the library's own pnorm_upper (the routine behind every normal tail of stats.cpp), through its test export"""
    import ctypes as C

    from plaid_amd import _lib
    f = _lib.load().plaidhip_debug_pvalue
    f.argtypes = [C.c_int, C.c_double, C.c_double]
    f.restype = C.c_double
    return lambda x: f(3, float(x), 0.0)


def z_ranks(x, ties="average"):
    """(z, valid): z = 2 rank of x among its non-NaN entries as Python ints (0 outside), by scipy"""
    x = np.asarray(x, dtype=np.float64)
    ok = ~np.isnan(x)
    z = np.zeros(len(x), dtype=np.int64)
    if ok.any():
        r = rankdata(x, method=ties, nan_policy="omit")
        z[ok] = np.rint(2.0 * r[ok]).astype(np.int64)
    return z, ok


def int_sums(z, ok, mem):
    """(n, T1, T2, k, A) as Python ints from z, the validity of the rows and a set's member rows"""
    zz = [int(v) for v in z[ok]]
    mem = np.asarray(mem, dtype=np.int64)
    inV = mem[ok[mem]] if len(mem) else mem
    return len(zz), sum(zz), sum(v * v for v in zz), int(len(inV)), sum(int(v) for v in z[inV])


def _npq(n, T1, T2, k, A):
    num = n * A - k * T1
    P = k * (n - k) * (n * T2 - T1 * T1)
    return num, P, P - num * num


def rankcor_exact(n, T1, T2, k, A):
    """(rho, t) as mpmath numbers at 50 digits from the exact integers; None where the pinned form gives NaN or +-Inf"""
    if n <= 1 or k <= 0 or k >= n:
        return None, None
    num, P, Q = _npq(n, T1, T2, k, A)
    assert Q >= 0
    if P == 0:
        return None, None
    with mpmath.workdps(50):
        rho = mpmath.mpf(num) / mpmath.sqrt(mpmath.mpf(P))
        t = None
        if n > 2 and Q > 0:
            t = mpmath.sqrt(mpmath.mpf((n - 2) * num * num) / mpmath.mpf(Q)) * (1 if num >= 0 else -1)
        return rho, t


def rankcor_form(n, T1, T2, k, A):
    """(rho, t) of the pinned epilogue, operation for operation, as Python floats"""
    if n <= 1 or k <= 0 or k >= n:
        return NAN, NAN
    num, P, Q = _npq(n, T1, T2, k, A)
    if P == 0:
        return NAN, NAN
    if Q == 0:
        s = -1.0 if num < 0 else 1.0
        return s, (s * math.inf if n > 2 else NAN)
    rho = float(num) / math.sqrt(float(P))
    if n <= 2:
        return rho, NAN
    tsq = (float(n - 2) * float(num * num)) / float(Q)
    return rho, math.copysign(math.sqrt(tsq), float(num))


def value_form_t(rho, n):
    """value mode's t from its rho, operation for operation"""
    if n <= 2 or rho != rho:
        return NAN
    w = (1.0 - rho) * (1.0 + rho)
    if w <= 0.0:
        return math.copysign(math.inf, rho)
    return rho * math.sqrt(float(n - 2) / w)


def gamma(q):
    """gamma_q = q u / (1 - q u), u = 2^-53"""
    return Fraction(q) * EPS / (1 - Fraction(q) * EPS)


def _mp(fr):
    return mpmath.mpf(fr.numerator) / mpmath.mpf(fr.denominator)


class ValueList:
    """value mode of one list in exact rational arithmetic: what depends on the list alone is computed once.  x: the list
    (NaN: not in V; every other entry finite)."""

    def __init__(self, x):
        self.x = np.asarray(x, dtype=np.float64)
        self.ok = ~np.isnan(self.x)
        self.fr = {int(i): Fraction(float(self.x[i])) for i in np.flatnonzero(self.ok)}
        xs = list(self.fr.values())
        self.n = n = len(xs)
        if n == 0:
            return
        self.sum = sum(xs)
        self.mu = self.sum / n
        self.W = sum(v * v for v in xs) - self.sum * self.sum / n          # sum (x - mean)^2, exactly
        # the device's mu is within E_mu of the exact mean: n - 1 additions in some order and one division
        self.Emu = gamma(n) * sum(abs(v) for v in xs) / n
        self.Sa = sum(abs(v - self.mu) for v in xs) + n * self.Emu        # >= sum |x_i - mu_device| over V

    def members(self, mem):
        mem = np.asarray(mem, dtype=np.int64)
        return [int(i) for i in (mem[self.ok[mem]] if len(mem) else mem)]

    def exact(self, mem):
        """(rho as an mpmath number at 50 digits, or None where the statistic is undefined; k)"""
        inV = self.members(mem)
        n, k = self.n, len(inV)
        if n <= 1 or k <= 0 or k >= n or self.W == 0:
            return None, k
        num = sum(self.fr[i] for i in inV) - Fraction(k) * self.sum / n
        with mpmath.workdps(50):
            return _mp(num) / mpmath.sqrt(_mp(Fraction(k * (n - k), n) * self.W)), k

    def bound(self, mem):
        """the forward bound of DESIGN.md section 21 on |rho_hat - rho|: (bound, the largest first-order relative term).
        With d_i = x_i - mu_device exactly (rho does not depend on the shift), u = 2^-53:
            |A_hat - A|   <= gamma_k sum_members |d_i|               (one rounding per d_i, at most k - 1 per sum)
            |T1_hat - T1| <= gamma_n sum_V |d_i|,   |T2_hat - T2| <= gamma_(n+2) sum_V d_i^2
            d_num = gamma_k S_m + (k / n) gamma_(n+2) S_a + u |num|
            d_W   = gamma_(n+2) T2 + (2 |T1| gamma_n S_a + (gamma_n S_a)^2) (1 + 2u) / n + 2u T1^2 / n + u W
            |rho_hat - rho| <= d_num / den + |rho| (d_W / (2 W) + 3.5 u)
        to first order; |T1| <= n E_mu, T2 <= W + n E_mu^2 and the sums of |d_i| are taken around the exact mean and widened
        by E_mu per term.  The factor (1 + 2^-19) covers the products of two first-order terms as long as each is below
        2^-20, which the caller asserts on the second value returned."""
        inV = self.members(mem)
        n, k, mu, Emu = self.n, len(inV), self.mu, self.Emu
        Sm = sum(abs(self.fr[i] - mu) for i in inV) + k * Emu
        num = sum(self.fr[i] - mu for i in inV)                      # (sum_V (x - mu) = 0: the second term vanishes)
        with mpmath.workdps(50):
            den_lo = Fraction(float(mpmath.sqrt(_mp(Fraction(k * (n - k), n) * self.W)))) * (1 - 4 * EPS)
        rho_hi = abs(num) / den_lo
        dnum = gamma(k) * Sm + Fraction(k, n) * gamma(n + 2) * self.Sa + EPS * (abs(num) + k * Emu)
        T1 = n * Emu
        dW = (gamma(n + 2) * (self.W + n * Emu * Emu) + (2 * T1 * gamma(n) * self.Sa + (gamma(n) * self.Sa) ** 2) * (1 + 2 * EPS) / n
              + 2 * EPS * T1 * T1 / n + EPS * self.W)
        bound = (dnum / den_lo + rho_hi * (dW / self.W / 2 + Fraction(7, 2) * EPS)) * (1 + Fraction(1, 2**19))
        return bound, max(dW / self.W, dnum / den_lo)


def rankcor_ref(stat, Gp, Gi, ties="average", pnorm_upper=None):
    """rank mode of plaidhip_rankcor as a whole: (out m x 5 x c, tot c) by scipy's ranks, the integer sums and the pinned
    epilogue; p from `pnorm_upper` (the library's own export) so that it has the library's bits"""
    stat = np.asarray(stat, dtype=np.float64).reshape(len(stat), -1)
    g, c = stat.shape
    m = len(Gp) - 1
    out = np.full((m, 5, c), np.nan, order="F")
    tot = np.zeros(c)
    for l in range(c):
        z, ok = z_ranks(stat[:, l], ties)
        for j in range(m):
            n, T1, T2, k, A = int_sums(z, ok, Gi[Gp[j]:Gp[j + 1]])
            rho, t = rankcor_form(n, T1, T2, k, A)
            out[j, 0:3, l] = k, rho, t
            if t == t:
                out[j, 3, l] = 2.0 * pnorm_upper(abs(t))
        tot[l] = int(ok.sum())
        out[:, 4, l] = bh(out[:, 3, l])
    return out, tot


def rankcor_scipy(stat, Gp, Gi, use_rank=True, ties="average"):
    """the statistic as a user would write it down: corrcoef of the ranks (or the values) with the membership over the
    list's non-NaN genes, t = rho sqrt((n - 2) / (1 - rho^2)), p = 2 pnorm(-|t|), q = BH; (m x 5 x c, c)"""
    from scipy.stats import norm
    stat = np.asarray(stat, dtype=np.float64).reshape(len(stat), -1)
    g, c = stat.shape
    m = len(Gp) - 1
    out = np.full((m, 5, c), np.nan, order="F")
    tot = np.zeros(c)
    for l in range(c):
        ok = ~np.isnan(stat[:, l])
        n = int(ok.sum())
        tot[l] = n
        v = stat[ok, l]
        if use_rank and n:
            v = rankdata(v, method=ties)
        for j in range(m):
            mem = np.zeros(g)
            mem[Gi[Gp[j]:Gp[j + 1]]] = 1.0
            mem = mem[ok]
            k = int(mem.sum())
            out[j, 0, l] = k
            if n < 2 or k == 0 or k == n or np.ptp(v) == 0 or not np.isfinite(v).all():
                continue
            rho = np.corrcoef(v, mem)[0, 1]
            out[j, 1, l] = rho
            if n > 2:
                with np.errstate(divide="ignore"):
                    t = rho * np.sqrt((n - 2) / ((1 - rho) * (1 + rho))) if abs(rho) < 1 else np.copysign(np.inf, rho)
                out[j, 2, l] = t
                out[j, 3, l] = 2.0 * norm.sf(abs(t))
        out[:, 4, l] = bh(out[:, 3, l])
    return out, tot


FIXED_TABLES = [   # (n, k, levels): levels 0 = tie-free, else the number of distinct values
    (3, 1, 0), (3, 2, 0), (4, 2, 0), (10, 3, 0), (10, 5, 2), (64, 1, 0), (65, 64, 0), (1000, 500, 5), (1500, 63, 0),
    (20000, 150, 0), (20000, 19999, 3), (131072, 1, 0), (131072, 65536, 0), (131072, 131071, 0), (131072, 65536, 2),
]


def table_sums(n, k, levels, ties="average", seed=0, extreme=None):
    """(n, T1, T2, k, A) of a list of n genes (tie-free, or `levels` distinct values) and a set of k of them: drawn at
    random, or with extreme = "top" / "bottom" the k highest / lowest (|rho| as large as the ties allow)"""
    rng = np.random.default_rng(seed)
    x = rng.permutation(n).astype(np.float64) if levels == 0 else rng.integers(0, levels, size=n).astype(np.float64)
    z, ok = z_ranks(x, ties)
    if extreme is None:
        mem = rng.choice(n, size=k, replace=False)
    else:
        o = np.argsort(x, kind="stable")
        mem = o[n - k:] if extreme == "top" else o[:k]
    return int_sums(z, ok, mem)


def random_tables(count=300, seed=11, nmax=4000):
    """`count` seeded (n, k, levels, ties): n < nmax, 0 <= k <= n, every third list tie-free, the others of 2 .. 7 levels"""
    rng = np.random.default_rng(seed)
    tabs = []
    for q in range(count):
        n = int(rng.integers(1, nmax))
        k = int(rng.integers(0, n + 1))
        levels = 0 if q % 3 == 0 else int(rng.integers(2, 8))
        tabs.append((n, k, levels, ("average", "min", "max")[q % 3 if levels else 0]))
    return tabs
