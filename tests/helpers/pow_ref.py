"""The rank weights r^p of the scorers that take an exponent (replaid.ssgsea, replaid.gsva, the exact scorers), held to
exact powers over EVERY value a rank can take (host only, no GPU).

A rank is a half-integer, and a ranker that takes g rows can produce every half-integer in [1, g] and nothing else: the
domain of the weight routines is finite (393,215 values up to the partitioned ranker's 196,608 rows), so they are tested
exhaustively, not sampled.  u = 2^-53 throughout; an error "in u" is |got - exact| / (u exact).

Three pieces of device code produce the weights (plaid_amd/csrc/rank_bucket.h, kernels_rank.hip):

  pow_quarters   4p an integer q in 1..16 (p != 1), bucket and partitioned rankers, expand_sparse_ranks_kernel, walk_pow,
                 gsva_ks_table_kernel: r^(q >> 2) by square-and-multiply, times sqrt(r) (q & 2), times sqrt(sqrt(r))
                 (q & 1); (q & 3) == 1 takes the hand-written root4_pos instead of the two square roots
  pow()          the same kernels for any other exponent
  pow()          the sorting-network kernels, for every exponent

pow_allowance_u() is the bound on one weight's error that the suite's derived bounds build on.  For the quarters it is
COUNTED from the code: one u per inexact product or square root, an error halves through a square root, and r, r^2 and
1.0 * x are exact because a rank has at most 19 significant bits (r^2 at most 38; r^3 and r^4 round once):

    q          1    2    3    4   5     6   7    8   9     10  11   12  13    14  15   16
    derived u  rho  1    3.5  0   rho+1 2   4.5  0   rho+1 2   4.5  1   rho+2 3   5.5  1

(re-derived here from pow_quarters as it stands: the counts are the ones the table states).  rho is root4_pos's own
allowance, RHO_U = 2 u, asserted directly on the device by tests/test_gpu_rank_weights.py.  pow() keeps the project's
3 u (POW_LIBM_U), there as a claim under test.
"""
from __future__ import annotations

import numpy as np

ld = np.longdouble
assert np.finfo(ld).eps == 2.0 ** -63, "the references need x87 extended precision (long double with a 64-bit significand)"
U = 2.0 ** -53
G_MAX = 196608            # kPartMax * kPartTarget: the longest column any ranker with a fused power takes
RHO_U = 2.0               # root4_pos against the exact r^(1/4)
POW_LIBM_U = 3.0          # pow() against the exact r^p
LD_SLACK_U = 0.01         # on top of every comparison: the long-double reference's own 2^-64 is 0.0005 u per operation
GENERIC_POWERS = (0.1, 0.3, 0.7, 1.3, 1.9, 2.6, 4.25)      # 4.25: 4p = 17, past the quarter table, so pow()

_DERIVED = {1: (1, 0.0), 2: (0, 1.0), 3: (0, 3.5), 4: (0, 0.0), 5: (1, 1.0), 6: (0, 2.0), 7: (0, 4.5), 8: (0, 0.0),
            9: (1, 1.0), 10: (0, 2.0), 11: (0, 4.5), 12: (0, 1.0), 13: (1, 2.0), 14: (0, 3.0), 15: (0, 5.5), 16: (0, 1.0)}


def quarter_of(p):
    """q = 4p when the device takes pow_quarters for the fp64 exponent p (launch_ranks' decode), else 0"""
    p = float(p)
    q4 = p * 4.0
    return int(q4) if (p != 1.0 and 1.0 <= q4 <= 16.0 and q4 == float(int(q4))) else 0


def quarters_allowance_u(q, rho=RHO_U):
    """the derived count for pow_quarters(r, q), q in 1..16 (q = 4 and 8 are exact)"""
    n_rho, rest = _DERIVED[int(q)]
    return n_rho * float(rho) + rest


def pow_allowance_u(p, route="any", rho=RHO_U):
    """The allowance, in u, for one device weight r^p.

    route = "quarters": pow_quarters' derived count (p must be a quarter exponent);  "pow": pow()'s 3 u;
    "any" (what a scorer's bound takes): the larger of the routes a column of any length can meet -- a quarter exponent
    goes through pow_quarters in the bucket and partitioned rankers but through pow() in the sorting network (columns of at
    most 256 rows, and clustered columns the bucket ranker hands over).  p = 1 is exact on every route."""
    p = float(p)
    if p == 1.0:
        return 0.0
    q = quarter_of(p)
    if route == "pow" or (q == 0 and route == "any"):
        return POW_LIBM_U
    if q == 0:
        raise ValueError(f"{p} is no quarter exponent")
    a = quarters_allowance_u(q, rho)
    return a if route == "quarters" else max(a, POW_LIBM_U)


# ------------------------------------------------------------------ the domain
def half_integer_ranks(g=G_MAX):
    """every value an average rank of a g-row column can take: 1, 1.5, ..., g"""
    return 0.5 * np.arange(2, 2 * int(g) + 1, dtype=np.float64)


def rank_domain_columns(g, seed=0):
    """A g x 3 Fortran matrix whose average ranks are every half-integer in [1, g]: column 0 holds g distinct values (ranks
    1..g), column 1 tied pairs floor(i / 2) (1.5, 3.5, ...), column 2 a single value, then tied pairs floor((i + 1) / 2)
    (1, 2.5, 4.5, ...).  The values are the small integers themselves, evenly spread (a clustered column would make the
    bucket ranker hand the column to the sorting network, which has another power routine); the rows of every column
    are permuted.  Asserted here: the oracle's ranks of the three columns are exactly {1, 1.5, ..., g}."""
    from oracle import c_oracle
    g = int(g)
    rng = np.random.default_rng(seed)
    i = np.arange(g, dtype=np.int64)
    X = np.empty((g, 3), dtype=np.float64, order="F")
    for c, v in enumerate((i, i // 2, (i + 1) // 2)):
        X[:, c] = v[rng.permutation(g)].astype(np.float64)
    got = np.unique(c_oracle.colranks_dense(X, "average", False))
    assert np.array_equal(got, half_integer_ranks(g)), "the three columns must produce every half-integer rank in [1, g]"
    return X


# ------------------------------------------------------------------ pow_quarters in numpy
def quarters_emulated(r, q, root4=None):
    """pow_quarters(r, q)'s operation sequence in numpy fp64 (IEEE products, correctly rounded sqrt): the device's bits
    for (q & 3) != 1.  (q & 3) == 1 multiplies by `root4`, the fourth roots the caller supplies (the device's own q = 1
    output, or sqrt(sqrt(r)) as a stand-in)."""
    r = np.asarray(r, dtype=np.float64)
    q = int(q)
    res, base = np.ones_like(r), r.copy()
    e = q >> 2
    while e:
        if e & 1:
            res = res * base
        base = base * base
        e >>= 1
    if (q & 3) == 1:
        if root4 is None:
            raise ValueError("(q & 3) == 1 needs the fourth roots")
        return res * np.asarray(root4, dtype=np.float64)
    if q & 3:
        s = np.sqrt(r)
        if q & 2:
            res = res * s
        if q & 1:
            res = res * np.sqrt(s)
    return res


def root4_sqrt_sqrt(r):
    """sqrt(sqrt(r)) in fp64: what root4_pos claims to be within 1 ulp of"""
    return np.sqrt(np.sqrt(np.asarray(r, dtype=np.float64)))


# ------------------------------------------------------------------ exact powers
def exact_power(r, p):
    """r^p in long double, p the fp64 exponent the device receives (0.3 is fl(0.3), not 3/10)"""
    return np.power(np.asarray(r, dtype=np.float64).astype(ld), ld(np.float64(p)))


def exact_power_mp(r, p, digits=50):
    """the same at `digits` decimal digits (mpmath), rounded to long double: for any subset, to check exact_power"""
    import mpmath
    out = np.empty(len(r), dtype=ld)
    with mpmath.workdps(digits):
        pe = mpmath.mpf(float(np.float64(p)))
        for k, x in enumerate(np.asarray(r, dtype=np.float64)):
            v = mpmath.power(mpmath.mpf(float(x)), pe)
            hi = float(v)                                   # head and tail: 106 bits, more than long double holds
            out[k] = ld(hi) + ld(float(v - mpmath.mpf(hi)))
    return out


def err_u(got, exact):
    """|got - exact| / (u exact), elementwise, in fp64 (the difference is taken in long double)"""
    exact = np.asarray(exact, dtype=ld)
    return (np.abs(np.asarray(got, dtype=np.float64).astype(ld) - exact) / (exact * ld(U))).astype(np.float64)


def ulp_distance(a, b):
    """|a - b| in units in the last place, for positive finite doubles (their bit patterns are ordered integers)"""
    a = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float64).view(np.int64)
    return np.abs(a - b)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.int64),
                          np.ascontiguousarray(b, dtype=np.float64).view(np.int64))


# ------------------------------------------------------------------ what a quarter route has to satisfy
def check_quarter_route(r, weights, exact=None, rho=RHO_U, collect=False):
    """The assertions every pow_quarters route is held to, on the weights it gave at the ranks r.

    weights: {q: array over r} for the q in 1..16 that were run (q = 4 is p = 1: the plain ranks), q = 1 among them.
    exact: {q: exact_power(r, q / 4)} when the caller caches them.  Every claim is evaluated; the first that failed is
    raised as an AssertionError (collect = True: none is raised and the figures carry "failed", {claim: message}).
    Returns the figures met.

      (1) q = 4 (power = 1): the ranks themselves
      (2) (q & 3) != 1: the bits of quarters_emulated
      (3) q = 1 is root4_pos itself (res = 1.0): at most 1 ulp from sqrt(sqrt(r)), and within rho u of the exact r^(1/4)
      (4) q = 5, 9, 13: the bits of quarters_emulated with the route's own q = 1 output -- an identity of the code
      (6) every weight within quarters_allowance_u(q) (+ the long-double slack) of the exact power"""
    r = np.asarray(r, dtype=np.float64)
    root4 = np.ascontiguousarray(weights[1], dtype=np.float64)
    failed = {}
    fig = {"root4_ulp_vs_sqrt_sqrt": int(ulp_distance(root4, root4_sqrt_sqrt(r)).max()), "err_u": {}, "ratio": 0.0,
           "failed": failed}
    if fig["root4_ulp_vs_sqrt_sqrt"] > 1:
        failed.setdefault(3, f"root4_pos is {fig['root4_ulp_vs_sqrt_sqrt']} ulp from sqrt(sqrt(r)) (the header's claim: 1)")
    for q in sorted(weights):
        w = np.ascontiguousarray(weights[q], dtype=np.float64)
        if q == 4:
            if not same_bits(w, r):
                failed.setdefault(1, "power = 1 must return the ranks themselves")
            continue
        if (q & 3) != 1:
            emu = quarters_emulated(r, q)
            bad = np.flatnonzero(w.view(np.int64) != emu.view(np.int64))
            if bad.size:
                failed.setdefault(2, f"q = {q}: {bad.size} weights differ from pow_quarters' operation sequence, first at "
                                     f"r = {r[bad[0]]}: {w[bad[0]]!r} != {emu[bad[0]]!r}")
        elif q != 1 and not same_bits(w, quarters_emulated(r, q, root4)):
            failed.setdefault(4, f"q = {q}: not res * root4_pos(r) with the route's own fourth roots")
        ex = exact[q] if exact is not None else exact_power(r, q / 4.0)
        e = float(err_u(w, ex).max())
        allow = quarters_allowance_u(q, rho)
        fig["err_u"][q] = e
        if not e <= allow + LD_SLACK_U:
            failed.setdefault(3 if q == 1 else 6, f"q = {q}: {e:.3f} u from the exact power, allowance {allow} u")
        if allow > 0:
            fig["ratio"] = max(fig["ratio"], e / allow)
    if failed and not collect:
        k = min(failed)
        raise AssertionError(f"claim ({k}): {failed[k]}")
    return fig
