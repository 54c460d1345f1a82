"""The device's rank weights r^p against exact powers, over every rank a column can hold (`pytest -m gpu -s`).

Every scorer with an exponent turns a rank into r^p by pow_quarters (4p an integer in 1..16: square roots, products and
the hand-written root4_pos), or by pow().  The derived fp64 bounds of the suite rest on an allowance for ONE such weight
(tests/helpers/pow_ref.py: pow_allowance_u), which the bound tests see only through sums of dozens of terms.  Here the
weights are read directly: dev_colranks_dense(power = p) on three columns whose average ranks are every half-integer in
[1, g], for every kernel a column can reach and at the edges of its range, ldr > g with guard values behind every column.

Per route and exponent, in order of strength:
  (1) power = 1: the bits of the oracle's ranks; the guards are intact (every call)
  (2) quarters, (q & 3) != 1: the bits of pow_quarters' operation sequence in numpy (a contraction, a wrong branch of the
      decode of q, or a route that silently took pow() all show)
  (3) q = 1 is root4_pos itself: at most 1 ulp from sqrt(sqrt(r)), and within rho = 2 u of the exact r^(1/4)
  (4) q = 5, 9, 13: the bits of res * (the route's own q = 1 output)
  (5) every quarter route gives the bits of every other on the ranks they share (one inline function)
  (6) every weight within pow_allowance_u of the exact power (long double, checked against 50 digits on the host); the
      domain is exhaustive for the quarters, so nothing is added but the reference's 0.01 u
  (7) pow(): exponents are sampled though ranks are not, so the largest error over all listed exponents plus 1 u has to
      fit the 3 u (the rule of DESIGN.md 6.1)
  (8) signed = TRUE with random signs: -w and +w with the bits of the unsigned weights
  (9) colmax[c]: the bits of the largest |weight| written to column c

Measured on an MI355X (largest over all routes and every rank up to 196,608; u = 2^-53 relative to the exact power):
  root4_pos      1 ulp from sqrt(sqrt(r)); 1.479 u from r^(1/4) (1.448 u up to rank 20,352), rho = 2
  pow_quarters   q: u   1: 1.48  2: 1.00  3: 3.29  5: 2.31  6: 1.93  7: 3.90  8: 0  9: 2.30  10: 1.99  11: 3.96  12: 1.00
                        13: 3.00  14: 2.53  15: 3.96  16: 1.00 -- the same on every quarter route; largest error /
                        allowance 1.000 (q = 12 and 16: one rounding against an allowance of one)
  pow()          1.997 u in the sorting-network kernels (22 exponents), 1.979 u in the bucket and partitioned rankers'
                 generic loop (7 exponents); + 1 u = 2.997 <= 3
"""
import numpy as np
import pytest

from tests.helpers import pow_ref as pr

pytestmark = pytest.mark.gpu

GUARD = -7.0
QUARTER_POWERS = tuple(q / 4.0 for q in range(1, 17))
ALL_POWERS = QUARTER_POWERS + pr.GENERIC_POWERS

# (rank_kernel option, rows, the kernel the column reaches, pow_quarters for quarter exponents?)
NETWORK = [("network", g, k, False) for g, k in
           [(256, "colranks_f64_kernel<false>"), (2049, "colranks_f64_kernel<false>"), (8192, "colranks_f64_kernel<false>"),
            (8193, "colranks_regs_kernel"), (20448, "colranks_regs_kernel"),
            (20449, "colranks_f64_kernel<true>"), (196608, "colranks_f64_kernel<true>")]]
QUARTERS = [("bucket", 2048, "bucket<256,8>", True), ("bucket", 4096, "bucket<256,16>", True),
            ("bucket", 8192, "bucket<512,16>", True), ("bucket", 12288, "bucket<512,24>", True),
            ("bucket", 20352, "bucket<1024,20>", True), ("bucket512", 20352, "bucket<512,40>", True),
            ("auto", 20353, "partitioned", True), ("auto", 131072, "partitioned", True), ("auto", 196608, "partitioned", True)]
ROUTES = NETWORK + QUARTERS
_id = lambda rt: f"{rt[0]}-{rt[1]}"

_cache = {}


def _exact(p, g):
    """exact_power over the ranks 1, 1.5, ..., g: computed once per exponent for the whole domain, then sliced"""
    key = ("exact", float(p))
    if key not in _cache:
        _cache[key] = pr.exact_power(pr.half_integer_ranks(), p)
    return _cache[key][:2 * g - 1]


def _columns(g):
    """(X, oracle ranks, k = index of every element's rank in 1, 1.5, ..., g), once per g"""
    from oracle import c_oracle
    key = ("cols", g)
    if key not in _cache:
        X = pr.rank_domain_columns(g, seed=g)
        R = c_oracle.colranks_dense(X, "average", False)
        _cache[key] = (X, R, np.rint(2.0 * R - 2.0).astype(np.int64))
    return _cache[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


class _Dev:
    """device copies of one matrix, column-major with ldx > g, and the result buffers with guards behind every column"""

    def __init__(self, X):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.g, self.n = X.shape
        self.ldx, self.ldr = self.g + 3, self.g + 5
        self.X = torch.full((self.n, self.ldx), 1e300, dtype=torch.float64, device=self.dev)
        self.X[:, :self.g] = torch.from_numpy(np.ascontiguousarray(X.T)).to(self.dev)
        self.R = torch.empty((self.n, self.ldr), dtype=torch.float64, device=self.dev)
        self.cm = torch.empty(self.n, dtype=torch.float64, device=self.dev)

    def ranks(self, ctx, power, signed=False):
        """(weights g x n, colmax) of dev_colranks_dense(ties = average); asserts the guards"""
        self.R.fill_(GUARD)
        self.cm.fill_(GUARD)
        self.torch.cuda.synchronize()
        ctx.dev_colranks_dense(self.X.data_ptr(), self.ldx, self.g, self.n, self.R.data_ptr(), self.ldr, "average", signed,
                               float(power), self.cm.data_ptr())
        ctx.synchronize()
        Rh = self.R.cpu().numpy()
        assert np.all(Rh[:, self.g:] == GUARD), "a rank kernel wrote behind a column"
        return np.ascontiguousarray(Rh[:, :self.g].T), self.cm.cpu().numpy()


def _per_rank(W, k, g, what):
    """the weight of every rank 1, 1.5, ..., g from the g x 3 result (every element of one rank must carry the same bits)"""
    out = np.empty(2 * g - 1, dtype=np.float64)
    out[k.ravel()] = W.ravel()
    assert np.array_equal(_bits(out[k]), _bits(W)), f"{what}: two elements of one rank got different weights"
    return out


def _colmax_is_largest_written(W, cm, what):
    assert np.array_equal(_bits(cm), _bits(np.abs(W).max(axis=0))), f"{what}: colmax {cm!r} is not the largest |weight| written"


def _pow_figures(r, weights, g):
    """claims (1), (6), (7) for weights that came from pow(): {p: per-rank weights}.  Returns the largest error in u"""
    worst = 0.0
    for p, w in weights.items():
        if p == 1.0:
            assert np.array_equal(_bits(w), _bits(r)), "power = 1 must return the ranks themselves"
            continue
        e = float(pr.err_u(w, _exact(p, g)).max())
        assert e <= pr.pow_allowance_u(p, "pow") + pr.LD_SLACK_U, f"pow(r, {p}): {e:.3f} u from the exact power"
        worst = max(worst, e)
    assert worst + 1.0 <= pr.POW_LIBM_U, (f"pow(): largest error over the sampled exponents {worst:.3f} u; + 1 u for the "
                                          f"exponents not sampled exceeds the {pr.POW_LIBM_U} u allowance")
    return worst


def _canonical_root4(pinned_ctx):
    """root4_pos over the whole domain, as the partitioned ranker at 196,608 rows gives it (q = 1): what every other
    quarter route is compared with on the ranks it shares (5), and the fourth roots of the CSC cases"""
    if "root4" not in _cache:
        g = pr.G_MAX
        X, R, k = _columns(g)
        W, _ = _Dev(X).ranks(pinned_ctx(rank_kernel="auto"), 0.25)
        _cache["root4"] = _per_rank(W, k, g, "canonical q = 1")
    return _cache["root4"]


@pytest.mark.parametrize("route", ROUTES, ids=_id)
def test_weights_of_every_rank(pinned_ctx, route):
    option, g, kernel, quarters = route
    X, R, k = _columns(g)
    r = pr.half_integer_ranks(g)
    ctx = pinned_ctx(rank_kernel=option)
    d = _Dev(X)
    per = {}
    for p in ALL_POWERS:
        W, cm = d.ranks(ctx, p)
        what = f"{kernel} g = {g} p = {p}"
        _colmax_is_largest_written(W, cm, what)                                  # (9)
        per[p] = _per_rank(W, k, g, what)
    if quarters:
        canon = _canonical_root4(pinned_ctx)
        wq = {q: per[q / 4.0] for q in range(1, 17)}
        fig = pr.check_quarter_route(r, wq, {q: _exact(q / 4.0, g) for q in range(1, 17)})     # (1) (2) (3) (4) (6)
        for q in (1, 5, 9, 13):                                                  # (5)
            want = pr.quarters_emulated(r, q, canon[:2 * g - 1])
            assert np.array_equal(_bits(wq[q]), _bits(want)), f"{kernel} g = {g}: q = {q} differs from the partitioned ranker's bits"
        worst_pow = _pow_figures(r, {p: per[p] for p in pr.GENERIC_POWERS}, g)   # (6) (7): the same kernels' pow()
        errs = " ".join(f"{q}:{fig['err_u'][q]:.2f}" for q in sorted(fig["err_u"]))
        print(f"\n{kernel} g = {g}: root4_pos {fig['root4_ulp_vs_sqrt_sqrt']} ulp from sqrt(sqrt(r)), {fig['err_u'][1]:.3f} u "
              f"from r^(1/4) (rho = {pr.RHO_U}); quarters u per q {errs}; largest error / allowance {fig['ratio']:.3f}; "
              f"pow() {worst_pow:.3f} u (+ 1 <= {pr.POW_LIBM_U})")
    else:
        worst_pow = _pow_figures(r, per, g)                                      # (1) (6) (7): pow() for every exponent
        print(f"\n{kernel} g = {g}: pow() over {len(per) - 1} exponents {worst_pow:.3f} u (+ 1 <= {pr.POW_LIBM_U}); "
              f"largest error / allowance {worst_pow / pr.POW_LIBM_U:.3f}")


@pytest.mark.parametrize("route", ROUTES, ids=_id)
def test_signed_weights_carry_the_unsigned_bits(pinned_ctx, route):
    """(8): the same columns moved up by one (no zero among them: a zero's signed weight is 0) with random signs; signed
    ranks are the ranks of |x|, so -w and +w must carry the unsigned weights' bits; (9) for the signed call"""
    option, g, kernel, _ = route
    X, R, k = _columns(g)
    rng = np.random.default_rng(g + 1)
    sign = np.where(rng.random(X.shape) < 0.5, -1.0, 1.0)
    ctx = pinned_ctx(rank_kernel=option)
    plain, signed = _Dev(X), _Dev((X + 1.0) * sign)
    for p in (1.25, 1.3):
        W, _ = plain.ranks(ctx, p)
        S, cm = signed.ranks(ctx, p, signed=True)
        assert np.array_equal(_bits(S), _bits(sign * W)), f"{kernel} g = {g} p = {p}: signed weights are not +-(unsigned weights)"
        _colmax_is_largest_written(S, cm, f"{kernel} g = {g} p = {p} signed")


def _check_elements(W, R, p, canon, what):
    """the claims for weights given element by element (the CSC entries): R the oracle's ranks of the same elements"""
    k = np.rint(2.0 * R - 2.0).astype(np.int64)
    q = pr.quarter_of(p)
    if p == 1.0:
        assert np.array_equal(_bits(W), _bits(R)), what
        return 0.0
    if q:
        emu = pr.quarters_emulated(R, q, canon[k] if (q & 3) == 1 else None)
        assert np.array_equal(_bits(W), _bits(emu)), f"{what}: not pow_quarters' bits"
    e = float(pr.err_u(W, pr.exact_power(R, p)).max())
    allow = pr.pow_allowance_u(p, "quarters" if q else "pow")
    assert e + (0.0 if q else 1.0) <= allow + (pr.LD_SLACK_U if q else 0.0), f"{what}: {e:.3f} u, allowance {allow} u"
    return e / allow if allow else 0.0


@pytest.mark.parametrize("length", [20352, 20353], ids=["bucket", "partitioned"])
def test_csc_stored_values(pinned_ctx, length):
    """dev_colranks_csc (stored values only): three columns of 20,352 stored values (bucket ranker on CSC columns) and of
    20,353 (one more than it takes: partitioned)"""
    import torch
    from oracle import c_oracle
    dev = torch.device("cuda", 0)
    ctx = pinned_ctx()
    canon = _canonical_root4(pinned_ctx)
    X = pr.rank_domain_columns(length, seed=3)
    Xp = (np.arange(4) * length).astype(np.int32)
    Xx = np.ascontiguousarray(X.T).ravel()
    R = c_oracle.sparse_colranks(Xp, Xx, "average", False)
    dXp, dXx = torch.from_numpy(Xp).to(dev), torch.from_numpy(Xx).to(dev)
    Rx = torch.empty(3 * length + 4, dtype=torch.float64, device=dev)
    cm = torch.empty(3, dtype=torch.float64, device=dev)
    worst = 0.0
    for p in ALL_POWERS:
        Rx.fill_(GUARD)
        torch.cuda.synchronize()
        ctx.dev_colranks_csc(dXp.data_ptr(), dXx.data_ptr(), 3, length, Rx.data_ptr(), "average", False, p, cm.data_ptr())
        ctx.synchronize()
        out = Rx.cpu().numpy()
        assert np.all(out[3 * length:] == GUARD)
        W = out[:3 * length]
        worst = max(worst, _check_elements(W, R, p, canon, f"csc {length} p = {p}"))
        assert np.array_equal(_bits(cm.cpu().numpy()), _bits(W.reshape(3, length).max(axis=1)))
    print(f"\ndev_colranks_csc, {length} stored values: largest error / allowance {worst:.3f}")


def test_csc_dense_result_from_stored_values(pinned_ctx):
    """dev_colranks_csc_dense_nz at 131,072 rows: a column of 20,000 distinct positive stored values (the weights of
    rank + z) and one with negatives and stored zeros (the zero group's average rank), expand_sparse_ranks_kernel"""
    import torch
    import scipy.sparse as sp
    from oracle import c_oracle
    dev = torch.device("cuda", 0)
    ctx = pinned_ctx()
    canon = _canonical_root4(pinned_ctx)
    g, ldr = 131072, 131072 + 6
    rng = np.random.default_rng(17)
    X = np.zeros((g, 2))
    X[rng.choice(g, size=20000, replace=False), 0] = rng.permutation(20000) + 1.0
    rows = rng.choice(g, size=15000, replace=False)
    X[rows, 1] = np.round(rng.normal(0.0, 40.0, size=rows.size))                 # negatives, ties
    Xs = sp.csc_matrix(X)
    Xs.data[Xs.indptr[1]:Xs.indptr[2]:11] = 0.0                                  # stored zeros stay stored
    X = Xs.toarray()
    assert (X[:, 1] < 0).any() and np.diff(Xs.indptr).max() <= 20352
    R = c_oracle.colranks_dense(X, "average", False)
    dXp = torch.from_numpy(Xs.indptr.astype(np.int32)).to(dev)
    dXi = torch.from_numpy(Xs.indices.astype(np.int32)).to(dev)
    dXx = torch.from_numpy(Xs.data.astype(np.float64)).to(dev)
    Rx = torch.empty(Xs.nnz, dtype=torch.float64, device=dev)
    out = torch.empty((2, ldr), dtype=torch.float64, device=dev)
    cm = torch.empty(2, dtype=torch.float64, device=dev)
    worst = 0.0
    for p in ALL_POWERS:
        out.fill_(GUARD)
        torch.cuda.synchronize()
        ctx.dev_colranks_csc_dense_nz(dXp.data_ptr(), dXi.data_ptr(), dXx.data_ptr(), g, 2, int(np.diff(Xs.indptr).max()),
                                      Rx.data_ptr(), out.data_ptr(), ldr, "average", False, p, cm.data_ptr())
        ctx.synchronize()
        oh = out.cpu().numpy()
        assert np.all(oh[:, g:] == GUARD)
        W = np.ascontiguousarray(oh[:, :g].T)
        worst = max(worst, _check_elements(W, R, p, canon, f"csc_dense_nz p = {p}"))
        _colmax_is_largest_written(W, cm.cpu().numpy(), f"csc_dense_nz p = {p}")
    print(f"\ndev_colranks_csc_dense_nz, 131,072 rows: largest error / allowance {worst:.3f}")


@pytest.mark.parametrize("g", [4097, 20353], ids=["bucket", "partitioned"])
def test_ssgsea_exact_operands_carry_the_rankers_weights(pinned_ctx, g):
    """dev_ssgsea_exact_operands: W has the bits of colranks(power = alpha) at that column length (walk_pow)"""
    import torch
    dev = torch.device("cuda", 0)
    ctx = pinned_ctx()
    X, R, k = _columns(g)
    d = _Dev(X)
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
    for alpha in (0.25, 0.75, 0.3):
        want, _ = d.ranks(ctx, alpha)
        Q, W, P = (torch.full((3, g), GUARD, dtype=torch.float64, device=dev) for _ in range(3))
        colnan = torch.full((3,), 7, dtype=torch.int32, device=dev)
        scratch = torch.empty(2 * g * 3, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.dev_ssgsea_exact_operands(dX.data_ptr(), g, g, 3, alpha, Q.data_ptr(), g, scratch.data_ptr(), colnan.data_ptr(),
                                      W.data_ptr(), P.data_ptr())
        ctx.synchronize()
        assert np.array_equal(_bits(W.cpu().numpy().T), _bits(want)), f"g = {g} alpha = {alpha}"
        assert not colnan.cpu().numpy().any()


# ------------------------------------------------------------------ the column maximum of a signed all-zero column
@pytest.mark.parametrize("p", [1.5, 1.3])
@pytest.mark.parametrize("g", [300, 20353])
def test_colmax_of_signed_zero_columns_is_the_same_on_every_route(pinned_ctx, g, p):
    """signed = TRUE writes 0 for a zero, but every route takes the column maximum BEFORE the sign and the zero mask: an
    all-zero column has colmax ((g + 1) / 2)^p, its zeros' common weight -- finite, so 0 / colmax scores 0 (R's 0 / 0 would
    be NaN there).  The bucket ranker's pow() loop used to skip the zeros and left -inf.  Every route must
    give the sorting network's value: the bits of its own unsigned weight of that rank, within the two routines'
    allowances of the network's.  A column with a zero group next to other values: the largest |weight| written."""
    rng = np.random.default_rng(g)
    X = np.zeros((g, 2))
    X[:, 1] = np.round(rng.normal(0.0, 30.0, size=g))
    X[rng.random(g) < 0.3, 1] = 0.0
    assert (X[:, 1] == 0).sum() > 10 and (X[:, 1] < 0).any()
    d = _Dev(X)
    r0 = 0.5 * (g + 1)
    exact = float(pr.exact_power(np.array([r0]), p)[0])
    got = {}
    for option in ("network", "bucket", "auto"):
        ctx = pinned_ctx(rank_kernel=option)
        Wu, _ = d.ranks(ctx, p)                          # unsigned: every zero of column 0 weighs r0^p
        W, cm = d.ranks(ctx, p, signed=True)
        assert np.all(W[:, 0] == 0.0) and np.all(Wu[:, 0] == Wu[0, 0])
        assert _bits(cm[:1])[0] == _bits(Wu[:1, 0])[0], f"{option}: colmax of the all-zero column is {cm[0]!r}, not {Wu[0, 0]!r}"
        assert np.all(W[X[:, 1] == 0.0, 1] == 0.0)
        assert _bits(cm[1:])[0] == _bits(np.abs(W[:, 1]).max(keepdims=True))[0], f"{option}: colmax of the mixed column"
        got[option] = cm.copy()
    allow = pr.pow_allowance_u(p, "pow") + pr.pow_allowance_u(p, "any")
    for option in ("bucket", "auto"):
        assert np.all(np.abs(got[option] - got["network"]) <= allow * pr.U * got["network"]), (option, got)
    assert abs(got["network"][0] - exact) <= pr.POW_LIBM_U * pr.U * exact
    print(f"\nsigned all-zero column, g = {g}, p = {p}: colmax {got['network'][0]!r} on every route (exact {exact!r})")
