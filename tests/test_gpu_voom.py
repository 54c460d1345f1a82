"""plaid.voom on the device (include/plaidhip.h: plaidhip_voom).

  1. library sizes, offsets and the all-zero rows: lib.size is the exact column sum, the offsets are the host's, and the knots
     are plaidhip_lowess's on the trend points of exactly the rows that are not all zero (bit for bit)
  2. log-CPM against correctly rounded values, in ulp
  3. the weights pass follows the header to the bit: the numpy emulation of the chain, the bisection and the interpolation from
     the device's own effects -- with the call's knots, and with a planted table that puts lambda below the first knot, above
     the last, exactly on knots, and on a non-positive trend value
  4. end to end: plaid_voom then plaid_limma(weights = ) against the same pins in numpy / mpmath with their own lowess
  5. a negative count, a NaN count and more than 256 planted knots are EINVAL with nothing written
  6. shards 1, 2, 3 have the one-device bits

Shapes: whole calls at counts (600, 131) with p = 3 and (41, 6) with p = 2; items 3 and 6 also at (300, 40) with p = 9, where
the unweighted fit and the weights pass run their 16-register instances.  plaidhip_dev_voom_weights alone on planted operands
at p = 4, 5, 8, 9, 16, 17, 32 (both ends of every register count), 257 rows (a second workgroup of 256 that holds one row),
129 samples (a column block and a tail of one), ldw = rows + 3 with the padding checked, the mean's row of the effects NaN.
A bad count at rows 39 of 41, and at rows 300 and 599 of 600 (a thread's second and third trip in the check kernel).
"""
import math

import numpy as np
import pytest

import plaid_amd
from plaid_amd import _lib, engine
from tests.helpers import exact_ref as er
from tests.helpers import limma_w_ref as wr
from tests.helpers import voom_ref as vr
from tests.helpers.sharded_hooks import _status, hook

pytestmark = pytest.mark.gpu

CASES = [(600, 131, 3), (41, 6, 2)]
IDS = [f"rows{c[0]}-n{c[1]}-p{c[2]}" for c in CASES]
# one whole call past eight coefficients: the unweighted fit and the weights pass both at their 16-register instance
P9_CASES = [(300, 40, 9)]
P9_IDS = [f"rows{c[0]}-n{c[1]}-p{c[2]}" for c in P9_CASES]
# the planted operands: both ends of every register count of the weights kernel (p <= 4, 8, 16, 32)
PLANTED_P = [4, 5, 8, 9, 16, 17, 32]
# the device's log2 against the correctly rounded value on these inputs, in ulp: measured on the MI355X;
# the test holds it to twice that, never less than 2 ulp and never more than 4
LOG2_ULP_MEASURED = 1.0
LOG2_ULP_BOUND = min(4.0, max(2.0, 2.0 * LOG2_ULP_MEASURED))
# the trend between the device and the reference (item 4): their trend points differ by rounding -- sy to about 1e-12 relative
# (s2 through section 20's rss_bound at these shapes) --, a lowess pass is a linear smoother whose weights have sum |w| <= 4,
# there are four of them, and a robustness weight moves by at most 4 |dres| / cmad: 4^4 times a few units, rounded up to 1e3
TREND_REL = 1e-9
_CACHE = {}


def case_results(ctx, case):
    if case not in _CACHE:
        rows, n, p = case
        counts, D = vr.make_counts(rows, n, p, 28)
        c = dict(counts=counts, D=D, voom=ctx.voom(counts, D))
        c["des"] = engine.limma_design(D)
        c["fit"] = ctx.limma(c["voom"]["E"], D)                  # the unweighted fit of E: its AveExpr is M, its sigma2 is s2
        _CACHE[case] = c
    return _CACHE[case]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_library_sizes_offsets_and_the_trend(hip_ctx, case):
    c = case_results(hip_ctx, case)
    v, counts = c["voom"], c["counts"]
    rows, n, p = case
    assert np.array_equal(v["lib_size"], counts.sum(axis=0))                     # (integers: exact in any order)
    assert np.array_equal(v["offset"], [math.log2(L + 1.0) - math.log2(1e6) for L in v["lib_size"]])
    M, s2 = c["fit"][0][:, 1, 0, 0], c["fit"][0][:, 5, 0, 0]
    ml = 0.0
    for L in v["lib_size"]:
        ml = ml + math.log2(L + 1.0)
    take = (counts.sum(axis=1) != 0) & np.isfinite(s2)
    assert not take[[2, 9, rows - 1]].any() and take.sum() == (counts.sum(axis=1) != 0).sum() >= rows - 8
    sx, sy = (M + (ml / n - math.log2(1e6)))[take], np.sqrt(np.sqrt(s2[take]))
    o = np.argsort(sx, kind="stable")
    x, y = sx[o], sy[o]
    low = engine.lowess(x, y, 0.5, 3, 0.01 * (x[-1] - x[0]))
    kx, ky = vr.knots_of(x, low["ys"], low["anchor"])
    assert np.array_equal(v["knots_x"], kx) and np.array_equal(v["knots_y"], ky)
    assert 2 <= len(kx) <= 202 and (ky > 0).all()
    # lib.size given: it is used and returned, and E moves with it
    lib = v["lib_size"] * 1.5 + 3.0
    v2 = hip_ctx.voom(counts, c["D"], lib_size=lib)
    assert np.array_equal(v2["lib_size"], lib) and not np.array_equal(v2["E"], v["E"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_log_cpm_against_correctly_rounded_values(hip_ctx, case):
    c = case_results(hip_ctx, case)
    ref = vr.logcpm_cr(c["counts"], c["voom"]["lib_size"])
    worst = float(vr.ulps(c["voom"]["E"], ref).max())
    print(f"[measure] log2-CPM {case}: worst deviation from the correctly rounded value {worst:.3f} ulp")
    assert worst <= LOG2_ULP_BOUND


def device_weights(ctx, Q, offset, Eff, kx, ky, rows, sentinel=-7.0, ldw=None):
    """(status, W rows x n) of plaidhip_dev_voom_weights; W (leading dimension ldw, `rows` if None) holds the sentinel before
    the call, and its padding past `rows` must hold it afterwards"""
    import torch
    dev = torch.device("cuda", 0)
    n, p = Q.shape
    ldw = rows if ldw is None else ldw
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    Qd, od, Ed, kxd, kyd = t(Q.T), t(offset), t(Eff), t(kx), t(ky)
    W = torch.full((n, ldw), sentinel, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    status, _ = _status(lambda: ctx.dev_voom_weights(Qd.data_ptr(), od.data_ptr(), n, p, Ed.data_ptr(), rows, kxd.data_ptr(),
                                                     kyd.data_ptr(), len(kx), W.data_ptr(), ldw))
    ctx.synchronize()
    Wh = W.cpu().numpy()
    assert (Wh[:, rows:] == sentinel).all()                                       # the padding of W is not written
    return status, Wh[:, :rows].T


def device_effects(ctx, c):
    from tests.test_gpu_limma import device_passes
    E = c["voom"]["E"]
    Q = c["des"]["Q"][:, :, None]
    return device_passes(ctx, np.asfortranarray(E), E.shape[0] + (E.shape[0] & 1), Q, None, np.array([E.shape[1]], dtype=np.int64))[0]


@pytest.mark.parametrize("case", CASES + P9_CASES, ids=IDS + P9_IDS)
def test_the_weights_pass_follows_the_header_to_the_bit(hip_ctx, case):
    c = case_results(hip_ctx, case)
    v = c["voom"]
    rows, n, p = case
    Eff = device_effects(hip_ctx, c)                                              # [p + 1][rows]
    pick = list(range(0, rows, max(1, rows // 40)))
    lam, w = vr.emulate_weights(c["des"]["Q"], v["offset"], Eff[:p, pick], v["knots_x"], v["knots_y"])
    er.assert_same_bits(v["weights"][pick], w, "the call's weights")
    assert np.isfinite(w).all() and (w > 0).all()
    # a planted table: knots taken from the lambda themselves (so some lambda sit exactly on a knot), inside their range (so
    # some lie below the first and above the last), one trend value non-positive (the weight is NaN)
    flat = np.sort(lam.ravel())
    kx = np.unique(flat[np.linspace(len(flat) * 0.2, len(flat) * 0.8, 9).astype(int)])
    ky = np.linspace(0.4, 1.6, len(kx))
    ky[3] = -0.25
    status, W = device_weights(hip_ctx, c["des"]["Q"], v["offset"], Eff[:, pick], kx, ky, len(pick))
    assert status == _lib.OK
    _, wp = vr.emulate_weights(c["des"]["Q"], v["offset"], Eff[:p, pick], kx, ky)
    er.assert_same_bits(W, wp, "the planted knots")
    assert (lam < kx[0]).any() and (lam > kx[-1]).any() and np.isin(lam, kx).sum() >= len(kx) and np.isnan(wp).any()
    on = np.isin(lam, kx[[0, 1, 2, 4]])
    assert np.array_equal(wp[on], [1.0 / ((f * f) * (f * f)) for f in ky[np.searchsorted(kx, lam[on])]])   # exactly Y_k at a knot


@pytest.mark.parametrize("p", PLANTED_P, ids=[f"p{p}" for p in PLANTED_P])
def test_the_weights_kernel_on_planted_operands_at_every_register_count(hip_ctx, p):
    """plaidhip_dev_voom_weights alone: 257 rows (a second workgroup that holds one row), 129 samples (a column block and a
    tail of one), W with leading dimension rows + 3, a random Q and offsets, and effects of six patterns -- row r carries
    pattern r % 6, so the emulation of six rows is the reference of all 257.  The mean's row of Eff is NaN: the kernel does
    not read it.  The knots are planted as above."""
    rows, n, npat = 257, 129, 6
    rng = np.random.default_rng([28, p])
    Q, offset = rng.normal(size=(n, p)), rng.normal(size=n)
    pat = rng.normal(size=(p, npat))
    Eff = np.full((p + 1, rows), np.nan)
    Eff[:p] = pat[:, np.arange(rows) % npat]
    lam, _ = vr.emulate_weights(Q, offset, pat, [0.0], [1.0])                     # (lambda does not depend on the knots)
    flat = np.sort(lam.ravel())
    kx = np.unique(flat[np.linspace(len(flat) * 0.2, len(flat) * 0.8, 9).astype(int)])
    ky = np.linspace(0.4, 1.6, len(kx))
    ky[3] = -0.25
    _, wp = vr.emulate_weights(Q, offset, pat, kx, ky)
    assert (lam < kx[0]).any() and (lam > kx[-1]).any() and np.isin(lam, kx).sum() >= len(kx) and np.isnan(wp).any()
    assert np.isfinite(wp[~np.isnan(wp)]).all() and not np.isnan(wp).all(axis=1).any()
    status, W = device_weights(hip_ctx, Q, offset, Eff, kx, ky, rows, ldw=rows + 3)
    assert status == _lib.OK
    want = wp[np.arange(rows) % npat]
    assert np.array_equal(np.isnan(W), np.isnan(want))                            # finite, or the planted NaN
    er.assert_same_bits(W, want, f"planted operands, p = {p}")


def test_end_to_end_against_the_pins_in_numpy(hip_ctx):
    """case (600, 131, 3): E within the log2 bound; the trend within TREND_REL of the reference's own lowess at every lambda, so
    the weights within 4 TREND_REL + 8 ulp; then plaid_limma(E, design, weights = W) on a dozen rows against numpy's weighted
    least squares with the REFERENCE's E and weights, within section 28's bound plus what a relative weight error dw moves:
    |H^-1| (1 + |H^-1| H_n) |mag| dw |v_j| for logFC (the propagation of section 28 with |dH| <= dw H_n, |db| <= dw |mag| + |dE|)"""
    case = CASES[0]
    c = case_results(hip_ctx, case)
    rows, n, p = case
    v, D = c["voom"], c["D"]
    ref = vr.voom_np(c["counts"], D)
    assert np.array_equal(v["lib_size"], ref["lib_size"])
    assert float(vr.ulps(v["E"], ref["E"]).max()) <= LOG2_ULP_BOUND
    f_dev = np.array([[vr.trend(v["knots_x"], v["knots_y"], t) for t in row] for row in ref["lambda"][::10]])
    f_ref = np.array([[vr.trend(ref["knots_x"], ref["knots_y"], t) for t in row] for row in ref["lambda"][::10]])
    worst_f = float(np.abs(f_dev / f_ref - 1.0).max())
    dw = 4.0 * TREND_REL + 8 * 2.0 ** -52
    worst_w = float(np.abs(v["weights"] / ref["weights"] - 1.0).max())
    print(f"[measure] end to end: trend {worst_f:.3g}, weights {worst_w:.3g} relative (allowed {TREND_REL:.1g}, {dw:.3g})")
    assert worst_f <= TREND_REL and worst_w <= dw
    names = [f"g{i}" for i in range(rows)], [f"s{i}" for i in range(n)]
    out = plaid_amd.plaid_voom(plaid_amd.NamedMatrix(c["counts"], *names), D, ctx=hip_ctx)
    er.assert_same_bits(out["E"].values, v["E"], "plaid_voom")
    tabs, hyper = plaid_amd.plaid_limma(out["E"], D, ctx=hip_ctx, weights=out["weights"])
    des = c["des"]
    eta = wr.basis_error(D, None, None, des)
    sel = np.arange(n)
    worst = 0.0
    for r in list(range(0, 12)) + [rows - 2]:
        if r in (2, 9):
            continue                                                               # (all zero: a constant row, logFC = 0 up to rounding)
        rw = wr.mp_wls(ref["E"][r], ref["weights"][r], D)
        hinv, Hn = wr.exact_H(des["Q"], ref["weights"][r], rw["live"])
        unit = wr.units(ref["E"][r], ref["weights"][r], des["Q"], list(sel), des["v"], rw, hinv, Hn, eta[0], eta[1])
        ox = ref["weights"][r] * np.abs(ref["E"][r])
        nm = float(np.linalg.norm([np.sum(ox * np.abs(des["Q"][:, k])) for k in range(p)]))
        de = LOG2_ULP_BOUND * 2.0 ** -52
        for j, nm_j in enumerate(tabs):
            allow = unit["logFC"][j] + 2.0 * float(np.linalg.norm(des["v"][:, j])) * hinv * (1.0 + hinv * Hn) * nm * (dw + de)
            dev = abs(tabs[nm_j].values[r, 0] - float(rw["logFC"][j]))
            worst = max(worst, dev / allow)
            assert dev <= allow, (r, j, dev, allow)
    print(f"[measure] end to end: logFC, worst share of the composed allowance {worst:.3g}")
    assert hyper["n.ok"] == rows and np.isfinite(tabs["coef2"].values).all()


def test_error_paths_write_nothing(hip_ctx):
    c = case_results(hip_ctx, CASES[1])
    rows, n, p = CASES[1]
    for bad in (-1.0, np.nan, np.inf):
        counts = c["counts"].copy(order="F")
        counts[rows - 2, n - 1] = bad
        out = dict(E=np.full((rows, n), -7.0, order="F"), W=np.full((rows, n), -7.0, order="F"), lib=np.full(n, -7.0),
                   off=np.full(n, -7.0), kx=np.full(engine.VOOM_MAX_KNOTS, -7.0), ky=np.full(engine.VOOM_MAX_KNOTS, -7.0))
        status, _ = _status(lambda: engine._voom(hip_ctx.lib.plaidhip_voom, (hip_ctx.handle,), counts, c["D"], out=out))
        assert status == _lib.EINVAL and "finite and >= 0" in _lib.load().plaidhip_last_error_string().decode()
        assert all((a == -7.0).all() for a in out.values())
    Eff = device_effects(hip_ctx, c)
    kx = np.arange(257, dtype=np.float64)
    status, W = device_weights(hip_ctx, c["des"]["Q"], c["voom"]["offset"], Eff, kx, np.ones(257), rows)
    assert status == _lib.EINVAL and (W == -7.0).all()
    status, W = device_weights(hip_ctx, c["des"]["Q"], c["voom"]["offset"], Eff, kx[:256], np.ones(256), rows)
    assert status == _lib.OK and (W == 1.0).all()


@pytest.mark.parametrize("where", ["row300-col0", "last-row-last-col"])
def test_a_bad_count_on_a_threads_later_trip_writes_nothing(hip_ctx, where):
    """the check kernel's 256 threads stride over the rows: of the 600-row case, row 300 is seen on a thread's second trip
    and row 599 on its third"""
    c = case_results(hip_ctx, CASES[0])
    rows, n, p = CASES[0]
    r, col = (300, 0) if where == "row300-col0" else (rows - 1, n - 1)
    for bad in (-1.0, np.nan, np.inf):
        counts = c["counts"].copy(order="F")
        counts[r, col] = bad
        out = dict(E=np.full((rows, n), -7.0, order="F"), W=np.full((rows, n), -7.0, order="F"), lib=np.full(n, -7.0),
                   off=np.full(n, -7.0), kx=np.full(engine.VOOM_MAX_KNOTS, -7.0), ky=np.full(engine.VOOM_MAX_KNOTS, -7.0))
        status, _ = _status(lambda: engine._voom(hip_ctx.lib.plaidhip_voom, (hip_ctx.handle,), counts, c["D"], out=out))
        assert status == _lib.EINVAL and "finite and >= 0" in _lib.load().plaidhip_last_error_string().decode()
        assert all((a == -7.0).all() for a in out.values())


@pytest.mark.parametrize("case", CASES + P9_CASES, ids=IDS + P9_IDS)
def test_every_sharding_has_the_one_device_bits(hip_ctx, case):
    c = case_results(hip_ctx, case)
    one = c["voom"]
    for nshards in (1, 2, 3):
        status, got = _status(lambda: engine._voom(hook("voom"), (0, nshards, -1), c["counts"], c["D"]))
        assert status == _lib.OK
        for key in one:
            er.assert_same_bits(got[key], one[key], f"{nshards} shards, {key}")
    rows, n, p = case
    out = dict(E=np.full((rows, n), -7.0, order="F"), W=np.full((rows, n), -7.0, order="F"))
    status, _ = _status(lambda: engine._voom(hook("voom"), (0, 3, 1), c["counts"], c["D"], out=out))
    assert status == _lib.EHIP and (out["E"] == -7.0).all() and (out["W"] == -7.0).all()
