"""plaidhip_lowess on the host (include/plaidhip.h), without a GPU, against an independent Python
restatement (tests/helpers/voom_ref.py): bit for bit with the default delta (the anchor walk) and with delta = 0 (a local
regression at every point); heavy ties in x, n < ns, constant y, an outlier whose robustness weight is 0; the bound on the
number of knots; the trend on the host (voom_trend_knots through plaid.voom is the GPU test's)."""
import numpy as np
import pytest

from plaid_amd import _lib, engine
from tests.helpers import voom_ref as vr


def deck(kind, n=120, seed=3):
    rng = np.random.default_rng([seed, n])
    x = np.sort(rng.normal(size=n) * 2.0 + 3.0)
    y = 1.5 - 0.2 * x + 0.05 * x * x + 0.2 * rng.normal(size=n)
    if kind == "ties":
        x = np.sort(np.round(x * 2.0) / 2.0)
    elif kind == "constant":
        y = np.full(n, 0.75)
    elif kind == "outlier":
        y[n // 2] += 25.0
    elif kind == "clumps":                                   # long gaps and dense clumps: anchors both ways
        x = np.sort(np.concatenate([rng.normal(0.0, 1e-3, n // 2), rng.uniform(5.0, 9.0, n - n // 2)]))
    return x, y


KINDS = ("plain", "ties", "constant", "outlier", "clumps")


@pytest.mark.parametrize("f", [0.5, 0.1, 1.0])
@pytest.mark.parametrize("kind", KINDS)
def test_anchor_walk_bit_for_bit(kind, f):
    x, y = deck(kind)
    delta = 0.01 * (x[-1] - x[0])
    got = engine.lowess(x, y, f, 3, delta)
    ys, anchor = vr.lowess_walk(x, y, f, 3, delta)
    assert np.array_equal(got["ys"], ys) and np.array_equal(got["anchor"], anchor)
    assert anchor[0] and anchor[-1] and (anchor.sum() < len(x) or kind == "ties")     # (ties 0.5 apart: every point is a fit or a copy)


@pytest.mark.parametrize("kind", KINDS)
def test_delta_zero_is_a_local_regression_at_every_point(kind):
    x, y = deck(kind, n=60)
    got = engine.lowess(x, y, 0.5, 3, 0.0)
    assert np.array_equal(got["ys"], vr.lowess_direct(x, y, 0.5, 3))
    assert got["anchor"].all()


def test_properties():
    # n < ns is clamped (f n < 2 -> two points; f > 1 -> all of them); n = 1 and 2
    x, y = deck("plain", n=5)
    for f in (0.1, 0.3, 3.0):
        assert np.array_equal(engine.lowess(x, y, f, 3, 0.0)["ys"], vr.lowess_direct(x, y, f, 3))
    assert engine.lowess([2.0], [7.0], 0.5)["ys"][0] == 7.0
    two = engine.lowess([1.0, 2.0], [3.0, 5.0], 0.5, 3, 0.0)["ys"]
    assert np.array_equal(two, vr.lowess_direct([1.0, 2.0], [3.0, 5.0], 0.5, 3))
    # constant y comes back up to the rounding of sum w y: ns = 60 terms, (ns + 3) 2^-53 sum |w| |y|, and the linear correction
    # keeps sum |w| below 4 (at the ends of the range, where it extrapolates); the passes stop at once (cmad < 1e-7 mean|res|)
    x, y = deck("constant")
    assert np.abs(engine.lowess(x, y, 0.5)["ys"] - 0.75).max() <= 63 * 2.0 ** -53 * 4 * 0.75
    # one outlier gets the robustness weight 0: the fit beside it is that of the data without it, to 1e-3 of the noise
    x, y = deck("outlier")
    base = engine.lowess(np.delete(x, 60), np.delete(y, 60), 0.5, 3, 0.0)["ys"]
    with_out = engine.lowess(x, y, 0.5, 3, 0.0)["ys"]
    assert np.abs(np.delete(with_out, 60) - base).max() < 0.05 and abs(with_out[60] - y[60]) > 20.0
    first = engine.lowess(x, y, 0.5, 0, 0.0)["ys"]
    assert np.abs(np.delete(first, 60) - base).max() > 0.2          # (without the robustness passes it is pulled)
    # all x equal: every point copies the first fit
    got = engine.lowess(np.full(7, 2.0), np.arange(7.0), 0.5)
    assert np.all(got["ys"] == got["ys"][0]) and got["anchor"].all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [50, 1000, 5000])
def test_knot_count_bound(kind, n):
    """with delta = 0.01 (max - min) every second anchor lies more than delta beyond the one two back (section 28): at most
    202 knots at distinct x, under PLAIDHIP_VOOM_MAX_KNOTS"""
    x, y = deck(kind, n=n)
    delta = 0.01 * (x[-1] - x[0])
    got = engine.lowess(x, y, 0.5, 3, delta)
    kx, _ = vr.knots_of(x, got["ys"], got["anchor"])
    assert np.all(np.diff(kx) > 0) and len(kx) <= 202 < engine.VOOM_MAX_KNOTS
    assert np.all(kx[2:] - kx[:-2] > delta)


def test_arguments():
    lib = _lib.load()
    for bad, word in ((dict(x=[1.0, 0.5]), "ascending"), (dict(f=0.0), "f ="), (dict(x=[1.0, np.nan]), "not finite"),
                      (dict(delta=-1.0), "delta")):
        a = dict(x=[1.0, 2.0], y=[1.0, 2.0], f=0.5, delta=0.0)
        a.update(bad)
        with pytest.raises(_lib.PlaidHipError, match=word):
            engine.lowess(a["x"], a["y"], a["f"], 3, a["delta"])
    assert lib.plaidhip_lowess(None, None, 0, 0.5, 3, 0.0, None, None) == _lib.EINVAL
