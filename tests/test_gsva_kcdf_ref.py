"""The two host forms of GSVA's Gaussian kernel CDF estimate against each other (tests/helpers/gsva_kcdf.py: the literal
double loop in Python floats, the numpy form with sequential sums), the argument checks of replaid.gsva.exact's "gauss"
row transform that need no device, and the library's exported table of Phi against an independent Phi.  Host only."""
import math

import numpy as np
import pytest

from tests.helpers import exact_ref as er
from tests.helpers import gsva_kcdf as gk


def _rows(n, seed=5):
    """normal rows, integer-tied rows, a constant row (row 8), seam rows (h = 2^p and 5 * 2^p), an outlier row (|v| > 10)"""
    rng = np.random.default_rng(seed)
    rows = [rng.normal(7, 2, size=n) for _ in range(4)]
    rows += [np.round(rng.normal(0, 2, size=n), 0) for _ in range(4)]
    rows.append(np.full(n, 3.25))
    if n >= 16:
        rows += [gk.seam_row(n, m, p, rng) for m, p in ((1, 0), (1, 3), (5, 0), (5, 2))]
    out = rng.normal(0, 1, size=n)
    out[n // 2] = 40.0
    rows.append(out)
    return np.array(rows)


@pytest.mark.parametrize("n", [2, 17, 64, 65])
def test_literal_loop_equals_the_numpy_form_bit_for_bit(n):
    T = gk.table_erfc()
    X = _rows(n)
    er.assert_same_bits(gk.pinned(X, T), gk.literal(X, T), f"n={n}")


def test_constant_row_is_half_the_samples_and_a_nan_row_is_nan():
    T = gk.table_erfc()
    n = 65
    X = _rows(n)
    X = np.vstack([X, X[0], X[1]])
    X[-2, 3] = np.nan
    X[-1, 9] = np.inf
    for V in (gk.pinned(X, T), gk.literal(X, T)):
        assert (V[8] == n / 2).all()                       # the constant row: every term reads T[0] = 0.5
        assert np.isnan(V[-2]).all() and np.isnan(V[-1]).all()
        assert np.isfinite(V[:-2]).all()
    er.assert_same_bits(gk.pinned(X, T), gk.literal(X, T), "NaN rows")


def test_seam_rows_have_the_bandwidth_and_the_terms_they_are_built_for():
    rng = np.random.default_rng(8)
    for n in (16, 65, 257):
        for m, p in ((1, 0), (1, 3), (5, 0), (5, 2)):
            x = gk.seam_row(n, m, p, rng)
            h = m * 2.0 ** p
            assert gk.bandwidths(x[None, :])[0] == h
            v = (x[:, None] - x[None, :]) / h
            assert (v == 10.0).any() and (v == -10.0).any() and (np.abs(v) > 10.0).any()
            u = np.abs(v[np.abs(v) <= 10.0]) / 10.0 * 10000.0
            frac = u - np.floor(u)
            assert (frac == 0.0).any()                              # on an integer
            beside = (frac > 0.0) & ((frac < 1e-9) | (frac > 1.0 - 1e-9))
            assert beside.any() == (m == 5)                         # one rounding beside an integer


def test_columns_subset_equals_the_full_form():
    T = gk.table_erfc()
    X = _rows(65)
    er.assert_same_bits(gk.pinned(X, T, cols=np.arange(20, 41)), gk.pinned(X, T)[:, 20:41], "column range")


def test_one_minus_t_is_exact_for_every_table_value():
    from fractions import Fraction
    T = gk.table_erfc()
    assert (T >= 0.5).all()
    assert all(Fraction(1.0 - float(t)) == 1 - Fraction(float(t)) for t in T)


# ------------------------------------------------------------------------------------------------- the Python entry
def test_gauss_is_a_row_transform_and_kcdf_is_not():
    from plaid_amd.engine import GSVA_EXACT_ROWTF, check_gsva_exact_args
    assert check_gsva_exact_args(1, "gauss") == (1.0, 3)
    assert GSVA_EXACT_ROWTF == {"z": 0, "ecdf": 1, "none": 2, "gauss": 3}
    with pytest.raises(ValueError):
        check_gsva_exact_args(1, "kcdf")


def test_exports():
    import plaid_amd
    assert callable(plaid_amd.gsva_kcdf_table)
    assert callable(plaid_amd.Context.gsva_kcdf) and callable(plaid_amd.Context.gsva_kcdf_table)


# ------------------------------------------------------------------------------------------------- the library's table
def _phi_reference(t):
    """Phi(t) for the fp64 numbers t, rounded to fp64 once, from 50 digits where mpmath is installed"""
    try:
        import mpmath
    except ImportError:
        return np.array([0.5 * math.erfc(-x / math.sqrt(2.0)) for x in t]), False
    mpmath.mp.dps = 50
    return np.array([float(mpmath.ncdf(mpmath.mpf(float(x)))) for x in t]), True


def test_library_table_against_an_independent_phi():
    """The library builds T[i] = 0.5 * erfc(-t / sqrt(2.0)), t = 10.0 * i / 10000.0, with the C library's erfc (it needs
    no device).  Allowed distance from the correctly rounded Phi(t): 6 ulp of the value.  The results lie in [0.5, 1],
    where erfc's argument x = -t / sqrt(2) carries two roundings (1.5 ulp relative at most) and Phi's relative
    condition number |x erfc'(x) / erfc(x)| is below 0.5 (its maximum, at |x| = 0.707, is 0.48 / erfc >= 0.48 / 1):
    under 1 ulp from the argument; the halving is exact; the rest is the erfc itself, for which the GNU C library's
    manual lists a known maximum error of up to 5 ulp in double precision, the largest figure among the common libms.
    (Against math.erfc, where mpmath is missing, both sides may err: the same bound then compares two libms.)"""
    import plaid_amd
    T = plaid_amd.gsva_kcdf_table()
    assert T.shape == (gk.TABLE,) and T.dtype == np.float64
    assert T[0] == 0.5 and T[10000] == 1.0
    assert (np.diff(T) >= 0.0).all()
    t = np.array([10.0 * float(i) / 10000.0 for i in range(gk.TABLE)])
    ref, exact = _phi_reference(t)
    ulp = np.spacing(np.minimum(T, ref))
    dist = np.abs(T - ref) / ulp
    print(f"table vs {'mpmath' if exact else 'math.erfc'}: max distance {dist.max():.2f} ulp at index {int(dist.argmax())}")
    assert dist.max() <= 6.0
