"""plaid.fisher on the host (no GPU): the pinned tail of include/plaidhip.h (tests/helpers/fisher_ref.py: tail_form) against
exact rational arithmetic (tail_exact) at the bound DESIGN.md section 19 derives, the library's host entry
plaidhip_hyper_tail against tail_form bit for bit, the definition against scipy, and plaid_sig's truth table."""
from fractions import Fraction

import numpy as np
import pytest

import plaid_amd
from plaid_amd import _lib, engine
from plaid_amd.matrix import NamedMatrix
from tests.helpers import fisher_ref as ref

_exact = {}


def tables():
    return ref.FIXED_TABLES + ref.random_tables()


def exact(tab):
    if tab not in _exact:
        _exact[tab] = ref.tail_exact(*tab)
    return _exact[tab]


def check_against_exact(p, tab):
    """the contract of the pinned form: within (4 n + 2) 2^-53, relatively, of an exact p >= 2^-900; below that only
    0 <= p <= 2^-890"""
    e = exact(tab)
    assert p == p, tab
    if e >= ref.P_FLOOR:
        err = abs(Fraction(p) - e) / e
        assert err <= ref.tail_bound(*tab[:3]), f"{tab}: relative error {float(err):.3g}, bound {float(ref.tail_bound(*tab[:3])):.3g}"
    else:
        assert 0.0 <= p <= ref.P_SMALL, (tab, p)


def test_random_tables_cover_the_tail_and_the_bulk():
    """a condition on the seeded inputs: N < 5000, tables on both sides of the mode, trivial ones (x at lo, x past hi) and
    some whose exact p is below the floor"""
    tabs = ref.random_tables()
    assert len(tabs) == 300 and all(N < 5000 for N, _, _, _ in tabs)
    ps = [exact(t) for t in tabs]
    assert sum(p == 1 for p in ps) >= 1 and sum(p == 0 for p in ps) >= 1
    assert sum(Fraction(1, 2) < p < 1 for p in ps) >= 20 and sum(ref.P_FLOOR <= p < Fraction(1, 2) for p in ps) >= 20
    assert sum(0 < p < ref.P_FLOOR for p in ps) >= 1


def test_tail_form_is_within_the_derived_bound_of_the_exact_tail():
    worst = Fraction(0)
    for tab in tables():
        p = ref.tail_form(*tab)
        check_against_exact(p, tab)
        e = exact(tab)
        if e >= ref.P_FLOOR:
            worst = max(worst, abs(Fraction(p) - e) / e / ref.tail_bound(*tab[:3]))
    print(f"worst error / bound = {float(worst):.3g}")


def test_hyper_tail_has_the_bits_of_tail_form():
    for tab in tables():
        got, want = engine.hyper_tail(*tab), ref.tail_form(*tab)
        assert got == want, f"{tab}: {got!r} != {want!r}"


@pytest.mark.parametrize("tab,want", [
    ((100, 30, 20, 0), 1.0), ((100, 30, 20, -3), 1.0),          # x <= lo = 0
    ((100, 90, 20, 10), 1.0), ((100, 90, 20, 9), 1.0),          # x <= lo = 10
    ((100, 30, 20, 21), 0.0), ((100, 10, 20, 11), 0.0),         # x > hi
    ((100, 0, 20, 0), 1.0), ((100, 0, 20, 1), 0.0),             # K = 0
    ((100, 100, 20, 20), 1.0), ((100, 100, 20, 21), 0.0),       # K = N: lo = hi = k
    ((100, 30, 0, 0), 1.0), ((100, 30, 0, 1), 0.0),             # k = 0 (the NaN rule belongs to plaidhip_fisher, not the tail)
    ((100, 30, 100, 30), 1.0), ((100, 30, 100, 31), 0.0),       # k = N
    ((0, 0, 0, 0), 1.0), ((1, 1, 1, 1), 1.0),
])
def test_hyper_tail_edges(tab, want):
    assert engine.hyper_tail(*tab) == want == ref.tail_form(*tab) == float(ref.tail_exact(*tab))


def test_hyper_tail_at_the_first_and_last_live_x():
    """x = lo + 1 (everything but one term) and x = hi (one term), against the exact value"""
    for N, K, k in ((100, 30, 20), (100, 90, 20), (4097, 100, 4096), (64, 64, 10), (65, 1, 64)):
        lo, hi = ref.bounds(N, K, k)
        for x in {min(lo + 1, hi), hi}:
            p = engine.hyper_tail(N, K, k, x)
            assert p == ref.tail_form(N, K, k, x)
            check_against_exact(p, (N, K, k, x))


def test_hyper_tail_refuses_bad_tables():
    lib = _lib.load()
    import ctypes as C
    p = C.c_double(-7.0)
    for N, K, k, code, word in ((10, 11, 3, _lib.EINVAL, "K = 11"), (10, 3, 11, _lib.EINVAL, "k = 11"),
                                (10, -1, 3, _lib.EINVAL, "K = -1"), (-1, 0, 0, _lib.EINVAL, "N = -1"),
                                ((1 << 26) + 1, 5, 5, _lib.EUNSUPPORTED, "at most 67108864")):
        assert lib.plaidhip_hyper_tail(N, K, k, 1, C.byref(p)) == code
        assert word in lib.plaidhip_last_error_string().decode()
    assert lib.plaidhip_hyper_tail(10, 3, 3, 1, None) == _lib.EINVAL
    assert p.value == -7.0
    assert lib.plaidhip_hyper_tail(1 << 26, 1 << 25, 3, 3, C.byref(p)) == _lib.OK and 0.124 < p.value < 0.126


def test_the_definition_is_fisher_exact_greater():
    """tail_exact against scipy.stats.fisher_exact(alternative="greater") on every 2 x 2 table with N <= 12 (1,820 tables).
    This checks the definition, not precision.  The largest relative discrepancy observed on the CPU was 2.89e-16 (scipy's
    own rounding); the tolerance is ten times that."""
    from scipy.stats import fisher_exact
    worst = Fraction(0)
    for N in range(13):
        for a in range(N + 1):
            for b in range(N + 1 - a):
                for c in range(N + 1 - a - b):
                    d = N - a - b - c
                    p = fisher_exact([[a, b], [c, d]], alternative="greater")[1]
                    e = ref.tail_exact(N, a + c, a + b, a)
                    assert e > 0
                    worst = max(worst, abs(Fraction(float(p)) - e) / e)
    print(f"largest relative discrepancy = {float(worst):.3g}")
    assert worst <= Fraction(2.89e-15)


def test_fisher_ref_on_a_hand_worked_case():
    """N = 6; list: rows 0, 1 up, row 5 down.  Set A = {0, 1, 2}: ovUp 2, ovDn 0; up: P(X >= 2), X ~ Hyper(6, 2, 3)
    = C(2,2) C(4,1) / C(6,3) = 4 / 20; any: K = 3, x = 2: (C(3,2) C(3,1) + C(3,3)) / 20 = 10 / 20; down: x = 0: 1.
    Set B = {5, 0}: the overlap keeps the set's own order."""
    sig = np.array([1, 1, 0, 0, 0, -1], dtype=np.int8)
    Gp, Gi = np.array([0, 3, 5, 5, 11], dtype=np.int32), np.array([0, 1, 2, 5, 0, 0, 1, 2, 3, 4, 5], dtype=np.int32)
    out, tot, ov_len, ov_idx = ref.fisher_ref(sig, Gp, Gi)
    assert tot[:, 0].tolist() == [2.0, 1.0]
    assert out[0, :3, 0].tolist() == [3.0, 2.0, 0.0] and out[0, 4, 0] == 1.0
    assert abs(out[0, 3, 0] - 0.2) < 1e-15 and abs(out[0, 5, 0] - 0.5) < 1e-15
    assert out[0, 9, 0] == float("inf") and out[0, 10, 0] == 0.0 and out[0, 11, 0] == (2.0 * 2.0) / (1.0 * 1.0)
    assert out[1, :3, 0].tolist() == [2.0, 1.0, 1.0]
    assert np.isnan(out[2, 3:, 0]).all() and np.isnan(out[3, 3:, 0]).all()          # k = 0 and k = N
    assert out[2, :3, 0].tolist() == [0.0, 0.0, 0.0] and out[3, :3, 0].tolist() == [6.0, 2.0, 1.0]
    assert ov_len[:, 0].tolist() == [2, 2, 0, 3]
    assert ov_idx[:, 0].tolist() == [0, 1, -1, 5, 0, 0, 1, 5, -1, -1, -1]
    # Benjamini-Hochberg over the two sets that have a p: pUp = (0.2, 0.6)
    assert out[1, 3, 0] == ref.tail_form(6, 2, 2, 1) and abs(out[1, 3, 0] - 0.6) < 1e-15
    assert out[0, 6, 0] == out[0, 3, 0] * 2.0 and out[1, 6, 0] == out[1, 3, 0]


@pytest.mark.parametrize("fc,p,want", [
    (0.3, 0.01, 1), (-0.3, 0.01, -1), (0.3, 0.06, 0), (-0.3, 0.06, 0), (0.1, 0.01, 0), (-0.1, 0.01, 0),
    (0.2, 0.01, 0), (-0.2, 0.01, 0),                       # exactly at lfc: the comparisons are strict
    (0.3, 0.05, 0), (-0.3, 0.05, 0),                       # exactly at pcut
    (np.nan, 0.01, 0), (0.3, np.nan, 0), (np.nan, np.nan, 0),
    (np.inf, 0.0, 1), (-np.inf, 0.0, -1), (0.0, 0.0, 0),
])
def test_plaid_sig_truth_table(fc, p, want):
    s = plaid_amd.plaid_sig(np.array([fc]), np.array([p]))
    assert s.dtype == np.int8 and s.tolist() == [want]


def test_plaid_sig_shapes_names_and_cutoffs():
    fc = NamedMatrix(np.array([[1.0, -1.0], [0.5, 2.0], [-3.0, 0.0]]), ["a", "b", "c"], ["c1", "c2"])
    pv = np.array([[0.01, 0.2], [0.01, 0.001], [0.04, 0.0]])
    s = plaid_amd.plaid_sig(fc, pv, lfc=0.75, pcut=0.05)
    assert isinstance(s, NamedMatrix) and list(s.rownames) == ["a", "b", "c"] and list(s.colnames) == ["c1", "c2"]
    assert s.values.tolist() == [[1, 0], [0, 1], [-1, 0]]
    d = plaid_amd.plaid_sig({"a": 1.0, "b": -1.0}, {"b": 0.01, "a": 0.5})
    assert list(d.rownames) == ["a", "b"] and d.values.ravel().tolist() == [0, -1]
    with pytest.raises(ValueError):
        plaid_amd.plaid_sig(np.zeros(3), np.zeros(4))


def test_the_entries_are_declared_and_exported():
    lib = _lib.load()
    for name, nargs in (("plaidhip_fisher", 11), ("plaidhip_fisher_multi", 12), ("plaidhip_hyper_tail", 5)):
        assert len(_lib.SIGNATURES[name]) == nargs and hasattr(lib, name)
    assert hasattr(lib, "plaidhip_debug_fisher_sharded_on_one_device")
    assert engine.FISHER_COLUMNS == ref.COLUMNS and len(ref.COLUMNS) == 12
