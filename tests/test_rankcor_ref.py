"""plaid.rankcor's rank-mode epilogue on the host (include/plaidhip.h: plaidhip_rankcor, plaidhip_rankcor_finish; DESIGN.md
section 21), without a GPU.

The pinned form (tests/helpers/rankcor_ref.py: rankcor_form) lies within 3 * 2^-53 (rho) and 4 * 2^-53 (t), relatively, of the
exact integers evaluated by mpmath at 50 digits; plaidhip_rankcor_finish has the bits of the form on every table, at the
integer limits (n = 131,072) and where Q = 0; rho agrees with numpy.corrcoef of ranks and membership; p lies within
(6 (t^2 + 1) + E) 2^-53 of mpmath's erfc at the computed t wherever p is a normal double, E twice libm's measured erfc error
(at least 2)."""
import math
import os
import re
from fractions import Fraction

import mpmath
import numpy as np
import pytest

from plaid_amd import _lib, engine
from tests.helpers import rankcor_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = Fraction(1, 2**53)
_tables = {}


def tables():
    """name -> (n, T1, T2, k, A): the fixed tables drawn at random and with the k highest / lowest genes, and the 300
    seeded ones; computed once"""
    if not _tables:
        for q, (n, k, lv) in enumerate(ref.FIXED_TABLES):
            for ex in (None, "top", "bottom"):
                _tables[f"fixed{q}-{ex}"] = ref.table_sums(n, k, lv, "average", seed=q, extreme=ex)
        for q, (n, k, lv, ties) in enumerate(ref.random_tables()):
            _tables[f"seeded{q}"] = ref.table_sums(n, k, lv, ties, seed=1000 + q, extreme=(None, None, "top", "bottom")[q % 4])
    return _tables


def same_bits(a, b):
    return a == b or (a != a and b != b)


def test_the_pinned_form_is_within_its_bounds_of_exact_arithmetic():
    worst_rho, worst_t, n_rho, n_t = Fraction(0), Fraction(0), 0, 0
    for name, tab in tables().items():
        rho, t = ref.rankcor_form(*tab)
        erho, et = ref.rankcor_exact(*tab)
        if erho is None:
            assert rho != rho and t != t, (name, tab)
            continue
        num, P, Q = ref._npq(*tab)
        if Q == 0:
            assert abs(rho) == 1.0 and (tab[0] <= 2 or math.isinf(t)), (name, tab)
            continue
        with mpmath.workdps(50):
            err = Fraction(float(abs(mpmath.mpf(rho) - erho) / abs(erho))) if erho != 0 else Fraction(abs(rho))
            assert err <= 3 * EPS, (name, tab, rho, float(err / EPS))
            worst_rho, n_rho = max(worst_rho, err / EPS), n_rho + 1
            if et is None:
                assert t != t
                continue
            err = Fraction(float(abs(mpmath.mpf(t) - et) / abs(et))) if et != 0 else Fraction(abs(t))
            assert err <= 4 * EPS, (name, tab, t, float(err / EPS))
            worst_t, n_t = max(worst_t, err / EPS), n_t + 1
    print(f"{n_rho} rho, worst {float(worst_rho):.3f} eps (bound 3); {n_t} t, worst {float(worst_t):.3f} eps (bound 4)")
    assert n_rho >= 250 and n_t >= 250


def finish_one(tab):
    n, T1, T2, k, A = tab
    return engine.rankcor_finish([n], [T1], [T2], [[k]], [[A]])[0, :, 0]


def test_finish_has_the_bits_of_the_pinned_form_on_every_table():
    pn = ref.library_pnorm_upper()
    for name, tab in tables().items():
        got = finish_one(tab)
        rho, t = ref.rankcor_form(*tab)
        assert got[0] == tab[3]
        assert same_bits(got[1], rho) and same_bits(got[2], t), (name, tab, got, rho, t)
        assert same_bits(got[3], 2.0 * pn(abs(t)) if t == t else ref.NAN), (name, tab)
        assert same_bits(got[4], got[3])                        # Benjamini-Hochberg of one p-value


def limit_tables():
    """n = 131,072 with k = 1, 65,536 and 131,071: tie-free and two-level lists, random sets and the extreme ones; and Q = 0:
    a two-level list whose set is exactly its upper (lower) level"""
    n, out = engine.RANKCOR_MAX_GENES, {}
    for k in (1, 65536, 131071):
        for lv in (0, 2):
            for ex in (None, "top", "bottom"):
                out[f"n{n}-k{k}-lv{lv}-{ex}"] = ref.table_sums(n, k, lv, "average", seed=k + lv, extreme=ex)
    for nn, kk in ((131072, 65536), (131072, 1), (131072, 131071), (3, 1), (2, 1), (10, 4)):
        x = np.array([0.0] * (nn - kk) + [1.0] * kk)
        for ties in ("average", "min", "max"):
            z, ok = ref.z_ranks(x, ties)
            out[f"q0-{nn}-{kk}-{ties}-top"] = ref.int_sums(z, ok, np.arange(nn - kk, nn))
            out[f"q0-{nn}-{kk}-{ties}-bottom"] = ref.int_sums(z, ok, np.arange(0, nn - kk))
    return out


def test_finish_at_the_integer_limits_and_where_q_is_zero():
    pn = ref.library_pnorm_upper()
    zero_q = 0
    for name, tab in limit_tables().items():
        num, P, Q = ref._npq(*tab)
        assert abs(num) < 2**53 and 0 <= P < 2**102 and Q >= 0, name
        got = finish_one(tab)
        rho, t = ref.rankcor_form(*tab)
        assert same_bits(got[1], rho) and same_bits(got[2], t), (name, tab, got, rho, t)
        assert same_bits(got[3], 2.0 * pn(abs(t)) if t == t else ref.NAN), name
        if name.startswith("q0"):
            assert Q == 0 and P > 0 and abs(got[1]) == 1.0, (name, tab)
            assert (got[1] > 0) == name.endswith("top")
            if tab[0] > 2:
                assert math.isinf(got[2]) and got[3] == 0.0 and (got[2] > 0) == (got[1] > 0)
            else:
                assert got[2] != got[2] and got[3] != got[3]
            zero_q += 1
    assert zero_q == 36


def test_degenerate_tables_are_nan_and_bad_operands_are_refused():
    z = [2, 4, 6, 8]
    T1, T2 = sum(z), sum(v * v for v in z)
    for k, A in ((0, 0), (4, T1)):                                # k = 0 and k = n
        assert np.isnan(finish_one((4, T1, T2, k, A))[1:]).all()
    assert np.isnan(finish_one((4, 20, 100, 2, 10))[1:]).all()    # an all-tied list: z = 5 everywhere, n T2 = T1^2
    assert np.isnan(finish_one((1, 2, 4, 0, 0))[1:]).all() and np.isnan(finish_one((0, 0, 0, 0, 0))[1:]).all()
    out = engine.rankcor_finish([4, 4], [T1, 20], [T2, 100], [[1, 2], [2, 2]], [[8, 10], [6, 10]])
    assert out.shape == (2, 5, 2) and not np.isnan(out[:, :, 0]).any() and np.isnan(out[:, 1:, 1]).all()
    np.testing.assert_allclose(out[:, 4, 0], ref.bh(out[:, 3, 0]), rtol=1e-15, atol=0)
    for bad, word in (((4, T1, T2, 5, 8), "k = 5"), ((4, T1, T2, 1, T1 + 1), "A ="), ((-1, 0, 0, 0, 0), "n = -1"),
                      ((131073, 0, 0, 0, 0), "n = 131073"), ((4, T1, 90, 1, 8), "n T2 < T1^2"), ((4, T1, T2, 1, 20), "P < num^2")):
        with pytest.raises(_lib.PlaidHipError, match=re.escape(word)):
            finish_one(bad)


def test_rho_agrees_with_numpy_corrcoef_of_ranks_and_membership():
    rng = np.random.default_rng(3)
    checked = 0
    for n, levels in ((12, 0), (40, 3), (97, 0), (97, 5), (300, 2)):
        x = rng.permutation(n).astype(float) if levels == 0 else rng.integers(0, levels, size=n).astype(float)
        x[rng.random(n) < 0.1] = np.nan
        for ties in ("average", "min", "max"):
            z, ok = ref.z_ranks(x, ties)
            for k in (1, 2, n // 3, n - 5):
                mem = rng.choice(n, size=k, replace=False)
                tab = ref.int_sums(z, ok, mem)
                rho, _ = ref.rankcor_form(*tab)
                ind = np.zeros(n)
                ind[mem] = 1.0
                if tab[3] in (0, tab[0]):
                    assert rho != rho
                    continue
                want = np.corrcoef(z[ok].astype(float), ind[ok])[0, 1]
                assert abs(rho - want) <= 1e-13, (n, levels, ties, k, rho, want)
                checked += 1
    assert checked >= 50


def erfc_error_in_eps(pn):
    """the largest error of the library's pnorm_upper(t) = 0.5 erfc(t / sqrt(2)) against mpmath AT THE DOUBLE ARGUMENT
    a = t / sqrt(2) (so that only libm's erfc and the exact halving are measured), in units of 2^-53, over a grid of t in
    [0, 38]"""
    worst, at = 0.0, 0.0
    with mpmath.workdps(60):
        for t in np.concatenate([np.linspace(0.0, 38.0, 3801), np.random.default_rng(1).uniform(0.0, 38.0, 1500)]):
            a = float(t) / math.sqrt(2.0)
            want = mpmath.erfc(mpmath.mpf(a)) / 2
            got = pn(float(t))
            if got < 2.0**-1021:
                continue
            e = float(abs(mpmath.mpf(got) - want) / want * mpmath.mpf(2) ** 53)
            if e > worst:
                worst, at = e, float(t)
    return worst, at


def test_p_is_within_its_allowance_of_mpmath_erfc_at_the_computed_t():
    pn = ref.library_pnorm_upper()
    E_meas, at = erfc_error_in_eps(pn)
    E = max(2.0, 2.0 * E_meas)
    print(f"libm erfc through pnorm_upper: worst {E_meas:.3f} * 2^-53 at t = {at:.4f}; allowed E = {E:.3f}")
    checked, worst = 0, 0.0
    with mpmath.workdps(60):
        for name, tab in {**tables(), **limit_tables()}.items():
            got = finish_one(tab)
            t, p = float(got[2]), float(got[3])
            if t != t or math.isinf(t) or p < 2.0**-1022:
                continue
            want = mpmath.erfc(abs(mpmath.mpf(t)) / mpmath.sqrt(2))
            err = float(abs(mpmath.mpf(p) - want) / want * mpmath.mpf(2) ** 53)
            allow = 6.0 * (t * t + 1.0) + E
            assert err <= allow, (name, t, p, err, allow)
            worst = max(worst, err / allow)
            checked += 1
    print(f"{checked} p-values, worst error / allowance = {worst:.3g}")
    assert checked >= 250


def test_the_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "plaidhip.h")).read()
    lib = _lib.load()
    for name, nargs in (("plaidhip_rankcor", 11), ("plaidhip_rankcor_multi", 12), ("plaidhip_rankcor_finish", 8)):
        assert re.search(r"\bint\s+%s\s*\(" % name, header)
        assert len(_lib.SIGNATURES[name]) == nargs and hasattr(lib, name)
    assert hasattr(lib, "plaidhip_debug_rankcor_sharded_on_one_device")
    assert "PLAIDHIP_RANKCOR_MAX_GENES 131072" in header and "PLAIDHIP_RANKCOR_LIST_TILE 8" in header
    assert engine.RANKCOR_MAX_GENES == 131072 and engine.RANKCOR_COLUMNS == ref.COLUMNS
    import plaid_amd
    assert callable(plaid_amd.plaid_rankcor) and callable(plaid_amd.rankcor_multi)
    rsrc = open(os.path.join(ROOT, "r-pkg", "R", "plaid-hip.R")).read()
    assert re.search(r"^plaid\.rankcor\s*<-\s*function", rsrc, re.M)
    assert re.search(r"\bplaid\.rankcor\b", open(os.path.join(ROOT, "r-pkg", "NAMESPACE")).read())
    assert "R_plaidhip_rankcor" in open(os.path.join(ROOT, "r-pkg", "src", "plaidhip_R.c")).read()
