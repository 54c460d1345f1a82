"""tests/helpers/pow_ref.py on the host (no GPU): the emulation of pow_quarters against exact powers over every half-
integer rank in [1, 196608], the allowance function the derived bounds use, the long-double reference against 50 digits,
the domain helper -- and deliberately wrong weight routines, which the claims of tests/test_gpu_rank_weights.py catch.

Where the device's root4_pos is needed and only a GPU has it, sqrt(sqrt(r)) stands in (the starred columns below), and a
numpy restatement of root4_pos (a 24-bit reciprocal square root for v_rsq_f64, the Newton steps with exactly computed
fused operations) shows what the checks do to a routine with one step too few."""
import numpy as np
import pytest

from tests.helpers import pow_ref as pr

ld = np.longdouble

# max error / u of pow_quarters' operation sequence over every half-integer rank in [1, 196608], against long double
# (q = 1, 5, 9, 13 with root4_pos := sqrt(sqrt(r))), to two decimals; q = 13 is 2.9549, which went into the table this was
# taken from as 2.96 by way of 2.955
TABLE = {1: 1.47, 2: 1.00, 3: 3.29, 5: 2.40, 6: 1.93, 7: 3.90, 9: 2.31, 10: 1.99, 11: 3.96, 12: 1.00, 13: 2.955, 14: 2.53,
         15: 3.96, 16: 1.00}
BELOW_20352 = {3: 3.18, 7: 3.46, 11: 3.53, 15: 3.74}      # the same for the ranks a bucket ranker's column can hold


@pytest.fixture(scope="module")
def domain():
    r = pr.half_integer_ranks()
    assert r.size == 2 * pr.G_MAX - 1 and r[0] == 1.0 and r[-1] == pr.G_MAX
    root4 = pr.root4_sqrt_sqrt(r)
    exact = {q: pr.exact_power(r, q / 4.0) for q in range(1, 17)}
    emu = {q: pr.quarters_emulated(r, q, root4) for q in range(1, 17)}
    err = {q: pr.err_u(emu[q], exact[q]) for q in range(1, 17)}
    return {"r": r, "root4": root4, "exact": exact, "emu": emu, "err": err}


def test_allowance_table_and_the_exponents_the_suite_uses():
    rho = pr.RHO_U
    derived = [rho, 1, 3.5, 0, rho + 1, 2, 4.5, 0, rho + 1, 2, 4.5, 1, rho + 2, 3, 5.5, 1]
    assert [pr.quarters_allowance_u(q) for q in range(1, 17)] == derived
    assert pr.pow_allowance_u(1.0) == 0.0
    for p in pr.GENERIC_POWERS:
        assert pr.quarter_of(p) == 0 and pr.pow_allowance_u(p) == pr.POW_LIBM_U == 3.0
    assert [pr.quarter_of(q / 4.0) for q in range(1, 18)] == [1, 2, 3, 0, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 0]
    # every exponent the bound tests used before the allowance became a function keeps 3 u or less
    for p in (1.25, 1.5, 1.3, 0.25, 0.5, 2.0):
        assert pr.pow_allowance_u(p) <= 3.0, p
    assert pr.pow_allowance_u(1.25) == 3.0 and pr.pow_allowance_u(1.25, "quarters") == rho + 1
    assert pr.pow_allowance_u(1.5) == 3.0 and pr.pow_allowance_u(1.5, "quarters") == 2.0     # ("any": pow() in the network)
    assert pr.pow_allowance_u(1.75) == 4.5 and pr.pow_allowance_u(0.75) == 3.5 and pr.pow_allowance_u(3.75) == 5.5
    with pytest.raises(ValueError):
        pr.pow_allowance_u(1.3, "quarters")


def test_emulation_inside_the_allowance_over_the_whole_domain(domain):
    worst = 0.0
    for q in range(1, 17):
        e, allow = float(domain["err"][q].max()), pr.quarters_allowance_u(q)
        assert e <= allow + pr.LD_SLACK_U, (q, e, allow)
        if allow:
            worst = max(worst, e / allow)
    print(f"\npow_quarters (host emulation, root4 := sqrt(sqrt)): largest error / allowance {worst:.3f}")
    fig = pr.check_quarter_route(domain["r"], domain["emu"], domain["exact"])
    assert fig["root4_ulp_vs_sqrt_sqrt"] == 0 and not fig["failed"]


def test_table_of_maxima_reproduced(domain):
    r = domain["r"]
    low = r <= 20352.0
    for q, want in TABLE.items():
        got = float(domain["err"][q].max())
        assert abs(got - want) <= 0.005 + 1e-9, (q, got, want)
    for q, want in BELOW_20352.items():
        got = float(domain["err"][q][low].max())
        assert abs(got - want) <= 0.005 + 1e-9, (q, got, want)
    for q in (4, 8):
        assert float(domain["err"][q].max()) == 0.0


def test_three_u_is_exceeded_at_q_3_7_11_15(domain):
    """why the constant became a function: tau or alpha = 0.75 / 2.75 (q = 3, 7, 11, 15) exceed the former 3 u per
    weight, already at ranks a 20,352-row column holds, with nothing but IEEE products and square roots"""
    low = domain["r"] <= 20352.0
    for q in (3, 7, 11, 15):
        assert float(domain["err"][q][low].max()) > 3.0 + pr.LD_SLACK_U, q
        assert pr.quarters_allowance_u(q) > 3.0
    for q in (2, 6, 10, 12, 14, 16):
        assert float(domain["err"][q].max()) <= 3.0


def test_long_double_reference_against_50_digits(domain):
    r = domain["r"]
    rng = np.random.default_rng(5)
    sample = np.sort(rng.choice(r.size, size=150, replace=False))
    worst = 0.0
    powers = [(q / 4.0, domain["err"][q]) for q in range(1, 17)]
    for p in pr.GENERIC_POWERS:
        powers.append((p, pr.err_u(np.power(r, p), pr.exact_power(r, p))))      # (numpy's fp64 pow picks the hard cases)
    for p, err in powers:
        idx = np.union1d(sample, np.argsort(err)[-100:])
        a, b = pr.exact_power(r[idx], p), pr.exact_power_mp(r[idx], p)
        d = float((np.abs(a - b) / (b * ld(pr.U))).max())
        worst = max(worst, d)
        assert d <= 0.5 * pr.LD_SLACK_U, (p, d)
    print(f"\nlong double against 50 digits: largest difference {worst:.5f} u (slack {pr.LD_SLACK_U} u)")


@pytest.mark.parametrize("g", [1, 2, 7, 256, 20353])
def test_rank_domain_columns(g):
    from oracle import c_oracle
    X = pr.rank_domain_columns(g, seed=g)                 # (asserts the union itself)
    assert X.shape == (g, 3) and X.flags.f_contiguous
    R = c_oracle.colranks_dense(X, "average", False)
    assert np.array_equal(np.sort(R[:, 0]), np.arange(1, g + 1, dtype=np.float64))
    assert np.array_equal(X, np.round(X)) and X.min() == 0.0 and X.max() == g - 1
    if g > 2:
        assert not np.array_equal(X[:, 0], np.sort(X[:, 0])), "the rows are permuted"
    assert np.array_equal(X, pr.rank_domain_columns(g, seed=g))


# ------------------------------------------------------------------ deliberately wrong routines
def _two_product(a, b):
    """a * b = hi + lo exactly (Veltkamp / Dekker), fp64"""
    def split(x):
        t = 134217729.0 * x
        h = t - (t - x)
        return h, x - h
    hi = a * b
    ah, al = split(a)
    bh, bl = split(b)
    lo = ((ah * bh - hi) + ah * bl + al * bh) + al * bl
    return hi, lo


def _rsq24(x):
    """1 / sqrt(x) to 24 bits: a stand-in for v_rsq_f64 (about 23 bits)"""
    return (ld(1.0) / np.sqrt(x.astype(ld))).astype(np.float32).astype(np.float64)


def _root4_pos_host(r, steps=2):
    """root4_pos restated in numpy: the raw estimates, then `steps` Newton steps whose fused operations are computed from
    exact products and rounded once (the last sum in long double: 11 guard bits)"""
    y = _rsq24(r)
    z = _rsq24(y)
    c = 0.25 * (y * y)
    for _ in range(steps):
        w = z * z
        hi, lo = _two_product(w, w)
        e = (r - hi) - lo                                   # fma(-w, w, r): r - hi is exact, one rounding
        hi, lo = _two_product(z * c, e)
        z = ((z.astype(ld) + hi.astype(ld)) + lo.astype(ld)).astype(np.float64)
    return z


def _quarters_swapped(r, q, root4):
    """pow_quarters with the tests of q & 2 and q & 1 exchanged"""
    res, base = np.ones_like(r), r.copy()
    e = q >> 2
    while e:
        if e & 1:
            res = res * base
        base = base * base
        e >>= 1
    if (q & 3) == 1:
        return res * root4
    if q & 3:
        s = np.sqrt(r)
        if q & 1:
            res = res * s
        if q & 2:
            res = res * np.sqrt(s)
    return res


@pytest.fixture(scope="module")
def bucket_domain(domain):
    """the ranks of a 20,352-row column: enough for every wrong routine to show"""
    n = 2 * 20352 - 1
    return {"r": domain["r"][:n], "exact": {q: domain["exact"][q][:n] for q in range(1, 17)}}


def test_the_restated_root4_pos_passes(bucket_domain):
    r, exact = bucket_domain["r"], bucket_domain["exact"]
    root4 = _root4_pos_host(r)
    fig = pr.check_quarter_route(r, {q: pr.quarters_emulated(r, q, root4) for q in range(1, 17)}, exact)
    assert fig["root4_ulp_vs_sqrt_sqrt"] <= 1 and fig["err_u"][1] <= pr.RHO_U
    print(f"\nroot4_pos restated on the host: {fig['root4_ulp_vs_sqrt_sqrt']} ulp from sqrt(sqrt(r)), "
          f"{fig['err_u'][1]:.3f} u from r^(1/4)")


def test_wrong_routines_fail_the_claims(bucket_domain):
    r, exact = bucket_domain["r"], bucket_domain["exact"]
    good4 = _root4_pos_host(r)
    good = {q: pr.quarters_emulated(r, q, good4) for q in range(1, 17)}
    assert not pr.check_quarter_route(r, good, exact, collect=True)["failed"]

    # root4_pos with one Newton step: 2^-44 instead of 2^-66 before the last rounding
    bad4 = _root4_pos_host(r, steps=1)
    one_step = {q: pr.quarters_emulated(r, q, bad4) for q in range(1, 17)}
    failed = pr.check_quarter_route(r, one_step, exact, collect=True)["failed"]
    assert 3 in failed and 6 in failed, failed
    with pytest.raises(AssertionError, match=r"claim \(3\)"):
        pr.check_quarter_route(r, one_step, exact)

    # q & 2 and q & 1 exchanged: r^(1/2) and r^(1/4) change places
    swapped = {q: _quarters_swapped(r, q, good4) for q in range(1, 17)}
    failed = pr.check_quarter_route(r, swapped, exact, collect=True)["failed"]
    assert 2 in failed and 6 in failed, failed

    # pow() in place of the quarters: a fine power, but not this code's bits
    libm = {q: np.power(r, q / 4.0) for q in range(1, 17)}
    failed = pr.check_quarter_route(r, libm, exact, collect=True)["failed"]
    assert 2 in failed and 4 in failed, failed

    # a route whose q = 5, 9, 13 take other fourth roots than its q = 1: the identity (4) alone
    mixed = dict(good)
    mixed[1] = pr.root4_sqrt_sqrt(r)
    assert not pr.same_bits(mixed[1], good4), "the stand-in must differ from the restated root4_pos somewhere"
    failed = pr.check_quarter_route(r, mixed, exact, collect=True)["failed"]
    assert set(failed) == {4}, failed

    # (5) two routes share one inline function, so they agree bit for bit: each wrong routine differs from the right one
    for name, other in (("one step", one_step), ("swapped", swapped), ("pow", libm)):
        assert any(not pr.same_bits(good[q], other[q]) for q in range(1, 17)), name
