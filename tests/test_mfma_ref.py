"""Self-tests of tests/helpers/mfma_ref.py (host only): the restated bf16 x 3 split against exact rational arithmetic, and
the bound mfma_bound against the mistakes it has to see -- a dropped `lo` plane, a dropped K step -- and against the
arithmetic it has to let through.  The conditions here are conditions, not tolerances."""
from fractions import Fraction

import numpy as np

from tests.helpers import exact_ref as er
from tests.helpers import mfma_ref as mr


def _values():
    rng = np.random.default_rng(7)
    v = [rng.gamma(2.0, 1.0, 60) + 0.25, rng.normal(size=60), np.where(rng.random(60) < 0.5, 1e6, -1e6) + rng.normal(size=60),
         10.0 ** rng.uniform(-30.0, 30.0, 60) * np.where(rng.random(60) < 0.5, 1.0, -1.0), np.arange(1, 61) ** 0.25,
         np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -100, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53, 255.0, 255.5, 256.0, 257.0, 65535.5,
                   3.0e38, -3.0e38, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -9 + 2.0 ** -40])]
    return np.concatenate(v)


def test_split3_is_exact_in_rationals_and_leaves_24_bits():
    x = _values()
    assert len(x) >= 300 and mr.splittable(x).all()
    hi, mid, lo, res = mr.split3(x)
    for a, h, m_, l_, r in zip(x, hi, mid, lo, res):
        assert Fraction(float(h)) + Fraction(float(m_)) + Fraction(float(l_)) + Fraction(float(r)) == Fraction(float(a)), a
        assert abs(Fraction(float(r))) <= Fraction(1, 2 ** 24) * abs(Fraction(float(a))), (a, r)
        for p in (h, m_, l_):                                # every plane is a bf16 number: at most 8 significant bits
            fr, _ = np.frexp(p)
            assert fr * 256.0 == np.rint(fr * 256.0), (a, p)
    # round to nearest EVEN on a tie, to nearest otherwise
    assert mr.split3(1.0 + 2.0 ** -8)[0] == 1.0 and mr.split3(1.0 + 3 * 2.0 ** -8)[0] == 1.0 + 2.0 ** -6
    assert mr.split3(1.0 + 2.0 ** -8 + 2.0 ** -20)[0] == 1.0 + 2.0 ** -7


def test_half_integer_ranks_split_exactly():
    r = np.arange(1, 2 * int(mr.HALF_INT_EXACT) + 1) / 2.0           # 0.5 ... 20,448
    hi, mid, lo, res = mr.split3(r)
    assert np.all(res == 0.0) and np.all(lo == 0.0) and np.array_equal(hi + mid, r)
    hi, mid, lo, res = mr.split3(-r)
    assert np.all(res == 0.0) and np.all(lo == 0.0)


def test_what_the_split_cannot_carry():
    edge = (2.0 - 2.0 ** -8) * 2.0 ** 127                            # halfway between the largest bf16 and 2^128: a tie to even
    bad = np.array([np.nan, np.inf, -np.inf, 1e39, -1e39, 2.0 ** 128, edge, -edge, np.nextafter(edge, 0.0)])
    assert not mr.splittable(bad)[:8].any()
    assert not mr.splittable(bad)[8]         # (fp64 -> fp32 rounds it onto the tie first: the device tests the head, not x)
    ok = np.array([(2.0 - 2.0 ** -7) * 2.0 ** 127, edge * (1.0 - 2.0 ** -23), -3.38e38, 0.0, 1e-45, 2.0 ** -149, 1e-320])
    assert mr.splittable(ok).all()
    for p in mr.split3(bad):
        assert np.all(p == 0.0)
    hi, mid, lo, res = mr.split3(ok)
    # (below 2^-126 a bf16 plane is a subnormal, spaced 2^-133: half of that is lost at most -- inside the bound's 2^-126)
    assert np.all(np.isfinite(hi + mid + lo)) and np.all(np.abs(res) <= 2.0 ** -24 * np.abs(ok) + 2.0 ** -134)


def _case(g, n, seed):
    """gamma(2, 1) + 0.25 data; sets of size 1 (every gene once), size 2, and the sizes of mfma_ref.SIZES"""
    rng = np.random.default_rng(seed)
    X = mr.data("well", g, n, seed)
    lists = [np.array([i]) for i in range(g)] + [rng.choice(g, size=2, replace=False) for _ in range(g)]
    lists += [rng.choice(g, size=s, replace=False) for s in mr.SIZES if 2 < s <= g]
    Gp = np.concatenate([[0], np.cumsum([len(s) for s in lists])]).astype(np.int32)
    Gi = np.concatenate(lists).astype(np.int32)
    return X, Gp, Gi


def _outside(got, ref, bound):
    return ~(np.abs(got - ref) <= bound)


def test_the_bound_sees_a_dropped_plane_and_a_dropped_k_step_and_passes_the_complete_sum():
    g, n = 128, 6                        # gk = 128: the last K step of 32 genes is genes 96 ... 127, all of them real
    X, Gp, Gi = _case(g, n, 11)
    sizes = np.diff(Gp)
    ref, mag, k = er.set_sums(Gp, Gi, X)
    bound = mr.mfma_bound(mag, k, 1)
    full = mr.emulate_sets(Gp, Gi, X)
    assert not _outside(full, ref, bound).any()
    worst = float((np.abs(full - ref) / bound).max())
    print(f"[measure] complete emulation: worst error / bound {worst:.3g}")
    # the third plane dropped: hi + mid leave up to 2^-17 |x|, the bound allows 3 * 2^-23 |x| for one term
    nolo = mr.emulate_sets(Gp, Gi, X, drop_lo=True)
    frac1 = float(_outside(nolo, ref, bound)[sizes == 1].mean())
    frac2 = float(_outside(nolo, ref, bound)[sizes == 2].mean())
    print(f"[measure] lo plane dropped: outside the bound {frac1:.2f} of the size-1 scores, {frac2:.2f} of size 2")
    assert frac1 > 0.5
    # the last K step dropped: every set that holds one of its genes, in every sample
    last = np.arange(g) >= g - 32
    nok = mr.emulate_sets(Gp, Gi, X, skip_genes=last)
    holds = np.array([last[Gi[Gp[j]:Gp[j + 1]]].any() for j in range(len(sizes))])
    assert holds.sum() >= 32 + 2 and (~holds).sum() >= 96
    assert _outside(nok, ref, bound)[holds].all()
    assert not _outside(nok, ref, bound)[~holds].any()


def test_the_fp64_route_restated_on_the_host_lies_inside_the_bound():
    """plain fp64 sums in gene order (what the fp64 kernels do up to the order) on every data kind: inside mfma_bound, and
    the complete emulation too -- cancelling, signed, tiny and half-integer data included"""
    g, n = 192, 3
    for kind in mr.KINDS:
        X = mr.data(kind, g, n, 5)
        Gp, Gi, names = mr.sets(g, 40, 3)
        ref, mag, k = er.set_sums(Gp, Gi, X)
        bound = mr.mfma_bound(mag, k, 1)
        plain = np.array([[np.cumsum(X[np.sort(Gi[Gp[j]:Gp[j + 1]]), c])[-1] if Gp[j + 1] > Gp[j] else 0.0
                           for c in range(n)] for j in range(len(Gp) - 1)])
        er.assert_within(plain, ref, bound, f"fp64 restated, {kind}")
        emu = mr.emulate_sets(Gp, Gi, X)
        er.assert_within(emu, ref, bound, f"emulation, {kind}")
        if kind == "half_ranks":
            assert np.array_equal(emu, ref)          # exact split, exact fp32 sums below 2^23
        assert names["last"] is not None and names["ends"] is not None and names["empty"] is not None


def test_sets_helper_keeps_the_edge_sets_at_every_m():
    for g, m in ((1, 1), (31, 63), (33, 65), (64, 255), (2049, 65), (64, 2), (129, 1)):
        Gp, Gi, names = mr.sets(g, m, 1)
        assert len(Gp) == m + 1 and Gi.min() >= 0 and Gi.max() <= g - 1
        lists = [set(Gi[Gp[j]:Gp[j + 1]].tolist()) for j in range(m)]
        assert all(len(s) == Gp[j + 1] - Gp[j] for j, s in enumerate(lists))            # no duplicate members
        assert {g - 1} in lists
        if m >= 2:
            assert {0, g - 1} in lists
        if m >= 14 and g >= 400:
            assert sorted(len(s) for s in lists[:10]) == sorted(mr.SIZES)
