"""The references of tests/test_gpu_compact_staging.py, tested on the host alone (no GPU): the integer rank sums are exact,
the derived bound of the fp32 staging holds for the kernel's arithmetic -- and does NOT hold for the mistakes the GPU tests
are there to catch (chunk partials accumulated in fp32; one term dropped or added twice), on the very data they use."""
import numpy as np
import pytest

from tests.helpers import compact_ref as cr
from tests.helpers import exact_ref as er

G = 20448                               # the most genes the compact stagings take
KS = [1, 4, 7, 64, 500, G]
KINDS = ["well", "cancel"]


def _nested_sets(g, ks, seed):
    """one set per k: k genes in a random order (the order emulate_mixed() walks them in)"""
    rng = np.random.default_rng(seed)
    lists = [rng.permutation(g)[:k] for k in ks]
    Gp = np.concatenate([[0], np.cumsum([len(s) for s in lists])]).astype(np.int32)
    return Gp, np.concatenate(lists).astype(np.int32), lists


_CACHE = {}


def _case(kind):
    """x (one column), the sets of KS, their exact sums, mags and term counts -- computed once per data kind"""
    if kind not in _CACHE:
        x = cr.data(kind, G, 1, 77)
        Gp, Gi, lists = _nested_sets(G, KS, 78)
        ref, mag, k = er.set_sums(Gp, Gi, x)
        _CACHE[kind] = (x[:, 0], lists, ref[:, 0], mag[:, 0], k[:, 0])
    return _CACHE[kind]


@pytest.mark.parametrize("signed", [False, True])
def test_rank_sums_equal_the_exact_fraction_sums(signed):
    rng = np.random.default_rng(5 + int(signed))
    g, n = 97, 3
    R = rng.integers(1, 2 * g + 1, size=(g, n)) / 2.0          # half-integers, as average ranks are
    R[0, 0] = 32767.5                                          # the largest admissible value
    if signed:
        R *= np.where(rng.random((g, n)) < 0.5, -1.0, 1.0)
    lists = [rng.permutation(g)[:s] for s in (1, 2, 7, 40, g)] + [np.zeros(0, dtype=np.int64)]
    Gp = np.concatenate([[0], np.cumsum([len(s) for s in lists])]).astype(np.int32)
    Gi = np.concatenate(lists).astype(np.int32)
    S, k = cr.rank_sums(Gp, Gi, R)
    assert S.shape == (len(lists), n) and list(k) == [1, 2, 7, 40, g, 0]
    for j, s in enumerate(lists):
        for c in range(n):
            assert S[j, c] == er.fraction_sum(R[s, c])
    assert np.all(S[-1] == 0.0)
    mean = cr.expected_bits(S, k, "mean")
    assert np.all(mean[-1] == 0.0)
    assert mean[0, 0] == S[0, 0] * (1.0 / (1e-8 + 1.0))
    with pytest.raises(AssertionError):
        cr.rank_sums(Gp, Gi, R + 0.25)                         # not half-integers
    with pytest.raises(AssertionError):
        cr.rank_sums(Gp, Gi, np.where(R == R[1, 1], 32768.0, R))   # 2x does not fit 16 bits


def test_shared_sets_hold_the_edge_sets_in_unsorted_order():
    g = 8193
    Gp, Gi, names = cr.sets(g, 3)
    m = len(Gp) - 1
    assert m == 134 and 1 <= np.diff(Gp)[:130].min() and np.diff(Gp)[:130].max() == 400
    assert Gp[names["empty"] + 1] == Gp[names["empty"]]
    assert list(Gi[Gp[names["last"]]:Gp[names["last"] + 1]]) == [g - 1]
    assert list(Gi[Gp[names["before_last"]]:Gp[names["before_last"] + 1]]) == [g - 2]
    allg = Gi[Gp[names["all"]]:Gp[names["all"] + 1]]
    assert np.array_equal(np.sort(allg), np.arange(g)) and not np.array_equal(allg, np.arange(g))
    unsorted = sum(bool(np.any(np.diff(Gi[Gp[j]:Gp[j + 1]]) < 0)) for j in range(130))
    assert unsorted > 100
    for j in range(m):
        s = Gi[Gp[j]:Gp[j + 1]]
        assert len(np.unique(s)) == len(s)


@pytest.mark.parametrize("kind", KINDS)
def test_kernel_arithmetic_stays_within_the_mixed_bound(kind, capsys):
    x, lists, ref, mag, k = _case(kind)
    bound = cr.mixed_bound(mag, k, 1)
    ratios = []
    for j, s in enumerate(lists):
        got = cr.emulate_mixed(x[s])
        ratios.append(abs(got - ref[j]) / bound[j])
    with capsys.disabled():
        print(f"\n[compact ref] {kind}: kernel form, error / bound for k = {KS}: " + " ".join(f"{r:.3f}" for r in ratios))
    assert max(ratios) <= 1.0


def test_fp32_accumulation_across_chunks_leaves_the_bound(capsys):
    """the set of every gene on positive data: fp32 accumulators lose ~k u / 8 of the sum, far past 3 u"""
    x, lists, ref, mag, k = _case("well")
    bound = cr.mixed_bound(mag, k, 1)
    r32 = [abs(cr.emulate_mixed(x[s], acc32=True) - ref[j]) / bound[j] for j, s in enumerate(lists)]
    r64 = [abs(cr.emulate_mixed(x[s]) - ref[j]) / bound[j] for j, s in enumerate(lists)]
    with capsys.disabled():
        print(f"\n[compact ref] well: fp32 accumulation, error / bound for k = {KS}: " + " ".join(f"{r:.3f}" for r in r32))
    assert KS[-1] == G and r32[-1] > 1.0
    assert max(r64) <= 1.0
    # the same over the five columns a GPU case has (the error is a random walk of ~2,556 roundings of up to 2^-10 each
    # against a bound of 0.008: typically three times the bound, in no column far inside it)
    X = cr.data("well", G, 5, 79)
    Gp = np.array([0, G], dtype=np.int32)
    ref5, mag5, k5 = er.set_sums(Gp, lists[-1].astype(np.int32), X)
    b5 = cr.mixed_bound(mag5, k5, 1)[0]
    c32 = [abs(cr.emulate_mixed(X[lists[-1], c], acc32=True) - ref5[0, c]) / b5[c] for c in range(5)]
    c64 = [abs(cr.emulate_mixed(X[lists[-1], c]) - ref5[0, c]) / b5[c] for c in range(5)]
    with capsys.disabled():
        print("[compact ref] well, k = 20448, five columns: fp32 accumulation " + " ".join(f"{r:.2f}" for r in c32) +
              "; kernel form " + " ".join(f"{r:.4f}" for r in c64))
    assert max(c32) > 1.0 and max(c64) <= 1.0


@pytest.mark.parametrize("kind", KINDS)
def test_a_dropped_or_doubled_term_leaves_the_bound(kind):
    """every set size the GPU tests use (1 ... 400, the singletons, every gene of 8,193 ... 20,448): the smallest term of
    the set, dropped or added twice, is outside the bound -- so a stale or missing gene cannot hide in it"""
    x, lists, ref, mag, k = _case(kind)
    bound = cr.mixed_bound(mag, k, 1)
    for j, s in enumerate(lists):
        t = x[s]
        i = int(np.argmin(np.abs(t)))
        dropped = cr.emulate_mixed(np.delete(t, i))
        doubled = cr.emulate_mixed(np.append(t, t[i]))
        assert abs(dropped - ref[j]) > bound[j], (kind, KS[j])
        assert abs(doubled - ref[j]) > bound[j], (kind, KS[j])
    # and at the other gene counts of the GPU tests, the set of every gene: the smallest term against the bound itself
    for g in (8193, 8194, 10240):
        t = x[:g]
        b = cr.mixed_bound(np.abs(t).sum(), g, 3)
        assert np.abs(t).min() > 2.0 * b, (kind, g)


@pytest.mark.parametrize("kind", KINDS)
def test_cast_alone_is_within_one_fp32_rounding_of_mag(kind):
    """the exact sum of the fp32-rounded values: <= 2^-24 mag from the exact sum of the doubles"""
    x, lists, ref, mag, k = _case(kind)
    Gp = np.concatenate([[0], np.cumsum([len(s) for s in lists])]).astype(np.int32)
    Gi = np.concatenate(lists).astype(np.int32)
    x32 = x.astype(np.float32).astype(np.float64)
    assert np.any(x32 != x)
    ref32, _, _ = er.set_sums(Gp, Gi, x32[:, None])
    assert np.all(np.abs(ref32[:, 0] - ref) <= cr.U32 * mag)
    assert np.any(ref32[:, 0] != ref)


def test_mixed_bound_terms():
    """3 * 2^-24 (1 + 2^-22) mag + the fp64 bound + k 2^-149, elementwise"""
    mag = np.array([0.0, 1.0, 1e6])
    k = np.array([0, 1, 500])
    b = cr.mixed_bound(mag, k, 3)
    exp = 3.0 * 2.0 ** -24 * (1.0 + 2.0 ** -22) * mag + er.fp64_bound(mag, k, 3) + k * 2.0 ** -149
    assert np.array_equal(b, exp)
    assert b[0] == er.fp64_bound(0.0, 0, 3) and b[1] > 3.0 * 2.0 ** -24
    # specials of the cast: overflow to +Inf, underflow to 0
    assert cr.emulate_mixed([1e39, 1.0]) == np.inf and cr.emulate_mixed([1e-46]) == 0.0
    assert cr.emulate_mixed([]) == 0.0 and cr.emulate_mixed([0.1]) == float(np.float32(0.1))
