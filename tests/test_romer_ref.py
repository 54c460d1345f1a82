"""plaid.romer's references against each other and the host entries against them, without a GPU.

  * The 50-digit end-to-end reference (romer_ref.romer_mp) asserts, while it runs, that its cases are decidable (the module
    docstring of romer_ref has the condition and the derivation of the allowance); here every case the GPU tests use is
    run, none skipped, and its shape is checked: the empty set and the set outside the universe have no count, the
    duplicated gene ties exactly, the all-zero gene sits where the header puts it.
  * The numpy restatement (keys_np, rank2_np, sides_np) against the exact integer ranks of the 50-digit form and against a
    sort for mean50.
  * plaidhip_romer_shrink against shrink_mp over romer_ref.SHRINK_CASES: pi = 0, pi tiny (ntarget = 1), pi near 1, df0 = inf,
    df0 = 0, the clamp met below and above.  Allowed: FACTOR x MEASURED["shrink"], measured here as well and printed.
  * plaidhip_romer_finish bit for bit against finish_np: Benjamini-Hochberg per side and the m = 0 rows."""
import numpy as np
import pytest

from plaid_amd import engine
from tests.helpers import romer_ref as mr
from tests.test_gpu_romer import E2E


@pytest.mark.parametrize("case", E2E, ids=["-".join(c) for c in E2E])
def test_every_end_to_end_case_is_decidable(case):
    name, stat, mode = case
    ref = mr.e2e_reference(name, stat, mode)[0]          # (raises where two keys are not decided)
    X, D, use, K, sets, W, twins = mr.e2e_case(name)
    nrot = W.shape[1]
    assert ref["U"] == X.shape[0] - 1 and ref["rot"].shape == (len(sets), nrot, 3)
    assert ref["msize"][5] == 0 and ref["msize"][6] == 0 and (ref["cnt"][5:7] == 0).all()
    assert ref["msize"][7] == ref["U"]
    # the whole universe: the sum of all ranks is a constant of U alone (ties averaged), so every rotation counts; the h
    # largest of them are not (a tie changes the multiset of ranks)
    assert stat == "mean50" or (ref["cnt"][7] == nrot).all()
    live = ref["msize"] >= 1
    assert (ref["cnt"][live] >= 0).all() and (ref["cnt"][live] <= nrot).all()
    if stat == "mean":
        flip = 2 * (ref["U"] + 1)
        assert (ref["rot"][live, :, 0] + ref["rot"][live, :, 1] == (flip * ref["msize"][live])[:, None]).all()
    assert (ref["pi"] > 0) == (mode == "shrunk")


def test_numpy_ranks_are_the_exact_ranks():
    rng = np.random.default_rng(3)
    t = np.round(rng.normal(size=(57, 9)) * 3) / 3
    t[:, 2] = 0.5
    t[5, 3], t[6, 3], t[7, 3] = np.inf, -np.inf, -0.0
    for stat in mr.STATS:
        a, b, c = mr.keys_np(t, stat)
        for key in (a, b, c):
            if key is None:
                continue
            got = mr.rank2_np(key)
            for k in range(t.shape[1]):
                assert list(got[:, k]) == mr._rank2_exact([float(v) for v in key[:, k]])
            assert got.min() >= 2 and got.max() <= 2 * t.shape[0] and (got.sum(axis=0) == t.shape[0] * (t.shape[0] + 1)).all()


def test_numpy_sides_are_the_headers_words():
    rng = np.random.default_rng(4)
    nu = 41
    t = np.round(rng.normal(size=(nu, 6)) * 2) / 2
    for stat in mr.STATS:
        a, b, c = mr.keys_np(t, stat)
        Ra, Rc = mr.rank2_np(a), mr.rank2_np(c)
        Rb = mr.rank2_np(b) if b is not None else None
        for mem in ([3], [1, 2], [0, 5, 9, 11, 40], list(range(nu))):
            got = mr.sides_np(Ra, Rb, Rc, mem, stat, nu)
            m = len(mem)
            for k in range(t.shape[1]):
                ra, rc = sorted(Ra[mem, k]), sorted(Rc[mem, k])
                if stat == "mean":
                    want = [sum(ra), 2 * m * (nu + 1) - sum(ra), sum(rc)]
                elif stat == "floormean":
                    want = [sum(ra), int(Rb[mem, k].sum()), sum(rc)]
                else:
                    h = m // 2 + 1
                    want = [sum(ra[-h:]), 2 * h * (nu + 1) - sum(ra[:h]), sum(rc[-h:])]
                assert list(got[k]) == want, (stat, mem, k)


def test_shrink_against_the_50_digit_form():
    worst = mr.measure_shrink()
    for name, (dc, dpi) in worst.items():
        print(f"[measure] shrink {name}: c within {dc:.3g} relative, pi within {dpi:.3g}")
        assert dc <= mr.FACTOR * mr.MEASURED["shrink"], (name, dc)
        assert dpi <= mr.FACTOR * mr.MEASURED["shrink"], (name, dpi)
    assert max(v[0] for v in worst.values()) >= mr.MEASURED["shrink"] / 8       # (the measured value is not a loose guess)


def test_the_shrink_cases_cover_what_they_name():
    seen = {}
    for name in mr.SHRINK_CASES:
        t, u, s02, nu = mr.shrink_case(name)
        info = {}
        c, pi, _ = mr.shrink_mp([float(x) for x in t], u, s02, nu, info)
        got, prop = engine.romer_shrink(t, u, s02, nu)
        seen[name] = (float(pi), info, got)
    assert seen["null"][0] <= 0 and (seen["null"][2] == 1.0).all()                # no shrink: the factor's bits are 1.0
    assert 0 < seen["tiny"][0] < 0.01 and seen["tiny"][1]["ntarget"] == 1
    assert seen["most"][0] > 0.99
    assert seen["clamp_lo"][1]["low"] >= 1 and seen["clamp_hi"][1]["high"] >= 1
    assert np.isinf(mr.shrink_case("inf")[3]) and mr.shrink_case("nodf0")[3] == 4.0
    for name in mr.SHRINK_CASES[1:]:
        assert ((seen[name][2] > 0) & (seen[name][2] < 1)).all(), name
    # a NaN t counts as 0.0; U = 0 writes nothing but pi = 0
    t = np.array([0.3, np.nan, -2.0, 4.0, 0.1, -0.2, 0.7, 5.0])
    a, pa = engine.romer_shrink(t, 0.5, 1.0, 9.0)
    b, pb = engine.romer_shrink(np.where(np.isnan(t), 0.0, t), 0.5, 1.0, 9.0)
    assert np.array_equal(a.view(np.int64), b.view(np.int64)) and pa == pb
    assert engine.romer_shrink(np.zeros(0), 0.5, 1.0, 9.0)[1] == 0.0


@pytest.mark.parametrize("stat", mr.STATS)
def test_finish_bit_for_bit(stat):
    rng = np.random.default_rng(8)
    m, q, nfit, nrot = 23, 2, 2, 199
    cnt = rng.integers(0, nrot + 1, size=(m, 3, q, nfit)).astype(np.int32)
    cnt[3] = cnt[4]                                                    # tied p-values
    msize = rng.integers(1, 50, size=(m, nfit)).astype(np.float64)
    msize[5, 0] = 0
    msize[9, :] = 0
    msize[11, 1] = mr.MEAN50_MAX + 1
    msize[12, 1] = mr.MEAN50_MAX
    out = engine.romer_finish(cnt, msize, nrot, stat)
    for f in range(nfit):
        for j in range(q):
            want = mr.finish_np(cnt[:, :, j, f], msize[:, f], nrot, stat)
            assert np.array_equal(out[:, :, j, f].view(np.int64), want.view(np.int64)), (f, j)
    assert np.isnan(out[9, 1:]).all() and (out[9, 0] == 0).all()
    assert np.isnan(out[11, 1:, :, 1]).all() == (stat == "mean50") and np.isfinite(out[12, 1:, :, 1]).all()
