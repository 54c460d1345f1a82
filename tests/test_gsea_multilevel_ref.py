"""The host restatement of plaid.gsea's multilevel p-values (tests/helpers/gsea_multilevel_ref.py; include/plaidhip.h:
plaidhip_gsea_multilevel) held to its own words and to exhaustive enumeration.

The estimator is a condition on the METHOD, not a tuning knob: at N = 28, k = 7 every one of the 1,184,040 subsets is
scored, so the exact tail of any target is known, and over 60 seeds per target at most 5 % of the runs may miss it by more
than 3 log2err, and none may stall."""
import os

import numpy as np
import pytest

from tests.helpers import gsea_edge_ref as er
from tests.helpers import gsea_multilevel_ref as ml
from tests.helpers import gsea_perm_ref as ref

SIDES = [(er.STD, 0), (er.STD, 1), (er.POS, 0), (er.NEG, 1)]


def test_philox_columns_is_philox():
    rng = np.random.default_rng(1)
    c = rng.integers(0, 2**32, size=(4, 50), dtype=np.uint64)
    key = (0x12345678, 0x9ABCDEF0)
    got = ml.philox_columns(c[0], c[1], 7, c[3], key)
    for q in range(50):
        assert tuple(int(w[q]) for w in got) == ref.philox4x32_10((c[0, q], c[1, q], 7, c[3, q]), key)


@pytest.mark.parametrize("N,k", [(65, 7), (65, 32), (64, 32), (65, 33), (65, 62), (28, 27), (28, 1)])
def test_initial_states(N, k):
    """the first min(k, N - k) distinct draws of words (d & 3) of the counters 0x80000000 | (d >> 2), or their complement"""
    seed, l, side = 0x1234567890ABCDEF, 5, 1
    key = (seed & 0xFFFFFFFF, seed >> 32)
    for slot in (0, 3):
        draws = [ml.below(ref.philox4x32_10((0x80000000 | (d >> 2), slot, k, 0x80000000 | (l << 1) | side), key)[d & 3], N)
                 for d in range(40 * N)]
        first = list(dict.fromkeys(draws))[:min(k, N - k)]
        want = sorted(first) if 2 * k <= N else sorted(set(range(N)) - set(first))
        got = ml.initial_state(N, k, slot, l, side, seed)
        assert len(got) == k and got.tolist() == want
    assert ml.initial_state(N, k, 0, l, side, seed).tolist() != ml.initial_state(N, k, 1, l, side, seed).tolist() or k in (N - 1,)
    if 1 < k < N - 1:
        assert ml.initial_state(N, k, 0, l, 0, seed).tolist() != ml.initial_state(N, k, 0, l, 1, seed).tolist()


@pytest.mark.parametrize("st,side", SIDES)
@pytest.mark.parametrize("weights", ["unit", "abs"])
def test_the_two_forms_are_one(st, side, weights):
    """a slot and a proposal at a time with the scalar Philox and extremes_numpy, or all slots of a step at once"""
    _, _, Wpos, gamma = ml.ruler_case(40, 6, st, side, weights, 3)
    a = ml.run_ruler(Wpos, 6, 2, side, st, gamma, 11, 7, 2, 1e-4, fast=False)
    b = ml.run_ruler(Wpos, 6, 2, side, st, gamma, 11, 7, 2, 1e-4, fast=True)
    assert a["stages"] == b["stages"] >= 3 and a["status"] == b["status"] and a["gap"] == b["gap"]
    assert np.array_equal(a["m"], b["m"]) and np.array_equal(a["s"], b["s"]) and np.array_equal(a["h"], b["h"])
    assert np.all(np.diff(a["m"]) > 0) and np.all(a["s"] <= 3)            # the levels rise strictly; s <= (n - 1) / 2
    assert np.all(a["h"][1:].min(axis=1) > a["m"][:-1])                    # every slot stands above the level it was given


def test_a_row_does_not_depend_on_gamma_max():
    _, _, Wpos, gamma = ml.ruler_case(65, 7, er.STD, 0, "int", 8)
    far = ml.run_ruler(Wpos, 7, 0, 0, er.STD, gamma, 4, 21, 2, 1e-50)
    assert far["status"] == ml.ESTIMATED and far["stages"] > 6
    for stage in (1, 3, 5):
        ga = float(far["m"][stage])                      # a target met exactly at a level, and one between two levels
        for target in (ga, 0.5 * (ga + float(far["m"][stage - 1]))):
            near = ml.run_ruler(Wpos, 7, 0, 0, er.STD, target, 4, 21, 2, 1e-50)
            assert near["stages"] == stage + 1 and np.array_equal(near["h"], far["h"][:stage + 1])
            assert ml.read_off(near, target) == ml.read_off(far, target)
            assert ml.read_off(far, target)[2:4] == (stage, ml.ESTIMATED)


def test_read_off_words():
    tr = {"stages": 3, "status": ml.FLOOR, "m": np.array([0.1, 0.2, 0.3]), "s": np.array([2, 1, 2], dtype=np.int32),
          "h": np.array([[0.0, 0.1, 0.1, 0.3, 0.4], [0.15, 0.2, 0.2, 0.2, 0.5], [0.25, 0.3, 0.3, 0.6, 0.7]])}
    q, e, lstar, status, c = ml.read_off(tr, 0.2)
    assert (lstar, status, c) == (1, ml.ESTIMATED, 4) and q == (2 / 5) * (4 / 5)
    assert e == np.sqrt(3 / 10 + 1 / 20) / np.log(2.0)
    q, e, lstar, status, c = ml.read_off(tr, 0.9)         # never reached: the last stage, an upper bound, c' = 1
    assert (lstar, status, c) == (2, ml.FLOOR, 0) and q == ((2 / 5) * (1 / 5)) * (1 / 5)


_enum = {}


def enumeration():
    if not _enum:
        rng = np.random.default_rng(5)
        N, k = 28, 7
        Wpos = np.abs(np.sort(rng.standard_normal(N))[::-1])               # weights |stat| of a sorted normal draw, in walk order
        hall = ml.all_scores(Wpos, k, er.STD, 0)
        assert len(hall) == 1184040
        _enum.update(Wpos=Wpos, hall=hall, sorted=np.sort(hall))
    return _enum


@pytest.mark.parametrize("tail", [2e-3, 3e-5, 0.0])
def test_against_exhaustive_enumeration(tail):
    """std, positive side: the exact tail of about 2e-3, 3e-5 and of the single best subset"""
    e = enumeration()
    hs = e["sorted"]
    gamma = float(hs[-1] if tail == 0.0 else hs[-int(round(tail * len(hs)))])
    exact = float(np.mean(e["hall"] >= gamma))
    assert exact == 1 / 1184040 if tail == 0.0 else abs(exact / tail - 1) < 0.05
    miss, ratios, errs = 0, [], []
    for seed in range(60):
        tr = ml.run_ruler(e["Wpos"], 7, 0, 0, er.STD, gamma, seed)         # n = 101, sweeps = 4, eps = 1e-50: the defaults
        qhat, log2err, _, status, _ = ml.read_off(tr, gamma)
        assert tr["status"] != ml.STALLED and status == ml.ESTIMATED
        ratios.append(np.log2(qhat / exact))
        errs.append(log2err)
        miss += abs(ratios[-1]) > 3 * log2err
    print(f"exact tail {exact:.3e}: log2(qhat / exact) mean {np.mean(ratios):+.3f} sd {np.std(ratios):.3f}, mean log2err "
          f"{np.mean(errs):.3f}, {miss} of 60 beyond 3 log2err")
    assert miss <= 3                                                        # 5 % of 60


def test_ml_min_zero_keeps_the_permutation_p_values():
    rng = np.random.default_rng(9)
    N, B = 60, 70
    stat = rng.standard_normal((N, 2))
    weight = np.abs(stat)
    Gp, Gi = ref.make_sets(N, [3, 9, 9, 20], seed=2)
    P = ref.placements(N, B, 5)
    plain = er.gsea_scored_ref(stat, weight, Gp, Gi, P)[er.STD][0]
    out0, ml0, _ = ml.table(stat, weight, Gp, Gi, P, 5, er.STD, 11, 1, 1e-50, ml_min=0)
    assert np.array_equal(out0, plain, equal_nan=True)
    out, mlt, _ = ml.table(stat, weight, Gp, Gi, P, 5, er.STD, 11, 1, 1e-50, ml_min=B + 1)   # every pair reports pvalML
    assert np.array_equal(mlt, ml0, equal_nan=True) and np.array_equal(out[:, 2, :], mlt[:, 0, :])
    for l in range(2):
        assert np.allclose(out[:, 3, l], ref.bh(mlt[:, 0, l]), rtol=0, atol=0)
    side_neg = plain[:, 0, :] < 0
    assert np.array_equal(mlt[:, 5, :], (1.0 + np.where(side_neg, plain[:, 9, :], plain[:, 8, :])) / (1.0 + B))
    assert np.all(mlt[:, 0, :] <= 1.0) and np.all(mlt[:, 4, :] > 0.0)


@pytest.mark.parametrize("case", ml.GOLDEN_RULERS, ids=ml.golden_key)
def test_recorded_traces_open_as_the_restatement_does(golden_dir, case):
    """the recorded rulers (k next to N = 4097; minutes to restate in full) against the restatement's stage 0 and the
    words every stage must obey"""
    N, k, st, side, weights, dseed, cseed, n, sweeps = case
    _, _, Wpos, gamma = ml.ruler_case(N, k, st, side, weights, dseed)
    rec, key = np.load(os.path.join(golden_dir, "gsea_ml_traces.npz")), ml.golden_key(case)
    m, s, h = rec[key + "_m"], rec[key + "_s"], rec[key + "_h"]
    pos = np.stack([ml.initial_state(N, k, i, 3, side, cseed) for i in range(n)])
    assert np.array_equal(h[0], ml.h_rows(pos, Wpos, st, side))
    assert np.array_equal(m, np.sort(h, axis=1)[:, (n + 1) // 2 - 1]) and np.array_equal(s, np.sum(h > m[:, None], axis=1))
    assert np.all(h[1:].min(axis=1) > m[:-1]) and h.shape == (len(m), n)
    end = int(rec[key + "_status"][0])
    assert end == (ml.ESTIMATED if m[-1] >= gamma else ml.STALLED if s[-1] == 0 else ml.FLOOR)
