"""plaid.gsea on the host: the three restatements of the pinned statistic agree, the generator's known answers hold, the
generated placements are permutations, the wrappers' argument checks run without a device, and every layer declares the
entries (include/plaidhip.h: plaidhip_gsea)."""
import os
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import gsea_perm_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(N, seed, weights):
    rng = np.random.default_rng(seed)
    stat = np.round(rng.normal(size=N), 1)                      # ties: the stable order matters
    if weights == "one":
        w = np.ones(N)
    elif weights == "int":
        w = rng.integers(0, 2**20, size=N).astype(np.float64)
    else:
        w = np.abs(rng.normal(size=N))
    pos = ref.observed_placement(stat)
    return pos, ref.walk_weights(pos, w), rng


SIZES = (0, 1, 2, 5, 63, 64, 65)


def _near(v, place, mem, Wpos, bound, what):
    """v within `bound` of the rational score; where the rational extremes tie in magnitude (score 0) a rounding may pick
    either of them in fp64"""
    mx, mn = ref.es_fraction(place, mem, Wpos, parts=True)
    if mx == -mn:
        assert min(abs(Fraction(v)), abs(abs(Fraction(v)) - mx)) <= bound, what
    else:
        assert abs(Fraction(v) - ref.es_fraction(place, mem, Wpos)) <= bound, what


@pytest.mark.parametrize("N", [4, 64, 65, 130])
@pytest.mark.parametrize("weights", ["one", "int"])
def test_three_forms_agree_bit_for_bit_where_the_sums_are_exact(N, weights):
    pos, Wpos, rng = _case(N, 11 + N, weights)
    Gp, Gi = ref.make_sets(N, SIZES + (N - 1, N), seed=N)
    P = ref.placements(N, 5, seed=77)
    for j in range(len(Gp) - 1):
        mem = Gi[Gp[j]:Gp[j + 1]].astype(np.int64)
        for place in [pos] + [P[:, b] for b in range(P.shape[1])]:
            a, b, f = ref.es_numpy(place, mem, Wpos), ref.es_literal(place, mem, Wpos), ref.es_fraction(place, mem, Wpos)
            if f is None:
                assert a != a and b != b
                continue
            assert a == b, (N, j)
            _near(a, place, mem, Wpos, Fraction(3, 2**53), (N, j))         # two divisions and a subtraction


@pytest.mark.parametrize("N", [64, 65, 130])
def test_three_forms_agree_within_the_bound_for_general_weights(N):
    pos, Wpos, rng = _case(N, 5 + N, "normal")
    Gp, Gi = ref.make_sets(N, SIZES + (N - 1,), seed=N + 1)
    P = ref.placements(N, 5, seed=3)
    for j in range(len(Gp) - 1):
        mem = Gi[Gp[j]:Gp[j + 1]].astype(np.int64)
        k = len(mem)
        bound = Fraction(2 * k + 4, 2**53)
        for place in [pos] + [P[:, b] for b in range(P.shape[1])]:
            a, b, f = ref.es_numpy(place, mem, Wpos), ref.es_literal(place, mem, Wpos), ref.es_fraction(place, mem, Wpos)
            if f is None:
                continue
            _near(a, place, mem, Wpos, bound, (N, j))
            _near(b, place, mem, Wpos, bound, (N, j))


def test_first_and_last_of_four_scores_exactly_zero():
    pos = np.arange(4, dtype=np.int32)
    mem = np.array([0, 3])
    for es in (ref.es_numpy, ref.es_literal):
        v = es(pos, mem, np.ones(4))
        assert v == 0.0 and not np.signbit(v)
    assert ref.es_fraction(pos, mem, np.ones(4)) == 0


def test_zero_weight_members_fall_back_to_the_unweighted_walk():
    pos = np.arange(10, dtype=np.int32)
    w = np.array([3.0, 0, 0, 2, 0, 1, 0, 0, 4, 0])
    mem = np.array([1, 4, 9])                                     # all of weight 0
    assert ref.es_numpy(pos, mem, w) == ref.es_numpy(pos, mem, np.ones(10)) == ref.es_literal(pos, mem, w)
    assert ref.es_fraction(pos, mem, w) == ref.es_fraction(pos, mem, np.ones(10))


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for counter, key, want in kat:
        assert ref.philox4x32_10(counter, key) == want
    # the vectorised form the placements use is the same generator
    seed = (0x299f31d0 << 32) | 0xa4093822
    o0, o1 = ref._philox_o0_o1(np.array([7, 65536], dtype=np.uint64), 12345, seed)
    for i, a, b in zip((7, 65536), o0, o1):
        w = ref.philox4x32_10((i, 12345, 0, 0), (0xa4093822, 0x299f31d0))
        assert (int(a), int(b)) == w[:2]


@pytest.mark.parametrize("g", [1, 2, 65, 1000])
def test_generated_placements_are_permutations_and_depend_on_gene_and_permutation_alone(g):
    P = ref.placements(g, 7, seed=2**40 + 3)
    for b in range(7):
        assert np.array_equal(np.sort(P[:, b]), np.arange(g))
    assert np.array_equal(ref.placements(g, 3, seed=2**40 + 3, b0=4), P[:, 4:7])


def test_null_statistics_and_bh():
    null = np.array([0.5, -0.25, 0.0, 0.5, 0.75, -0.5])
    s = ref.null_stats(0.5, null)
    assert list(s[6:10]) == [3.0, 5.0, 4.0, 3.0] and s[10] == 1.75 and s[11] == -0.75
    assert s[1] == 0.5 / (1.75 / 4.0) and s[2] == min(6.0 / 4.0, 4.0 / 5.0) and s[4] == 3.0
    q = ref.bh(np.array([0.01, np.nan, 0.04, 0.03, 0.5]))
    assert np.isnan(q[1]) and np.allclose(q[[0, 2, 3, 4]], [0.04, 0.04 * 4 / 3, 0.04 * 4 / 3, 0.5])


def test_wrapper_argument_checks_need_no_device():
    import plaid_amd
    from plaid_amd import engine
    st = np.zeros(10)
    with pytest.raises(ValueError, match="nperm"):
        engine.check_gsea_args(st, st + 1, None, 0)
    with pytest.raises(ValueError, match="weight"):
        engine.check_gsea_args(st, st - 1, None, 10)
    with pytest.raises(ValueError, match="weight"):
        engine.check_gsea_args(st, st + np.nan, None, 10)
    with pytest.raises(ValueError, match="one shape"):
        engine.check_gsea_args(st, np.ones(9), None, 10)
    with pytest.raises(ValueError, match="perm"):
        engine.check_gsea_args(st, st + 1, np.zeros((9, 3), dtype=np.int32), 10)
    big = np.zeros(engine.GSEA_KS_MAX_GENES + 1)
    with pytest.raises(plaid_amd.PlaidHipError) as e:
        engine.check_gsea_args(big, big + 1, None, 10)
    assert e.value.code == 4
    s, w, p, n = engine.check_gsea_args(st, st + 1, np.zeros((10, 3), dtype=np.int32), 99)
    assert s.shape == (10, 1) and n == 3 and p.flags.f_contiguous
    with pytest.raises(ValueError, match="gseaParam"):
        plaid_amd.plaid_gsea(plaid_amd.NamedMatrix(st, [f"g{i}" for i in range(10)]), {"a": ["g1"]}, gseaParam=-1)


def test_every_layer_declares_the_entries():
    import re

    from plaid_amd import _lib, engine

    def text(*path):
        return open(os.path.join(ROOT, *path)).read()

    header = text("include", "plaidhip.h")
    for name in ("plaidhip_gsea", "plaidhip_gsea_multi", "plaidhip_gsea_permutations"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header) and name in _lib.SIGNATURES
    assert re.search(r"#\s*define\s+PLAIDHIP_GSEA_PERM_BLOCK\s+64\b", header) and re.search(r"\bRECALLED\b", header)
    assert hasattr(engine.Context, "gsea") and len(engine.GSEA_COLUMNS) == 12 == len(ref.COLUMNS)
    call_h = text("plaid_amd", "csrc", "call.h")
    assert re.search(r"\bkGsea\s*=\s*14\b", call_h) and re.search(r"\bCall\s+gsea_call\s*\(", call_h)
    multi = text("plaid_amd", "csrc", "multi.cpp")
    assert re.search(r"\bint\s+plaidhip_debug_gsea_sharded_on_one_device\s*\(", multi)
    assert re.search(r"case\s+kGsea\s*:\s*return\s+check_gsea_call\s*\(", multi)
    shim = text("r-pkg", "src", "plaidhip_R.c")
    assert re.search(r"\bplaidhip_gsea\s*\(", shim) and "R_plaidhip_gsea" in shim
    assert re.search(r"\bplaid\.gsea\b", text("r-pkg", "NAMESPACE"))
    assert re.search(r"\bplaid\.gsea\s*<-\s*function\b", text("r-pkg", "R", "plaid-hip.R"))
