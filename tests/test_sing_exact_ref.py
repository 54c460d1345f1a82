"""The references of replaid.sing.exact against each other (host only): the pinned form of include/plaidhip.h in numpy,
the literal form (scipy's rankdata, np.median, 1.4826) and the same operations in exact rationals
(tests/helpers/sing_mad.py); the window identity and the crossing search the device uses in place of a sort; the affine
relation to the oracle's replaid.sing; the committed expected matrices of the pbmc3k-50 fixture; and the Python entry's
export and argument checks, which need no device."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import exact_ref as er
from tests.helpers import sing_mad as sm

U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sized_sets(g, sizes, seed=17):
    rng = np.random.default_rng(seed)
    Gi, Gp = [], [0]
    for k in sizes:
        Gi.extend(sorted(rng.choice(g, size=k, replace=False)))
        Gp.append(len(Gi))
    return np.array(Gp, dtype=np.int32), np.array(Gi, dtype=np.int32)


def _columns(N, seed=3):
    """tied (-0.0 beside 0.0), tie-free, constant and NaN columns"""
    rng = np.random.default_rng(seed)
    X = np.empty((N, 5))
    X[:, 0] = np.round(rng.normal(0, 2, size=N), 0)
    X[rng.random(N) < 0.1, 0] = -0.0
    X[:, 1] = rng.permutation(N).astype(np.float64)
    X[:, 2] = 4.0
    X[:, 3] = np.round(rng.normal(0, 1, size=N), 0)
    X[N // 2, 3] = np.nan
    X[:, 4] = np.round(rng.normal(0, 30, size=N), 0)
    return X


def pbmc_case(golden_dir):
    """the inputs of the committed tests/golden/sing_exact_pbmc3k50.npz: the 50-cell fixture, hallmarks.gmt as the up sets
    and the same collection in reverse column order as the down sets.  The file holds sing_mad.pinned() of them, centred:
        np.savez_compressed(path, **sing_mad.pinned(X.toarray(), Gp, Gi, Dp, Di, True))"""
    import plaid_amd
    d = dict(np.load(os.path.join(golden_dir, "pbmc3k50.npz"), allow_pickle=False))
    X = sp.csc_matrix((d["x"], d["i"], d["p"]), shape=tuple(d["dim"]))
    Xn = plaid_amd.NamedMatrix(X, d["rownames"], d["colnames"])
    matG = plaid_amd.gmt2mat(plaid_amd.read_gmt(os.path.join(golden_dir, "hallmarks.gmt")))
    G = sp.csc_matrix(matG.values)
    m = G.shape[1]
    matD = plaid_amd.NamedMatrix(G[:, ::-1].tocsc(), matG.rownames, [f"down{j}" for j in range(m)])
    return Xn, matG, matD


@pytest.mark.parametrize("N", [5, 60, 97, 512])
@pytest.mark.parametrize("center", [True, False])
def test_three_forms_agree_bit_for_bit(N, center):
    X = _columns(N)
    sizes = sorted({k for k in (0, 1, 2, 3, 4, 63, 64, 65, N // 2, N - 1, N) if 0 <= k <= N})
    Gp, Gi = _sized_sets(N, sizes)
    Dp, Di = _sized_sets(N, sizes[::-1], seed=23)
    a = sm.pinned(X, Gp, Gi, Dp, Di, center)
    b = sm.literal(X, Gp, Gi, Dp, Di, center)
    for name in sm.NAMES:
        er.assert_same_bits(a[name], b[name], f"pinned vs literal {name} N={N}")
    if N <= 97:
        c = sm.rational(X, Gp, Gi, Dp, Di, center)
        for name in sm.NAMES:
            er.assert_same_bits(a[name], c[name], f"pinned vs rationals {name} N={N}")
    up = sm.pinned(X, Gp, Gi, None, None, center)
    assert sorted(up) == ["UpDispersion", "UpScore"]
    er.assert_same_bits(up["UpScore"], a["UpScore"], "up only")
    er.assert_same_bits(up["UpDispersion"], a["UpDispersion"], "up only")
    assert np.isnan(a["UpScore"][:, 3]).all() and np.isnan(a["TotalDispersion"][:, 3]).all()      # the NaN column
    j0, jN = sizes.index(0), sizes.index(N)
    fin = [0, 1, 2, 4]
    assert np.isnan(a["UpScore"][[j0, jN]][:, fin]).all()                                           # k = 0, k = N: 0 / 0
    assert np.isnan(a["UpDispersion"][j0, fin]).all() and np.isfinite(a["UpDispersion"][jN, fin]).all()
    assert np.isnan(a["TotalScore"][len(sizes) - 1 - j0, fin]).all()                               # an empty down column
    assert (a["UpDispersion"][:, 2] [1:] == 0.0).all()                                              # one tie group


def test_down_dispersion_is_the_dispersion_of_the_ranks():
    N = 97
    X = _columns(N)
    Gp, Gi = _sized_sets(N, [1, 2, 5, 6, 40, 41, N])
    a = sm.pinned(X, Gp, Gi, Gp, Gi, True)
    er.assert_same_bits(a["DownDispersion"], a["UpDispersion"], "reflection")


def test_hand_case():
    X = np.array([[5.0], [1.0], [3.0], [3.0], [2.0]])
    assert sm.min_ranks(X[:, 0]).tolist() == [5, 1, 3, 3, 2]
    Gp = np.array([0, 3, 5], dtype=np.int32)
    Gi = np.array([0, 2, 3, 0, 1], dtype=np.int32)
    for form in (sm.pinned, sm.literal, sm.rational):
        c = form(X, Gp, Gi, None, None, True)
        u = form(X, Gp, Gi, None, None, False)
        assert u["UpScore"][0, 0] == (11.0 / 3.0 - 2.0) / 2.0 and c["UpScore"][0, 0] == (11.0 / 3.0 - 2.0) / 2.0 - 0.5
        assert u["UpScore"][1, 0] == 0.5 and c["UpScore"][1, 0] == 0.0
        assert c["UpDispersion"][:, 0].tolist() == [0.0, 1.4826 * 2.0]


@pytest.mark.parametrize("seed", range(6))
def test_window_identity_and_crossing_search_equal_a_sort(seed):
    rng = np.random.default_rng(seed)
    for k in list(range(1, 40)) + [63, 64, 65, 128, 129, 500]:
        hi = [3, 10, 1000][seed % 3] * k
        s = np.sort(rng.integers(1, hi + 1, size=k)).astype(np.int64)
        M2 = int(2 * s[k // 2] if k % 2 else s[k // 2 - 1] + s[k // 2])
        d2 = np.sort(np.abs(2 * s - M2))
        for j in sorted({1, max(k // 2, 1), k // 2 + 1, k}):
            if j > k:
                continue
            assert sm.kth_dev2_windows(s, M2, j) == d2[j - 1], (k, j)
            assert sm.kth_dev2_crossing(s, M2, j)[0] == d2[j - 1], (k, j)
        assert sm.mad4_device(s) == sm.mad4(s), k


def test_centred_up_score_is_the_affine_map_of_the_oracle_sing():
    """replaid.sing = mean(r) / N - 0.5, so score = (N (sing + 0.5) - low) / (N - k) - 0.5.  The reference's mean is
    sum / (k + 1e-8) (R/plaid.R:75-76, kept by the oracle); that factor is taken out here in exact rationals, with the
    double fl(k + 1e-8) the oracle divides by, before the map.  Bound.  The oracle divides every rank by N and subtracts
    0.5 (two roundings of values at most 1: 2 u), weighs the term by fl(1 / fl(k + 1e-8)) (a division and a product: 2 u
    relative on a value at most 0.5) and sums k terms in some order (k - 1 roundings of partial sums at most 0.5: at most
    k u / 2): within (k + 4) u of the exact value.  The map, evaluated in exact rationals from the oracle's double,
    multiplies that by N / (N - k).  The pinned form rounds mean and mean - low (values at most N: 2 N u, over N - k), the
    quotient and the centring (values at most 1: 2 u).  Together N (k + 6) u / (N - k) + 2 u."""
    from oracle import plaid_oracle as po
    N, n = 300, 6
    rng = np.random.default_rng(5)
    X = np.round(rng.normal(0, 3, size=(N, n)), 0)
    sizes = [1, 2, 7, 50, 151, N - 1]
    Gp, Gi = _sized_sets(N, sizes)
    G = sp.csc_matrix((np.ones(len(Gi)), Gi, Gp), shape=(N, len(sizes)))
    names = [f"g{i}" for i in range(N)]
    sing = po.replaid_sing(X, names, G, names)
    got = sm.pinned(X, Gp, Gi, None, None, True)["UpScore"]
    worst = 0.0
    for j, k in enumerate(sizes):
        bound = N * (k + 6) * U / (N - k) + 2 * U
        for c in range(n):
            so = Fraction(float(sing[j, c])) * Fraction(float(np.float64(1e-8) + np.float64(k))) / k
            mapped = (N * (so + Fraction(1, 2)) - Fraction(k + 1, 2)) / (N - k) - Fraction(1, 2)
            err = abs(Fraction(float(got[j, c])) - mapped)
            worst = max(worst, float(err) / bound)
            assert err <= bound, (j, c, float(err), bound)
    print(f"worst |score - map(sing)| / bound = {worst:.3g}")


def test_golden_file_is_the_pinned_form_of_the_fixture(golden_dir):
    import plaid_amd
    Xn, matG, matD = pbmc_case(golden_dir)
    Gp, Gi = plaid_amd.aligned_pattern(Xn, matG)
    Dp, Di = plaid_amd.aligned_pattern(Xn, matD)
    exp = dict(np.load(os.path.join(golden_dir, "sing_exact_pbmc3k50.npz"), allow_pickle=False))
    got = sm.pinned(Xn.values.toarray(), Gp, Gi, Dp, Di, True)
    assert sorted(exp) == sorted(sm.NAMES)
    for name in sm.NAMES:
        er.assert_same_bits(got[name], exp[name], name)
    assert np.isfinite(exp["TotalScore"]).any()


def test_python_entry_is_exported_and_checks_its_arguments_without_a_device():
    import plaid_amd
    from plaid_amd import _lib
    assert "replaid_sing_exact" in plaid_amd.__all__ and callable(plaid_amd.replaid_sing_exact)
    assert "sing_exact_multi" in plaid_amd.__all__ and hasattr(plaid_amd.Context, "sing_exact")
    assert hasattr(plaid_amd.Context, "dev_sing_mad")
    header = open(os.path.join(ROOT, "include", "plaidhip.h")).read()
    for fn in ("plaidhip_sing_exact", "plaidhip_sing_exact_multi", "plaidhip_dev_sing_mad_f64"):
        assert re.search(r"\bint\s+" + fn + r"\s*\(", header), f"{fn} is not declared in include/plaidhip.h"
        assert fn in _lib.SIGNATURES and hasattr(_lib.load(), fn)
    assert "as recalled" in header.lower()
    rows = ["a", "b", "c", "d"]
    X = plaid_amd.NamedMatrix(np.arange(8.0).reshape(4, 2), rows, ["s1", "s2"])
    G = plaid_amd.NamedMatrix(np.eye(4)[:, :2], rows, ["set1", "set2"])
    D3 = plaid_amd.NamedMatrix(np.eye(4)[:, :3], rows, ["d1", "d2", "d3"])
    with pytest.raises(ValueError, match="matD has 3 columns, matG 2"):
        plaid_amd.replaid_sing_exact(X, G, D3)
    with pytest.raises(ValueError, match="down sets have 2 columns, the up sets 1"):
        plaid_amd.sing_exact_multi(X.values, [0, 1], [0], [0, 1, 2], [0, 1])
    g = 131072 + 1                                           # one row over the dispersion kernel's bitmap
    big = plaid_amd.NamedMatrix(np.zeros((g, 1)), [f"g{i}" for i in range(g)], ["s1"])
    Gb = plaid_amd.NamedMatrix(sp.csc_matrix((np.ones(2), ([0, 1], [0, 0])), shape=(g, 1)), big.rownames, ["set1"])
    with pytest.raises(plaid_amd.PlaidHipError) as e:
        plaid_amd.replaid_sing_exact(big, Gb)
    assert e.value.code == _lib.EUNSUPPORTED and "131072" in str(e.value)
    with pytest.raises(plaid_amd.PlaidHipError) as e:
        plaid_amd.sing_exact_multi(big.values, [0, 2], [0, 1])
    assert e.value.code == _lib.EUNSUPPORTED
    # the C entry refuses the same before it looks for a device (there may be none here)
    lib = _lib.load()
    Xb = np.zeros((g, 1), order="F")
    Gp, Gi = np.array([0, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    out = np.zeros((1, 1), order="F")
    rc = lib.plaidhip_sing_exact(None, None, None, Xb.ctypes.data, g, 1, Gp.ctypes.data, Gi.ctypes.data, None, None, 1, 1,
                                 None, out.ctypes.data, None, None, out.ctypes.data, None)
    assert rc == _lib.EUNSUPPORTED
    rc = lib.plaidhip_sing_exact(None, None, None, Xb.ctypes.data, g, 1, Gp.ctypes.data, Gi.ctypes.data, None, None, 1, 1,
                                 out.ctypes.data, out.ctypes.data, None, None, None, None)
    assert rc == _lib.EINVAL                                  # a total without down sets
