"""replaid.ssgsea.exact without a GPU: the test helper's literal walk against its closed form and against exact rationals,
the declarations of the new entry points in the header, the ctypes table, the R shim and NAMESPACE, and the argument
checks that run before any device is touched."""
import math
import os
import re

import numpy as np
import pytest

from tests.helpers import ssgsea_walk as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tied(g, n, seed, levels=4):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, levels, size=(g, n)).astype(np.float64)
    X[rng.random((g, n)) < 0.1] *= -1.0                     # -0.0 among the zeros
    return X


def _sets(g, sizes, seed):
    rng = np.random.default_rng(seed)
    Gi, Gp = [], [0]
    for k in sizes:
        Gi.extend(sorted(rng.choice(g, size=k, replace=False)))
        Gp.append(len(Gi))
    return np.array(Gp, dtype=np.int32), np.array(Gi, dtype=np.int32)


@pytest.mark.parametrize("alpha", [0.0, 0.25, 1.0, 2.0])
@pytest.mark.parametrize("scale", [False, True])
def test_literal_walk_equals_the_closed_form(alpha, scale):
    g, n = 40, 6
    X = _tied(g, n, 1)
    X[:, 5] = 3.0                                            # an all-equal column
    Gp, Gi = _sets(g, [0, 1, 3, 17, g - 1, g], 2)
    walk = sw.walk_scores(X, Gp, Gi, alpha, scale)
    closed = sw.closed_form(X, Gp, Gi, alpha, scale)
    assert np.array_equal(np.isnan(walk), np.isnan(closed))
    assert np.isnan(closed[[0, 5]]).all(), "k = 0 and k = N are 0 / 0"
    ok = ~np.isnan(closed)
    np.testing.assert_allclose(walk[ok], closed[ok], rtol=0, atol=1e-13 * max(1.0, np.abs(closed[ok]).max()))


@pytest.mark.parametrize("norm", [False, True])
def test_norm_and_nan_columns(norm):
    g, n = 30, 5
    X = _tied(g, n, 3)
    Gp, Gi = _sets(g, [1, 4, 12, g - 1], 4)
    S = sw.closed_form(X, Gp, Gi, 0.5, True, norm)
    walk = sw.walk_scores(X, Gp, Gi, 0.5, True, norm)
    np.testing.assert_allclose(walk, S, rtol=0, atol=1e-13)
    if norm:
        plain = sw.closed_form(X, Gp, Gi, 0.5, True, False)
        assert np.array_equal(S, plain / (plain.max() - plain.min()))
    X[7, 2] = np.nan
    S = sw.closed_form(X, Gp, Gi, 0.5, True, norm)
    if norm:
        assert np.isnan(S).all(), "one NaN makes diff(range(es)) NaN"
    else:
        assert np.isnan(S[:, 2]).all() and not np.isnan(np.delete(S, 2, axis=1)).any()


@pytest.mark.parametrize("alpha", [0.0, 0.25, 1.0])
def test_fraction_closed_form_equals_the_fp64_closed_form(alpha):
    g, n = 25, 3
    X = _tied(g, n, 5, levels=3)
    Gp, Gi = _sets(g, [0, 1, 2, 9, g - 1, g], 6)
    exact = sw.fraction_scores(X, Gp, Gi, alpha)
    S = sw.closed_form(X, Gp, Gi, alpha)
    for j in range(len(Gp) - 1):
        for c in range(n):
            if exact[j][c] is None:
                assert math.isnan(S[j, c])
            elif alpha in (0.0, 1.0):                       # sums exact: four correctly rounded operations
                assert abs(S[j, c] - float(exact[j][c])) <= 8 * 2.0 ** -53 * max(1.0, abs(float(exact[j][c])))
            else:
                assert abs(S[j, c] - float(exact[j][c])) <= 1e-14


def test_last_ranks_follow_r():
    x = np.array([[1.0], [1.0], [1.0], [0.0], [-0.0], [2.0]])
    assert sw.last_ranks(x)[:, 0].tolist() == [5.0, 4.0, 3.0, 2.0, 1.0, 6.0]     # rank(c(1,1,1,0,-0,2), ties = "last")


# ---------------------------------------------------------------------------------------------------- declarations
def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def _nargs(text, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", text, flags=re.S), re.S)
    assert m, f"{name} is not declared"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_ctypes_shim_and_namespace_declare_the_new_entries():
    from plaid_amd import _lib
    hdr = _read("include", "plaidhip.h")
    for name, nargs in (("plaidhip_ssgsea_exact", 13), ("plaidhip_ssgsea_exact_multi", 14),
                        ("plaidhip_dev_ssgsea_exact_operands_f64", 12), ("plaidhip_dev_ssgsea_exact_operands_csc_f64", 15)):
        assert _nargs(hdr, name) == nargs
        assert len(_lib.SIGNATURES[name]) == nargs
    shim = _read("r-pkg", "src", "plaidhip_R.c")
    for name, nargs in (("R_plaidhip_ssgsea_exact", 10), ("R_plaidhip_ssgsea_exact_multi", 11)):
        assert re.search(r'\{"' + name + r'", \(DL_FUNC\)&' + name + r", " + str(nargs) + r"\}", shim)
    rsrc = _read("r-pkg", "R", "plaid-hip.R")
    body = rsrc[rsrc.index("replaid.ssgsea.exact <- function("):]
    body = body[:body.index("\n}\n")]
    assert "alpha = 0.25, scale = TRUE, norm = FALSE" in body
    head, branch = body.split("if (length(dev) > 1L)", 1)
    assert "dev <- .devices()" in head and '.Call("R_plaidhip_ssgsea_exact_multi"' in branch.split("else")[0]
    assert "replaid.ssgsea.exact" in _read("r-pkg", "NAMESPACE")
    import plaid_amd
    assert callable(plaid_amd.replaid_ssgsea_exact) and callable(plaid_amd.ssgsea_exact_multi)
    assert hasattr(plaid_amd.Context, "ssgsea_exact")


# ---------------------------------------------------------------------------------------------------- argument checks
def _small():
    from plaid_amd import synth
    Gp, Gi = synth.geneset_csc(200, 7, kmin=3, kmax=30)
    X = synth.dense_columns(200, 0, 5)
    return X, Gp, Gi


def test_bad_arguments_are_refused_before_any_device():
    """the checks run before a context is created: they fail the same way on a machine without a GPU"""
    import scipy.sparse as sp

    import plaid_amd
    from plaid_amd import _lib
    X, Gp, Gi = _small()
    for a in (np.inf, -np.inf, np.nan):
        with pytest.raises(plaid_amd.PlaidHipError, match="alpha must be finite"):
            plaid_amd.ssgsea_exact_multi(X, Gp, Gi, alpha=a)
    with pytest.raises(plaid_amd.PlaidHipError, match="listed twice"):
        plaid_amd.ssgsea_exact_multi(X, Gp, Gi, devices=[0, 0])
    lib = _lib.load()
    Gp32, Gi32 = np.ascontiguousarray(Gp, dtype=np.int32), np.ascontiguousarray(Gi, dtype=np.int32)
    S = np.empty((len(Gp) - 1, X.shape[1]), order="F")
    Xf = np.asfortranarray(X)
    args = (200, X.shape[1], Gp32.ctypes.data, Gi32.ctypes.data, len(Gp) - 1, 0.25, 1, 0)
    for xv, s_out, what in ((None, S.ctypes.data, "null X"), (Xf.ctypes.data, None, "null S_out")):
        rc = lib.plaidhip_ssgsea_exact_multi(None, 1, None, None, xv, *args, s_out)
        assert rc != 0 and what in lib.plaidhip_last_error_string().decode()
    rc = lib.plaidhip_ssgsea_exact(None, None, None, Xf.ctypes.data, *args, S.ctypes.data)
    assert rc != 0 and "null plaidhip_ctx" in lib.plaidhip_last_error_string().decode()
    # a dgCMatrix whose row indices are not increasing inside a column
    Xs = sp.csc_matrix(np.eye(200)[:, :5] + np.eye(200)[:, 5:10])
    ind = Xs.indices.copy()
    ind[0], ind[1] = ind[1], ind[0]
    p_ = np.ascontiguousarray(Xs.indptr, dtype=np.int32)
    i_ = np.ascontiguousarray(ind, dtype=np.int32)
    x_ = np.ascontiguousarray(Xs.data)
    rc = lib.plaidhip_ssgsea_exact_multi(None, 1, p_.ctypes.data, i_.ctypes.data, x_.ctypes.data, *args, S.ctypes.data)
    assert rc != 0 and "not increasing" in lib.plaidhip_last_error_string().decode()
