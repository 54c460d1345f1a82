"""The argument checks of replaid.plage and replaid.zscore (multi.cpp: check_plage_call) through every entry and the sharded
test hook, without a GPU: every fault returns its status and text before any device is touched (there is none here), in
the order include/plaidhip.h states; a null context is reported after a bad argument, a bad device list before it."""
import numpy as np
import pytest

import plaid_amd
from plaid_amd import _lib, engine
from tests.helpers import plage_hooks

G_ROWS, N = 10, 4
GP = np.array([0, 3, 5], dtype=np.int32)
GI = np.array([0, 1, 2, 8, 9], dtype=np.int32)


def ptr(a):
    return None if a is None else a.ctypes.data


def call(which, X, g, n, Gp, Gi, m, tol, maxit, S, info, load):
    lib = _lib.load()
    G = (ptr(Gp), ptr(Gi), m)
    out = (ptr(S), ptr(info), ptr(load))
    rc = {
        "plage": lambda: lib.plaidhip_plage(None, ptr(X), g, n, *G, tol, maxit, *out),
        "plage_multi": lambda: lib.plaidhip_plage_multi(None, 2, None, None, ptr(X), g, n, *G, tol, maxit, *out),
        "plage_hook": lambda: plage_hooks.hook()(0, 3, -1, plage_hooks.PLAGE, None, None, ptr(X), g, n, *G, tol, maxit, *out),
        "zscore": lambda: lib.plaidhip_zscore(None, ptr(X), g, n, *G, ptr(S), ptr(info)),
        "zscore_multi": lambda: lib.plaidhip_zscore_multi(None, 2, None, None, ptr(X), g, n, *G, ptr(S), ptr(info)),
        "zscore_hook": lambda: plage_hooks.hook()(0, 3, -1, plage_hooks.ZSCORE, None, None, ptr(X), g, n, *G, tol, maxit, *out),
    }[which]()
    return rc, lib.plaidhip_last_error_string().decode()


def good():
    rng = np.random.default_rng(3)
    return dict(X=np.asfortranarray(rng.normal(size=(G_ROWS, N))), g=G_ROWS, n=N, Gp=GP, Gi=GI, m=2, tol=2.0 ** -40, maxit=1000,
                S=np.full((2, N), -7.0, order="F"), info=np.full((2, 6), -7.0, order="F"), load=np.full(5, -7.0))


BIG = np.array([0, 4097, 4099], dtype=np.int32)
COMMON = [   # name, change, status, the text -- in the order of the checks
    ("dims", dict(g=0), _lib.EINVAL, "bad dims g=0 n=4 m=2"),
    ("null Gp", dict(Gp=None), _lib.EINVAL, "null Gp"),
    ("one sample", dict(n=1), _lib.EINVAL, "{who}: 1 samples (at least 2)"),
    ("no sample", dict(n=0), _lib.EINVAL, "{who}: 0 samples (at least 2)"),
]
PLAGE_ONLY = [
    ("tol zero", dict(tol=0.0), _lib.EINVAL, "plage: tol = 0 (a positive number)"),
    ("tol negative", dict(tol=-1.0), _lib.EINVAL, "plage: tol = -1 (a positive number)"),
    ("tol nan", dict(tol=float("nan")), _lib.EINVAL, "plage: tol = nan (a positive number)"),
    ("maxit", dict(maxit=0), _lib.EINVAL, "plage: maxit = 0 (at least 1)"),
]
TAIL = [
    ("Gp start", dict(Gp=np.array([1, 3, 5], dtype=np.int32)), _lib.EINVAL, "{who}: Gp[0] = 1 (a column pointer starts at 0)"),
    ("Gp order", dict(Gp=np.array([0, 4, 3], dtype=np.int32)), _lib.EINVAL, "{who}: Gp[2] = 3 after 4"),
]
CAP = [("cap", dict(Gp=BIG, Gi=None), _lib.EINVAL, "plage: set 1 has 4097 members (at most 4096)")]
LAST = [
    ("null X", dict(X=None), _lib.EINVAL, "{who}: null X"),
    ("null S", dict(S=None), _lib.EINVAL, "{who}: null S_out"),
    ("null Gi", dict(Gi=None), _lib.EINVAL, "{who}: null Gi"),
    ("Gi high", dict(Gi=np.array([0, 1, 2, 8, 10], dtype=np.int32)), _lib.EINVAL, "{who}: Gi[4] = 10 (rows are 0..9)"),
]
FAULTS = {"plage": COMMON + PLAGE_ONLY + TAIL + CAP + LAST, "zscore": COMMON + TAIL + LAST}
CASES = [(w, e, f) for w in ("plage", "zscore") for e in ("", "_multi", "_hook") for f in FAULTS[w]]


@pytest.mark.parametrize("who,entry,fault", CASES, ids=[f"{w}{e}-{f[0]}" for w, e, f in CASES])
def test_every_fault_is_refused_before_any_device(who, entry, fault):
    _, change, status, text = fault
    a = {**good(), **change}
    rc, msg = call(who + entry, **a)
    assert rc == status and text.format(who=who) in msg, (rc, msg)
    for o in ("S", "info", "load"):
        if a[o] is not None:
            assert (a[o] == -7).all(), o


@pytest.mark.parametrize("who", ["plage", "zscore"])
def test_two_faults_report_the_earlier_check(who):
    faults = FAULTS[who]
    for q in range(len(faults) - 1):
        first, second = faults[q], faults[q + 1]
        if set(first[1]) & set(second[1]):
            continue
        a = {**good(), **second[1], **first[1]}
        rc, msg = call(who, **a)
        assert rc == first[2] and first[3].format(who=who) in msg, (first[0], second[0], msg)


def test_zscore_takes_a_set_above_the_cap_of_plage():
    rc, msg = call("zscore", **{**good(), "Gp": BIG, "Gi": None})
    assert rc == _lib.EINVAL and "zscore: null Gi" in msg


@pytest.mark.parametrize("which", ["plage", "zscore"])
def test_a_null_context_comes_after_a_bad_argument(which):
    rc, msg = call(which, **good())
    assert rc == _lib.EINVAL and "null plaidhip_ctx" in msg
    rc, msg = call(which, **{**good(), "n": 1})
    assert rc == _lib.EINVAL and "1 samples (at least 2)" in msg


def test_a_bad_device_list_comes_before_a_bad_argument():
    a = good()
    lib = _lib.load()
    tail = (None, None, ptr(a["X"]), G_ROWS, 1, ptr(GP), ptr(GI), 2)          # n = 1: a bad argument
    twice = np.array([0, 0], dtype=np.int32)
    assert lib.plaidhip_plage_multi(None, 0, *tail, 0.0, 0, ptr(a["S"]), None, None) == _lib.EINVAL
    assert "multi: ndev = 0" in lib.plaidhip_last_error_string().decode()
    assert lib.plaidhip_plage_multi(twice.ctypes.data, 2, *tail, 0.0, 0, ptr(a["S"]), None, None) == _lib.EINVAL
    assert "multi: device 0 listed twice" in lib.plaidhip_last_error_string().decode()
    assert lib.plaidhip_zscore_multi(None, 65, *tail, ptr(a["S"]), None) == _lib.EINVAL
    assert "multi: ndev = 65" in lib.plaidhip_last_error_string().decode()
    assert plage_hooks.hook()(0, 0, -1, plage_hooks.PLAGE, *tail, 0.0, 0, ptr(a["S"]), None, None) == _lib.EINVAL
    assert "debug_sharded: nshards = 0" in lib.plaidhip_last_error_string().decode()
    assert plage_hooks.hook()(0, 2, -1, 5, *tail, 0.0, 0, ptr(a["S"]), None, None) == _lib.EINVAL
    assert "debug_plage_sharded: method = 5" in lib.plaidhip_last_error_string().decode()


def test_csc_entries_want_the_slots():
    a = good()
    lib = _lib.load()
    rc = lib.plaidhip_plage_csc(None, None, None, ptr(a["X"]), G_ROWS, N, ptr(GP), ptr(GI), 2, 2.0 ** -40, 10, ptr(a["S"]), None, None)
    assert rc == _lib.EINVAL and "plage_csc: null Xp" in lib.plaidhip_last_error_string().decode()
    rc = lib.plaidhip_zscore_csc(None, None, None, ptr(a["X"]), G_ROWS, N, ptr(GP), ptr(GI), 2, ptr(a["S"]), None)
    assert rc == _lib.EINVAL and "zscore_csc: null Xp" in lib.plaidhip_last_error_string().decode()
    Xp = np.array([0, 2, 2, 2, 2], dtype=np.int32)
    Xi = np.array([3, 1], dtype=np.int32)
    rc = lib.plaidhip_plage_csc(None, ptr(Xp), ptr(Xi), ptr(a["X"]), G_ROWS, N, ptr(GP), ptr(GI), 2, 2.0 ** -40, 10, ptr(a["S"]),
                                None, None)
    assert rc == _lib.EINVAL and "plage: row indices of column 0 are not increasing (Xi[1] = 1 after 3)" in \
        lib.plaidhip_last_error_string().decode()


def test_no_sets_is_the_empty_result():
    a = {**good(), "Gp": np.array([0], dtype=np.int32), "Gi": None, "m": 0, "S": None, "info": None, "load": None}
    for which in ("plage_multi", "plage_hook", "zscore_multi", "zscore_hook"):
        rc, msg = call(which, **a)
        assert rc == _lib.OK, msg
    rc, msg = call("plage_multi", **{**a, "tol": 0.0})
    assert rc == _lib.EINVAL and "plage: tol = 0" in msg


def test_python_checks_and_exports():
    for name in ("replaid_plage", "replaid_zscore", "plage_multi", "zscore_multi"):
        assert name in plaid_amd.__all__ and callable(getattr(plaid_amd, name))
    assert callable(engine.Context.plage) and callable(engine.Context.zscore)
    assert engine.PLAGE_MAX_SET == 4096 and engine.PLAGE_TOL == 2.0 ** -40
    assert engine.PLAGE_COLUMNS == ("size", "lambda", "explained", "iterations", "residual", "converged")
    X = plaid_amd.NamedMatrix(np.zeros((3, 2)), ["a", "b", "c"], ["s1", "s2"])
    G = plaid_amd.NamedMatrix(np.ones((3, 1)), ["a", "b", "c"], ["set"])
    with pytest.raises(ValueError, match="maxSize = 4097 \\(at most 4096 members\\)"):
        plaid_amd.replaid_plage(X, G, maxSize=4097)
    with pytest.raises(ValueError, match="tol = 0"):
        plaid_amd.replaid_plage(X, G, tol=0)
    with pytest.raises(ValueError, match="tol = nan"):
        plaid_amd.replaid_plage(X, G, tol=float("nan"))
    with pytest.raises(ValueError, match="maxit = 0"):
        plaid_amd.replaid_plage(X, G, maxit=0)
