"""plaid.test.contrasts without a device: the argument checks of the C entries (status and text, before any device is
touched: the context entries are called with a null context, which is refused only after the arguments), the host API's
handling of Y, names and sorting against plaid_test's on a stub context, and the R shim's new routine."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import plaid_amd
from plaid_amd import _lib, engine
from tests.helpers import sharded_hooks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_i32 = lambda *v: np.array(v, dtype=np.int32)   # noqa: E731


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


BASE = dict(X=np.ones((4, 3), order="F"), g=4, n=3, Y=np.asfortranarray(_i32([0, 1], [1, -1], [0, 0])), C=2, Gp=_i32(0, 2, 4),
            Gi=_i32(0, 1, 2, 3), m=2, gsetX=None, tests=7, metap=0, out=np.zeros((2, 6, 2), order="F"))
CSC = dict(Xp=_i32(0, 2, 3, 4), Xi=_i32(0, 1, 2, 3), X=np.array([1.0, 2.0, 3.0, 4.0]))


def _call(entry, **kw):
    """(status, text) of one entry: "dense" / "csc" on a null context, "multi" on one device, "hook" on two shards"""
    a = dict(BASE, Xp=None, Xi=None)
    if entry == "csc":
        a.update(CSC)
    a.update(kw)
    lib = _lib.load()
    tail = (a["g"], a["n"], _ptr(a["Y"]), a["C"], _ptr(a["Gp"]), _ptr(a["Gi"]), a["m"], _ptr(a["gsetX"]), a["tests"],
            a["metap"], _ptr(a["out"]))
    slots = (_ptr(a["Xp"]), _ptr(a["Xi"]), _ptr(a["X"]))
    if entry == "dense":
        rc = lib.plaidhip_plaid_test_contrasts(None, _ptr(a["X"]), *tail)
    elif entry == "csc":
        rc = lib.plaidhip_plaid_test_contrasts_csc(None, *slots, *tail)
    elif entry == "multi":
        rc = lib.plaidhip_plaid_test_contrasts_multi(None, 1, *slots, *tail)
    else:
        rc = sharded_hooks.hook("plaid_test_contrasts")(0, 2, -1, *slots, *tail)
    return rc, lib.plaidhip_last_error_string().decode()


ENTRIES = ["dense", "csc", "multi", "hook"]
FAULTS = [
    (dict(Y=np.asfortranarray(_i32([0, 1], [1, -1], [0, 2]))), "elements of Y must be 0, 1 or NA (-1): contrast 2, sample 3 is 2"),
    (dict(Y=np.asfortranarray(_i32([0, 1], [-2, -1], [0, 0]))), "elements of Y must be 0, 1 or NA (-1): contrast 1, sample 2 is -2"),
    (dict(C=-1), "plaid_test_contrasts: C = -1 (0 <= C <= 65535)"),
    (dict(C=65536), "plaid_test_contrasts: C = 65536 (0 <= C <= 65535)"),
    (dict(Y=None), "plaid_test_contrasts: null Y"),
    (dict(out=None), "plaid_test_contrasts: null out"),
    (dict(X=None), "plaid_test_contrasts: null X"),
    (dict(Gp=None), "null Gp"),
    (dict(g=0), "bad dims g=0 n=3 m=2"),
    (dict(n=-1), "bad dims g=4 n=-1 m=2"),
    (dict(tests=0), "plaid_test: tests is a bit mask of 1 (one), 2 (two), 4 (lm)"),
    (dict(tests=8), "plaid_test: tests is a bit mask of 1 (one), 2 (two), 4 (lm)"),
    (dict(metap=2), "Invalid method: 2"),
]


@pytest.mark.parametrize("entry", ENTRIES)
def test_wrong_calls_are_refused_before_any_device(entry):
    for change, text in FAULTS:
        if entry == "csc" and "X" in change:
            change = dict(Xp=None)                       # the CSC entry's X is its slots
        if entry in ("multi", "hook") and "X" in change:
            change = dict(X=None, Xp=None)
        rc, msg = _call(entry, **change)
        assert rc == _lib.EINVAL and msg == text, (entry, change, rc, msg)
    if entry in ("dense", "csc"):                        # a correct call reaches the context check, and only then
        rc, msg = _call(entry)
        assert rc == _lib.EINVAL and msg == "null plaidhip_ctx", (entry, rc, msg)
    if entry == "multi":
        lib = _lib.load()
        rc = lib.plaidhip_plaid_test_contrasts_multi(None, 0, None, None, None, 4, 3, None, 2, None, None, 2, None, 7, 0, None)
        assert rc == _lib.EINVAL and lib.plaidhip_last_error_string().decode() == "multi: ndev = 0"


def test_a_python_y_of_the_wrong_length_is_refused():
    Gp, Gi = _i32(0, 2, 4), _i32(0, 1, 2, 3)
    with pytest.raises(ValueError, match="one row per column of X"):
        engine._plaid_test_contrasts(None, (None,), np.ones((4, 3), order="F"), np.zeros((4, 2)), Gp, Gi, None, 7, 0, dense=True)
    with pytest.raises(ValueError, match="one row per column of X"):
        engine.contrast_labels(np.zeros(5), 3)


def test_contrast_labels():
    Y = np.array([[0.0, np.nan], [1.0, -1.0], [np.nan, 1.0]])
    L = engine.contrast_labels(Y, 3)
    assert L.dtype == np.int32 and L.flags.f_contiguous and L.tolist() == [[0, -1], [1, -1], [-1, 1]]
    assert engine.contrast_labels(np.array([0, 1, -1]), 3).tolist() == [[0], [1], [-1]]
    assert engine.contrast_labels(np.array([[True], [False], [True]]), 3).tolist() == [[1], [0], [1]]
    # what is no label stays one that the library refuses
    assert engine.contrast_labels(np.array([[0.5], [3.0], [-7.0]]), 3).tolist() == [[2], [2], [2]]
    assert engine.contrast_labels(np.array([[5], [-3], [1]]), 3).tolist() == [[2], [2], [1]]
    with pytest.raises(ValueError):
        engine.contrast_labels(np.array([["a"], ["b"], ["c"]]), 3)
    assert engine.contrast_tile() >= 8


# ------------------------------------------------------------------------------------------------ api.py on a stub context
class StubContext:
    """records what reaches the engine; returns numbers that identify (contrast, set, column)"""

    def __init__(self):
        self.calls = []

    def _out(self, m, labels):
        labels = np.asarray(labels)
        ncon = 1 if labels.ndim == 1 else labels.shape[1]
        rng = np.random.default_rng(5)
        out = rng.random((m, 6, ncon))                    # distinct p.meta values per contrast: another order for each
        return np.asfortranarray(out)

    def plaid_test(self, X, y, Gp, Gi, gsetX=None, tests=7, metap_method=0):
        self.calls.append(("dense", X, y, Gp, Gi, gsetX, tests, metap_method))
        return self._out(len(Gp) - 1, y)[:, :, 0]

    def plaid_test_csc(self, Xp, Xi, Xx, g, y, Gp, Gi, gsetX=None, tests=7, metap_method=0):
        self.calls.append(("csc", (Xp, Xi, Xx, g), y, Gp, Gi, gsetX, tests, metap_method))
        return self._out(len(Gp) - 1, y)[:, :, 0]

    def plaid_test_contrasts(self, X, Y, Gp, Gi, gsetX=None, tests=7, metap_method=0):
        self.calls.append(("dense", X, Y, Gp, Gi, gsetX, tests, metap_method))
        return self._out(len(Gp) - 1, Y)

    def plaid_test_contrasts_csc(self, Xp, Xi, Xx, g, Y, Gp, Gi, gsetX=None, tests=7, metap_method=0):
        self.calls.append(("csc", (Xp, Xi, Xx, g), Y, Gp, Gi, gsetX, tests, metap_method))
        return self._out(len(Gp) - 1, Y)


def _pbmc_rows(golden_dir):
    d = dict(np.load(os.path.join(golden_dir, "pbmc3k50.npz"), allow_pickle=False))
    Xs = sp.csc_matrix((d["x"], d["i"], d["p"]), shape=tuple(d["dim"]))
    matG = plaid_amd.gmt2mat(plaid_amd.read_gmt(os.path.join(golden_dir, "hallmarks.gmt")))
    return plaid_amd.NamedMatrix(Xs, d["rownames"], d["colnames"]), matG, d


def _same(a, b):
    if isinstance(a, tuple):
        return all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("dense", [False, True])
def test_api_aligns_names_as_plaid_test_does(golden_dir, dense):
    """the rows of X and G, the pattern, gsetX's row order, the tests' bits and the meta-p code that reach the engine are
    plaid_test's own (one helper serves both); Y goes down as int32 with -1 for NaN"""
    Xn, matG, d = _pbmc_rows(golden_dir)
    if dense:
        Xn = plaid_amd.NamedMatrix(np.asarray(Xn.values.todense()), Xn.rownames, Xn.colnames)
    n = Xn.shape[1]
    rng = np.random.default_rng(1)
    Y = (rng.random((n, 3)) < 0.4).astype(np.float64)
    Y[rng.random((n, 3)) < 0.3] = np.nan
    gx = plaid_amd.NamedMatrix(rng.random((len(matG.colnames), n)), list(reversed(matG.colnames)), Xn.colnames)
    for gsetX, tests, metap in ((None, ("one", "two", "lm"), "fisher"), (gx, ("one", "lm"), "stouffer"), (gx, "lm", "sumz")):
        one, many = StubContext(), StubContext()
        plaid_amd.plaid_test(Xn, (rng.random(n) < 0.5).astype(int), matG, gsetX=gsetX, tests=tests, metap_method=metap, ctx=one)
        res = plaid_amd.plaid_test_contrasts(Xn, plaid_amd.NamedMatrix(Y, Xn.colnames, ["a", "b", "c"]), matG, gsetX=gsetX,
                                             tests=tests, metap_method=metap, ctx=many)
        a, b = one.calls[0], many.calls[0]
        assert a[0] == b[0] == ("dense" if dense else "csc")
        for k in (1, 3, 4, 5, 6, 7):                       # X, Gp, Gi, gsetX, tests, metap: identical
            assert _same(a[k], b[k]), k
        lab = b[2]
        assert lab.dtype == np.int32 and lab.shape == (n, 3)
        assert np.array_equal(lab == -1, np.isnan(Y)) and np.array_equal(lab[~np.isnan(Y)], Y[~np.isnan(Y)].astype(np.int32))
        assert list(res) == ["a", "b", "c"]
        # per contrast: plaid_test's columns, each contrast sorted by its own p.meta
        names = ["gsetFC"] + ["p." + t for t in ("one", "two", "lm") if t in ([tests] if isinstance(tests, str) else tests)]
        names += ["p.meta", "q.meta"]
        raw = many._out(len(matG.colnames), lab)
        orders = []
        for j, nm in enumerate(res):
            r = res[nm]
            assert r.colnames == names and sorted(r.rownames) == sorted(matG.colnames)
            pm = r.values[:, names.index("p.meta")]
            assert np.all(np.diff(pm) >= 0)
            o = np.argsort(raw[:, 4, j], kind="stable")
            assert r.rownames == [matG.colnames[k] for k in o]
            assert np.array_equal(r.values[:, 0], raw[o, 0, j])
            orders.append(tuple(r.rownames))
        assert len(set(orders)) == 3
    res = plaid_amd.plaid_test_contrasts(Xn, Y, matG, sort_by=None, ctx=StubContext())   # an array: contrasts "1", "2", ...
    assert list(res) == ["1", "2", "3"] and res["2"].rownames == matG.colnames
    with pytest.raises(ValueError, match="0, 1 or NA"):
        plaid_amd.plaid_test_contrasts(Xn, np.full((n, 1), 3.0), matG, ctx=StubContext())
    with pytest.raises(ValueError, match="one row per column"):
        plaid_amd.plaid_test_contrasts(Xn, np.zeros((n + 1, 2)), matG, ctx=StubContext())


def test_plaid_test_contrasts_is_exported():
    assert "plaid_test_contrasts" in plaid_amd.__all__ and "plaid_test_contrasts_multi" in plaid_amd.__all__
    for name in ("plaidhip_plaid_test_contrasts", "plaidhip_plaid_test_contrasts_csc", "plaidhip_plaid_test_contrasts_multi",
                 "plaidhip_dev_row_contrast_sums", "plaidhip_dev_row_contrast_ssd"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)


def test_r_shim_has_the_new_routine():
    """statically, as tests/test_host_logic.py does for the whole shim: registered with the arguments the .Call passes,
    calling the three entries with the header's argument counts, exported and defined"""
    rsrc = open(os.path.join(ROOT, "r-pkg", "R", "plaid-hip.R")).read()
    csrc = open(os.path.join(ROOT, "r-pkg", "src", "plaidhip_R.c")).read()
    header = open(os.path.join(ROOT, "include", "plaidhip.h")).read()
    ns = open(os.path.join(ROOT, "r-pkg", "NAMESPACE")).read()
    reg = re.search(r'\{"R_plaidhip_plaid_test_contrasts",\s*\(DL_FUNC\)&R_plaidhip_plaid_test_contrasts,\s*(\d+)\}', csrc)
    assert reg and int(reg.group(1)) == 12
    sig = re.search(r"^SEXP R_plaidhip_plaid_test_contrasts\(([^)]*)\)\s*\{", csrc, re.M | re.S)
    assert sig and sig.group(1).count("SEXP") == 12
    call = re.search(r'\.Call\("R_plaidhip_plaid_test_contrasts",(.*?)PACKAGE = "plaidhip"\)', rsrc, re.S)
    assert call and len([a for a in call.group(1).split(",") if a.strip()]) == 12
    assert re.search(r"^plaid\.test\.contrasts\s*<-\s*function", rsrc, re.M) and "plaid.test.contrasts" in ns
    hdr = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("plaidhip_plaid_test_contrasts", "plaidhip_plaid_test_contrasts_csc", "plaidhip_plaid_test_contrasts_multi"):
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        used = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", csrc, re.S)
        assert proto and used, name
        assert proto.group(1).count(",") == used.group(1).count(","), name
