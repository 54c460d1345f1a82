"""The argument checks of plaidhip_gsea_multilevel, its _multi entry, its hook and plaidhip_gsea_ruler without a device:
every check comes before a context or a device is looked at, in the order include/plaidhip.h states."""
import ctypes as C

import numpy as np
import pytest

from plaid_amd import _lib, engine

G, LISTS, M, B = 40, 2, 2, 8
_rng = np.random.default_rng(3)
STAT = np.asfortranarray(_rng.standard_normal((G, LISTS)))
W = np.ones((G, LISTS), order="F")
GP, GI = np.array([0, 3, 7], dtype=np.int32), np.array([0, 5, 9, 1, 2, 3, 39], dtype=np.int32)
OUT, ML = np.full((M, 12, LISTS), -7.0, order="F"), np.full((M, 6, LISTS), -7.0, order="F")


def refused(rc):
    try:
        _lib.check(rc)
    except _lib.PlaidHipError as e:
        return e.code, str(e)
    return rc, ""


def table_call(head=(None,), fn="plaidhip_gsea_multilevel", sample=21, sweeps=2, eps=1e-50, ml_min=10, c=LISTS, st=0, nperm=B,
               mlp=True, weight=W):
    lib = _lib.load()
    f = getattr(lib, fn)
    if fn.startswith("plaidhip_debug"):
        f.argtypes = [C.c_int, C.c_int, C.c_int] + _lib.SIGNATURES["plaidhip_gsea_multilevel_multi"][2:]
        f.restype = C.c_int
    return refused(f(*head, STAT.ctypes.data, weight.ctypes.data, G, c, GP.ctypes.data, GI.ctypes.data, M, None, nperm, 1, st,
                     sample, sweeps, eps, ml_min, OUT.ctypes.data, None, None, None, ML.ctypes.data if mlp else None))


ENTRIES = [((None,), "plaidhip_gsea_multilevel"), ((None, 1), "plaidhip_gsea_multilevel_multi"),
           ((0, 2, -1), "plaidhip_debug_gsea_multilevel_sharded_on_one_device")]


@pytest.mark.parametrize("head,fn", ENTRIES)
def test_the_first_wrong_argument_speaks(head, fn):
    wneg = W.copy(order="F")
    wneg[3, 1] = -1.0
    later = dict(nperm=0, st=7, weight=wneg)          # wrong in everything that comes later as well
    for kw, word in [(dict(sample=20, sweeps=0, eps=1.0, ml_min=-1), "sample_size"), (dict(sample=1025, sweeps=0), "sample_size"),
                     (dict(sample=1, sweeps=33), "sample_size"), (dict(sweeps=0, eps=-0.5, ml_min=-1), "sweeps"),
                     (dict(sweeps=33, eps=1.0), "sweeps"), (dict(eps=1.0, ml_min=-1), "eps ="), (dict(eps=float("nan"), ml_min=-1), "eps ="),
                     (dict(ml_min=-1, c=1 << 30), "ml_min"), (dict(c=1 << 30, mlp=False), "ranked lists"), (dict(mlp=False), "ml_out"),
                     (dict(), "score_type"), (dict(st=0), "nperm"), (dict(st=0, nperm=B), "weight")]:
        rc, text = table_call(head, fn, **{**later, **kw})
        assert rc == _lib.EINVAL and word in text, (kw, text)
    assert np.all(OUT == -7.0) and np.all(ML == -7.0)


def test_a_null_context_comes_after_the_arguments():
    rc, text = table_call()
    assert rc == _lib.EINVAL and "plaidhip_ctx" in text


def ruler_call(k=5, l=0, side=0, st=0, gamma=0.5, sample=21, sweeps=2, eps=1e-50, g=G, weight=W, outs=True):
    lib = _lib.load()
    nst, end = C.c_int32(0), C.c_int32(0)
    m, s, h = np.zeros(256), np.zeros(256, dtype=np.int32), np.zeros((256, max(sample, 1)))
    o = (C.byref(nst), C.byref(end), m.ctypes.data, s.ctypes.data, h.ctypes.data) if outs else (None,) * 5
    return refused(lib.plaidhip_gsea_ruler(None, STAT.ctypes.data, weight.ctypes.data, g, k, l, side, st, gamma, 1, sample, sweeps,
                                           eps, *o))


def test_ruler_arguments_in_their_order():
    wnan = W.copy(order="F")
    wnan[2, 0] = np.nan
    later = dict(side=2, l=-1, k=0, gamma=float("nan"), st=5, weight=wnan, outs=False)
    for kw, word in [(dict(sample=4), "sample_size"), (dict(sweeps=40), "sweeps"), (dict(eps=1.5), "eps ="), (dict(), "side ="),
                     (dict(side=1), "list number"), (dict(side=1, l=1 << 30), "list number"), (dict(side=1, l=3), "k ="),
                     (dict(side=1, l=3, k=G), "k ="), (dict(side=1, l=3, k=5), "gamma"), (dict(side=1, l=3, k=5, gamma=0.5), "score_type"),
                     (dict(side=1, l=3, k=5, gamma=0.5, st=1), "does not go with"),
                     (dict(side=1, l=3, k=5, gamma=0.5, st=2), "null output"),
                     (dict(side=1, l=3, k=5, gamma=0.5, st=2, outs=True), "weight[2]")]:
        rc, text = ruler_call(**{**later, **kw})
        assert rc == _lib.EINVAL and word in text, (kw, text)
    rc, text = ruler_call(g=engine.GSEA_KS_MAX_GENES + 1, k=5)
    assert rc == _lib.EUNSUPPORTED and "genes" in text
    rc, text = ruler_call()
    assert rc == _lib.EINVAL and "plaidhip_ctx" in text


def test_the_wrappers_check_in_the_same_order():
    with pytest.raises(ValueError, match="sample_size"):
        engine._gsea_multilevel(None, (), STAT, W, GP, GI, nperm=0, sample_size=100, sweeps=0)
    with pytest.raises(ValueError, match="sweeps"):
        engine._gsea_multilevel(None, (), STAT, W, GP, GI, nperm=0, sweeps=0, eps=2.0)
    with pytest.raises(ValueError, match="eps"):
        engine._gsea_multilevel(None, (), STAT, W, GP, GI, nperm=0, eps=1.0, ml_min=-1)
    with pytest.raises(ValueError, match="ml_min"):
        engine._gsea_multilevel(None, (), STAT, W, GP, GI, nperm=0, ml_min=-1)
    with pytest.raises(ValueError, match="nperm"):
        engine._gsea_multilevel(None, (), STAT, W, GP, GI, nperm=0)


def test_the_surface_is_declared_everywhere():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "plaidhip.h")).read()
    for name, nargs in (("plaidhip_gsea_multilevel", 21), ("plaidhip_gsea_multilevel_multi", 22), ("plaidhip_gsea_ruler", 18)):
        assert re.search(r"\bint\s+%s\s*\(" % name, header) and len(_lib.SIGNATURES[name]) == nargs
        assert hasattr(_lib.load(), name)
    for name, value in (("PLAIDHIP_GSEA_ML_MAX_STAGES", 256), ("PLAIDHIP_GSEA_ML_MAX_SAMPLE", 1023), ("PLAIDHIP_GSEA_ML_ESTIMATED", 0),
                        ("PLAIDHIP_GSEA_ML_FLOOR", 1), ("PLAIDHIP_GSEA_ML_STALLED", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header)
    assert (engine.GSEA_ML_MAX_STAGES, engine.GSEA_ML_MAX_SAMPLE) == (256, 1023)
    shim = open(os.path.join(root, "r-pkg", "src", "plaidhip_R.c")).read()
    rsrc = " ".join(open(os.path.join(root, "r-pkg", "R", "plaid-hip.R")).read().split())
    assert '{"R_plaidhip_gsea_multilevel", (DL_FUNC)&R_plaidhip_gsea_multilevel, 12}' in shim
    assert '.Call("R_plaidhip_gsea_multilevel"' in rsrc and "multilevel = FALSE, sampleSize = 101, eps = 1e-50, sweeps = 4, mlMin = 10" in rsrc
