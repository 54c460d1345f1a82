"""The library's seven test hooks (multi.cpp: plaidhip_debug_*_sharded_on_one_device), bound once.

A hook runs the engine behind a plaidhip_*_multi entry with `nshards` contexts on one device, which is how a 1-GPU box
reaches worker threads, rendezvous and the failure path.  Its C signature is the entry's with (device, nshards,
fail_shard) in place of (devices, ndev); the two hooks that serve several entries take the Method ordinal next.  They stay
out of include/plaidhip.h and of _lib.SIGNATURES.  Calls go through the package's own marshaller (engine._score) with the
head (0, nshards, fail); a failed call returns its status instead of raising."""
import ctypes as C

import numpy as np

from plaid_amd import _lib, engine

_int, _vp, _i32, _f64 = C.c_int, C.c_void_p, C.c_int32, C.c_double
_X_G = [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32]   # Xp, Xi, X_or_x, g, n, Gp, Gi, m
_OWN = {   # the two by-ordinal hooks: what follows (device, nshards, fail_shard)
    "": [_int] + _X_G + [_int, _int, _f64, _vp],                                        # method, ..., stat, normalize, alpha, S
    "scorer": [_int] + _X_G + [_vp, _f64, _f64, _int, _int, _f64, _int, _vp, C.POINTER(_int)],
}
PLAID, SING, SSGSEA, UCELL, AUCELL, SCSE, GSVA = range(7)   # enum Method (csrc/call.h)


def hook(name):
    """the hook of plaidhip_<name>_multi ("plaid_test", "ssgsea_exact", "ssgsea_exact_ks", "gsva_exact", "sing_exact"), or
    "" (plaid / sing / ssgsea) and "scorer" (ucell / aucell / scse / gsva)"""
    fn = getattr(_lib.load(), "plaidhip_debug_" + (name + "_" if name else "") + "sharded_on_one_device")
    fn.argtypes = [_int, _int, _int] + (_OWN[name] if name in _OWN else _lib.SIGNATURES[f"plaidhip_{name}_multi"][2:])
    fn.restype = _int
    return fn


def _status(call):
    try:
        return _lib.OK, call()
    except _lib.PlaidHipError as e:
        return e.code, None


def score(name, nshards, X, Gp, Gi, *tail, fail=-1, method=None, out=None, **kw):
    """(status, S) of engine._score on the hook: X dense or scipy CSC, `tail` the entry's own parameters.  S is NaN before
    the call (or the caller's `out`), so a shard that writes nothing shows"""
    fn = hook(name)
    call = fn if method is None else (lambda *a: fn(*a[:3], method, *a[3:]))
    if out is None:
        out = np.full((len(Gp) - 1, kw.get("cols", X.shape[1])), np.nan, order="F")
    return _status(lambda: engine._score(call, (0, nshards, fail), X, Gp, Gi, *tail, out=out, **kw))[0], out


def scorer(nshards, method, X, Gp, Gi, fail=-1, k_full=None, rmax=1500.0, auc_max_rank=1.0, remove_log2=None,
           score_mean=False, tau=0.0, rowtf=0, out=None):
    """(status, S, removed_log2) of ucell / aucell / scse / gsva; what a method does not take is ignored"""
    m = len(Gp) - 1
    kf = np.ascontiguousarray(k_full if k_full is not None else np.zeros(m), dtype=np.float64)
    removed = C.c_int(-7)
    status, S = score("scorer", nshards, X, Gp, Gi, kf.ctypes.data, float(rmax), float(auc_max_rank),
                      engine._remove_log2(remove_log2), int(bool(score_mean)), float(tau), int(rowtf), fail=fail, method=method,
                      out=out, post=(C.byref(removed),))
    return status, S, removed.value


def plaid_test(nshards, X, y, Gp, Gi, gsetX=None, tests=7, metap=0, fail=-1, out=None):
    """(status, sets x 6) of plaid.test; the result holds -7 before the call unless it is the caller's `out`"""
    out = np.full((len(Gp) - 1, 6), -7.0, order="F") if out is None else out
    status, _ = _status(lambda: engine._plaid_test(hook("plaid_test"), (0, nshards, fail), X, y, Gp, Gi, gsetX, tests, metap,
                                                   out=out))
    return status, out


def sing_exact(nshards, X, Gp, Gi, Dp=None, Di=None, center=True, dispersion=True, fail=-1):
    """(status, dict of results or None) of replaid.sing.exact; the results hold -7 before the call"""
    return _status(lambda: engine._sing_exact_call(hook("sing_exact"), (0, nshards, fail), X, Gp, Gi, Dp, Di, center,
                                                   dispersion, fill=-7.0))
