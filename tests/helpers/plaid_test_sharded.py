"""The sharded plaid.test engine (multi.cpp) with `nshards` contexts on one device, through the library's test hook."""
import ctypes as C

import numpy as np
import scipy.sparse as sp


def _hook():
    from plaid_amd._lib import load
    fn = load().plaidhip_debug_plaid_test_sharded_on_one_device
    vp = C.c_void_p
    fn.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int32, C.c_int32, vp, vp, vp, C.c_int32, vp, C.c_int, C.c_int,
                   vp]
    return fn


def run(nshards, X, y, Gp, Gi, gsetX=None, tests=7, metap=0, fail=-1):
    """(status, sets x 6) of the sharded engine with nshards contexts on device 0; X dense or scipy CSC"""
    fn = _hook()
    g, n = X.shape
    m = len(Gp) - 1
    out = np.full((m, 6), -7.0, order="F")
    Gp, Gi = np.ascontiguousarray(Gp, dtype=np.int32), np.ascontiguousarray(Gi, dtype=np.int32)
    y = np.ascontiguousarray(y, dtype=np.int32)
    keep = []
    if sp.issparse(X):
        X = sp.csc_matrix(X)
        keep = [np.ascontiguousarray(X.indptr, dtype=np.int32), np.ascontiguousarray(X.indices, dtype=np.int32),
                np.ascontiguousarray(X.data, dtype=np.float64)]
        xp, xi, xv = (a.ctypes.data for a in keep)
    else:
        keep = [np.asfortranarray(X, dtype=np.float64)]
        xp, xi, xv = None, None, keep[0].ctypes.data
    sx = None if gsetX is None else np.asfortranarray(gsetX, dtype=np.float64)
    rc = fn(0, nshards, fail, xp, xi, xv, g, n, y.ctypes.data, Gp.ctypes.data, Gi.ctypes.data, m,
            None if sx is None else sx.ctypes.data, int(tests), int(metap), out.ctypes.data)
    return rc, out
