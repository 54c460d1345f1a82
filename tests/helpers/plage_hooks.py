"""plaidhip_debug_plage_sharded_on_one_device (multi.cpp), bound once: the engine behind plaidhip_plage_multi and
plaidhip_zscore_multi with `nshards` contexts on one device, which is how a 1-GPU box reaches the sharded route.  Its C
signature is plaidhip_plage_multi's with (device, nshards, fail_shard, method) in place of (devices, ndev); method is the
ordinal of enum Method (csrc/call.h).  plaidhip_debug_plage_gram picks the Gram kernel (0 the product's, 1 the MFMA form)."""
import ctypes as C

from plaid_amd import _lib, engine

PLAGE, ZSCORE = 18, 19   # enum Method


def hook():
    fn = _lib.load().plaidhip_debug_plage_sharded_on_one_device
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int] + _lib.SIGNATURES["plaidhip_plage_multi"][2:]
    fn.restype = C.c_int
    return fn


def plage(nshards, X, Gp, Gi, tol=engine.PLAGE_TOL, maxit=1000, loadings=False, fail=-1):
    """(S, info[, loadings]) of replaid.plage over `nshards` shards on device 0; raises PlaidHipError on a failure"""
    fn = hook()
    return engine._plage(lambda *a: fn(*a[:3], PLAGE, *a[3:]), (0, nshards, fail), X, Gp, Gi, tol, maxit, loadings)


def zscore(nshards, X, Gp, Gi, fail=-1):
    """(S, size) of replaid.zscore over `nshards` shards on device 0"""
    fn = hook()

    def call(*a):   # (the hook's zscore form ignores tol, maxit and load_out)
        return fn(*a[:3], ZSCORE, *a[3:-2], 0.0, 0, *a[-2:], None)
    return engine._zscore(call, (0, nshards, fail), X, Gp, Gi)


def gram_mode(mode):
    fn = _lib.load().plaidhip_debug_plage_gram
    fn.argtypes, fn.restype = [C.c_int], C.c_int
    _lib.check(fn(int(mode)))
