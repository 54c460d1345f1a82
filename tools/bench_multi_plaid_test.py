"""plaid.test over several devices: the single-device entry (plaidhip_plaid_test, or plaidhip_plaid_test_csc for a
dgCMatrix) against its multi-device form on one device (plaid_amd.plaid_test_multi(..., devices=[0])) and against the
N-shards-on-one-device test hook at 2 and 4 shards (each hook call also creates and destroys its N contexts), with
tests = one + two + lm and gsetX = NULL.  Two shapes: 20,000 x 10,000 x 5,000 dense (C2), 20,000 x 100,000 at 5 %
stored.  Median wall milliseconds of --reps calls after one warm-up call each; each result against the single-device
one: bit equality, or the largest relative difference.  With more than one GPU also devices=[0, 1] (otherwise a
`skipped` record).  Prints JSON lines.
    python3 tools/bench_multi_plaid_test.py [--reps 3] [--shapes dense,csc]
    python3 tools/bench_multi_plaid_test.py --profile multi|single   (shape 1 alone, for a rocprofv3 --kernel-trace run)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TESTS = 7


def _median_ms(fn, reps):
    fn()                                   # warm-up: code objects, context buffers, the gene-set plan
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def _hook(X, y, Gp, Gi, nshards, out):
    from tests.helpers import sharded_hooks

    def call():
        assert sharded_hooks.plaid_test(nshards, X, y, Gp, Gi, tests=TESTS, out=out)[0] == 0
        return out
    return call


def _compare(a, b):
    if np.array_equal(a, b, equal_nan=True):
        return {"bit_equal": True}
    ok = np.isfinite(a) & np.isfinite(b)
    rel = np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1e-300)
    return {"bit_equal": False, "max_rel_diff": float(rel.max()) if rel.size else 0.0,
            "nan_pattern_equal": bool(np.array_equal(np.isnan(a), np.isnan(b)))}


def _inputs(kind, g, n, m, density):
    from plaid_amd import synth
    Gp, Gi = synth.geneset_csc(g, m)
    Gp, Gi = np.ascontiguousarray(Gp, dtype=np.int32), np.ascontiguousarray(Gi, dtype=np.int32)
    y = np.ascontiguousarray(np.arange(n) % 3 == 1, dtype=np.int32)
    if kind == "dense":
        X = synth.dense_columns(g, 0, n, tied=True)
    else:
        Xp, Xi, Xx = synth.sparse_columns(g, 0, n, density=density)
        X = sp.csc_matrix((Xx, Xi, Xp), shape=(g, n))
        X.indptr = np.ascontiguousarray(X.indptr, dtype=np.int32)
        X.indices = np.ascontiguousarray(X.indices, dtype=np.int32)
    return X, y, Gp, Gi


def _single(ctx, X, y, Gp, Gi):
    if sp.issparse(X):
        return lambda: ctx.plaid_test_csc(X.indptr, X.indices, X.data, X.shape[0], y, Gp, Gi, None, TESTS, 0)
    return lambda: ctx.plaid_test(X, y, Gp, Gi, None, TESTS, 0)


def bench_shape(kind, g, n, m, density, reps):
    import plaid_amd
    X, y, Gp, Gi = _inputs(kind, g, n, m, density)
    rec = {"shape": kind, "genes": g, "cells": n, "sets": m, "tests": "one+two+lm", "gsetX": None, "reps": reps, "ms": {},
           "vs_single": {}}
    if kind == "csc":
        rec["density"] = density
    ctx = plaid_amd.Context(0)
    single = _single(ctx, X, y, Gp, Gi)
    rec["ms"]["single"] = round(_median_ms(single, reps), 2)
    ref = single()
    ctx.close()
    multi = lambda: plaid_amd.plaid_test_multi(X, y, Gp, Gi, tests=TESTS, devices=[0])   # noqa: E731
    rec["ms"]["multi_1dev"] = round(_median_ms(multi, reps), 2)
    rec["vs_single"]["multi_1dev"] = _compare(multi(), ref)
    plaid_amd.multi_finalize()
    for k in (2, 4):
        out = np.empty((m, 6), order="F")
        call = _hook(X, y, Gp, Gi, k, out)
        rec["ms"][f"hook_{k}_shards"] = round(_median_ms(call, reps), 2)
        rec["vs_single"][f"hook_{k}_shards"] = _compare(call(), ref)
    print(json.dumps(rec), flush=True)
    ndev = plaid_amd.device_count()
    if ndev > 1:
        two = lambda: plaid_amd.plaid_test_multi(X, y, Gp, Gi, tests=TESTS, devices=[0, 1])   # noqa: E731
        r2 = {"shape": kind, "record": "devices_0_1", "ms": round(_median_ms(two, reps), 2),
              "ms_multi_1dev": rec["ms"]["multi_1dev"], "vs_single": _compare(two(), ref)}
        plaid_amd.multi_finalize()
    else:
        r2 = {"shape": kind, "record": "devices_0_1", "skipped": f"{ndev} device(s) visible"}
    print(json.dumps(r2), flush=True)


def profile(which, reps):
    """shape 1 alone, `reps` calls of one route: the kernel trace of the one-device _multi call or of the single entry"""
    import plaid_amd
    X, y, Gp, Gi = _inputs("dense", 20000, 10000, 5000, 0.0)
    if which == "multi":
        for _ in range(reps):
            plaid_amd.plaid_test_multi(X, y, Gp, Gi, tests=TESTS, devices=[0])
        plaid_amd.multi_finalize()
    else:
        ctx = plaid_amd.Context(0)
        for _ in range(reps):
            ctx.plaid_test(X, y, Gp, Gi, None, TESTS, 0)
        ctx.close()
    print(json.dumps({"profile": which, "calls": reps}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="dense,csc")
    ap.add_argument("--profile", choices=("multi", "single"))
    a = ap.parse_args()
    if a.profile:
        profile(a.profile, a.reps)
        return
    shapes = {"dense": (20000, 10000, 5000, 0.0), "csc": (20000, 100000, 5000, 0.05)}
    for kind in a.shapes.split(","):
        g, n, m, d = shapes[kind]
        bench_shape(kind, g, n, m, d, a.reps)


if __name__ == "__main__":
    main()
