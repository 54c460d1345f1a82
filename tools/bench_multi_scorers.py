"""replaid.ucell / aucell / scse / gsva: each context entry (Context.ucell ...) against its multi-device form on one device
(plaid_amd.ucell_multi(..., devices=[0]) ...), dense X and a dgCMatrix, and the gsva z transform's chained row reduction
through the N-shards-on-one-device test hook (5 shards against 1: the same call, the chain and four more contexts).
Median wall milliseconds of --reps calls after one warm-up call each; prints one JSON line.
    python3 tools/bench_multi_scorers.py [--genes 20000 --cells 10000 --sets 5000 --density 0.05 --reps 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(fn, reps):
    fn()                                   # warm-up: code objects, context buffers, the result's pages
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def _hook_gsva(X, Gp, Gi, nshards):
    from tests.helpers import sharded_hooks
    m = len(Gp) - 1
    S, kf = np.empty((m, X.shape[1]), order="F"), np.zeros(m)   # (allocated once: the timed call touches no fresh page)

    def call():
        assert sharded_hooks.scorer(nshards, sharded_hooks.GSVA, X, Gp, Gi, k_full=kf, out=S)[0] == 0
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=20000)
    ap.add_argument("--cells", type=int, default=10000)
    ap.add_argument("--sets", type=int, default=5000)
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import plaid_amd
    from plaid_amd import synth
    g, n = a.genes, a.cells
    Gp, Gi = synth.geneset_csc(g, a.sets)
    Gp, Gi = np.ascontiguousarray(Gp, dtype=np.int32), np.ascontiguousarray(Gi, dtype=np.int32)
    kf = np.diff(Gp).astype(np.float64)
    X = synth.dense_columns(g, 0, n, tied=True)
    Xp, Xi, Xx = synth.sparse_columns(g, 0, n, density=a.density)
    Xs = sp.csc_matrix((Xx, Xi, Xp), shape=(g, n))
    ctx = plaid_amd.Context(0)
    out = {"genes": g, "cells": n, "sets": a.sets, "density": a.density, "reps": a.reps, "ms": {}}
    for kind, Xin in (("dense", X), ("csc", Xs)):
        pairs = {
            "ucell": (lambda: ctx.ucell(Xin, Gp, Gi, kf, 1500.0),
                      lambda: plaid_amd.ucell_multi(Xin, Gp, Gi, kf, 1500.0, devices=[0])),
            "aucell": (lambda: ctx.aucell(Xin, Gp, Gi, 1000.0),
                       lambda: plaid_amd.aucell_multi(Xin, Gp, Gi, 1000.0, devices=[0])),
            "scse": (lambda: ctx.scse(Xin, Gp, Gi, None, False),
                     lambda: plaid_amd.scse_multi(Xin, Gp, Gi, None, False, devices=[0])),
            "gsva": ((lambda: ctx.gsva(Xin, Gp, Gi, 0.0, "z")) if kind == "dense" else
                     (lambda: ctx.gsva_csc(Xs.indptr, Xs.indices, Xs.data, g, Gp, Gi, 0.0, "z")),
                     lambda: plaid_amd.gsva_multi(Xin, Gp, Gi, 0.0, "z", devices=[0])),
        }
        for name, (single, multi) in pairs.items():
            t_ctx = _median_ms(single, a.reps)
            t_multi = _median_ms(multi, a.reps)
            out["ms"][f"{name}_{kind}"] = {"context": round(t_ctx, 2), "multi_1dev": round(t_multi, 2),
                                          "ratio": round(t_multi / t_ctx, 3)}
    plaid_amd.multi_finalize()
    ctx.close()
    t1 = _median_ms(_hook_gsva(X, Gp, Gi, 1), a.reps)
    t5 = _median_ms(_hook_gsva(X, Gp, Gi, 5), a.reps)
    out["gsva_dense_hook_ms"] = {"shards_1": round(t1, 2), "shards_5": round(t5, 2), "difference": round(t5 - t1, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
