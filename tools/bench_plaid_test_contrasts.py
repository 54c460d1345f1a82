"""plaid.test.contrasts (Context.plaid_test_contrasts) against one plaid.test call per contrast at the same shape: dense
20,000 genes x 10,000 samples x 5,000 sets, gsetX = NULL, tests = 7.  One call at C = 1, 8, 32 contrasts (about 30 % NA
each), and C times the median plaid.test call.  Medians of --reps host calls after one warm-up call; one JSON line.
    python3 tools/bench_plaid_test_contrasts.py [--reps 3] [--contrasts 1,8,32]
--baseline-root DIR times plaid.test in a child process on another built checkout of the project (the parent commit's:
its package and its library), in the same session on the same device; without it the baseline is this build's
plaid.test, whose path this feature does not touch.  --only C runs one contrasts call and nothing else (what a profiler wraps); --only 0 the plaid.test call alone."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.environ.get("PLAID_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = dict(genes=20000, cells=10000, sets=5000)


def _median_ms(fn, reps):
    fn()                                   # warm-up: code objects, context buffers, the result's pages
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def _inputs(ncon):
    from plaid_amd import synth
    g, n = SHAPE["genes"], SHAPE["cells"]
    Gp, Gi = synth.geneset_csc(g, SHAPE["sets"])
    X = synth.dense_columns(g, 0, n)
    rng = np.random.default_rng(7)
    Y = (rng.random((n, max(ncon, 1))) < 0.4).astype(np.int32)
    y = Y[:, 0].copy()
    Y[rng.random(Y.shape) < 0.3] = -1
    return X, y, np.asfortranarray(Y), Gp, Gi


def plaid_test_ms(reps):
    import plaid_amd
    X, y, _, Gp, Gi = _inputs(1)
    ctx = plaid_amd.Context(0)
    try:
        return _median_ms(lambda: ctx.plaid_test(X, y, Gp, Gi, None, 7, 0), reps)
    finally:
        ctx.close()


def contrasts_ms(ncon, reps):
    import plaid_amd
    X, _, Y, Gp, Gi = _inputs(ncon)
    ctx = plaid_amd.Context(0)
    try:
        return _median_ms(lambda: ctx.plaid_test_contrasts(X, Y, Gp, Gi, None, 7, 0), reps)
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--contrasts", default="1,8,32")
    ap.add_argument("--baseline-root", default=None, help="another built checkout to time plaid.test on")
    ap.add_argument("--only", type=int, default=None, help="one call in this process: C contrasts, or 0 for plaid.test")
    a = ap.parse_args()
    if a.only is not None:
        ms = plaid_test_ms(a.reps) if a.only == 0 else contrasts_ms(a.only, a.reps)
        print(json.dumps({"C": a.only, "ms": round(ms, 2)}))
        return
    out = {"bench": "plaid_test_contrasts", **SHAPE, "tests": 7, "gsetX": None, "reps": a.reps}
    base = plaid_test_ms(a.reps)
    out["plaid_test_ms"] = round(base, 2)
    if a.baseline_root:                    # a fresh process that imports the other checkout's package and library
        env = dict(os.environ, PLAID_BENCH_ROOT=os.path.abspath(a.baseline_root))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "0", "--reps", str(a.reps)], env=env,
                           capture_output=True, text=True, check=True)
        base = json.loads(r.stdout.strip().splitlines()[-1])["ms"]
        out["baseline_plaid_test_ms"] = base
    for ncon in (int(v) for v in a.contrasts.split(",")):
        ms = contrasts_ms(ncon, a.reps)
        out[f"contrasts_{ncon}_ms"] = round(ms, 2)
        out[f"contrasts_{ncon}_vs_{ncon}_calls"] = round(ms / (ncon * base), 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
