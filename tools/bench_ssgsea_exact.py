"""replaid.ssgsea.exact (Context.ssgsea_exact) against replaid.ssgsea (Context.ssgsea_dense / ssgsea_csc) at the same
shape: dense 20,000 genes x 10,000 samples x 5,000 sets at alpha 0 and 0.25, and a dgCMatrix of 20,000 x 100,000 at 5 %
stored values at alpha 0.25.  Every case runs in a fresh process (no context, plan or page cache shared between cases);
each reports the median wall milliseconds of --reps host calls after one warm-up call.  Prints one JSON line.
    python3 tools/bench_ssgsea_exact.py [--reps 3] [--cases dense_a0,dense_a025,sparse_a025]
    python3 tools/bench_ssgsea_exact.py --case dense_a025 --reps 1     (one case in this process: what a profiler wraps)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    "dense_a0": dict(kind="dense", genes=20000, cells=10000, sets=5000, alpha=0.0),
    "dense_a025": dict(kind="dense", genes=20000, cells=10000, sets=5000, alpha=0.25),
    "sparse_a025": dict(kind="sparse", genes=20000, cells=100000, sets=5000, alpha=0.25, density=0.05),
}


def _median_ms(fn, reps):
    fn()                                   # warm-up: code objects, context buffers, the result's pages
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def run_case(name, reps):
    import scipy.sparse as sp

    import plaid_amd
    from plaid_amd import synth
    p = CASES[name]
    g, n, alpha = p["genes"], p["cells"], p["alpha"]
    Gp, Gi = synth.geneset_csc(g, p["sets"])
    ctx = plaid_amd.Context(0)
    try:
        if p["kind"] == "dense":
            X = synth.dense_columns(g, 0, n)
            exact = _median_ms(lambda: ctx.ssgsea_exact(X, Gp, Gi, alpha), reps)
            base = _median_ms(lambda: ctx.ssgsea_dense(X, Gp, Gi, alpha), reps)
        else:
            Xp, Xi, Xx = synth.sparse_columns(g, 0, n, density=p["density"])
            Xs = sp.csc_matrix((Xx, Xi, Xp), shape=(g, n))
            exact = _median_ms(lambda: ctx.ssgsea_exact(Xs, Gp, Gi, alpha), reps)
            base = _median_ms(lambda: ctx.ssgsea_csc(Xp, Xi, Xx, g, Gp, Gi, alpha), reps)
    finally:
        ctx.close()
    return {"case": name, **p, "reps": reps, "ssgsea_exact_ms": round(exact, 2), "ssgsea_ms": round(base, 2),
            "ratio": round(exact / base, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="run one case in this process and print its JSON")
    a = ap.parse_args()
    if a.case is not None:
        print(json.dumps(run_case(a.case, a.reps)))
        return
    out = []
    for name in a.cases.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            out.append({"case": name, "error": (r.stderr or r.stdout)[-500:], "returncode": r.returncode})
            break                          # a failed case ends the run: nothing more is started on the device
        out.append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps({"tool": "bench_ssgsea_exact", "cases": out}))


if __name__ == "__main__":
    main()
