"""replaid.ssgsea.exact (Context.ssgsea_exact) against replaid.ssgsea (Context.ssgsea_dense / ssgsea_csc) at the same
shape: dense 20,000 genes x 10,000 samples x 5,000 sets at alpha 0 and 0.25, and a dgCMatrix of 20,000 x 100,000 at 5 %
stored values at alpha 0.25.  Every case runs in a fresh process (no context, plan or page cache shared between cases);
each reports the median wall milliseconds of --reps host calls after one warm-up call.  Prints one JSON line.
    python3 tools/bench_ssgsea_exact.py [--reps 3] [--cases dense_a0,dense_a025,sparse_a025]
    python3 tools/bench_ssgsea_exact.py --case dense_a025 --reps 1     (one case in this process: what a profiler wraps)
--single-false adds replaid.ssgsea.exact(single = FALSE), the walk kernel of kernels_ks.hip, as a third entry of each case
(ssgsea_exact_ks_ms, and its ratio to single = TRUE); --only-single-false runs that entry alone (a profile of its own)."""
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


def run_case(name, reps, single_false=False, only_single_false=False):
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
            ks = _median_ms(lambda: ctx.ssgsea_exact(X, Gp, Gi, alpha, single=False), reps) if single_false else None
            if only_single_false:
                return {"case": name, **p, "reps": reps, "ssgsea_exact_ks_ms": round(ks, 2)}
            exact = _median_ms(lambda: ctx.ssgsea_exact(X, Gp, Gi, alpha), reps)
            base = _median_ms(lambda: ctx.ssgsea_dense(X, Gp, Gi, alpha), reps)
        else:
            Xp, Xi, Xx = synth.sparse_columns(g, 0, n, density=p["density"])
            Xs = sp.csc_matrix((Xx, Xi, Xp), shape=(g, n))
            ks = _median_ms(lambda: ctx.ssgsea_exact(Xs, Gp, Gi, alpha, single=False), reps) if single_false else None
            if only_single_false:
                return {"case": name, **p, "reps": reps, "ssgsea_exact_ks_ms": round(ks, 2)}
            exact = _median_ms(lambda: ctx.ssgsea_exact(Xs, Gp, Gi, alpha), reps)
            base = _median_ms(lambda: ctx.ssgsea_csc(Xp, Xi, Xx, g, Gp, Gi, alpha), reps)
    finally:
        ctx.close()
    out = {"case": name, **p, "reps": reps, "ssgsea_exact_ms": round(exact, 2), "ssgsea_ms": round(base, 2),
           "ratio": round(exact / base, 3)}
    if ks is not None:
        out.update(ssgsea_exact_ks_ms=round(ks, 2), ks_ratio_to_single=round(ks / exact, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="run one case in this process and print its JSON")
    ap.add_argument("--single-false", action="store_true", help="also time single = FALSE (the max-deviation score)")
    ap.add_argument("--only-single-false", action="store_true", help="time single = FALSE alone")
    a = ap.parse_args()
    sf = a.single_false or a.only_single_false
    if a.case is not None:
        print(json.dumps(run_case(a.case, a.reps, sf, a.only_single_false)))
        return
    out = []
    for name in a.cases.split(","):
        flags = (["--single-false"] if a.single_false else []) + (["--only-single-false"] if a.only_single_false else [])
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps)] + flags,
                           capture_output=True, text=True)
        if r.returncode != 0:
            out.append({"case": name, "error": (r.stderr or r.stdout)[-500:], "returncode": r.returncode})
            break                          # a failed case ends the run: nothing more is started on the device
        out.append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps({"tool": "bench_ssgsea_exact", "cases": out}))


if __name__ == "__main__":
    main()
