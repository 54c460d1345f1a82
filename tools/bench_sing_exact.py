"""replaid.sing.exact (Context.sing_exact) with the dispersion off and on against replaid.sing (Context.sing_dense) at the
same shape, one MI355X, and the nearest existing per-pair kernel beside it: replaid.gsva.exact at tau = 0 (gsva_ks_kernel).
Each case runs in a fresh process (the context's buffers and the result's pages start cold, then one warm-up call).

    python3 tools/bench_sing_exact.py [--reps 3] [--cases dense]
    python3 tools/bench_sing_exact.py --case dense --reps 1 --only disp      (one call kind in this process: what a
                                                                               profiler wraps; kinds: sing, off, disp, gsva)
"""
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
    "dense": dict(genes=20000, cells=10000, sets=5000),
    "small": dict(genes=20000, cells=1000, sets=500),
}
KINDS = ("sing", "off", "disp", "gsva")


def _times_ms(fn, reps):
    fn()                                   # warm-up: code objects, context buffers, the result's pages
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def run_case(name, reps, only=None):
    import plaid_amd
    from plaid_amd import synth
    p = CASES[name]
    g, n = p["genes"], p["cells"]
    Gp, Gi = synth.geneset_csc(g, p["sets"])
    ctx = plaid_amd.Context(0)
    calls = {
        "sing": lambda: ctx.sing_dense(X, Gp, Gi),
        "off": lambda: ctx.sing_exact(X, Gp, Gi, dispersion=False),
        "disp": lambda: ctx.sing_exact(X, Gp, Gi, dispersion=True),
        "gsva": lambda: ctx.gsva_exact(X, Gp, Gi, 0.0, "none", True),
    }
    out = {"case": name, **p, "reps": reps}
    try:
        X = synth.dense_columns(g, 0, n)
        for kind in KINDS if only is None else (only,):
            ts = _times_ms(calls[kind], reps)
            out[kind + "_ms"] = round(float(np.median(ts)), 2)
            out[kind + "_all_ms"] = [round(t, 2) for t in ts]
    finally:
        ctx.close()
    if "sing_ms" in out and "off_ms" in out:
        out["off_over_sing"] = round(out["off_ms"] / out["sing_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="dense")
    ap.add_argument("--case", default=None, help="run one case in this process and print its JSON")
    ap.add_argument("--only", default=None, choices=KINDS, help="time one kind of call alone")
    a = ap.parse_args()
    if a.case is not None:
        print(json.dumps(run_case(a.case, a.reps, a.only)))
        return
    out = []
    for name in a.cases.split(","):
        flags = ["--only", a.only] if a.only else []
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps)] + flags,
                           capture_output=True, text=True)
        if r.returncode != 0:
            out.append({"case": name, "error": (r.stderr or r.stdout)[-500:], "returncode": r.returncode})
            break                          # a failed case ends the run: nothing more is started on the device
        out.append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps({"tool": "bench_sing_exact", "cases": out}))


if __name__ == "__main__":
    main()
