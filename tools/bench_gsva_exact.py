"""replaid.gsva.exact (Context.gsva_exact) against replaid.gsva (Context.gsva) at the same shape, one MI355X.
Each case runs in a fresh process (the context's buffers and the result's pages start cold, then one warm-up call).

    python3 tools/bench_gsva_exact.py [--reps 3] [--cases dense_t0,dense_t1]
    python3 tools/bench_gsva_exact.py --case dense_t1 --reps 1 --only-exact     (one case in this process, replaid.gsva.exact
                                                                                 alone: what a profiler wraps)
    python3 tools/bench_gsva_exact.py --case gauss_10k --reps 1 --only-exact --kcdf-mode 1   (the kernel CDF estimate with the
                                                                                 exact operations for every term; 2: the fast
                                                                                 index, counting the terms it leaves to them)
The gauss cases time rowtf = "z" at the same shape beside them (gsva_exact_z_ms), not replaid.gsva.
The walk kernel to compare with is replaid.ssgsea.exact(single = FALSE)'s: tools/bench_ssgsea_exact.py --only-single-false."""
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
    "dense_t0": dict(genes=20000, cells=10000, sets=5000, tau=0.0, rowtf="z"),
    "dense_t1": dict(genes=20000, cells=10000, sets=5000, tau=1.0, rowtf="z"),
    "dense_t1_none": dict(genes=20000, cells=10000, sets=5000, tau=1.0, rowtf="none"),
    "gauss_2k": dict(genes=20000, cells=2000, sets=5000, tau=1.0, rowtf="gauss"),
    "gauss_10k": dict(genes=20000, cells=10000, sets=5000, tau=1.0, rowtf="gauss"),
}


def _median_ms(fn, reps):
    fn()                                   # warm-up: code objects, context buffers, the result's pages
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def run_case(name, reps, only_exact=False, kcdf_mode=0):
    import ctypes

    import plaid_amd
    from plaid_amd import _lib, synth
    p = CASES[name]
    g, n, tau, rowtf = p["genes"], p["cells"], p["tau"], p["rowtf"]
    Gp, Gi = synth.geneset_csc(g, p["sets"])
    ctx = plaid_amd.Context(0)
    try:
        X = synth.dense_columns(g, 0, n)
        if rowtf == "gauss":
            lib = _lib.load()
            if lib.plaidhip_debug_gsva_kcdf_set_mode(int(kcdf_mode)) != 0:
                raise RuntimeError("kcdf mode")
            exact = _median_ms(lambda: ctx.gsva_exact(X, Gp, Gi, tau, rowtf, True), reps)
            out = {"case": name, **p, "reps": reps, "kcdf_mode": kcdf_mode, "gsva_exact_ms": round(exact, 2),
                   "kcdf_terms": g * n * n}
            if kcdf_mode == 2:
                cnt = ctypes.c_ulonglong(0)
                lib.plaidhip_debug_gsva_kcdf_slow_terms(ctypes.byref(cnt))
                out["kcdf_slow_terms"] = cnt.value
                out["kcdf_slow_share"] = cnt.value / (g * n * n)
            lib.plaidhip_debug_gsva_kcdf_set_mode(0)
            if not only_exact:
                out["gsva_exact_z_ms"] = round(_median_ms(lambda: ctx.gsva_exact(X, Gp, Gi, tau, "z", True), reps), 2)
            return out
        exact = _median_ms(lambda: ctx.gsva_exact(X, Gp, Gi, tau, rowtf, True), reps)
        if only_exact:
            return {"case": name, **p, "reps": reps, "gsva_exact_ms": round(exact, 2)}
        base = _median_ms(lambda: ctx.gsva(X, Gp, Gi, tau, "z"), reps)
    finally:
        ctx.close()
    return {"case": name, **p, "reps": reps, "gsva_exact_ms": round(exact, 2), "gsva_ms": round(base, 2),
            "ratio": round(exact / base, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="run one case in this process and print its JSON")
    ap.add_argument("--only-exact", action="store_true", help="time replaid.gsva.exact alone")
    ap.add_argument("--kcdf-mode", type=int, default=0, choices=(0, 1, 2),
                    help="gauss cases: 0 the fast table index, 1 the exact operations for every term, 2 fast and counting")
    a = ap.parse_args()
    if a.case is not None:
        print(json.dumps(run_case(a.case, a.reps, a.only_exact, a.kcdf_mode)))
        return
    out = []
    for name in a.cases.split(","):
        flags = (["--only-exact"] if a.only_exact else []) + ["--kcdf-mode", str(a.kcdf_mode)]
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps)] + flags,
                           capture_output=True, text=True)
        if r.returncode != 0:
            out.append({"case": name, "error": (r.stderr or r.stdout)[-500:], "returncode": r.returncode})
            break                          # a failed case ends the run: nothing more is started on the device
        out.append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps({"tool": "bench_gsva_exact", "cases": out}))


if __name__ == "__main__":
    main()
