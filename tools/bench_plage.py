"""replaid.zscore and replaid.plage (Context.zscore, Context.plage) on one MI355X: 20,000 genes x 2,000 samples x 5,000 sets of
synth's hallmark-like size distribution (dense X: independent N(8, 2^2) genes plus one factor common to all genes, which
takes 0.2 to 0.7 of a gene's variance; `g20k_noise` is the same without the factor -- no first eigenvector to find, the power
iteration's worst case), and the reference's pbmc3k shape, 12,010 genes x 10,000 cells (a
dgCMatrix, 7 % stored) x 61,459 real-shaped sets (synth.geneset_csc_real; plage drops the sets above its cap of 4,096
members, as maxSize does).  `_mfma` cases run plage with the v_mfma_f64_16x16x4_f64 form of the Gram kernel (the test hook
plaidhip_debug_plage_gram), which the product does not launch: the comparison of DESIGN.md section 22.  Each case runs in a
fresh process, one warm-up call first.  There is no parent to compare against and no threshold.

    python3 tools/bench_plage.py [--reps 3] [--cases zscore_g20k,plage_g20k,...]   host call times, one JSON line
    python3 tools/bench_plage.py --profile DIR [--cases ...]                        the kernels' times as well
    python3 tools/bench_plage.py --case plage_g20k --reps 1                         one case in this process
    python3 tools/bench_plage.py ... --append profiles/plage_bench.jsonl            also append one line per case

--profile runs every case a second time, in a run of its own, as
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/CASE -- python3 tools/bench_plage.py --case CASE --reps 1
and reports, per kernel, its time per launch; for the Gram kernel also its FMAs per second (sum of k^2 n over its time)."""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    "g20k": dict(genes=20000, samples=2000, sets=5000, real=False, factor=True),
    "g20k_noise": dict(genes=20000, samples=2000, sets=5000, real=False),
    "pbmc3k": dict(genes=12010, samples=10000, sets=61459, real=True),
    "small": dict(genes=2000, samples=200, sets=300, real=False),
}
CASES = {}
for _k, _v in SHAPES.items():
    CASES[f"zscore_{_k}"] = dict(_v, what="zscore")
    CASES[f"plage_{_k}"] = dict(_v, what="plage")
    CASES[f"plage_{_k}_mfma"] = dict(_v, what="plage_mfma")


def _median_ms(fn, reps):
    fn()                                   # warm-up: code objects, buffers, the result's pages
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def make_case(name):
    import scipy.sparse as sp
    from plaid_amd import engine, synth
    p = CASES[name]
    g, n = p["genes"], p["samples"]
    Gp, Gi = (synth.geneset_csc_real if p["real"] else synth.geneset_csc)(g, p["sets"])
    if p["what"] != "zscore":              # the cap, as replaid_plage's maxSize applies it
        sizes = np.diff(Gp)
        keep = np.flatnonzero(sizes <= engine.PLAGE_MAX_SET)
        Gi = np.concatenate([Gi[Gp[j]:Gp[j + 1]] for j in keep]).astype(np.int32)
        Gp = np.concatenate([[0], np.cumsum(sizes[keep])]).astype(np.int32)
    if p["real"]:
        Xp, Xi, Xx = synth.sparse_columns(g, 0, n, density=0.07)
        X = sp.csc_matrix((Xx, Xi, Xp), shape=(g, n))
    else:
        X = synth.dense_columns(g, 0, n)
        if p.get("factor"):                # one factor common to all genes, its share of a gene's variance 0.2 .. 0.7
            rng = np.random.default_rng(31)
            X += rng.uniform(1.0, 3.0, size=g)[:, None] * rng.normal(size=n)[None, :]
    return p, X, Gp, Gi


def run_case(name, reps):
    import plaid_amd
    from plaid_amd import _lib
    p, X, Gp, Gi = make_case(name)
    if p["what"] == "plage_mfma":
        fn = _lib.load().plaidhip_debug_plage_gram
        fn.argtypes, fn.restype = [ctypes.c_int], ctypes.c_int
        _lib.check(fn(1))
    ctx = plaid_amd.Context(0)
    info = None
    try:
        if p["what"] == "zscore":
            ms = _median_ms(lambda: ctx.zscore(X, Gp, Gi), reps)
        else:
            ms = _median_ms(lambda: ctx.plage(X, Gp, Gi), reps)
            info = ctx.plage(X, Gp, Gi)[1]
    finally:
        ctx.close()
    k = np.diff(Gp).astype(np.float64)
    res = {"case": name, **p, "sets_scored": len(Gp) - 1, "memberships": int(Gp[-1]), "reps": reps, "host_ms": round(ms, 2),
           "scores": (len(Gp) - 1) * p["samples"], "gram_fma": float((k * k).sum() * p["samples"]),
           "lib": os.path.basename(os.environ.get("PLAIDHIP_LIB", "libplaidhip.so"))}
    if info is not None:
        it = info[:, 3][info[:, 0] > 0]
        res.update({"iterations_min": float(it.min()), "iterations_median": float(np.median(it)), "iterations_max": float(it.max()),
                    "not_converged": int((info[:, 5][info[:, 0] > 0] == 0).sum())})
    return res


def profile_case(name, outdir, limit_s, gram_fma):
    """the case under rocprofv3 --kernel-trace --stats in a process of its own: every kernel's time per launch"""
    import csv
    import glob
    d = os.path.join(outdir, name)
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--case", name, "--reps", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit_s)
    if r.returncode != 0:
        return {"error": (r.stderr or r.stdout)[-500:], "returncode": r.returncode}
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return {"error": f"no *kernel_stats.csv under {d}", "returncode": 0}
    res = {"stats_file": os.path.relpath(files[0], outdir), "kernels": {}}
    with open(files[0], newline="") as fh:
        for row in csv.DictReader(fh):
            hit = re.search(r"\b(\w*(?:plage|zscore|spmm|csc_expand)\w*)", row["Name"])
            if hit:
                short = hit.group(1)
                calls = int(row["Calls"])
                res["kernels"][short] = {"ms_total": round(int(row["TotalDurationNs"]) * 1e-6, 4), "launches": calls}
                if "plage_gram" in short:   # (three calls in the profiled process: the warm-up, the timed one, the one for info)
                    res["gram_fma_per_s"] = gram_fma * 3 / (int(row["TotalDurationNs"]) * 1e-9)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="zscore_g20k,plage_g20k,plage_g20k_mfma")
    ap.add_argument("--case", default=None, help="run one case in this process and print its JSON")
    ap.add_argument("--profile", default=None, metavar="DIR", help="also run every case under rocprofv3, stats files into DIR")
    ap.add_argument("--append", default=None, metavar="FILE", help="append one JSON line per case to FILE")
    ap.add_argument("--limit", type=int, default=300, help="seconds a case may take")
    a = ap.parse_args()
    if a.case is not None:
        print(json.dumps(run_case(a.case, a.reps)))
        return
    out = []
    for name in a.cases.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps)], capture_output=True,
                           text=True, timeout=a.limit)
        if r.returncode != 0:
            out.append({"case": name, "error": (r.stderr or r.stdout)[-500:], "returncode": r.returncode})
            break                          # a failed case ends the run: nothing more is started on the device
        out.append(json.loads(r.stdout.strip().splitlines()[-1]))
        if a.profile is not None:
            k = profile_case(name, a.profile, a.limit, out[-1]["gram_fma"])
            out[-1].update(k)
            if "error" in k:
                break
    if a.append is not None:
        with open(a.append, "a") as fh:
            for o in out:
                fh.write(json.dumps({"tool": "bench_plage", **o}) + "\n")
    print(json.dumps({"tool": "bench_plage", "cases": out}))


if __name__ == "__main__":
    main()
