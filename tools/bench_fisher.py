"""plaid.fisher (Context.fisher) on one MI355X at the enrichment experiments' shapes: 20,000 genes x 5,000 sets of synth's size
distribution with 1, 64 and 1,000 lists, and 12,010 genes x 61,459 real-shaped sets (synth.geneset_csc_real) with one list;
sig is drawn at 5 % up / 5 % down.  Each case runs in a fresh process, one warm-up call first.  There is no parent to
compare against and no threshold: the host call time stands beside the time of a CPU restatement of the same shape
(cpu_ms: scipy sparse counts and scipy.stats.hypergeom.sf, one process, on at most 8 of the lists -- cpu_lists says how
many; another form of the same statistic, timed for scale only).

    python3 tools/bench_fisher.py [--reps 3] [--cases g20k_c1,...]          host call times, one JSON line
    python3 tools/bench_fisher.py --profile DIR [--cases ...]                 the four kernels' times as well
    python3 tools/bench_fisher.py --case g20k_c64 --reps 1                    one case in this process: what the profiler wraps
    python3 tools/bench_fisher.py ... --append profiles/fisher_bench.jsonl    also append one line per case to that file

--profile runs every case a second time, in a run of its own, as
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/CASE -- python3 tools/bench_fisher.py --case CASE --reps 1
and reports, per kernel, its time per host call (over the warm-up and the one timed call).  The overlap lists are asked for
(and fisher_overlap_kernel runs) in the cases of at most 64 lists: at 1,000 lists ov_idx alone would be gigabytes."""
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
    "g20k_c1": dict(genes=20000, sets=5000, lists=1, real=False),
    "g20k_c64": dict(genes=20000, sets=5000, lists=64, real=False),
    "g20k_c1000": dict(genes=20000, sets=5000, lists=1000, real=False),
    "real_c1": dict(genes=12010, sets=61459, lists=1, real=True),
}
KERNELS = ("fisher_pack_kernel", "fisher_count_kernel", "fisher_tail_kernel", "fisher_overlap_kernel")


def _median_ms(fn, reps):
    fn()                                   # warm-up: code objects, buffers, the result's pages
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def make_case(name):
    from plaid_amd import synth
    p = CASES[name]
    Gp, Gi = (synth.geneset_csc_real if p["real"] else synth.geneset_csc)(p["genes"], p["sets"])
    rng = np.random.default_rng(23)
    u = rng.random(size=(p["genes"], p["lists"]))
    sig = np.asfortranarray((u < 0.05).astype(np.int8) - ((u >= 0.05) & (u < 0.10)).astype(np.int8))
    return p, sig, Gp, Gi


def cpu_restatement_ms(sig, Gp, Gi):
    """counts by a sparse product, the three tails by scipy.stats.hypergeom.sf, Benjamini-Hochberg by sorting: (ms, lists)"""
    import scipy.sparse as sp
    from scipy.stats import hypergeom
    s = sig[:, :min(sig.shape[1], 8)]
    N, c = s.shape
    m = len(Gp) - 1
    t0 = time.perf_counter()
    G = sp.csc_matrix((np.ones(len(Gi)), Gi, Gp), shape=(N, m))
    up, dn = (s == 1).astype(np.float64), (s == -1).astype(np.float64)
    ovU, ovD = G.T @ up, G.T @ dn
    k = np.diff(Gp).astype(np.float64)[:, None]
    nU, nD = up.sum(axis=0)[None, :], dn.sum(axis=0)[None, :]
    for K, x in ((nU, ovU), (nD, ovD), (nU + nD, ovU + ovD)):
        p = hypergeom.sf(x - 1, N, K, k)
        o = np.argsort(-p, axis=0, kind="stable")
        adj = np.take_along_axis(p, o, axis=0) * m / np.arange(m, 0, -1)[:, None]
        np.minimum(1.0, np.minimum.accumulate(adj, axis=0))
    return (time.perf_counter() - t0) * 1e3, c


def run_case(name, reps, cpu=True):
    import plaid_amd
    p, sig, Gp, Gi = make_case(name)
    overlap = p["lists"] <= 64
    ctx = plaid_amd.Context(0)
    try:
        ms = _median_ms(lambda: ctx.fisher(sig, Gp, Gi), reps)
        ms_ov = _median_ms(lambda: ctx.fisher(sig, Gp, Gi, overlap=True), reps) if overlap else None
    finally:
        ctx.close()
    tests = (len(Gp) - 1) * p["lists"] * 3
    res = {"case": name, **p, "memberships": int(Gp[-1]), "reps": reps, "host_ms": round(ms, 2),
           "host_overlap_ms": None if ms_ov is None else round(ms_ov, 2), "tests": tests,
           "host_tests_per_s": round(tests / (ms * 1e-3), 1)}
    if cpu:
        cms, cl = cpu_restatement_ms(sig, Gp, Gi)
        res.update({"cpu_ms": round(cms, 2), "cpu_lists": cl, "cpu_what": "scipy sparse counts + scipy.stats.hypergeom.sf + BH, one process"})
    return res


def profile_case(name, outdir, limit_s):
    """the case under rocprofv3 --kernel-trace --stats in a process of its own; the four kernels' rows of the stats file"""
    import csv
    import glob
    d = os.path.join(outdir, name)
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--case", name, "--reps", "1", "--no-cpu"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit_s)
    if r.returncode != 0:
        return {"error": (r.stderr or r.stdout)[-500:], "returncode": r.returncode}
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return {"error": f"no *kernel_stats.csv under {d}", "returncode": 0}
    ns = {k: 0 for k in KERNELS}
    launches = {k: 0 for k in KERNELS}
    with open(files[0], newline="") as fh:
        for row in csv.DictReader(fh):
            for k in KERNELS:
                if k in row["Name"]:
                    ns[k] += int(row["TotalDurationNs"])
                    launches[k] += int(row["Calls"])
    if launches["fisher_tail_kernel"] == 0:
        return {"error": f"fisher_tail_kernel is not in {files[0]}", "returncode": 0}
    # host calls in the profiled process: warm-up + 1 without the overlap lists, and the same again with them (<= 64 lists)
    res = {"stats_file": os.path.relpath(files[0], outdir)}
    for k in KERNELS:
        if launches[k]:
            res[k + "_ms"] = round(ns[k] * 1e-6 / launches[k], 4)
            res[k + "_launches"] = launches[k]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="run one case in this process and print its JSON")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU restatement's time")
    ap.add_argument("--profile", default=None, metavar="DIR", help="also run every case under rocprofv3, stats files into DIR")
    ap.add_argument("--append", default=None, metavar="FILE", help="append one JSON line per case to FILE")
    ap.add_argument("--limit", type=int, default=300, help="seconds a case may take")
    a = ap.parse_args()
    if a.case is not None:
        print(json.dumps(run_case(a.case, a.reps, cpu=not a.no_cpu)))
        return
    out = []
    for name in a.cases.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps)] +
                           (["--no-cpu"] if a.no_cpu else []), capture_output=True, text=True, timeout=a.limit)
        if r.returncode != 0:
            out.append({"case": name, "error": (r.stderr or r.stdout)[-500:], "returncode": r.returncode})
            break                          # a failed case ends the run: nothing more is started on the device
        out.append(json.loads(r.stdout.strip().splitlines()[-1]))
        if a.profile is not None:
            k = profile_case(name, a.profile, a.limit)
            out[-1].update(k)
            if "error" in k:
                break
    if a.append is not None:
        with open(a.append, "a") as fh:
            for o in out:
                fh.write(json.dumps({"tool": "bench_fisher", **o}) + "\n")
    print(json.dumps({"tool": "bench_fisher", "cases": out}))


if __name__ == "__main__":
    main()
