"""plaid.rankcor (Context.rankcor) on one MI355X at the enrichment experiments' shapes: 20,000 genes x 5,000 sets of synth's size
distribution with 1, 64 and 1,000 lists, and 12,010 genes x 61,459 real-shaped sets (synth.geneset_csc_real) with one list;
every case in rank mode and in value mode.  The statistics are standard normal draws; every second list has 10 % NaN.
Each case runs in a fresh process, one warm-up call first.  There is no parent to compare against and no threshold: the
host call time stands beside the time of a CPU restatement of the same shape (cpu_ms: scipy ranks, one sparse product per
list for the sums, the closed form, Benjamini-Hochberg; one process, on at most 8 of the lists -- cpu_lists says how many;
timed for scale only).

    python3 tools/bench_rankcor.py [--reps 3] [--cases g20k_c1_rank,...]       host call times, one JSON line
    python3 tools/bench_rankcor.py --profile DIR [--cases ...]                  the kernels' times as well
    python3 tools/bench_rankcor.py --case g20k_c64_rank --reps 1                one case in this process: what the profiler wraps
    python3 tools/bench_rankcor.py ... --append profiles/rankcor_bench.jsonl    also append one line per case to that file

--profile runs every case a second time, in a run of its own, as
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/CASE -- python3 tools/bench_rankcor.py --case CASE --reps 1
and reports, per kernel, its time per launch (over the warm-up and the one timed call).  PLAIDHIP_LIB picks another build of
the library (the A/B of the gather kernel's two mappings: make -C plaid_amd/csrc variant NAME=rclanes8
DEFS=-DPLAIDHIP_RANKCOR_LANES8)."""
import argparse
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
    "g20k_c1": dict(genes=20000, sets=5000, lists=1, real=False),
    "g20k_c64": dict(genes=20000, sets=5000, lists=64, real=False),
    "g20k_c1000": dict(genes=20000, sets=5000, lists=1000, real=False),
    "real_c1": dict(genes=12010, sets=61459, lists=1, real=True),
}
CASES = {f"{k}_{mode}": dict(v, use_rank=(mode == "rank")) for k, v in SHAPES.items() for mode in ("rank", "value")}


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
    rng = np.random.default_rng(29)
    stat = np.asfortranarray(rng.normal(size=(p["genes"], p["lists"])))
    for l in range(0 if p["lists"] == 1 else 1, p["lists"], 2):      # 10 % NaN in half of the lists (a single list: in it)
        stat[rng.random(p["genes"]) < 0.1, l] = np.nan
    return p, stat, Gp, Gi


def cpu_restatement_ms(stat, Gp, Gi, use_rank):
    """scipy ranks, the sums by a sparse product per list, the closed form, Benjamini-Hochberg by sorting: (ms, lists)"""
    import scipy.sparse as sp
    from scipy.stats import norm, rankdata
    s = stat[:, :min(stat.shape[1], 8)]
    g, c = s.shape
    m = len(Gp) - 1
    t0 = time.perf_counter()
    G = sp.csc_matrix((np.ones(len(Gi)), Gi, Gp), shape=(g, m))
    for l in range(c):
        ok = ~np.isnan(s[:, l])
        v = np.zeros(g)
        v[ok] = rankdata(s[ok, l]) if use_rank else s[ok, l]
        v[ok] -= v[ok].mean()
        n = ok.sum()
        k = G.T @ ok.astype(np.float64)
        A = G.T @ v
        with np.errstate(divide="ignore", invalid="ignore"):
            rho = A / np.sqrt(k * (n - k) / n * np.sum(v * v))
            t = rho * np.sqrt((n - 2) / ((1 - rho) * (1 + rho)))
        p = 2 * norm.sf(np.abs(t))
        o = np.argsort(-p, kind="stable")
        np.minimum(1.0, np.minimum.accumulate(p[o] * m / np.arange(m, 0, -1)))
    return (time.perf_counter() - t0) * 1e3, c


def run_case(name, reps, cpu=True):
    import plaid_amd
    p, stat, Gp, Gi = make_case(name)
    ctx = plaid_amd.Context(0)
    try:
        ms = _median_ms(lambda: ctx.rankcor(stat, Gp, Gi, use_rank=p["use_rank"]), reps)
    finally:
        ctx.close()
    tests = (len(Gp) - 1) * p["lists"]
    res = {"case": name, **p, "memberships": int(Gp[-1]), "reps": reps, "host_ms": round(ms, 2), "tests": tests,
           "host_tests_per_s": round(tests / (ms * 1e-3), 1), "lib": os.path.basename(os.environ.get("PLAIDHIP_LIB", "libplaidhip.so"))}
    if cpu:
        cms, cl = cpu_restatement_ms(stat, Gp, Gi, p["use_rank"])
        res.update({"cpu_ms": round(cms, 2), "cpu_lists": cl, "cpu_what": "scipy rankdata + sparse products + closed form + BH, one process"})
    return res


def profile_case(name, outdir, limit_s):
    """the case under rocprofv3 --kernel-trace --stats in a process of its own: every kernel's time per launch"""
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
    res = {"stats_file": os.path.relpath(files[0], outdir), "kernels": {}}
    with open(files[0], newline="") as fh:
        for row in csv.DictReader(fh):
            hit = re.search(r"\b(\w*(?:rankcor|colranks)\w*)", row["Name"])
            if hit:
                short = hit.group(1)
                res["kernels"][short] = {"ms_per_launch": round(int(row["TotalDurationNs"]) * 1e-6 / int(row["Calls"]), 4),
                                         "launches": int(row["Calls"])}
    if not any("rankcor_gather" in k for k in res["kernels"]):
        return {"error": f"the gather kernel is not in {files[0]}", "returncode": 0}
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
                fh.write(json.dumps({"tool": "bench_rankcor", **o}) + "\n")
    print(json.dumps({"tool": "bench_rankcor", "cases": out}))


if __name__ == "__main__":
    main()
