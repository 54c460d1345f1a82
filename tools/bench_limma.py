"""plaid.limma (Context.limma) on one MI355X at the enrichment experiments' shapes: 5,000 sets x 10,000 samples and 20,000 genes
x 10,000 samples, each with (p, nfit) = (2, 1), (4, 1), (3, 8) and (3, 2); 61,459 sets x 10,000 samples at (2, 1).  The rows are
Gaussian with a group effect, the designs [1, group, covariates], and every fit but the first leaves a fifth of the samples
out.  Each case runs in a fresh process, one warm-up call first.  There is no parent to compare against and no threshold.

    python3 tools/bench_limma.py [--reps 3] [--cases sets5k_p2f1,...]        host call times, one JSON line
    python3 tools/bench_limma.py --profile DIR [--cases ...]                  the kernels' times as well
    python3 tools/bench_limma.py --case sets5k_p2f1 --reps 1                  one case in this process: what the profiler wraps
    python3 tools/bench_limma.py ... --append profiles/limma_bench.jsonl      also append one line per case to that file

--profile runs every case a second time, in a run of its own, as
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/CASE -- python3 tools/bench_limma.py --case CASE --reps 1
and reports, per kernel, its time per launch and the share of the 8 TB/s peak its reads of the matrix come to: the effects
kernel reads it ceil(nfit (p + 1) / 8) times per launch, the RSS kernel nfit times.  The (3, 2) cases have W = 8 weight
columns, one full tile; they also run the one fair neighbour, row_contrast_partials_kernel (plaidhip_dev_row_contrast_sums
with 8 contrasts: the same rows, columns and tile, adds where this one has fma), on the same matrix held on the device."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"sets5k": 5000, "genes20k": 20000, "sets61k": 61459}
SAMPLES = 10000
CASES = {f"{s}_p{p}f{f}": dict(rows=SHAPES[s], n=SAMPLES, p=p, nfit=f)
         for s in ("sets5k", "genes20k") for p, f in ((2, 1), (4, 1), (3, 8), (3, 2))}
CASES["sets61k_p2f1"] = dict(rows=SHAPES["sets61k"], n=SAMPLES, p=2, nfit=1)
KERNELS = ("lmfit_masks_kernel", "row_design_effects_kernel", "row_design_rss_kernel", "reduce_blocks_flat_kernel",
           "row_contrast_partials_kernel")
PEAK = 8e12   # bytes per second


def _median_ms(fn, reps):
    fn()                                   # warm-up: code objects, buffers, the result's pages
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def make_case(name):
    c = CASES[name]
    rows, n, p, nfit = c["rows"], c["n"], c["p"], c["nfit"]
    rng = np.random.default_rng(29)
    D = np.empty((n, p, nfit), order="F")
    use = np.ones((n, nfit), dtype=np.int8, order="F")
    for f in range(nfit):
        D[:, 0, f] = 1.0
        D[:, 1, f] = rng.permutation(np.arange(n) % 2)
        D[:, 2:, f] = rng.normal(size=(n, p - 2))
        if f > 0:
            use[rng.random(n) < 0.2, f] = 0
    A = np.empty((rows, n), order="F")
    effect = 0.3 * rng.standard_normal(size=(rows, 1))
    for c0 in range(0, n, 500):            # (column slabs: the largest case is 4.9 GB)
        c1 = min(c0 + 500, n)
        A[:, c0:c1] = rng.standard_normal(size=(rows, c1 - c0)) + effect * D[c0:c1, 1, 0][None, :]
    K = np.zeros((p, 1))
    K[1, 0] = 1.0
    return c, A, D, (use if nfit > 1 else None), K


def neighbour(ctx, A):
    """plaidhip_dev_row_contrast_sums with 8 contrasts on A held on the device, twice (the profiler takes the kernel's time)"""
    import torch
    dev = torch.device("cuda", 0)
    rows, n = A.shape
    Ad = torch.from_numpy(np.ascontiguousarray(A.T)).to(dev)
    Y = torch.from_numpy((np.random.default_rng(5).random((8, n)) < 0.5).astype(np.int32)).to(dev)
    sums = torch.empty((8 * 2 * rows,), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    for _ in range(2):
        ctx.dev_row_contrast_sums(Ad.data_ptr(), rows, rows, n, Y.data_ptr(), 8, sums.data_ptr())
    ctx.synchronize()


def run_case(name, reps):
    import plaid_amd
    c, A, D, use, K = make_case(name)
    ctx = plaid_amd.Context(0)
    try:
        ms = _median_ms(lambda: ctx.limma(A, D, use, K), reps)
        out, hyper = ctx.limma(A, D, use, K)
        if c["p"] == 3 and c["nfit"] == 2:
            neighbour(ctx, A)
    finally:
        ctx.close()
    tests = c["rows"] * c["nfit"]
    return {"case": name, **c, "reps": reps, "host_ms": round(ms, 2), "tests": tests,
            "host_tests_per_s": round(tests / (ms * 1e-3), 1), "df_prior": [float(h) for h in hyper[:, 1]],
            "rows_ok": int(hyper[0, 3]), "p_below_0.05": int((out[:, 3, 0, 0] < 0.05).sum())}


def profile_case(name, outdir, limit_s):
    """the case under rocprofv3 --kernel-trace --stats in a process of its own; the kernels' rows of the stats file"""
    import csv
    import glob
    c = CASES[name]
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
    ns = {k: 0 for k in KERNELS}
    launches = {k: 0 for k in KERNELS}
    with open(files[0], newline="") as fh:
        for row in csv.DictReader(fh):
            for k in KERNELS:
                if k in row["Name"]:
                    ns[k] += int(row["TotalDurationNs"])
                    launches[k] += int(row["Calls"])
    if launches["row_design_effects_kernel"] == 0:
        return {"error": f"row_design_effects_kernel is not in {files[0]}", "returncode": 0}
    res = {"stats_file": os.path.relpath(files[0], outdir)}
    matrix = c["rows"] * c["n"] * 8
    reads = {"row_design_effects_kernel": -(-c["nfit"] * (c["p"] + 1) // 8), "row_design_rss_kernel": c["nfit"],
             "row_contrast_partials_kernel": 1}
    for k in KERNELS:
        if launches[k]:
            ms = ns[k] * 1e-6 / launches[k]
            res[k + "_ms"] = round(ms, 4)
            res[k + "_launches"] = launches[k]
            if k in reads:
                res[k + "_reads_of_A"] = reads[k]
                res[k + "_share_of_8TBs"] = round(matrix * reads[k] / (ms * 1e-3) / PEAK, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
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
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=a.limit)
        if r.returncode != 0:
            out.append({"case": name, "error": (r.stderr or r.stdout)[-500:], "returncode": r.returncode})
            break                          # a failed case ends the run: nothing more is started on the device
        out.append(json.loads(r.stdout.strip().splitlines()[-1]))
        if a.profile is not None:
            k = profile_case(name, a.profile, a.limit)
            out[-1].update(k)
            if "error" in k:
                break
        print(json.dumps(out[-1]), file=sys.stderr, flush=True)
    if a.append is not None:
        with open(a.append, "a") as fh:
            for o in out:
                fh.write(json.dumps({"tool": "bench_limma", **o}) + "\n")
    print(json.dumps({"tool": "bench_limma", "cases": out}))


if __name__ == "__main__":
    main()
