"""plaid.camera (Context.camera) on one MI355X at the enrichment experiments' shape: 20,000 genes x 1,000 samples x 5,000 sets
(10 to 200 members, about 70 on average) x 8 contrasts, each contrast a fit [1, group, covariate] of its own that leaves a
fifth of the samples out (what plaid_camera_contrasts sends).  Three cases on the same input: "estimate" (every set's
variance inflation factor from the residuals: Z, T = G'Z and the sums of squares, fit by fit), "fixed" (inter_gene_cor =
0.01: no Z) and "limma" (Context.limma alone: the fit both share, unchanged by plaid.camera).  Each case runs in a fresh
process, one warm-up call first, then `reps` calls: the median, the minimum and the maximum.  There is no threshold.

    python3 tools/bench_camera.py [--reps 5] [--cases estimate,fixed,limma]      host call times, one JSON line
    python3 tools/bench_camera.py --profile DIR [--cases ...]                     the kernels' times as well
    python3 tools/bench_camera.py --case estimate --reps 1                        one case in this process: what the profiler wraps

--profile runs every case a second time, in a run of its own, as
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/CASE -- python3 tools/bench_camera.py --case CASE --reps 1
and reports, per kernel, its time per launch; for the residual kernel also the share of the 8 TB/s peak that one read of X
and one write of Z come to, for the sum of squares one read of T."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GENES, SAMPLES, SETS, CONTRASTS, P = 20000, 1000, 5000, 8, 3
CASES = ("estimate", "fixed", "limma")
KERNELS = ("camera_residual_kernel", "camera_sumsq_kernel", "lmfit_masks_kernel", "row_design_effects_kernel",
           "row_design_rss_kernel", "reduce_blocks_flat_kernel", "spmm")
PEAK = 8e12   # bytes per second


def _times_ms(fn, reps):
    fn()                                   # warm-up: code objects, buffers, the prepared sets, the result's pages
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def make_input():
    rng = np.random.default_rng(31)
    n, g = SAMPLES, GENES
    D = np.empty((n, P, CONTRASTS), order="F")
    use = np.ones((n, CONTRASTS), dtype=np.int8, order="F")
    for f in range(CONTRASTS):
        D[:, 0, f] = 1.0
        D[:, 1, f] = rng.permutation(np.arange(n) % 2)
        D[:, 2, f] = rng.normal(size=n)
        use[rng.random(n) < 0.2, f] = 0
    factor = rng.standard_normal(size=(4, n))                  # shared factors: the genes of a set are correlated
    load = 0.4 * rng.standard_normal(size=(g, 4))
    X = np.asfortranarray(rng.standard_normal(size=(g, n)) + load @ factor + 0.3 * rng.standard_normal(size=(g, 1)) * D[:, 1, 0][None, :])
    sizes = rng.integers(10, 201, size=SETS)
    sizes = np.minimum(sizes, rng.integers(10, 201, size=SETS))   # skewed to the small side: about 70 on average
    Gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    Gi = np.concatenate([np.sort(rng.choice(g, size=int(k), replace=False)) for k in sizes]).astype(np.int32)
    K = np.zeros((P, 1))
    K[1, 0] = 1.0
    return X, D, use, K, Gp, Gi


def run_case(name, reps):
    import plaid_amd
    X, D, use, K, Gp, Gi = make_input()
    ctx = plaid_amd.Context(0)
    try:
        if name == "limma":
            call = lambda: ctx.limma(X, D, use, K)              # noqa: E731
        else:
            rho = None if name == "estimate" else 0.01
            call = lambda: ctx.camera(X, D, Gp, Gi, use, K, rho, False)   # noqa: E731
        ts = _times_ms(call, reps)
        out, hyper = call()
    finally:
        ctx.close()
    res = {"case": name, "genes": GENES, "samples": SAMPLES, "sets": SETS, "contrasts": CONTRASTS, "p": P, "reps": reps,
           "members": int(Gp[-1]), "host_ms_median": round(float(np.median(ts)), 2), "host_ms_min": round(min(ts), 2),
           "host_ms_max": round(max(ts), 2)}
    if name != "limma":
        res["vif_median"] = float(np.nanmedian(out[:, 2, 0, 0]))
        res["p_below_0.05"] = int((out[:, 6, 0, 0] < 0.05).sum())
        res["df_camera"] = [float(h) for h in hyper[:, 5]]
    return res


def profile_case(name, outdir, limit_s):
    """the case under rocprofv3 --kernel-trace --stats in a process of its own; the kernels' rows of the stats file"""
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
    ns = {k: 0 for k in KERNELS}
    launches = {k: 0 for k in KERNELS}
    with open(files[0], newline="") as fh:
        for row in csv.DictReader(fh):
            for k in KERNELS:
                if k in row["Name"]:
                    ns[k] += int(row["TotalDurationNs"])
                    launches[k] += int(row["Calls"])
    res = {"stats_file": os.path.relpath(files[0], outdir)}
    traffic = {"camera_residual_kernel": 2 * GENES * SAMPLES * 8, "camera_sumsq_kernel": SETS * SAMPLES * 8}
    for k in KERNELS:
        if launches[k]:
            ms = ns[k] * 1e-6 / launches[k]
            res[k + "_ms"] = round(ms, 4)
            res[k + "_launches"] = launches[k]
            if k in traffic:
                res[k + "_share_of_8TBs"] = round(traffic[k] / (ms * 1e-3) / PEAK, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="run one case in this process and print its JSON")
    ap.add_argument("--profile", default=None, metavar="DIR", help="also run every case under rocprofv3, stats files into DIR")
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
    print(json.dumps({"tool": "bench_camera", "cases": out}))


if __name__ == "__main__":
    main()
