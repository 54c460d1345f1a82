"""plaid.fry (Context.fry) on one MI355X beside plaid.camera with estimated VIF on the same input, at two shapes, one fit
[1, group, covariate] and one contrast each, 5,000 sets of 10 to 200 members (about 70 on average):

    large   20,000 genes x 1,000 samples: d + 1 = 998 effects, above the cap -- the directional test alone
    mixed   20,000 genes x 64 samples: d + 1 = 62 effects -- residual effects, Gram and eigen stages as well

Cases: fry_large, camera_large, fry_mixed, camera_mixed.  Each case runs in a fresh process, one warm-up call first, then
`reps` calls: the median, the minimum and the maximum.  There is no threshold.

    python3 tools/bench_fry.py [--reps 5] [--cases fry_large,camera_large,fry_mixed,camera_mixed]    host call times
    python3 tools/bench_fry.py --profile DIR [--cases ...]                                           the kernels' times as well
    python3 tools/bench_fry.py --case fry_mixed --reps 1                                             what the profiler wraps

--profile runs every case a second time, in a run of its own, as
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/CASE -- python3 tools/bench_fry.py --case CASE --reps 1
and reports, per kernel, its time per launch."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GENES, SETS, P = 20000, 5000, 3
SAMPLES = {"large": 1000, "mixed": 64}
CASES = ("fry_large", "camera_large", "fry_mixed", "camera_mixed")
KERNELS = ("fry_residual_kernel", "fry_gram_kernel", "fry_eigen_kernel", "camera_residual_kernel", "camera_sumsq_kernel",
           "lmfit_masks_kernel", "row_design_effects_kernel", "row_design_rss_kernel", "reduce_blocks_flat_kernel", "spmm")


def _times_ms(fn, reps):
    fn()                                   # warm-up: code objects, buffers, the prepared sets, the result's pages
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def make_input(shape):
    rng = np.random.default_rng(32)
    n, g = SAMPLES[shape], GENES
    D = np.empty((n, P), order="F")
    D[:, 0] = 1.0
    D[:, 1] = rng.permutation(np.arange(n) % 2)
    D[:, 2] = rng.normal(size=n)
    factor = rng.standard_normal(size=(4, n))                  # shared factors: the genes of a set are correlated
    load = 0.4 * rng.standard_normal(size=(g, 4))
    X = np.asfortranarray(rng.standard_normal(size=(g, n)) + load @ factor + 0.3 * rng.standard_normal(size=(g, 1)) * D[:, 1][None, :])
    sizes = rng.integers(10, 201, size=SETS)
    sizes = np.minimum(sizes, rng.integers(10, 201, size=SETS))
    Gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    Gi = np.concatenate([np.sort(rng.choice(g, size=int(k), replace=False)) for k in sizes]).astype(np.int32)
    K = np.zeros((P, 1))
    K[1, 0] = 1.0
    return X, D, K, Gp, Gi


def run_case(name, reps):
    import plaid_amd
    method, shape = name.split("_")
    X, D, K, Gp, Gi = make_input(shape)
    ctx = plaid_amd.Context(0)
    try:
        if method == "fry":
            call = lambda: ctx.fry(X, D, Gp, Gi, None, K)                     # noqa: E731
        else:
            call = lambda: ctx.camera(X, D, Gp, Gi, None, K, None, False)     # noqa: E731
        ts = _times_ms(call, reps)
        out, hyper = call()
    finally:
        ctx.close()
    res = {"case": name, "genes": GENES, "samples": SAMPLES[shape], "sets": SETS, "p": P, "reps": reps, "members": int(Gp[-1]),
           "host_ms_median": round(float(np.median(ts)), 2), "host_ms_min": round(min(ts), 2), "host_ms_max": round(max(ts), 2)}
    if method == "fry":
        res["mixed_offered"] = float(hyper[0, 6])
        res["p_below_0.05"] = int((out[:, 3, 0, 0] < 0.05).sum())
        res["p_mixed_below_0.05"] = int((out[:, 5, 0, 0] < 0.05).sum())
        res["p_mixed_nan"] = int(np.isnan(out[:, 5, 0, 0]).sum())
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
    for k in KERNELS:
        if launches[k]:
            res[k + "_ms"] = round(ns[k] * 1e-6 / launches[k], 4)
            res[k + "_launches"] = launches[k]
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
    print(json.dumps({"tool": "bench_fry", "cases": out}))


if __name__ == "__main__":
    main()
