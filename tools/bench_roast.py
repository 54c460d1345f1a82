"""plaid.roast (Context.roast) on one MI355X beside plaid.fry on the same input (tools/bench_fry.py makes it): 20,000 genes x
5,000 sets of 10 to 200 members, one fit [1, group, covariate], one contrast, nrot = 1,999 rotations, at

    large   1,000 samples (plaid.fry: directional only, above its cap)
    mixed   64 samples

Cases: roast_large, fry_large, roast_mixed, fry_mixed (set statistic mean50; --stat picks another).  Each case runs in a
fresh process, one warm-up call first, then `reps` calls: the median, the minimum and the maximum.  There is no threshold.

    python3 tools/bench_roast.py [--reps 3] [--stat mean50] [--cases ...]      host call times
    python3 tools/bench_roast.py --case roast_mixed --reps 1                   one case in this process (what a profiler wraps)"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_fry as bf  # noqa: E402

NROT = 1999
CASES = ("roast_large", "fry_large", "roast_mixed", "fry_mixed")


def run_case(name, reps, stat):
    import plaid_amd
    method, shape = name.split("_")
    X, D, K, Gp, Gi = bf.make_input(shape)
    ctx = plaid_amd.Context(0)
    try:
        if method == "roast":
            call = lambda: ctx.roast(X, D, Gp, Gi, None, K, stat, nrot=NROT, seed=1)     # noqa: E731
        else:
            call = lambda: ctx.fry(X, D, Gp, Gi, None, K)                                # noqa: E731
        ts = bf._times_ms(call, reps)
        out, hyper = call()
    finally:
        ctx.close()
    res = {"case": name, "genes": bf.GENES, "samples": bf.SAMPLES[shape], "sets": bf.SETS, "reps": reps, "members": int(Gp[-1]),
           "host_ms_median": round(float(np.median(ts)), 2), "host_ms_min": round(min(ts), 2), "host_ms_max": round(max(ts), 2)}
    pcol, mcol = (4, 6) if method == "roast" else (3, 5)
    if method == "roast":
        res.update(stat=stat, nrot=NROT)
    res["p_below_0.05"] = int((out[:, pcol, 0, 0] < 0.05).sum())
    res["p_mixed_below_0.05"] = int((out[:, mcol, 0, 0] < 0.05).sum())
    res["p_mixed_nan"] = int(np.isnan(out[:, mcol, 0, 0]).sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stat", default="mean50")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="run one case in this process and print its JSON")
    ap.add_argument("--limit", type=int, default=300, help="seconds a case may take")
    a = ap.parse_args()
    if a.case is not None:
        print(json.dumps(run_case(a.case, a.reps, a.stat)))
        return
    out = []
    for name in a.cases.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps), "--stat", a.stat],
                           capture_output=True, text=True, timeout=a.limit)
        if r.returncode != 0:
            out.append({"case": name, "error": (r.stderr or r.stdout)[-500:], "returncode": r.returncode})
            break                          # a failed case ends the run: nothing more is started on the device
        out.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(out[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"tool": "bench_roast", "cases": out}))


if __name__ == "__main__":
    main()
