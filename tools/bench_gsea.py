"""plaid.gsea (Context.gsea) at the enrichment experiments' shape, one MI355X: 20,000 genes, 5,000 sets of synth's size
distribution, 1,000 permutations, 1 and 8 ranked lists, unweighted (weight 1) and weighted (|N(0, 1)|).  The yardstick is
the walk kernel replaid.ssgsea.exact(single = FALSE) already has: gsea_ks_kernel at 20,000 genes x 1,000 columns x the same
sets, alpha 0 beside the unweighted cases and 0.25 beside the weighted ones -- the same number of (set, walk) pairs as one
list of the null.  Each case runs in a fresh process, one warm-up call first.  --score-type pos / neg runs the plaid.gsea
cases through plaidhip_gsea_scored; the cases of EDGE_CASES (named in --cases; not among the defaults) ask for the
leading edges as well, and under --profile report gsea_edge_kernel beside gsea_obs_kernel from the same run: both take one
walk per (set, list) pair, and the edge adds the emit.  The cases of ML_CASES (named in --cases likewise) run
Context.gsea_multilevel with its defaults; under --profile they report proposals / s of gsea_ml_mutate_kernel beside walks / s
of gsea_null_kernel from the same run, and the time between the chain kernels' launches.

    python3 tools/bench_gsea.py [--reps 3] [--cases c1_unweighted,...]      host call times, one JSON line
    python3 tools/bench_gsea.py --profile DIR [--cases ...]                 the kernel times as well, one JSON line
    python3 tools/bench_gsea.py --case c8_weighted --reps 1                 one case in this process: what the profiler wraps

--profile runs every case a second time, in a run of its own, as
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/CASE -- python3 tools/bench_gsea.py --case CASE --reps 1
reads the case's kernel (gsea_null_kernel, or gsea_ks_kernel for the yardstick) from the *kernel_stats.csv of that run and
reports kernel_ms, the kernel's time per host call (all of its launches, over the warm-up and the one timed call), and
pairs_per_s = sets x permutations x lists over that time.  The stats files stay in DIR."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GENES, SETS, PERMS = 20000, 5000, 1000
CASES = {
    "c1_unweighted": dict(lists=1, weighted=False),
    "c8_unweighted": dict(lists=8, weighted=False),
    "c1_weighted": dict(lists=1, weighted=True),
    "c8_weighted": dict(lists=8, weighted=True),
    "ks_alpha0": dict(ks=True, alpha=0.0),          # the yardstick: gsea_ks_kernel, 1,000 columns
    "ks_alpha025": dict(ks=True, alpha=0.25),
}
EDGE_CASES = {
    "c8_unweighted_edges": dict(lists=8, weighted=False, edges=True),
    "c8_weighted_edges": dict(lists=8, weighted=True, edges=True),
}
ML_CASES = {   # plaid.gsea with multilevel p-values (Context.gsea_multilevel), the defaults: 101 chains, 4 sweeps, eps 1e-50, mlMin 10
    "ml_c1_unweighted": dict(lists=1, weighted=False, ml=True),
    "ml_c8_unweighted": dict(lists=8, weighted=False, ml=True),
    "ml_c1_weighted": dict(lists=1, weighted=True, ml=True),
    "ml_c8_weighted": dict(lists=8, weighted=True, ml=True),
}
ALL_CASES = {**CASES, **EDGE_CASES, **ML_CASES}
ML_SAMPLE, ML_SWEEPS = 101, 4


def ml_proposals(out, ml):
    """(proposals, rulers, ruler stages) of a multilevel call from its tables: a ruler is one (list, side, size); it mutates
    once per stage before its last, and its last stage is the largest read-off stage of its sets"""
    proposals = rulers = stages = 0
    for l in range(out.shape[2]):
        ok = ~np.isnan(ml[:, 2, l])
        key = np.where(out[ok, 0, l] < 0, 1 << 20, 0) + out[ok, 5, l].astype(np.int64)
        for u in np.unique(key):
            last = int(ml[ok, 2, l][key == u].max())
            rulers += 1
            stages += last + 1
            proposals += ML_SAMPLE * ML_SWEEPS * int(u & ((1 << 20) - 1)) * last
    return proposals, rulers, stages


def _median_ms(fn, reps):
    fn()                                   # warm-up: code objects, buffers, the result's pages
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def run_case(name, reps, genes=GENES, sets=SETS, perms=PERMS, score_type="std"):
    import plaid_amd
    from plaid_amd import synth
    p = ALL_CASES[name]
    Gp, Gi = synth.geneset_csc(genes, sets)
    rng = np.random.default_rng(17)
    ctx = plaid_amd.Context(0)
    try:
        if p.get("ks"):
            X = synth.dense_columns(genes, 0, perms)
            ms = _median_ms(lambda: ctx.ssgsea_exact(X, Gp, Gi, p["alpha"], True, False, single=False), reps)
            pairs = sets * perms
        else:
            stat = rng.normal(size=(genes, p["lists"]))
            w = np.abs(rng.normal(size=stat.shape)) if p["weighted"] else np.ones_like(stat)
            kw = {} if score_type == "std" and not p.get("edges") else dict(score_type=score_type, leading_edge=bool(p.get("edges")))
            extra = {}
            if p.get("ml"):
                keep = []
                ms = _median_ms(lambda: keep.append(ctx.gsea_multilevel(stat, w, Gp, Gi, nperm=perms, seed=1, score_type=score_type)),
                                reps)
                out, ml = keep[-1]
                prop, rulers, stages = ml_proposals(out, ml)
                used = out[:, 4, :] < 10
                extra = {"proposals": prop, "rulers": rulers, "ruler_stages": stages, "pairs_reporting_pvalML": int(used.sum()),
                         "smallest_pval": float(np.nanmin(out[:, 2, :])),
                         "status_counts": [int(np.sum(ml[:, 3, :] == q)) for q in range(3)]}
            else:
                ms = _median_ms(lambda: ctx.gsea(stat, w, Gp, Gi, nperm=perms, seed=1, **kw), reps)
            pairs = sets * perms * p["lists"]
    finally:
        ctx.close()
    if not p.get("ks"):
        p = {**p, "score_type": score_type}
    return {"case": name, **p, "genes": genes, "sets": sets, "perms": perms, "reps": reps, "host_ms": round(ms, 2), "pairs": pairs,
            "host_pairs_per_s": round(pairs / (ms * 1e-3), 1), **(extra if not p.get("ks") else {})}


def _kernel_of(name):
    return "gsea_ks_kernel" if ALL_CASES[name].get("ks") else "gsea_null_kernel"


def profile_case(name, outdir, genes, sets, perms, limit_s, score_type="std"):
    """the case under rocprofv3 --kernel-trace --stats in a process of its own; its kernel's row of the stats file"""
    import csv
    import glob
    d = os.path.join(outdir, name)
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--case", name, "--reps", "1", "--genes", str(genes), "--sets", str(sets), "--perms", str(perms), "--score-type",
           score_type]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit_s)
    if r.returncode != 0:
        return {"error": (r.stderr or r.stdout)[-500:], "returncode": r.returncode}
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return {"error": f"no *kernel_stats.csv under {d}", "returncode": 0}
    if ALL_CASES[name].get("ml"):
        return _profile_ml(name, r.stdout, files[0], d, outdir, sets, perms)
    calls = total_ns = 0
    beside = {"gsea_obs_kernel": 0, "gsea_edge_kernel": 0} if ALL_CASES[name].get("edges") else {}
    with open(files[0], newline="") as fh:
        for row in csv.DictReader(fh):
            if _kernel_of(name) in row["Name"]:
                calls += int(row["Calls"])
                total_ns += int(row["TotalDurationNs"])
            for k in beside:
                if k in row["Name"]:
                    beside[k] += int(row["TotalDurationNs"])
    if calls == 0:
        return {"error": f"{_kernel_of(name)} is not in {files[0]}", "returncode": 0}
    host_calls = 2                                    # the warm-up and --reps 1
    ms = total_ns * 1e-6 / host_calls
    pairs = sets * perms * ALL_CASES[name].get("lists", 1)
    res = {"kernel": _kernel_of(name), "kernel_launches": calls, "kernel_ms": round(ms, 3), "pairs_per_s": round(pairs / (ms * 1e-3), 1),
           "stats_file": os.path.relpath(files[0], outdir)}
    for k, ns in beside.items():          # per host call, like kernel_ms: one walk per (set, list) pair each
        res[k + "_ms"] = round(ns * 1e-6 / host_calls, 3)
    return res


def _profile_ml(name, stdout, stats_file, d, outdir, sets, perms):
    """a multilevel case's profiled run: proposals / s of gsea_ml_mutate_kernel and, beside it from the same run, walks / s
    of gsea_null_kernel (the yardstick: a proposal should cost no more than 1.5 null walks), the other two kernels, and
    the time between the chain kernels' launches (from the kernel trace): the host loop's share"""
    import csv
    import glob
    run = json.loads(stdout.strip().splitlines()[-1])
    host_calls = 2                                    # the warm-up and --reps 1
    ns = {"gsea_ml_mutate_kernel": 0, "gsea_ml_stage_kernel": 0, "gsea_ml_init_kernel": 0, "gsea_null_kernel": 0}
    launches = dict.fromkeys(ns, 0)
    with open(stats_file, newline="") as fh:
        for row in csv.DictReader(fh):
            for k in ns:
                if k in row["Name"]:
                    ns[k] += int(row["TotalDurationNs"])
                    launches[k] += int(row["Calls"])
    if launches["gsea_ml_mutate_kernel"] == 0 or launches["gsea_null_kernel"] == 0:
        return {"error": f"the chain or the null kernel is not in {stats_file}", "returncode": 0}
    res = {"stats_file": os.path.relpath(stats_file, outdir)}
    for k in ns:
        res[k + "_ms"] = round(ns[k] * 1e-6 / host_calls, 3)
        res[k + "_launches"] = launches[k] // host_calls
    mut_s, null_s = ns["gsea_ml_mutate_kernel"] * 1e-9 / host_calls, ns["gsea_null_kernel"] * 1e-9 / host_calls
    walks = sets * perms * (ALL_CASES[name]["lists"] if ALL_CASES[name]["weighted"] else 1)   # (unit weights: one walk serves every list)
    res["proposals_per_s"] = round(run["proposals"] / mut_s, 1)
    res["null_walks_per_s"] = round(walks / null_s, 1)
    res["proposal_cost_in_null_walks"] = round((mut_s / run["proposals"]) / (null_s / walks), 3)
    traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if traces:
        spans = []
        with open(traces[0], newline="") as fh:
            for row in csv.DictReader(fh):
                if "gsea_ml_" in row["Kernel_Name"]:
                    spans.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
        spans.sort()
        gaps = [b[0] - a[1] for a, b in zip(spans, spans[1:]) if 0 < b[0] - a[1] < 50_000_000]   # (not the pause between two calls)
        if gaps:
            res["chain_launches"] = len(spans) // host_calls
            res["chain_launch_gap_mean_us"] = round(float(np.mean(gaps)) * 1e-3, 2)
            res["chain_launch_gap_total_ms"] = round(float(np.sum(gaps)) * 1e-6 / host_calls, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="run one case in this process and print its JSON")
    ap.add_argument("--genes", type=int, default=GENES)
    ap.add_argument("--sets", type=int, default=SETS)
    ap.add_argument("--perms", type=int, default=PERMS)
    ap.add_argument("--score-type", default="std", choices=["std", "pos", "neg"], help="scoreType of the plaid.gsea cases")
    ap.add_argument("--profile", default=None, metavar="DIR", help="also run every case under rocprofv3, stats files into DIR")
    ap.add_argument("--limit", type=int, default=300, help="seconds a profiled case may take")
    a = ap.parse_args()
    if a.case is not None:
        print(json.dumps(run_case(a.case, a.reps, a.genes, a.sets, a.perms, a.score_type)))
        return
    out = []
    for name in a.cases.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps), "--genes", str(a.genes),
                            "--sets", str(a.sets), "--perms", str(a.perms), "--score-type", a.score_type], capture_output=True,
                           text=True, timeout=a.limit)
        if r.returncode != 0:
            out.append({"case": name, "error": (r.stderr or r.stdout)[-500:], "returncode": r.returncode})
            break                          # a failed case ends the run: nothing more is started on the device
        out.append(json.loads(r.stdout.strip().splitlines()[-1]))
        if a.profile is not None:
            k = profile_case(name, a.profile, a.genes, a.sets, a.perms, a.limit, a.score_type)
            out[-1].update(k)
            if "error" in k:
                break
    print(json.dumps({"tool": "bench_gsea", "cases": out}))


if __name__ == "__main__":
    main()
