"""plaid.romer (Context.romer) on one MI355X: 20,000 genes x 100 samples x 5,000 sets of 10 to 200 members (tools/bench_fry.py
makes the input), one fit [1, group, covariate], one contrast, nrot = 9,999 rotations, set statistic "mean".

Cases, each in a fresh process:
    romer        the whole call (host time: upload, fit, host shrink, 9,999 rotations, tables)
    roast_mean   plaid.roast with set statistic "mean" at the same shape and nrot: the yardstick
    phases       the device passes of one chunk of CHUNK rotations on device pointers, timed one by one between stream
                 synchronisations -- rotate (roast_rotate_kernel, no z-score), keys, ranks (two key matrices), sides (the
                 entry prepares the collection on every call: that is in its time, and once per fit in the whole call) --
                 and scaled to 9,999 rotations; beside the sides of mean / floormean (the rank crossprod and a count
                 kernel), the crossprods alone on a collection prepared once, and the time of the dedicated
                 wave-per-(set, rotation) gather kernel that mean50 runs on the same ranks.  The values are random (the timing does not depend on them but for the rankers' ties).
One warm-up first, then `reps` runs: the median, the minimum and the maximum.  There is no threshold.

    python3 tools/bench_romer.py [--reps 3] [--cases romer,roast_mean,phases] [--stat mean]
    python3 tools/bench_romer.py --case phases --reps 3          one case in this process (what a profiler wraps)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_fry as bf  # noqa: E402

NROT = 9999
SAMPLES = 100
CHUNK = 1280          # rotations of the timed chunk: 20 tiles
CASES = ("romer", "roast_mean", "phases")


def make_input():
    bf.SAMPLES["romer"] = SAMPLES
    return bf.make_input("romer")


def _stats(ts):
    return {"ms_median": round(float(np.median(ts)), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}


def run_call(name, reps, stat):
    import plaid_amd
    X, D, K, Gp, Gi = make_input()
    ctx = plaid_amd.Context(0)
    try:
        if name == "romer":
            call = lambda: ctx.romer(X, D, Gp, Gi, None, K, stat, nrot=NROT, seed=1)            # noqa: E731
        else:
            call = lambda: ctx.roast(X, D, Gp, Gi, None, K, "mean", nrot=NROT, seed=1)          # noqa: E731
        ts = bf._times_ms(call, reps)
        out, hyper = call()
    finally:
        ctx.close()
    res = {"case": name, "genes": bf.GENES, "samples": SAMPLES, "sets": bf.SETS, "nrot": NROT, "reps": reps,
           "members": int(Gp[-1]), **{"host_" + k: v for k, v in _stats(ts).items()}}
    if name == "romer":
        res.update(stat=stat, up_below_0_05=int((out[:, 1, 0, 0] < 0.05).sum()), mixed_below_0_05=int((out[:, 3, 0, 0] < 0.05).sum()),
                   proportion=float(hyper[0, 8]))
    return res


def run_phases(reps, stat):
    import torch

    import plaid_amd
    from plaid_amd import engine
    dev = torch.device("cuda", 0)
    _, D, _, Gp, Gi = make_input()
    g, n, m = bf.GENES, SAMPLES, bf.SETS
    rng = np.random.default_rng(5)
    ld, ldu, ldw = g, g, CHUNK
    W = engine.roast_rotations(D, None, 0, CHUNK, 1)
    Rz = torch.from_numpy(rng.standard_normal(size=(n, ld))).to(dev)
    beta = torch.from_numpy(rng.standard_normal(size=g) * 2).to(dev)
    rss = (Rz * Rz).sum(dim=0).contiguous()
    Wd = torch.from_numpy(np.ascontiguousarray(W)).to(dev)
    Z = torch.empty((CHUNK // 64) * g * 64, dtype=torch.float64, device=dev)
    uidx = torch.arange(g, dtype=torch.int32, device=dev)
    nkeys = 3 if stat == "floormean" else 2
    K = [torch.empty(CHUNK * ldu, dtype=torch.float64, device=dev) for _ in range(3)]
    Rk = [torch.empty(CHUNK * ldu, dtype=torch.float64, device=dev) for _ in range(3)]
    Gpd, Gid = torch.from_numpy(Gp).to(dev), torch.from_numpy(Gi).to(dev)
    obs = torch.zeros(m * 3, dtype=torch.int64, device=dev)
    cnt = torch.zeros(m * 3, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx = plaid_amd.Context(0)
    sid = engine.ROMER_STATISTIC[stat]
    kb = K[1].data_ptr() if nkeys == 3 else None
    rb = Rk[1].data_ptr() if nkeys == 3 else None
    which = [0, 2] if nkeys == 2 else [0, 1, 2]
    sides = lambda sd: ctx.dev_romer_sides(Rk[0].data_ptr(), rb if sd == 1 else None, Rk[2].data_ptr(), ldu, g, Gpd.data_ptr(),   # noqa: E731
                                           Gid.data_ptr(), m, sd, CHUNK, 0, None, obs.data_ptr(), cnt.data_ptr())
    try:
        steps = {
            "rotate": lambda: ctx.dev_roast_rotate(Rz.data_ptr(), ld, g, n, beta.data_ptr(), rss.data_ptr(), Wd.data_ptr(), ldw, CHUNK,
                                                   float(n - 3), 4.0, 1.0, 1, 0, Z.data_ptr()),
            "keys": lambda: ctx.dev_romer_keys(Z.data_ptr(), g, uidx.data_ptr(), g, ldu, sid, CHUNK, 0, K[0].data_ptr(), kb,
                                               K[2].data_ptr(), None),
            "ranks": lambda: [ctx.dev_colranks_dense(K[e].data_ptr(), ldu, g, CHUNK, Rk[e].data_ptr(), ldu) for e in which],
            "sides": lambda: sides(sid),
        }
        if stat != "mean50":
            # the crossprods alone on a collection prepared once, as the whole call runs them (the entry above prepares it on
            # every call); and the other way to the sums: the wave-per-(set, rotation) gather kernel that mean50 runs
            gs = ctx.geneset(g, Gp, Gi)
            S = torch.empty(m * CHUNK, dtype=torch.float64, device=dev)
            steps["sides_crossprods_alone"] = lambda: [ctx.dev_spmm_ranks(gs, Rk[e].data_ptr(), ldu, CHUNK, S.data_ptr(), m,
                                                                          stat="sum") for e in which]
            steps["sides_by_gather_kernel"] = lambda: sides(engine.ROMER_STATISTIC["mean50"])
        res = {"case": "phases", "genes": g, "samples": n, "sets": m, "chunk": CHUNK, "nrot": NROT, "stat": stat, "reps": reps}
        scale = NROT / CHUNK
        for name, fn in steps.items():
            def timed():
                fn()
                ctx.synchronize()
            ts = bf._times_ms(timed, reps)
            st = _stats(ts)
            res[name] = {"chunk_" + k: v for k, v in st.items()}
            res[name]["ms_for_nrot"] = round(st["ms_median"] * scale, 1)
    finally:
        ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stat", default="mean")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="run one case in this process and print its JSON")
    ap.add_argument("--limit", type=int, default=400, help="seconds a case may take")
    a = ap.parse_args()
    if a.case is not None:
        t0 = time.perf_counter()
        r = run_phases(a.reps, a.stat) if a.case == "phases" else run_call(a.case, a.reps, a.stat)
        r["case_seconds"] = round(time.perf_counter() - t0, 1)
        print(json.dumps(r))
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
    print(json.dumps({"tool": "bench_romer", "cases": out}))


if __name__ == "__main__":
    main()
