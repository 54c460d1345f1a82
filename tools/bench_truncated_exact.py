"""replaid.ucell.exact and replaid.aucell.exact (Context.ucell_exact / aucell_exact) beside replaid.ucell / replaid.aucell
(Context.ucell / aucell) at the same shapes, one MI355X: host calls as a median of `reps`, and the peak device memory of
every kind of call (hipMemGetInfo through torch, sampled every few milliseconds by a thread WHILE the warm-up call runs, so
that the buffers a call frees before it returns -- the weight slots -- are counted; the timed calls run unsampled).  Each
case runs in a fresh process; the exact kinds come first, before the approximated wrappers grow the context's buffers.

    python3 tools/bench_truncated_exact.py [--reps 3] [--cases dense,sparse]
    python3 tools/bench_truncated_exact.py --case sparse --reps 1 --only ucell_exact    (one call kind in this process: what
                                              rocprofv3 --kernel-trace --stats wraps; kinds: ucell, ucell_exact, aucell, aucell_exact)
"""
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
    "dense": dict(genes=20000, cells=10000, sets=5000, sparse=False),
    "sparse": dict(genes=20000, cells=100000, sets=5000, sparse=True),
    "small": dict(genes=20000, cells=1000, sets=500, sparse=False),
    "small_sparse": dict(genes=20000, cells=4000, sets=500, sparse=True),
}
KINDS = ("ucell", "ucell_exact", "aucell", "aucell_exact")


def _used_mib():
    import torch
    free, total = torch.cuda.mem_get_info(0)
    return (total - free) / 2 ** 20


def _peak_mib_during(fn, base):
    """the largest device memory in use, above `base`, seen while fn() runs"""
    import threading
    peak, stop = [_used_mib()], threading.Event()

    def sample():
        while not stop.is_set():
            peak[0] = max(peak[0], _used_mib())
            time.sleep(0.003)

    th = threading.Thread(target=sample)
    th.start()
    try:
        fn()
    finally:
        stop.set()
        th.join()
    return max(peak[0], _used_mib()) - base


def run_case(name, reps, only=None):
    import scipy.sparse as sp

    import plaid_amd
    from plaid_amd import synth
    p = CASES[name]
    g, n = p["genes"], p["cells"]
    Gp, Gi = synth.geneset_csc(g, p["sets"])
    kf = np.diff(Gp).astype(np.float64)
    A = int(np.ceil(0.05 * g))
    if p["sparse"]:
        Xp, Xi, Xx = synth.sparse_columns(g, 0, n)
        X = sp.csc_matrix((Xx, Xi, Xp), shape=(g, n))
    else:
        X = synth.dense_columns(g, 0, n)
    base = _used_mib()
    ctx = plaid_amd.Context(0)
    calls = {
        "ucell": lambda: ctx.ucell(X, Gp, Gi, kf, 1500.0),
        "ucell_exact": lambda: ctx.ucell_exact(X, Gp, Gi, max_rank=1500),
        "aucell": lambda: ctx.aucell(X, Gp, Gi, float(A)),
        "aucell_exact": lambda: ctx.aucell_exact(X, Gp, Gi, A),
    }
    out = {"case": name, **p, "reps": reps, "maxRank": 1500, "aucMaxRank": A}
    try:
        order = [k for k in ("ucell_exact", "aucell_exact", "ucell", "aucell") if only is None or k == only]
        for kind in order:
            # warm-up (code objects, context buffers, the result's pages), sampled for its peak
            out[kind + "_peak_device_mib"] = round(_peak_mib_during(calls[kind], base), 1)
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                calls[kind]()
                ts.append((time.perf_counter() - t0) * 1e3)
            out[kind + "_ms"] = round(float(np.median(ts)), 2)
            out[kind + "_all_ms"] = [round(t, 2) for t in ts]
            out[kind + "_device_mib_after"] = round(_used_mib() - base, 1)
    finally:
        ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="dense,sparse")
    ap.add_argument("--case", default=None, help="run one case in this process and print its JSON")
    ap.add_argument("--only", default=None, choices=KINDS, help="time one kind of call alone")
    a = ap.parse_args()
    if a.case is not None:
        print(json.dumps(run_case(a.case, a.reps, a.only)))
        return
    out = []
    for name in a.cases.split(","):
        flags = ["--only", a.only] if a.only else []
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps)] + flags,
                           capture_output=True, text=True)
        if r.returncode != 0:
            out.append({"case": name, "error": (r.stderr or r.stdout)[-500:], "returncode": r.returncode})
            break                          # a failed case ends the run: nothing more is started on the device
        out.append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps({"tool": "bench_truncated_exact", "cases": out}))


if __name__ == "__main__":
    main()
