"""replaid.gsva ("z", "ecdf") and plaid.test on a sparse single-cell matrix through the two host routes: the CSC slots to
the device (plaidhip_gsva_csc / plaidhip_plaid_test_csc, a row view built there) against densifying on the host first
(toarray + plaidhip_gsva / plaidhip_plaid_test).  Every route runs in a fresh child process of its own: wall seconds of
the call (the densify route includes its toarray), the child's ru_maxrss (also as it stood before the call), and the
largest difference between the outputs of the two routes (ecdf: bit equality).  Prints one JSON line.
    python3 tools/bench_sparse_inputs.py [--genes 20000 --cells 100000 --density 0.05 --sets 5000 --tmpdir DIR]
    python3 tools/bench_sparse_inputs.py --profile ...   (the three sparse calls in this process: for a kernel-trace run)"""
import argparse
import json
import os
import resource
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = ("gsva_z", "gsva_ecdf", "plaid_test")
ROUTES = ("sparse", "densify")


def _make_input(a, d):
    from plaid_amd import synth
    Xp, Xi, Xx = synth.sparse_columns(a.genes, 0, a.cells, density=a.density)
    Gp, Gi = synth.geneset_csc(a.genes, a.sets)
    y = (np.random.default_rng(7).random(a.cells) < 0.5).astype(np.int32)
    for nm, v in (("Xp", Xp), ("Xi", Xi), ("Xx", Xx), ("Gp", Gp), ("Gi", Gi), ("y", y)):
        np.save(os.path.join(d, nm + ".npy"), v)
    return int(Xp[-1])


def _load(d):
    return {nm: np.load(os.path.join(d, nm + ".npy")) for nm in ("Xp", "Xi", "Xx", "Gp", "Gi", "y")}


def _run(ctx, call, route, v, g):
    """one call through one route; returns its output (the densify route builds the dense X inside)"""
    Xp, Xi, Xx, Gp, Gi, y = v["Xp"], v["Xi"], v["Xx"], v["Gp"], v["Gi"], v["y"]
    if route == "sparse":
        if call == "plaid_test":
            return ctx.plaid_test_csc(Xp, Xi, Xx, g, y, Gp, Gi, None, 7, 0)
        return ctx.gsva_csc(Xp, Xi, Xx, g, Gp, Gi, 0.0, call[5:])
    import scipy.sparse as sp
    X = sp.csc_matrix((Xx, Xi, Xp), shape=(g, len(Xp) - 1)).toarray(order="F")
    if call == "plaid_test":
        return ctx.plaid_test(X, y, Gp, Gi, None, 7, 0)
    return ctx.gsva(X, Gp, Gi, 0.0, call[5:])


def _warm_up(ctx, call, route):
    """the same call on a tiny input first: code-object loading and first-touch costs stay out of the timing"""
    from plaid_amd import synth
    g = 300
    Xp, Xi, Xx = synth.sparse_columns(g, 0, 40)
    Gp, Gi = synth.geneset_csc(g, 20, kmax=50)
    y = (np.arange(40) % 2).astype(np.int32)
    _run(ctx, call, route, dict(Xp=Xp, Xi=Xi, Xx=Xx, Gp=Gp, Gi=Gi, y=y), g)


def child(a):
    import plaid_amd
    v = _load(a.tmpdir)
    ctx = plaid_amd.Context(0)
    _warm_up(ctx, a.call, a.route)
    rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024   # input + runtime, before the timed call
    t0 = time.perf_counter()
    out = _run(ctx, a.call, a.route, v, a.genes)
    wall = time.perf_counter() - t0
    ctx.close()
    np.save(os.path.join(a.tmpdir, f"out_{a.call}_{a.route}.npy"), out)
    rss = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024
    print(json.dumps({"wall_s": round(wall, 4), "maxrss_bytes": int(rss), "maxrss_before_call_bytes": int(rss0)}))


def profile(a):
    import plaid_amd
    d = tempfile.mkdtemp(dir=a.tmpdir)
    try:
        _make_input(a, d)
        v = _load(d)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    ctx = plaid_amd.Context(0)
    for call in CALLS:
        _warm_up(ctx, call, "sparse")
        t0 = time.perf_counter()
        _run(ctx, call, "sparse", v, a.genes)
        print(f"{call}: {time.perf_counter() - t0:.3f} s", flush=True)
    ctx.close()


def _compare(d, call):
    """largest difference between the two routes' outputs, in column blocks (no second copy of a 4 GB output)"""
    a_out = np.load(os.path.join(d, f"out_{call}_sparse.npy"), mmap_mode="r")
    b_out = np.load(os.path.join(d, f"out_{call}_densify.npy"), mmap_mode="r")
    mx, eq = 0.0, a_out.shape == b_out.shape
    tol = eq   # the parity bar of the test suite: |a - b| <= 1e-9 + 1e-5 |b|
    for c0 in range(0, a_out.shape[1] if eq else 0, 4096):
        x, y = np.asarray(a_out[:, c0:c0 + 4096]), np.asarray(b_out[:, c0:c0 + 4096])
        both_nan = np.isnan(x) & np.isnan(y)
        if x.size:
            mx = max(mx, float(np.max(np.where(both_nan, 0.0, np.abs(x - y)))))
        eq = eq and bool(np.array_equal(x, y, equal_nan=True))
        tol = tol and bool(np.all(both_nan | (np.abs(x - y) <= 1e-9 + 1e-5 * np.abs(y))))
    print(json.dumps({"max_abs_diff": mx, "bit_equal": eq, "within_rtol_1e-5": tol}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=20000)
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--sets", type=int, default=5000)
    ap.add_argument("--tmpdir", default=None, help="where the input and the outputs are staged (default: the system's)")
    ap.add_argument("--child-timeout", type=float, default=1200.0)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--stage", choices=("make", "run", "compare"), help=argparse.SUPPRESS)
    ap.add_argument("--call", choices=CALLS, help=argparse.SUPPRESS)
    ap.add_argument("--route", choices=ROUTES, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.stage == "make":
        return print(json.dumps({"nnz": _make_input(a, a.tmpdir)}))
    if a.stage == "run":
        return child(a)
    if a.stage == "compare":
        return _compare(a.tmpdir, a.call)
    if a.profile:
        return profile(a)
    # The parent only starts children and touches no large array: Linux hands a child the parent's peak RSS at fork,
    # which would otherwise show up in every child's ru_maxrss.
    d = tempfile.mkdtemp(dir=a.tmpdir)
    res = {"shape": {"genes": a.genes, "cells": a.cells, "density": a.density, "sets": a.sets}}

    def stage(*args):
        cmd = [sys.executable, os.path.abspath(__file__), "--tmpdir", d, "--genes", str(a.genes), "--cells", str(a.cells),
               "--density", str(a.density), "--sets", str(a.sets), "--stage", *args]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
        if p.returncode != 0:   # stop at the first failing child: nothing more is started on the GPU
            sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
            res["error"] = f"{' '.join(args)}: exit status {p.returncode}"
            return None
        return json.loads(p.stdout.strip().splitlines()[-1])

    try:
        t0 = time.perf_counter()
        made = stage("make")
        if made is None:
            print(json.dumps(res))
            return 1
        res["shape"]["nnz"] = made["nnz"]
        print(f"[bench_sparse_inputs] input ready in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        for call in CALLS:
            r = {}
            for route in ROUTES:
                r[route] = stage("run", "--call", call, "--route", route)
                if r[route] is None:
                    print(json.dumps(res))
                    return 1
                print(f"[bench_sparse_inputs] {call} {route}: {r[route]}", file=sys.stderr, flush=True)
            cmp_ = stage("compare", "--call", call)
            if cmp_ is None:
                print(json.dumps(res))
                return 1
            r.update(cmp_)
            r["speedup"] = round(r["densify"]["wall_s"] / r["sparse"]["wall_s"], 3)
            for route in ROUTES:
                os.remove(os.path.join(d, f"out_{call}_{route}.npy"))
            res[call] = r
    finally:
        shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
