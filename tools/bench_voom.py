"""Cost of plaid.voom followed by plaid.limma with its weights: one JSON line.

    python tools/bench_voom.py [--rows 20000] [--samples 1000] [--coef 4] [--steps 5] [--warmup 1]

calls_ms: through the C ABI from host memory (counts in, E and weights out; then E and weights in, tables out), the median
of `steps` calls after `warmup`, min and max beside it; the unweighted fit beside them.  passes_ms: the device passes that
have a device-pointer entry, on resident matrices, timed on the host around the enqueue and a wait for the context's stream
(each entry is its kernel plus the reduction of its block partials): the weighted sums and RSS of the fit, voom's weights pass, and the unweighted effects and RSS that voom
runs on E.  voom's check and log-CPM kernels have no entry of their own and are inside calls_ms only.  bytes_read: what each
pass reads of its matrices (A: counts or E; W: the weights), from the launch geometry."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import plaid_amd  # noqa: E402
from plaid_amd import engine  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def device_timed(ctx, fn, steps, warmup):
    """an entry on device pointers: enqueue on the context's stream, then wait for it (host clock around both; the launch and
    the wait cost some tens of microseconds beside the kernels)"""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--coef", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    import torch
    rng = np.random.default_rng(28)
    rows, n, p = a.rows, a.samples, a.coef
    mu = np.exp(rng.uniform(np.log(0.5), np.log(5000.0), size=(rows, 1)))
    counts = np.asfortranarray(rng.poisson(mu * rng.gamma(5.0, 0.2, size=(rows, n))).astype(np.float64))
    D = np.column_stack([np.ones(n), np.arange(n) % 2] + [rng.normal(size=n) for _ in range(p - 2)])[:, :p]
    ctx = plaid_amd.Context(0)
    try:
        v = ctx.voom(counts, D)
        E, W = v["E"], v["weights"]
        calls = {"voom": timed(lambda: ctx.voom(counts, D), a.steps, a.warmup),
                 "limma_weights": timed(lambda: ctx.limma(E, D, na="fit", weights=W), a.steps, a.warmup),
                 "limma_no_weights": timed(lambda: ctx.limma(E, D), a.steps, a.warmup)}
        dev = torch.device("cuda", 0)
        des = engine.limma_design(D)
        wc, ld = p * (p + 1) // 2 + p + 1, rows + (rows & 1)
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
        Ed = torch.zeros((n, ld), dtype=torch.float64, device=dev)
        Wd = torch.ones((n, ld), dtype=torch.float64, device=dev)
        Ed[:, :rows], Wd[:, :rows] = t(E.T), t(W.T)
        Qd, inv, off = t(des["Q"].T), t([1.0 / n]), t(v["offset"])
        S = torch.zeros(wc * rows, dtype=torch.float64, device=dev)
        G = torch.zeros((p + 1) * rows, dtype=torch.float64, device=dev)
        R = torch.zeros(rows, dtype=torch.float64, device=dev)
        kx, ky = t(v["knots_x"]), t(v["knots_y"])
        Wo = torch.zeros((n, ld), dtype=torch.float64, device=dev)
        P = lambda x: x.data_ptr()
        passes = {
            "w_sums": device_timed(ctx, lambda: ctx.dev_limma_w_sums(P(Ed), P(Wd), None, ld, rows, n, P(Qd), None, P(inv), p, 1, None, P(S)),
                                   a.steps, a.warmup),
            "w_rss": device_timed(ctx, lambda: ctx.dev_limma_w_rss(P(Ed), P(Wd), None, ld, rows, n, P(Qd), None, p, 1, P(G), None, P(R)),
                                  a.steps, a.warmup),
            "effects": device_timed(ctx, lambda: ctx.dev_row_design_effects(P(Ed), ld, rows, n, P(Qd), None, P(inv), p, 1, None, P(G)),
                                    a.steps, a.warmup),
            "rss": device_timed(ctx, lambda: ctx.dev_row_design_rss(P(Ed), ld, rows, n, P(Qd), None, p, 1, P(G), None, P(R)),
                                a.steps, a.warmup),
            "voom_weights": device_timed(ctx, lambda: ctx.dev_voom_weights(P(Qd), P(off), n, p, P(G), rows, P(kx), P(ky), len(v["knots_x"]),
                                                                      P(Wo), ld), a.steps, a.warmup),
        }
    finally:
        ctx.close()
    tile = engine.limma_tile()
    mat = rows * n * 8
    tiles_w, tiles_u = -(-wc // tile), -(-(p + 1) // tile)
    res = {"rows": rows, "samples": n, "coef": p, "knots": int(len(v["knots_x"])), "steps": a.steps, "calls_ms": calls,
           "passes_ms": passes,
           "bytes_read": {"w_sums": {"A": tiles_w * mat, "W": tiles_w * mat}, "w_counts": {"A": mat, "W": mat},
                          "w_rss": {"A": mat, "W": mat}, "effects": {"A": tiles_u * mat, "W": 0}, "rss": {"A": mat, "W": 0},
                          "voom_check_rowsum_logcpm": {"A": 3 * mat, "W": 0}, "voom_weights": {"A": 0, "W": 0}}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
