#!/usr/bin/python3
"""The plaid() step phase by phase as bench.py's C2 block enqueues it (crossprod / medians + sum / shift, HIP events), random X
made on the device, 20,000 genes: one library per process (PLAIDHIP_LIB), one JSON line -- medians and minima of the
phases over `iters` steps after 10 warm-up steps, a checksum of the scores and the sum of the medians (equal between
builds that compute the same).  `profiles/norm_walks_step_ab.jsonl` is made of such lines.
    PLAIDHIP_LIB=plaid_amd/csrc/libplaidhip_<name>.so python3 tools/bench_step.py LABEL [iters = 40] [samples = 10000 sets = 5000]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    label = sys.argv[1]
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
    m = int(sys.argv[4]) if len(sys.argv) > 4 else 5000
    g = 20000
    import numpy as np
    import torch
    import plaid_amd
    from plaid_amd import synth
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    ctx = plaid_amd.Context(0, stream.cuda_stream)
    Gp, Gi = synth.geneset_csc(g, m)
    gs = ctx.geneset(g, Gp, Gi)
    torch.manual_seed(1)
    X = torch.randn((n, g), dtype=torch.float64, device=dev) * 2 + 8
    S = torch.empty((n, m), dtype=torch.float64, device=dev)
    flags = torch.zeros(4, dtype=torch.int32, device=dev)
    med = torch.empty(n, dtype=torch.float64, device=dev)
    red = torch.zeros(2, dtype=torch.float64, device=dev)
    rows = []
    for k in range(iters + 10):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        with torch.cuda.stream(stream):
            flags.zero_()
            e[0].record(stream)
            ctx.dev_spmm_dense(gs, X.data_ptr(), g, n, S.data_ptr(), m, "mean", 1.0, 0.0, flags.data_ptr())
            e[1].record(stream)
            ctx.dev_col_medians(S.data_ptr(), m, m, n, None, med.data_ptr(), flags.data_ptr())
            ctx.dev_sum(med.data_ptr(), n, red.data_ptr())
            e[2].record(stream)
            ctx.dev_shift_columns(S.data_ptr(), m, m, n, med.data_ptr(), 0.0, red.data_ptr())
            e[3].record(stream)
        if k % 10 == 9:
            torch.cuda.synchronize()
        rows.append(e)
    torch.cuda.synchronize()
    r = np.array([[e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]), e[2].elapsed_time(e[3]), e[0].elapsed_time(e[3])]
                  for e in rows[10:]])
    chk = float(S[::97, ::89].double().sum().item())
    out = {"label": label, "n": n, "m": m, "iters": iters,
           "median": dict(zip(("spmm", "med+sum", "shift", "total"), np.round(np.median(r, axis=0), 4).tolist())),
           "min": dict(zip(("spmm", "med+sum", "shift", "total"), np.round(r.min(axis=0), 4).tolist())),
           "checksum": chk, "med_sum": float(med.sum().item())}
    print(json.dumps(out), flush=True)
    gs.close()
    ctx.close()


if __name__ == "__main__":
    main()
