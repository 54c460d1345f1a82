#!/usr/bin/env python3
"""Digests of the exact scorers' results, for a bit-for-bit comparison between two builds of the library.

The GPU tests of these scorers hold general weights (alpha, tau outside {0, 1}, arbitrary gsea weights) to error bounds
only: an addition reordered inside the bitmap walk (csrc/bitmap_walk.h) would pass them.  This tool runs a fixed table of
seeded cases through the Context entries and prints one SHA-256 per case over the bytes of the result.
tests/golden/walk_bits.json holds the digests of a known build; tests/test_gpu_walk_bits.py compares the build under test
with them.

    python tools/walk_bits.py                     # one "<case> <sha256>" line per case
    python tools/walk_bits.py --json out.json --commit cbd959b    # the golden file's form: {"commit", "hipcc", "digests"}
    PLAIDHIP_LIB=/path/to/libplaidhip.so python tools/walk_bits.py    # another build

The sizes are the seams of the walk.  A map chunk is 64 words of 64 bits, so g = 65, 4097 and 8193 rows give a second word,
a second chunk and a third; n = 17 columns cross the 16-column tile and give a wavefront more than one pair.  Every matrix
has tied values, one column in row order (column 0: a set's rows are its walk positions there) and one column with a NaN.
The collection has sets of 1, 2, 63, 64, 65 and g - 1 rows, a set of neighbouring rows (one map word in column 0), a set
spread over every chunk, and three of random sizes.  All NaNs in the results are the ones the library writes.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = (65, 4097, 8193)
N_COLS = 17
N_LISTS = 9        # plaid.gsea: the list tile of 8 and one more
N_PERM = 65        # ... the permutation block of 64 and one more


def make_sets(g, seed):
    rng = np.random.default_rng(seed)
    sets = [np.sort(rng.choice(g, size=k, replace=False)) for k in (1, 2, 63, 64, 65, g - 1) if k <= g]
    sets.append(np.arange(3, 3 + min(40, g - 3)))                        # neighbours: one word of column 0's map
    sets.append(np.arange(0, g, max(1, g // 29)))                        # spread over every chunk
    sets += [np.sort(rng.choice(g, size=int(k), replace=False)) for k in rng.integers(3, max(4, g // 2), size=3)]
    Gp = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    return Gp, np.concatenate(sets).astype(np.int32)


def make_inputs(g):
    rng = np.random.default_rng(1000 + g)
    X = np.round(rng.normal(size=(g, N_COLS)), 1)                        # tied values
    X[:, 0] = np.arange(g, 0, -1)
    X[g // 3, 5] = np.nan
    X = np.asfortranarray(X)
    V = np.round(rng.gamma(2.0, 1.0, size=(g, N_COLS)), 1) * (rng.random((g, N_COLS)) < 0.05)   # about 5 % stored
    V[rng.random((g, N_COLS)) < 0.01] = -1.5
    V[g // 2, 7] = np.nan
    Xs = sp.csc_matrix(V)
    Xs.sort_indices()
    stat = np.round(rng.normal(size=(g, N_LISTS)), 1)
    stat[:, 0] = np.arange(g, 0, -1)
    stat[g // 4, 4] = np.nan
    weight = np.sqrt(rng.random((g, N_LISTS)) + 0.01)                    # irrational, positive
    Gp, Gi = make_sets(g, 2000 + g)
    Dp, Di = make_sets(g, 3000 + g)
    return dict(X=X, Xs=Xs, stat=np.asfortranarray(stat), weight=np.asfortranarray(weight), Gp=Gp, Gi=Gi, Dp=Dp, Di=Di)


def cases(ctx):
    """[(name, thunk)]: the whole table, in a fixed order"""
    from plaid_amd import engine
    out = []
    for g in SIZES:
        d = make_inputs(g)
        X, Xs, Gp, Gi, Dp, Di = d["X"], d["Xs"], d["Gp"], d["Gi"], d["Dp"], d["Di"]

        def add(name, fn, g=g):
            out.append((f"{name} g={g}", fn))

        add("ssgsea.exact single=FALSE alpha=0.5", lambda X=X, Gp=Gp, Gi=Gi: ctx.ssgsea_exact(X, Gp, Gi, 0.5, True, False, False))
        add("ssgsea.exact single=FALSE alpha=0.5 norm", lambda X=X, Gp=Gp, Gi=Gi: ctx.ssgsea_exact(X, Gp, Gi, 0.5, False, True, False))
        for md in (0, 1):
            add(f"gsva.exact none tau=0.5 max_diff={md}",
                lambda X=X, Gp=Gp, Gi=Gi, md=md: ctx.gsva_exact(X, Gp, Gi, 0.5, "none", bool(md)))
        for st in ("std", "pos", "neg"):
            add(f"plaid.gsea {st} edges",
                lambda d=d, st=st: engine._gsea(ctx.lib.plaidhip_gsea_scored, (ctx.handle,), d["stat"], d["weight"], d["Gp"], d["Gi"],
                                                None, N_PERM, 11, True, st, True))
        add("sing.exact down dispersion", lambda X=X, Gp=Gp, Gi=Gi, Dp=Dp, Di=Di: ctx.sing_exact(X, Gp, Gi, Dp, Di, True, True))
        add("ssgsea.exact single=TRUE alpha=0.5 dense", lambda X=X, Gp=Gp, Gi=Gi: ctx.ssgsea_exact(X, Gp, Gi, 0.5, True, False, True))
        add("ssgsea.exact single=TRUE alpha=0.5 norm", lambda X=X, Gp=Gp, Gi=Gi: ctx.ssgsea_exact(X, Gp, Gi, 0.5, True, True, True))
        add("ssgsea.exact single=TRUE alpha=0.5 dgCMatrix", lambda Xs=Xs, Gp=Gp, Gi=Gi: ctx.ssgsea_exact(Xs, Gp, Gi, 0.5, True, False, True))
        add("aucell.exact dgCMatrix", lambda Xs=Xs, Gp=Gp, Gi=Gi, g=g: ctx.aucell_exact(Xs, Gp, Gi, max(2, g // 3)))
        for ties in ("first", "last", "dense"):
            for signed in (False, True):
                add(f"colranks {ties} signed={int(signed)} dense", lambda X=X, t=ties, s=signed: ctx.colranks_dense(X, t, s))
                if ties != "dense":   # (the ranks of a dgCMatrix's stored values take "first" and "last")
                    add(f"colranks {ties} signed={int(signed)} dgCMatrix",
                        lambda Xs=Xs, t=ties, s=signed: ctx.colranks_csc(Xs.indptr, Xs.data, t, s))
    return out


def digest(res):
    """SHA-256 over dtype, shape and bytes of every array of a result (an array, a tuple of arrays or a dict of them)"""
    if isinstance(res, dict):
        res = [res[k] for k in sorted(res)]
    elif isinstance(res, np.ndarray):
        res = [res]
    h = hashlib.sha256()
    for a in res:
        a = np.asarray(a)
        h.update(f"{a.dtype.str}{a.shape}".encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_all(ctx):
    return {name: digest(fn()) for name, fn in cases(ctx)}


def hipcc_version():
    """the version lines of `hipcc --version` (for information: what compiled the recorded build)"""
    try:
        out = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True, text=True, timeout=60).stdout
        return "\n".join(ln for ln in out.splitlines() if "version" in ln or ln.startswith("Target"))
    except (OSError, subprocess.SubprocessError):
        return "unknown"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--json", help="write {commit, hipcc, digests} here (the form of tests/golden/walk_bits.json)")
    ap.add_argument("--commit", default="", help="the commit the library was built from, for the record in --json")
    args = ap.parse_args()
    import plaid_amd
    ctx = plaid_amd.Context(0)
    try:
        digests = run_all(ctx)
    finally:
        ctx.close()
    for name, dg in digests.items():
        print(f"{name} {dg}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"commit": args.commit, "hipcc": hipcc_version(), "digests": digests}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
