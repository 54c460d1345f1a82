#!/bin/bash
# A/B of library builds on the headline step, as the walk-order work of DESIGN.md 4.3 was measured, on ONE device in ONE visit:
#     bash tools/ab_norm.sh <outdir> <runs> <build> <build> [<build> ...]
# build "product" = plaid_amd/csrc/libplaidhip.so, any other name = libplaidhip_<name>.so (make -C plaid_amd/csrc variant
# NAME=<name> DEFS=..., or the parent commit's library copied there as libplaidhip_parent.so).  The builds run alternately
# (A B A B ...), every `bench.py --gpus 1 --steps 20 --warmup 5` in a fresh process under its own time limit; the first run
# that fails, aborts or times out ends the script.  <outdir>/ab.jsonl: one line per run (build, run, ms_per_step, phases_ms);
# then, per build, the median, min and max of ms_per_step and of every phase.
out=$1; runs=$2; shift 2
mkdir -p $out
: > $out/ab.jsonl
for i in $(seq 1 $runs); do
  for v in "$@"; do
    if [ "$v" = product ]; then lib=$PWD/plaid_amd/csrc/libplaidhip.so; else lib=$PWD/plaid_amd/csrc/libplaidhip_$v.so; fi
    PLAIDHIP_LIB=$lib timeout -k 10 300 python3 bench.py --gpus 1 --steps 20 --warmup 5 > $out/bench_${v}_$i.json 2> $out/bench_${v}_$i.err
    rc=$?
    if [ $rc -ne 0 ]; then echo "bench.py failed for build $v, run $i (exit $rc)"; tail -5 $out/bench_${v}_$i.err; exit 1; fi
    python3 - $out/bench_${v}_$i.json $v $i >> $out/ab.jsonl <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(json.dumps({"build": sys.argv[2], "run": int(sys.argv[3]), "ms_per_step": d["ms_per_step"], "phases_ms": d["phases_ms"]}))
PY
  done
done
python3 - $out/ab.jsonl <<'PY' | tee $out/ab_summary.txt
import json, statistics, sys
rows = [json.loads(l) for l in open(sys.argv[1])]
for b in dict.fromkeys(r["build"] for r in rows):
    mine = [r for r in rows if r["build"] == b]
    cols = {"ms_per_step": [r["ms_per_step"] for r in mine]}
    for k in mine[0]["phases_ms"]:
        cols[k] = [r["phases_ms"][k] for r in mine]
    print(b, " ".join(f"{k}: median {statistics.median(v):.4f} min {min(v):.4f} max {max(v):.4f};" for k, v in cols.items()))
PY
