#!/bin/bash
# usage (from the repository root): scratch/r6_bench_f64leg.sh OUT_DIR -- the bench line with its fp64 leg (--full), its wall time
O=${1:?output directory}; mkdir -p "$O"
SECONDS=0; python bench.py --full --steps 20 --warmup 5 > "$O/bench_20_5.json" 2> "$O/bench_20_5.err"
echo "bench.py wall: $SECONDS s"
grep "^{" "$O/bench_20_5.json" | tail -1 | python -c '
import sys, json
d = json.loads(sys.stdin.read())
print(d["value"], d["ms_per_step"], d["roofline"]["frac"])
print(json.dumps(d.get("fp64_inputs"), indent=1)[:1500])
print({k: v for k, v in d.get("measured", {}).items() if "fp64" in k})
'
