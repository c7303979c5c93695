#!/bin/bash
# k_grad_f16_v8<.., Y16> (Y sixteen bytes per lane) against the parent commit's build on one GPU: alternating bench lines, every run under its own time
# limit, nothing more started after a run that fails.  PARENT_LIB: libpmx.so built from the parent commit (PMX_LIB loads it instead of the tree's);
# the tree's build also runs with PMX_K1_Y16=0 (its 8-byte instances) as a second A/B.     usage: PARENT_LIB=/path/libpmx.so scratch/y16_ab.sh [REPS] > profiles/y16_ab.txt
REPS=${1:-3}
: ${PARENT_LIB:?PARENT_LIB=libpmx.so of the parent commit}
line() {  # tag, environment assignment, bench flags
  out=$(env $2 timeout -k 10 240 python bench.py $3 2>/dev/null) || { echo "$1: bench.py $3 failed (exit $?)"; exit 1; }
  echo "$out" | grep '^{' | tail -1 | python -c "
import sys, json
d = json.loads(sys.stdin.read())
print('%-14s %-28s %8.1f it/s   K1 %.4f ms   tail %.4f ms' % ('$1', '$3', d['value'], d['roofline']['avg_launch_ms'], d['tail_ms']))"
}
for FLAGS in "--steps 100 --warmup 20" "--steps 20 --warmup 5" "--config cfg5"; do
  for rep in $(seq $REPS); do
    line parent "PMX_LIB=$PARENT_LIB" "$FLAGS"
    line y16 "PMX_K1_Y16=1" "$FLAGS"
    line y16-off "PMX_K1_Y16=0" "$FLAGS"
  done
done
