#!/bin/bash
# The headline with and without the per-component operators (op 12) in the tree: bench lines of the parent commit's checkout (PARENT_TREE: built
# there, its own Python package and libpmx.so) against this tree on one GPU, alternating, every run under its own time limit, nothing more started
# after a run that fails.     usage: PARENT_TREE=/path/to/checkout scratch/components_ab.sh [REPS] > raw lines
REPS=${1:-4}
: ${PARENT_TREE:?PARENT_TREE=a built checkout of the parent commit}
ROOT=$(pwd)
line() {  # tag, directory, bench flags
  out=$(cd $2 && timeout -k 10 240 python bench.py $3 2>/dev/null) || { echo "$1: bench.py $3 failed (exit $?)"; exit 1; }
  echo "$out" | grep '^{' | tail -1 | python -c "
import sys, json
d = json.loads(sys.stdin.read())
print('%-14s %-28s %8.1f it/s   K1 %.4f ms   tail %.4f ms' % ('$1', '$3', d['value'], d['roofline']['avg_launch_ms'], d['tail_ms']))"
}
for FLAGS in "--steps 100 --warmup 20" "--steps 20 --warmup 5"; do
  for rep in $(seq $REPS); do
    line parent $PARENT_TREE "$FLAGS"
    line branch $ROOT "$FLAGS"
  done
done
