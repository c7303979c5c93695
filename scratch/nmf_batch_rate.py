"""nmf_batch against a Python loop of nmf() over the same problems -> profiles/nmf_batch_rate.txt

    python scratch/nmf_batch_rate.py --what batch                       # this tree
    python scratch/nmf_batch_rate.py --what loop --root <other checkout>  # e.g. the parent commit, built

Whole calls (packing, transfers, allocation, launch, scatter), median of 5 after one warm-up call; for the batch also the launches alone (HIP
events inside the entry point).  Every problem runs max_iter = 200 with e_rel = 0 (no stop).  Three workloads: B problems of 100 x 50 x 3
(the reference's example size), of 200 x 1000 x 5, and a ragged mix (M 20..200, N 50..1000, K 2..8).  A loop is linear in B by
construction: it is timed over at most --loop-cap problems and scaled, which the output says.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--what", choices=["batch", "loop"], required=True)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--loop-cap", type=int, default=48)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--max-iter", type=int, default=200)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import proxmin_amd as pm  # noqa: E402
from oracle import nmf_oracle as orc  # noqa: E402


def problems(kind, B):
    if kind == "ragged":
        rng = np.random.default_rng(99)
        shapes = [(int(rng.integers(20, 201)), int(rng.integers(50, 1001)), int(rng.integers(2, 9))) for _ in range(B)]
    else:
        shapes = [kind] * B
    ps = [orc.synthetic_problem(*s, dtype=np.float32, seed=i) for i, s in enumerate(shapes)]
    return [p[0] for p in ps], [p[1] for p in ps], [p[2] for p in ps]


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return ts, out


WORKLOADS = [((100, 50, 3), [1, 64, 256, 1024, 4096]), ((200, 1000, 5), [1, 64, 256, 1024]), ("ragged", [512])]
for kind, Bs in WORKLOADS:
    for B in Bs:
        Ys, A0, S0 = problems(kind, B)
        if args.what == "batch":
            launch = []

            def run():
                As, Ss = [a.copy() for a in A0], [s.copy() for s in S0]
                res = pm.nmf_batch(Ys, As, Ss, max_iter=args.max_iter, e_rel=0)
                launch.append(res.launch_ms)
                return int(res.iterations.sum())
            ts, its = timed(run, args.reps)
            row = dict(what="batch", workload=str(kind), B=B, call_s_median=statistics.median(ts), call_s_min=min(ts), call_s_max=max(ts),
                       launch_ms_median=statistics.median(launch[1:]), problem_iterations=its, problem_iterations_per_s=its / statistics.median(ts))
        else:
            n = min(B, args.loop_cap)

            def run():
                for b in range(n):
                    pm.nmf.nmf(Ys[b], A0[b].copy(), S0[b].copy(), max_iter=args.max_iter, e_rel=0)
                return n * args.max_iter
            ts, its = timed(run, min(args.reps, 3))
            med = statistics.median(ts) * B / n
            row = dict(what="loop", workload=str(kind), B=B, timed_over=n, call_s_median=med, call_s_min=min(ts) * B / n, call_s_max=max(ts) * B / n,
                       problem_iterations=B * args.max_iter, problem_iterations_per_s=B * args.max_iter / med)
        print(json.dumps(row), flush=True)
