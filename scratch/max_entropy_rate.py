"""What the fused prox_max_entropy buys: nmf() with the operator on S, Y in HBM, factors on the host, e_rel = 0 (nothing stops),
the clock around whole nmf() calls, one warm-up call, then REPS calls: median and spread.

  fused   prox_S = partial(prox_max_entropy, ...) of this library: the whole iteration on the device      (a tree with the operator)
  soft    the same call with prox_soft: the cost of the Lambert-W solve over the cheapest thresholding operator
  host    the same operator as a user Python callable (NumPy + SciPy's lambertw on the host copy of S, once per
          application): the only way to it before the operator existed; runs on any tree, the parent commit's included

    python scratch/max_entropy_rate.py --legs fused,soft [--reps 5]
    python scratch/max_entropy_rate.py --legs host --shapes pgm [--iters 200] [--reps 5]      ->  one JSON line per leg
"""
import argparse
import json
import logging
import os
import statistics
import sys
import time
from functools import partial

import numpy as np

sys.path.insert(0, os.getcwd())

CASES = {"pgm": (4096, 4096, 32), "adaprox": (16384, 16384, 64)}


def host_max_entropy(X, step, gamma=1.0, relative=True):
    """y + g ln y = x - g for the entries > 0, through SciPy's Lambert W (argument formed the way the reference forms it)"""
    from scipy.special import lambertw
    g = gamma * step if relative else gamma
    m = X > 0
    X[m] = g * lambertw(np.exp(X[m] / g - 1.0) / g).real
    return X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="fused,soft")
    ap.add_argument("--shapes", default="pgm,adaprox")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--prox-max-iter", type=int, default=None, help="adaprox: cap of the proximal loop (default: the solver's 1000)")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import proxmin_amd as pm
    logging.getLogger("proxmin").setLevel(logging.ERROR)
    ops = pm.operators
    for case in a.shapes.split(","):
        M, N, K = CASES[case]
        rng = np.random.default_rng(5)
        Y = torch.from_numpy(rng.random((M, K), dtype=np.float32) @ rng.random((K, N), dtype=np.float32)).cuda()
        A0 = rng.random((M, K), dtype=np.float32) + 0.25
        S0 = rng.random((K, N), dtype=np.float32) + 0.25
        kw = dict(max_iter=a.iters, e_rel=0)
        if case == "adaprox":
            kw.update(algorithm=pm.adaprox, scheme="adam")
            if a.prox_max_iter is not None:
                kw["prox_max_iter"] = a.prox_max_iter
        for leg in a.legs.split(","):
            if leg == "fused":
                prox = partial(ops.prox_max_entropy, gamma=0.1) if case == "pgm" else partial(ops.prox_max_entropy, gamma=0.1, type="absolute")
            elif leg == "soft":
                prox = partial(ops.prox_soft, thresh=0.1) if case == "pgm" else partial(ops.prox_soft, thresh=0.1, type="absolute")
            else:
                prox = partial(host_max_entropy, gamma=0.1, relative=(case == "pgm"))
            times = []
            for rep in range(a.reps + 1):
                A, S = A0.copy(), S0.copy()
                t0 = time.perf_counter()
                pm.nmf.nmf(Y, A, S, prox_S=prox, **kw)
                dt = time.perf_counter() - t0
                if rep or a.reps == 0:               # the first call is the warm-up
                    times.append(dt)
            med = statistics.median(times)
            print(json.dumps({"case": case, "shape": [M, N, K], "leg": leg, "max_iter": a.iters, "prox_max_iter": a.prox_max_iter, "reps": len(times),
                              "median_s": round(med, 4), "min_s": round(min(times), 4), "max_s": round(max(times), 4),
                              "it_per_s": round(a.iters / med, 1), "finite": bool(np.isfinite(A).all() and np.isfinite(S).all())}), flush=True)


if __name__ == "__main__":
    main()
