"""What the fused per-component operators buy: nmf() with the operator on S, Y in HBM, factors on the host, e_rel = 0 (nothing
stops), the clock around whole nmf() calls, one warm-up call, then REPS calls: median and spread.

  thresh       prox_S = partial(prox_soft, thresh=<K values, shape (K, 1)>): fused, one table               (a tree with op 12)
  mixed        prox_S = partial(prox_components, prox=[soft, plus, soft_plus, hard, ...], axis=0): fused
  soft         the same call with the scalar prox_soft: the ceiling
  host_thresh  the first two as user Python callables (NumPy on the host copy of S, once per application): the only way to
  host_mixed   them before; runs on any tree, the parent commit's included

    python scratch/components_rate.py --legs thresh,mixed,soft [--reps 5]
    python scratch/components_rate.py --legs host_thresh,host_mixed --shapes pgm [--iters 200] [--reps 5]     ->  one JSON line per leg
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


def thresholds(K):
    return np.linspace(0.05, 0.15, K).reshape(K, 1)


def host_soft(X, step, thresh, relative=True):
    t = thresh * step if relative else thresh
    X[...] = np.sign(X) * np.maximum(np.abs(X) - t, 0)
    return X


def host_hard(X, step, thresh, relative=True):
    t = thresh * step if relative else thresh
    X[np.abs(X) < t] = 0
    return X


def host_plus(X, step):
    X[X < 0] = 0
    return X


def host_mixed(X, step, relative=True):
    """row k of S gets member k % 4 of (soft 0.1, plus, soft_plus 0.05, hard 0.1); a per-component step reaches row k as its own"""
    st = np.asarray(step, dtype=X.dtype)
    for k in range(X.shape[0]):
        sk = st.reshape(-1)[k] if st.size > 1 else st
        m = k % 4
        if m == 0:
            host_soft(X[k], sk, 0.1, relative)
        elif m == 1:
            host_plus(X[k], sk)
        elif m == 2:
            host_plus(host_soft(X[k], sk, 0.05, relative), sk)
        else:
            host_hard(X[k], sk, 0.1, relative)
    return X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="thresh,mixed,soft")
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
        kind = "relative" if case == "pgm" else "absolute"
        if case == "adaprox":
            kw.update(algorithm=pm.adaprox, scheme="adam")
            if a.prox_max_iter is not None:
                kw["prox_max_iter"] = a.prox_max_iter
        for leg in a.legs.split(","):
            if leg == "thresh":
                prox = partial(ops.prox_soft, thresh=thresholds(K), type=kind)
            elif leg == "mixed":
                four = [partial(ops.prox_soft, thresh=0.1, type=kind), ops.prox_plus, partial(ops.prox_soft_plus, thresh=0.05, type=kind),
                        partial(ops.prox_hard, thresh=0.1, type=kind)]
                prox = partial(ops.prox_components, prox=[four[k % 4] for k in range(K)], axis=0)
            elif leg == "soft":
                prox = partial(ops.prox_soft, thresh=0.1, type=kind)
            elif leg == "host_thresh":
                prox = partial(host_soft, thresh=thresholds(K).astype(np.float32), relative=(kind == "relative"))
            else:
                prox = partial(host_mixed, relative=(kind == "relative"))
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
