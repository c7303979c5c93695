"""nmf() iterations per second of pgm with prox_A = prox_unity_plus(axis=0): A's columns sum to one, a sum over the factor's
long axis per iteration.  Fixed max_iter, e_rel = 0 (nothing stops); the clock is around whole nmf() calls (upload of Y,
iterations, download of the factors -- what a caller pays), one warm-up call, then REPS calls: median and spread.

    python scratch/long_axis_unity_rate.py [--reps 5]  ->  one JSON line per shape

Run it at two commits to compare the routes: before the fused update chain (k_pgm_unity) the operator was a host prox, one
iteration per call."""
import argparse
import json
import logging
import os
import statistics
import sys
import time
from functools import partial

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = (((4096, 4096, 32), 1000), ((16384, 16384, 64), 200))        # (M, N, K), max_iter


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import proxmin_amd as pm
    logging.getLogger("proxmin").setLevel(logging.ERROR)
    for (M, N, K), iters in SHAPES:
        rng = np.random.default_rng(5)
        At = rng.random((M, K), dtype=np.float32)
        St = rng.random((K, N), dtype=np.float32)
        Y = At @ St
        A0 = rng.random((M, K), dtype=np.float32) + 0.25
        S0 = rng.random((K, N), dtype=np.float32) + 0.25
        f = A0.sum(0, keepdims=True)
        A0, S0 = A0 / f, S0 * f.T
        rates = []
        for rep in range(a.reps + 1):
            A, S = A0.copy(), S0.copy()
            t0 = time.perf_counter()
            pm.nmf.nmf(Y, A, S, prox_A=partial(pm.operators.prox_unity_plus, axis=0), max_iter=iters, e_rel=0)
            dt = time.perf_counter() - t0            # (nmf() returns after the factors are back on the host)
            assert np.isfinite(A).all() and abs(float(A[:, 0].sum()) - 1.0) < 1e-3
            if rep:                                  # the first call is the warm-up
                rates.append(iters / dt)
        print(json.dumps({"shape": [M, N, K], "max_iter": iters, "reps": a.reps, "mode": pm.get_default_mode(),
                          "it_per_s_median": round(statistics.median(rates), 1), "it_per_s_min": round(min(rates), 1),
                          "it_per_s_max": round(max(rates), 1)}), flush=True)


if __name__ == "__main__":
    main()
