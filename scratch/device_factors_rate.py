"""nmf() with the factors on the host (NumPy: uploaded at entry, downloaded at exit and before every callback) against the
factors in HBM (torch tensors: moved device to device by csrc/k_xfer.hip), Y in HBM on both sides.  Fixed max_iter, e_rel = 0
(nothing stops); the clock is around whole nmf() calls, one warm-up call, then REPS calls: median and spread.  With a callback
(one that only counts, like a loss trace that is read later) every iteration is its own device call with a write-back.

    python scratch/device_factors_rate.py [--reps 5]  ->  one JSON line per (shape, max_iter, callback, factors)
"""
import argparse
import json
import logging
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((4096, 4096, 32), (16384, 16384, 64))
MAX_ITER = (1, 200)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import proxmin_amd as pm
    logging.getLogger("proxmin").setLevel(logging.ERROR)
    for M, N, K in SHAPES:
        rng = np.random.default_rng(5)
        Y = torch.from_numpy(rng.random((M, K), dtype=np.float32) @ rng.random((K, N), dtype=np.float32)).cuda()
        A0 = rng.random((M, K), dtype=np.float32) + 0.25
        S0 = rng.random((K, N), dtype=np.float32) + 0.25
        A0t, S0t = torch.from_numpy(A0).cuda(), torch.from_numpy(S0).cuda()
        for iters in MAX_ITER:
            for with_cb in (False, True):
                ends = {}
                for where in ("host", "device"):
                    times, seen = [], [0]

                    def cb(A, S, it=None):
                        seen[0] += 1
                    for rep in range(a.reps + 1):
                        if where == "host":
                            A, S = A0.copy(), S0.copy()
                        else:
                            A, S = A0t.clone(), S0t.clone()
                            torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        pm.nmf.nmf(Y, A, S, max_iter=iters, e_rel=0, callback=cb if with_cb else None)
                        dt = time.perf_counter() - t0    # (nmf() returns when the caller's arrays hold the result, on either side)
                        if rep:                          # the first call is the warm-up
                            times.append(dt)
                    ends[where] = A if where == "host" else A.cpu().numpy()
                    med = statistics.median(times)
                    print(json.dumps({"shape": [M, N, K], "max_iter": iters, "callback": with_cb, "factors": where, "reps": a.reps,
                                      "mode": pm.get_default_mode(), "ms_per_call_median": round(med * 1e3, 3),
                                      "ms_per_call_min": round(min(times) * 1e3, 3), "ms_per_call_max": round(max(times) * 1e3, 3),
                                      "it_per_s_median": round(iters / med, 1)}), flush=True)
                assert ends["host"].tobytes() == ends["device"].tobytes(), "the two sides computed different factors"


if __name__ == "__main__":
    main()
