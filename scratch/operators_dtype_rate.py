"""What an operator called on an array costs: whole calls, host clock around a call that ends synchronised, one warm-up call, then
REPS calls: the median.

  soft          prox_soft(X, 0.5, thresh=0.3)                     X: 16384 x 64
  unity_plus    prox_unity_plus(X, 0.5, axis=0)                   X: 16384 x 64   (the long axis: column sums over all rows)
  soft_S        prox_soft(S, 0.5, thresh=<64 values, (64, 1)>)    S: 64 x 16384   (S orientation: the components along axis 0)
each in float32 and float64, on
  host          a NumPy array (upload, kernel, download)          -- runs on any tree, the parent commit's included
  device        a torch tensor on the GPU, updated in place       -- needs a tree whose operators take device arrays
  copy          torch's device-to-device copy_ of the same array: the same bytes read and written, the yardstick of `device`

    python scratch/operators_dtype_rate.py --legs host[,device,copy] [--reps 5] [--tag parent]     ->  one JSON line per measurement
"""
import argparse
import json
import os
import statistics
import sys
import time
from functools import partial

import numpy as np

sys.path.insert(0, os.getcwd())


def cases(ops):
    K = 64
    th = np.linspace(0.05, 0.6, K).reshape(K, 1)
    return {"soft": ((16384, K), partial(ops.prox_soft, thresh=0.3)),
            "unity_plus": ((16384, K), partial(ops.prox_unity_plus, axis=0)),
            "soft_S": ((K, 16384), partial(ops.prox_soft, thresh=th))}


def median_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="host,device,copy")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tag", default="this")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    from proxmin_amd import operators as ops
    rng = np.random.default_rng(0)
    for name, (shape, prox) in cases(ops).items():
        for dtype in (np.float32, np.float64):
            X0 = (rng.random(shape) + 0.1).astype(dtype)
            for leg in a.legs.split(","):
                if leg == "host":
                    X = X0.copy()
                    fn = lambda: prox(X, 0.5)
                elif leg == "device":
                    T = torch.from_numpy(X0).cuda()
                    fn = lambda: prox(T, 0.5)                      # (complete on return: the library synchronises)
                else:
                    T, D = torch.from_numpy(X0).cuda(), torch.from_numpy(X0).cuda()

                    def fn():
                        D.copy_(T)
                        torch.cuda.synchronize()
                med, lo, hi = median_ms(fn, a.reps)
                print(json.dumps({"tree": a.tag, "case": name, "dtype": np.dtype(dtype).name, "leg": leg, "shape": list(shape),
                                  "median_ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4), "reps": a.reps}), flush=True)


if __name__ == "__main__":
    main()
