"""What the legacy stand-alone operator entry points cost: whole calls, host clock around a call that ends synchronised, one
warm-up call, then REPS calls: the median.  16384 x 64 float32 (the shape of scratch/operators_dtype_rate.py).

  prox_apply    DeviceNMF.prox_apply on BUF_A of a 16384 x 40 x 64 context (pmx_prox_apply: the array stays on the device)
  prox_array    pmx_prox_array on the host array (upload, kernels, download)
each with  soft (relative, 0.3)  and  unity_plus along the rows (column sums over all rows).

    [PMX_LIB=<another build's libpmx.so>] python scratch/standalone_prox_rate.py [--reps 5] [--tag parent]  ->  one JSON line per measurement
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tag", default="this")
    a = ap.parse_args()
    from proxmin_amd import _lib, operators
    from proxmin_amd.engine import DeviceNMF
    lib = _lib.require_gpu()
    rows, K = 16384, 64
    X0 = (np.random.default_rng(0).random((rows, K)) + 0.1).astype(np.float32)
    sk = np.full(K, 0.5, np.float32)
    seqs = {"soft": operators._seq([("soft", 0, 0.3, 1)]), "unity_plus": operators._seq([("unity_plus", 1, 0.0, 0)])}
    with DeviceNMF(rows, 40, K, mode="f32") as dev:
        dev.set_factors(X0, np.ones((K, 40), np.float32))
        for name, ps in seqs.items():
            X = X0.copy()
            legs = {"prox_apply": lambda: dev.prox_apply(_lib.BUF_A, ps, sk),
                    "prox_array": lambda: _lib.check(lib.pmx_prox_array(0, X.ctypes.data_as(C.c_void_p), rows, K, C.byref(ps), sk.ctypes.data_as(C.c_void_p)))}
            for leg, fn in legs.items():
                fn()
                t = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    fn()
                    t.append((time.perf_counter() - t0) * 1e3)
                print(json.dumps({"tree": a.tag, "case": name, "leg": leg, "shape": [rows, K], "median_ms": round(statistics.median(t), 4),
                                  "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "reps": a.reps}), flush=True)


if __name__ == "__main__":
    main()
