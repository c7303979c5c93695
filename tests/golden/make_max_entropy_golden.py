#!/usr/bin/env python3
"""Generate the prox_max_entropy fixtures (`max_entropy*.npz`) from the REAL reference and SciPy.

Run in the build container only (it needs the reference, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_max_entropy_golden.py

oracle/nmf_oracle.py does not know this operator, so the expected values of tests/test_gpu_max_entropy.py come from
`proxmin.operators.prox_max_entropy` (operators.py:163-184) itself:

  1. the stand-alone operator on fp32 and fp64 arrays (`op/...` in max_entropy.npz): its output, and for the fp32 inputs
     also its fp64 evaluation;
  2. final factors of `proxmin.nmf.nmf()` with the operator on one block and prox_plus on the other, 8 iterations, for
     every route and shape of SOLVER_ROUTES x SOLVER_SHAPES (`<shape>/<route>/<block>/A|S`).  The finals do not fit one file
     under the repository's size limit: they are dealt to volumes max_entropy_1.npz, .. and `volumes` in the meta record of
     max_entropy.npz says where each case lives.

Inputs are NOT stored: the tests regenerate them from the seeds with operator_inputs() / solver_problem() below (this
module imports the reference only inside main(), so the tests can import it), and verify the stored checksums.

The operator jumps at 0 (x = 1e-30 -> gamma_ W(1 / (e gamma_)), x = 0 -> 0), so a solver case in which rounding could flip
a sign would test luck.  The generator wraps the reference's operator, looks at every argument it is called with and
REFUSES a case in which any entry lies within 1e-3 max|X| of 0 or has X / gamma_ > 60 (beyond which the reference's fp32
exp() is near its overflow); it then tries the next gamma / seed of its list.  What it settled on is in the meta record.
"""
import json
import os
import sys
from functools import partial

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PROXMIN_REFERENCE", "/root/reference")
LIMIT = 900 * 1024                 # bytes of array data per volume (the repository takes files up to 1 MiB)

GAMMAS = (0.05, 1.0, 10.0)
OP_SHAPES = ((5, 7), (33, 200))    # the second is wider than MAXK = 128
# the step of the relative cases: 0.5, and for gamma = 10 one that makes gamma_ = e^19.5 -- the only way to an L of -20
# (L = x / gamma_ - 1 - ln gamma_ >= -1 - ln gamma_ for x > 0)
REL_STEP = {0.05: 0.5, 1.0: 0.5, 10.0: 2.9e7}

SOLVER_SHAPES = [("float64", 33, 47, 3), ("float64", 40, 56, 12),                         # fp64, small kernels
                 ("float64", 40, 56, 20), ("float64", 48, 72, 40), ("float64", 128, 160, 100),   # fp64, matrix-core kernels: 1, 2, 4 values per lane
                 ("float32", 64, 96, 8), ("float32", 48, 72, 40), ("float32", 128, 256, 64), ("float32", 128, 160, 100)]
SOLVER_ROUTES = ("pgm", "fista", "pgm_bt", "bsdmm_prox", "bsdmm_g", "adam_abs", "pgm_ap")
ITERATIONS = 8
E_REL = {"adam_abs": 1e-4}         # (adaprox: also the stopping test of the proximal sub-iterations); every other route 1e-9
TARGETS = (0.05, 0.1, 0.2, 0.03, 0.4)   # gamma_ the search tries, in data units (the factors are of order 1)
MARGIN, QMAX = 1e-3, 60.0


def gamma_eff(gamma, kind, step):
    return gamma * step if kind == "relative" else gamma


def operator_inputs(shape, gamma_, seed):
    """fp64 inputs of a stand-alone case: L = x / gamma_ - 1 - ln gamma_ spread evenly over [max(-20, Lmin), 60] in random
    order, with planted entries < 0, == 0, NaN, +inf, -inf and within 1e-6 of 0 on both sides (the first 13 of the flat
    array); the fp32 inputs are these rounded to float32."""
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    lmin = -1.0 - np.log(gamma_)
    lo = max(-20.0, lmin + 1e-3)
    L = rng.permutation(np.linspace(lo, 60.0, n))
    X = gamma_ * (L + 1.0 + np.log(gamma_))
    X[:13] = [-1.5 * gamma_, -1e-3, 0.0, -0.0, np.nan, np.inf, -np.inf, 1e-7, -1e-7, 9e-7, -9e-7, 1e-30, -1e-30]
    return X.reshape(shape)


def solver_problem(M, N, K, dtype, seed):
    """Y = At St + noise as in make_golden.problem; the initial factors in [0.25, 0.75): away from the operator's jump at 0, and
    A0 S0 of Y's size, so that the first gradient steps do not throw entries across 0 either."""
    dtype = np.dtype(dtype).type
    rng = np.random.default_rng(seed)
    At, St = rng.random((M, K)), rng.random((K, N))
    Y = (At @ St + 0.01 * rng.standard_normal((M, N))).astype(dtype)
    A0 = (0.25 + 0.5 * rng.random((M, K))).astype(dtype)
    S0 = (0.25 + 0.5 * rng.random((K, N))).astype(dtype)
    return Y, A0, S0


def bound(y64, x, gamma_, eps):
    """the derived relative bound of tests/test_gpu_max_entropy.py on |dy| / y, for the fp64 value y64 of input x"""
    w = y64 / gamma_
    return 8.0 * eps * (1.0 + (np.abs(x / gamma_) + abs(np.log(gamma_)) + 1.0) / (1.0 + w))


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    import scipy
    from proxmin import algorithms as ralg, nmf as rnmf, operators as rops

    blob = {}
    meta = {"numpy": np.__version__, "scipy": scipy.__version__, "reference": "proxmin 0.6.12", "iterations": ITERATIONS,
            "op": {}, "solver": {}, "volumes": {}}

    # ---- 1. the operator alone ------------------------------------------------------------------------------------
    for si, shape in enumerate(OP_SHAPES):
        for gi, gamma in enumerate(GAMMAS):
            for kind in ("relative", "absolute"):
                step = REL_STEP[gamma] if kind == "relative" else 0.5
                g_ = gamma_eff(gamma, kind, step)
                seed = 7000 + 100 * si + 10 * gi + (kind == "absolute")
                X64 = operator_inputs(shape, g_, seed)
                X32 = X64.astype(np.float32)
                name = "op/%dx%d/g%g/%s" % (shape[0], shape[1], gamma, kind)
                with np.errstate(all="ignore"):
                    out64 = rops.prox_max_entropy(X64.copy(), step, gamma=gamma, type=kind)
                    out32 = rops.prox_max_entropy(X32.copy(), step, gamma=gamma, type=kind)
                    out64of32 = rops.prox_max_entropy(X32.astype(np.float64), step, gamma=gamma, type=kind)
                assert out32.dtype == np.float32 and out64.dtype == np.float64
                touched = X32 > 0
                fin = touched & np.isfinite(X32)
                assert np.isfinite(out32[fin]).all() and np.isfinite(out64of32[fin]).all(), name
                # untouched entries keep their bits in the reference as well
                assert np.array_equal(out32[~touched].view(np.uint32), X32[~touched].view(np.uint32)), name
                # the reference's own fp32 output stays inside the bound the device is held to
                rel = np.abs(out32[fin].astype(np.float64) - out64of32[fin]) / out64of32[fin]
                bd = bound(out64of32[fin], X32[fin].astype(np.float64), g_, 2.0 ** -24)
                assert (rel <= bd).all(), "%s: the reference's fp32 output misses the bound by %g" % (name, (rel / bd).max())
                Lv = X64[X64 > 0][np.isfinite(X64[X64 > 0])] / g_ - 1.0 - np.log(g_)
                blob[name + "/ref32"] = out32
                blob[name + "/ref64of32"] = out64of32
                blob[name + "/ref64"] = out64
                meta["op"][name] = {"shape": list(shape), "gamma": gamma, "type": kind, "step": step, "seed": seed,
                                    "sum64": float(np.nansum(np.where(np.isfinite(X64), X64, 0.0))),
                                    "L": [float(Lv.min()), float(Lv.max())], "ref32_over_bound": float((rel / bd).max())}
                print("%-28s L %.2f .. %.2f   reference fp32 / bound %.3f" % (name, Lv.min(), Lv.max(), (rel / bd).max()))

    # ---- 2. solver finals ------------------------------------------------------------------------------------------
    class Recorder(object):
        """the reference's operator, watched: number of calls, the margin of its arguments around 0, the largest X / gamma_"""

        def __init__(self, gamma, kind):
            self.gamma, self.kind, self.calls, self.margin, self.q = gamma, kind, 0, np.inf, 0.0

        def __call__(self, X, step):
            g_ = self.gamma if self.kind == "absolute" else self.gamma * float(step)      # (adaprox passes arrays: absolute there)
            self.calls += 1
            self.margin = min(self.margin, float(np.abs(X).min() / np.abs(X).max()))
            self.q = max(self.q, float(X.max() / g_))
            return rops.prox_max_entropy(X, step, gamma=self.gamma, type=self.kind)

    class Counter(object):
        def __init__(self):
            self.calls = 0

        def __call__(self, X, step):
            self.calls += 1
            return rops.prox_plus(X, step)

    def run(route, j, Y, A0, S0, gamma):
        kind = "absolute" if route == "adam_abs" else "relative"
        rec, plus = Recorder(gamma, kind), Counter()
        A, S = A0.copy(), S0.copy()
        e_rel = E_REL.get(route, 1e-9)
        kw = dict(max_iter=ITERATIONS, e_rel=e_rel)
        me = rops.AlternatingProjections([rops.prox_plus, rec]) if route == "pgm_ap" else rec
        prox = [plus, plus]
        if route != "bsdmm_g":
            prox[j] = me
        if route == "fista":               # (half the Lipschitz steps, as make_golden.py's fista_half: with the full ones the reference's FISTA leaves for 1e5 here)
            kw.update(accelerated=True, step=lambda *X, it=None: tuple(0.5 * s for s in rnmf.step_pgm(*X)))
        if route == "pgm_bt":
            kw.update(backtracking=True, f=partial(rnmf.log_likelihood, Y=Y))
        if route == "bsdmm_g":
            kw["proxs_g"] = [[rec], None] if j == 0 else [None, [rec]]
        alg = {"adam_abs": ralg.adaprox, "bsdmm_prox": ralg.bsdmm, "bsdmm_g": ralg.bsdmm}.get(route, ralg.pgm)
        if alg is ralg.adaprox:
            kw["scheme"] = "adam"
        rnmf.nmf(Y, A, S, prox_A=prox[0], prox_S=prox[1], algorithm=alg, **kw)
        return A, S, rec, plus

    def step0(route, j, A0, S0):
        """the step the operator's first application sees (relative gamma = target / this)"""
        if route == "adam_abs":
            return 1.0
        s = float(rnmf.step_pgm(A0, S0)[j]) * (0.5 if route == "fista" else 1.0)
        return 2.0 * s if route == "bsdmm_g" else s          # step_g = 2 n_g step_f (utils.py:269-279)

    vol, vol_bytes, vols = 1, 0, {1: {}}
    for dt, M, N, K in SOLVER_SHAPES:
        for route in SOLVER_ROUTES:
            for j in range(2):
                name = "%s_%dx%dx%d/%s/%s" % ("f64" if dt == "float64" else "f32", M, N, K, route, "AS"[j])
                done = None
                for seed in (4321, 4322, 4323):
                    Y, A0, S0 = solver_problem(M, N, K, dt, seed)
                    for target in TARGETS:
                        gamma = float("%.3g" % (target / step0(route, j, A0, S0)))
                        try:
                            with np.errstate(all="ignore"):
                                A, S, rec, plus = run(route, j, Y, A0, S0, gamma)
                        except np.linalg.LinAlgError:            # (the iteration left for infinity)
                            print("   refused %s seed %d gamma %g: not finite" % (name, seed, gamma))
                            continue
                        if rec.calls and rec.margin >= MARGIN and rec.q <= QMAX and np.isfinite(A).all() and np.isfinite(S).all():
                            done = (seed, gamma, A, S, rec, plus, Y, A0, S0)
                            break
                        print("   refused %s seed %d gamma %g: margin %.2e, X / gamma_ up to %.1f" % (name, seed, gamma, rec.margin, rec.q))
                    if done:
                        break
                assert done, "no gamma / seed of the lists gives %s its margin" % name
                seed, gamma, A, S, rec, plus, Y, A0, S0 = done
                assert A.dtype == np.dtype(dt) and S.dtype == np.dtype(dt)
                nbytes = A.nbytes + S.nbytes
                if vol_bytes + nbytes > LIMIT:
                    vol, vol_bytes = vol + 1, 0
                    vols[vol] = {}
                vols[vol][name + "/A"] = A
                vols[vol][name + "/S"] = S
                vol_bytes += nbytes
                meta["volumes"][name] = vol
                meta["solver"][name] = {"dtype": dt, "M": M, "N": N, "K": K, "route": route, "block": j, "seed": seed, "gamma": gamma,
                                        "type": rec.kind, "e_rel": E_REL.get(route, 1e-9), "calls_me": rec.calls, "calls_plus": plus.calls,     # (adaprox: the blocks' sub-iteration counts)
                                        "margin": rec.margin, "qmax": rec.q,
                                        "sums": [float(Y.astype(np.float64).sum()), float(A0.astype(np.float64).sum()), float(S0.astype(np.float64).sum())]}
                print("%-36s seed %d gamma %-9g margin %.3f  X / gamma_ <= %5.1f  calls %d" % (name, seed, gamma, rec.margin, rec.q, rec.calls))

    blob["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(HERE, "max_entropy.npz"), **blob)
    for v, arrays in vols.items():
        np.savez_compressed(os.path.join(HERE, "max_entropy_%d.npz" % v), **arrays)
    for f in sorted(os.listdir(HERE)):
        if f.startswith("max_entropy") and f.endswith(".npz"):
            size = os.path.getsize(os.path.join(HERE, f))
            assert size < 1024 * 1024, (f, size)
            print("%-22s %7d bytes" % (f, size))


if __name__ == "__main__":
    main()
