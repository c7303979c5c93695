#!/usr/bin/env python3
"""Generate the per-component-threshold fixtures (`components*.npz`) from the REAL reference.

Run in the build container only (it needs the reference, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_components_golden.py

What the reference can compute of the per-component operators: an ARRAY `thresh` on prox_soft, prox_soft_plus, prox_hard and
prox_hard_plus, which it broadcasts -- (K,) against A (M x K), (K, 1) against S (K x N).  (prox_min / prox_max / prox_max_entropy
raise on an array there, and prox_components cannot run: tests/test_gpu_components.py holds those to the scalar operators
and to the oracle.)

  1. the stand-alone operators on fp32 and fp64 arrays of both orientations (`op/...` in components.npz);
  2. final factors of `proxmin.nmf.nmf()` after 8 iterations with the operator on one block and prox_plus on the other, for
     ROUTES x SHAPES x the four operators (`<shape>/<route>/<op>/<block>/A|S`), dealt to volumes components_1.npz, .. under
     the repository's size limit; `volumes` in the meta record of components.npz says where each case lives.

Inputs are NOT stored: the tests regenerate them from the seeds with operator_inputs() / solver_problem() / thresholds() below
(this module imports the reference only inside main()) and verify the stored checksums.

Thresholds are kinks (soft) and jumps (hard): the generator wraps the reference's operator, looks at every argument it is
called with and REFUSES a case in which any |argument| lies within 1e-3 max|X| of its row's threshold; it then tries the
next threshold level / seed of its lists.  What it settled on is in the meta record.
"""
import json
import os
import sys
from functools import partial

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PROXMIN_REFERENCE", "/root/reference")
LIMIT = 900 * 1024                 # bytes of array data per volume (the repository takes files up to 1 MiB)

OPS = ("soft", "soft_plus", "hard", "hard_plus")
SHAPES = [("float64", 33, 47, 3), ("float64", 48, 72, 40), ("float32", 48, 72, 40)]     # three of README_max_entropy.md's shapes
ROUTES = ("pgm", "fista", "adam_abs", "bsdmm_prox", "bsdmm_g")
ITERATIONS = 8
E_REL = {"adam_abs": 1e-4}         # (adaprox: also the stopping test of the proximal sub-iterations); every other route 1e-9
LEVELS = (0.02, 0.05, 0.01, 0.1, 0.005, 0.2)   # mean threshold x step the search tries, in data units (the factors are of order 1)
SEEDS = (5321, 5322, 5323, 5324)
MARGIN = 1e-3
OP_SHAPES = ((37, 5), (33, 100))


def thresholds(K, level):
    """K distinct values from half to one and a half times `level`, in an order that is not monotonic"""
    return level * (0.5 + ((np.arange(K) * 7) % K + 0.5) / K)


def per_component(t, block):
    return np.asarray(t) if block == 0 else np.asarray(t).reshape(-1, 1)


def solver_problem(M, N, K, dtype, seed):
    dtype = np.dtype(dtype).type
    rng = np.random.default_rng(seed)
    At, St = rng.random((M, K)), rng.random((K, N))
    Y = (At @ St + 0.01 * rng.standard_normal((M, N))).astype(dtype)
    A0 = (0.25 + 0.5 * rng.random((M, K))).astype(dtype)
    S0 = (0.25 + 0.5 * rng.random((K, N))).astype(dtype)
    return Y, A0, S0


def margin_of(X, t_eff):
    """smallest | |x| - t | / max|X| over the array, t_eff broadcast against X"""
    X = np.asarray(X, dtype=np.float64)
    return float(np.min(np.abs(np.abs(X) - t_eff)) / np.abs(X).max())


def operator_inputs(shape, t_eff, seed):
    """fp64 values in [-1, 1.5) with planted zeros; entries nearer than 2e-3 max|X| to their component's threshold are moved
    4e-3 away from it"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.5, shape)
    X.reshape(-1)[:4] = [0.0, -0.0, 1.25, -0.75]
    T = np.broadcast_to(t_eff, shape)
    near = np.abs(np.abs(X) - T) < 2e-3 * 1.5
    X = np.where(near, np.sign(X) * (T + 6e-3), X)
    return X


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    from proxmin import algorithms as ralg, nmf as rnmf, operators as rops

    blob = {}
    meta = {"numpy": np.__version__, "reference": "proxmin 0.6.12", "iterations": ITERATIONS, "op": {}, "solver": {}, "volumes": {}}

    # ---- 1. the operators alone ---------------------------------------------------------------------------------------
    for si, (R, K) in enumerate(OP_SHAPES):
        for oi, op in enumerate(OPS):
            for block in (0, 1):
                for kind in ("relative", "absolute"):
                    step = 0.5 if kind == "relative" else 0.7
                    t = thresholds(K, 0.6)
                    t_eff = per_component(t * (step if kind == "relative" else 1.0), block)
                    shape = (R, K) if block == 0 else (K, R)
                    seed = 8000 + 100 * si + 10 * oi + 2 * block + (kind == "absolute")
                    X64 = operator_inputs(shape, t_eff, seed)
                    X32 = X64.astype(np.float32)
                    name = "op/%dx%d/%s/%s/%s" % (shape[0], shape[1], op, "AS"[block], kind)
                    fn = getattr(rops, "prox_" + op)
                    out64 = fn(X64.copy(), step, thresh=per_component(t, block), type=kind)
                    out32 = fn(X32.copy(), step, thresh=per_component(t, block), type=kind)
                    m = min(margin_of(X64, t_eff), margin_of(X32, t_eff))
                    assert m >= MARGIN, (name, m)
                    assert out64.shape == shape and 0 < (out64 == 0).sum() < out64.size, name
                    blob[name + "/ref64"] = out64
                    blob[name + "/ref32"] = np.asarray(out32, dtype=np.float64)       # (the reference promotes fp32 x fp64 thresholds)
                    meta["op"][name] = {"shape": list(shape), "op": op, "block": block, "type": kind, "step": step, "level": 0.6,
                                        "seed": seed, "sum64": float(X64.sum()), "margin": m}

    # ---- 2. solver finals -----------------------------------------------------------------------------------------------
    class Recorder(object):
        """the reference's operator with its array threshold, watched: calls, and how near any argument came to its row's threshold"""

        def __init__(self, op, t, kind, block):
            self.fn, self.t, self.kind, self.block, self.calls, self.margin = getattr(rops, "prox_" + op), per_component(t, block), kind, block, 0, np.inf

        def __call__(self, X, step):
            self.calls += 1
            t_eff = self.t * np.asarray(step, dtype=np.float64) if self.kind == "relative" else self.t
            self.margin = min(self.margin, margin_of(X, t_eff))
            return self.fn(X, step, thresh=self.t, type=self.kind)

    class Counter(object):
        def __init__(self):
            self.calls = 0

        def __call__(self, X, step):
            self.calls += 1
            return rops.prox_plus(X, step)

    def run(route, op, j, Y, A0, S0, t):
        kind = "absolute" if route == "adam_abs" else "relative"
        rec, plus = Recorder(op, t, kind, j), Counter()
        A, S = A0.copy(), S0.copy()
        kw = dict(max_iter=ITERATIONS, e_rel=E_REL.get(route, 1e-9))
        prox = [plus, plus]
        if route != "bsdmm_g":
            prox[j] = rec
        if route == "fista":               # (half the Lipschitz steps, as make_golden.py's fista_half)
            kw.update(accelerated=True, step=lambda *X, it=None: tuple(0.5 * s for s in rnmf.step_pgm(*X)))
        if route == "bsdmm_g":
            kw["proxs_g"] = [[rec], None] if j == 0 else [None, [rec]]
        alg = {"adam_abs": ralg.adaprox, "bsdmm_prox": ralg.bsdmm, "bsdmm_g": ralg.bsdmm}.get(route, ralg.pgm)
        if alg is ralg.adaprox:
            kw["scheme"] = "adam"
        rnmf.nmf(Y, A, S, prox_A=prox[0], prox_S=prox[1], algorithm=alg, **kw)
        return A, S, rec, plus

    def step0(route, j, A0, S0):
        if route == "adam_abs":
            return 1.0
        s = float(rnmf.step_pgm(A0, S0)[j]) * (0.5 if route == "fista" else 1.0)
        return 2.0 * s if route == "bsdmm_g" else s          # step_g = 2 n_g step_f (utils.py:269-279)

    vol, vol_bytes, vols = 1, 0, {1: {}}
    for dt, M, N, K in SHAPES:
        for ri, route in enumerate(ROUTES):
            for oi, op in enumerate(OPS):
                j = (ri + oi) % 2                              # the operator's block alternates over the cases
                name = "%s_%dx%dx%d/%s/%s/%s" % ("f64" if dt == "float64" else "f32", M, N, K, route, op, "AS"[j])
                done = None
                for seed in SEEDS:
                    Y, A0, S0 = solver_problem(M, N, K, dt, seed)
                    for level in LEVELS:
                        scale = float("%.3g" % (1.0 / step0(route, j, A0, S0)))
                        t = thresholds(K, level) * scale
                        try:
                            with np.errstate(all="ignore"):
                                A, S, rec, plus = run(route, op, j, Y, A0, S0, t)
                        except np.linalg.LinAlgError:
                            continue
                        if rec.calls and rec.margin >= MARGIN and np.isfinite(A).all() and np.isfinite(S).all():
                            done = (seed, level, scale, A, S, rec, plus, Y, A0, S0)
                            break
                        print("   refused %s seed %d level %g: margin %.2e" % (name, seed, level, rec.margin))
                    if done:
                        break
                if not done:
                    print("!! no level / seed of the lists gives %s its margin: left out" % name)
                    continue
                seed, level, scale, A, S, rec, plus, Y, A0, S0 = done
                assert A.dtype == np.dtype(dt) and S.dtype == np.dtype(dt)
                nbytes = A.nbytes + S.nbytes
                if vol_bytes + nbytes > LIMIT:
                    vol, vol_bytes = vol + 1, 0
                    vols[vol] = {}
                vols[vol][name + "/A"] = A
                vols[vol][name + "/S"] = S
                vol_bytes += nbytes
                meta["volumes"][name] = vol
                meta["solver"][name] = {"dtype": dt, "M": M, "N": N, "K": K, "route": route, "op": op, "block": j, "seed": seed, "level": level,
                                        "scale": scale, "type": rec.kind, "e_rel": E_REL.get(route, 1e-9), "calls_op": rec.calls,
                                        "calls_plus": plus.calls, "margin": rec.margin, "zeros": int(((A, S)[j] == 0).sum()),
                                        "sums": [float(Y.astype(np.float64).sum()), float(A0.astype(np.float64).sum()), float(S0.astype(np.float64).sum())]}
                print("%-44s seed %d level %-6g margin %.4f zeros %d calls %d" % (name, seed, level, rec.margin, ((A, S)[j] == 0).sum(), rec.calls))

    blob["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(HERE, "components.npz"), **blob)
    for v, arrays in vols.items():
        np.savez_compressed(os.path.join(HERE, "components_%d.npz" % v), **arrays)
    for f in sorted(os.listdir(HERE)):
        if f.startswith("components") and f.endswith(".npz"):
            size = os.path.getsize(os.path.join(HERE, f))
            assert size < 1024 * 1024, (f, size)
            print("%-22s %7d bytes" % (f, size))


if __name__ == "__main__":
    main()
