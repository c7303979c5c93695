"""Every route from the Python drivers to an update kernel, on seeded inputs, with every returned array written as .npy.

    python scratch/route_dump.py OUTDIR                 run the routes with the libpmx.so in the tree (or $PMX_LIB), dump into OUTDIR
    python scratch/route_dump.py --compare DIR1 DIR2    list every file that differs in any byte (or exists on one side only)

Two builds whose kernels are identical can only differ in an argument a host route passes to a kernel: run this once per
build (PMX_LIB=<the other libpmx.so>) on the same GPU and compare.  A route that the host refuses (NotImplementedError, a failed
argument check) leaves the exception's text instead of arrays.  Shapes are the smallest that reach each code path; the whole script takes seconds."""
import filecmp
import os
import socket
import sys
from functools import partial

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compare(d1, d2):
    n1, n2 = set(os.listdir(d1)), set(os.listdir(d2))
    bad = sorted(n1 ^ n2)
    for name in sorted(n1 & n2):
        if not filecmp.cmp(os.path.join(d1, name), os.path.join(d2, name), shallow=False):
            bad.append(name)
    for name in bad:
        print("DIFFERS", name)
    print("%d files compared, %d differ" % (len(n1 | n2), len(bad)))
    return 1 if bad else 0


def flatten(prefix, obj, out):
    if isinstance(obj, (tuple, list)):
        for i, v in enumerate(obj):
            flatten("%s.%d" % (prefix, i), v, out)
    elif obj is None:
        out[prefix] = np.array("None")
    else:
        out[prefix] = np.asarray(obj)


def user_plus(X, step):                 # a prox the library cannot recognise: the host round trip
    return np.maximum(X, 0)


def routes():
    import torch
    import proxmin_amd as pm
    from proxmin_amd import distributed as pdist, engine
    from oracle import nmf_oracle as orc
    ops, nmf = pm.operators, pm.nmf.nmf
    unity0 = partial(ops.prox_unity_plus, axis=0)

    def problem(M, N, K, dtype=np.float32, seed=11, **kw):
        return orc.synthetic_problem(M, N, K, dtype, seed=seed, **kw)

    def solve(prob, mode=None, env=None, **kw):
        """-> (A, S, what nmf() returned)"""
        Y, A0, S0 = prob
        A, S = A0.copy(), S0.copy()
        if kw.get("backtracking"):      # the line search wants the likelihood of the same Y (and W)
            kw["f"] = partial(pm.nmf.log_likelihood, Y=Y, W=kw["W"]) if "W" in kw else partial(pm.nmf.log_likelihood, Y=Y)
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        engine.set_default_mode(mode)
        try:
            ret = nmf(Y, A, S, **kw)
        finally:
            engine.set_default_mode(None)
            for k, v in old.items():
                os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
        return A, S, ret

    small = problem(300, 420, 8)
    small_u = problem(300, 420, 8, unity_S=True)
    its = dict(max_iter=12, e_rel=1e-6)

    # ---- pgm / FISTA, default rule ------------------------------------------------------------------------------------------
    for M, N, K, mode in ((300, 420, 8, None), (300, 420, 40, None), (256, 512, 64, None), (256, 512, 64, "f32"), (200, 260, 96, None),
                          (200, 260, 128, None), (8200, 300, 8, None)):
        prob = problem(M, N, K)
        for acc in (False, True):
            yield "pgm_%dx%dx%d_%s_acc%d" % (M, N, K, mode or "default", acc), partial(solve, prob, mode=mode, accelerated=acc, **its)

    # ---- other pgm routes ---------------------------------------------------------------------------------------------------
    sA, sS = pm.nmf.step_pgm(small[1], small[2])
    for acc in (False, True):
        t = "_acc%d" % acc
        yield "pgm_constant_step" + t, partial(solve, small, step=pm.nmf.constant_step(sA, sS), accelerated=acc, **its)
        yield "pgm_bb" + t, lambda acc=acc: solve(small, step=pm.utils.BarzilaiBorweinStepper(), accelerated=acc, **its)
        yield "pgm_backtracking" + t, partial(solve, small, backtracking=True, accelerated=acc, **its)
        yield "pgm_unity_long_axis" + t, partial(solve, small, prox_A=unity0, accelerated=acc, **its)

        def with_callback(acc=acc):
            tb = pm.utils.Traceback()
            return solve(small, callback=tb, accelerated=acc, **its), len(tb.trace)      # (the iteration count)
        yield "pgm_callback" + t, with_callback
        yield "pgm_user_prox" + t, partial(solve, small, prox_S=user_plus, accelerated=acc, **its)

        def step_arrays(*X, it=None, **kw):
            a, s = pm.nmf.step_pgm(*X)
            return np.full(X[0].shape, a, X[0].dtype), s
        yield "pgm_user_step_arrays" + t, partial(solve, small, step=step_arrays, accelerated=acc, **its)
        yield "pgm_user_prox_bb" + t, lambda acc=acc: solve(small, prox_A=user_plus, step=pm.utils.BarzilaiBorweinStepper(), accelerated=acc, **its)
    small64 = problem(300, 420, 8, np.float64)
    big64 = problem(200, 260, 64, np.float64)
    W64 = np.random.RandomState(5).uniform(0.5, 1.5, big64[0].shape)
    for bt in (False, True):
        yield "pgm_f64_small_bt%d" % bt, partial(solve, small64, backtracking=bt, accelerated=True, **its)
        yield "pgm_f64_big_weights_bt%d" % bt, partial(solve, big64, W=W64, step=pm.nmf.step_pgm, backtracking=bt, accelerated=True, **its)

    # ---- adaprox ------------------------------------------------------------------------------------------------------------
    ada = dict(algorithm=pm.adaprox, prox_A=ops.prox_plus, prox_S=unity0, max_iter=8, e_rel=1e-3)
    for env in ({}, {"PMX_TAIL_FUSED": "0"}):
        t = "_chain" if env else "_fused"
        for scheme in ("adam", "nadam", "adamx", "amsgrad", "padam", "radam"):
            yield "ada_%s%s" % (scheme, t), partial(solve, small_u, env=env, scheme=scheme, **ada)
        for scheme in ("amsgrad", "adamx"):
            def warm(scheme=scheme, env=env):
                _, _, (_, M, V, _) = solve(small_u, env=env, scheme=scheme, **ada)      # (a cold start returns no Vhat)
                return solve(small_u, env=env, scheme=scheme, M=M, V=V, Vhat=[v.copy() for v in V], **ada)
            yield "ada_%s_warm%s" % (scheme, t), warm
        # the proximal loop of the first iterations outruns the passes enqueued with them (HALT_NEED_SUB), up to prox_max_iter and beyond it
        for pmi in (1000, 6):
            yield "ada_more_subs_pmi%d%s" % (pmi, t), partial(solve, small_u, env=env, scheme="adam", **dict(ada, e_rel=1e-7, prox_max_iter=pmi))
    yield "ada_user_prox_S", partial(solve, small, scheme="amsgrad", **dict(ada, prox_S=user_plus))
    yield "ada_user_step", partial(solve, small_u, scheme="adam", step=lambda *X, it=None: pm.nmf.step_adaprox(*X, it=it), **ada)
    yield "ada_f64_small", partial(solve, problem(300, 420, 8, np.float64, unity_S=True), scheme="amsgrad", **ada)
    yield "ada_f64_big", partial(solve, problem(200, 260, 64, np.float64, unity_S=True), scheme="amsgrad", **ada)

    # ---- bsdmm --------------------------------------------------------------------------------------------------------------
    soft = partial(ops.prox_soft, thresh=0.01)
    bsd = dict(algorithm=pm.bsdmm, max_iter=8, e_rel=1e-6)
    for order in (None, [1, 0]):
        for ng, pg in ((1, [[ops.prox_plus], [ops.prox_plus]]), (2, [[ops.prox_plus, soft], [ops.prox_plus, soft]])):
            yield "bsdmm_order%s_g%d" % ("default" if order is None else "10", ng), partial(solve, small, proxs_g=pg, update_order=order, **bsd)
    yield "bsdmm_user_constraint", partial(solve, small, proxs_g=[[ops.prox_plus, user_plus], [ops.prox_plus]], **bsd)
    yield "bsdmm_f64_small", partial(solve, small64, proxs_g=[[ops.prox_plus, soft], [ops.prox_plus]], **bsd)
    yield "bsdmm_f64_big", partial(solve, big64, proxs_g=[[ops.prox_plus, soft], [ops.prox_plus]], **bsd)

    # ---- row-sharded, world size 1 (tests/test_gpu_distributed.py) ------------------------------------------------------------
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(s.getsockname()[1])
    s.close()
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)

    def sharded(fn, prob, env=None, **kw):
        Y, A0, S0 = prob
        A, S = A0.copy(), S0.copy()
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            ret = fn(Y, A, S, Y.shape[0], **kw)
        finally:
            for k, v in old.items():
                os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
        return A, S, ret

    p_ada, p_ada_u = problem(700, 900, 24, seed=4), problem(700, 900, 24, seed=4, unity_S=True)
    sh = dict(prox_A=ops.prox_plus, scheme="amsgrad", e_rel=1e-3, max_iter=7)
    yield "shard_ada_fused", partial(sharded, pdist.nmf_adaprox_sharded, p_ada_u, prox_S=unity0, **sh)
    yield "shard_ada_chain", partial(sharded, pdist.nmf_adaprox_sharded, p_ada_u, env={"PMX_TAIL_FUSED": "0"}, prox_S=unity0, **sh)
    yield "shard_ada_s_split", partial(sharded, pdist.nmf_adaprox_sharded, p_ada, prox_S=ops.prox_plus, s_split=True, **sh)
    p_pgm = problem(520, 700, 12, seed=6)
    yield "shard_pgm_plain", partial(sharded, pdist.nmf_pgm_sharded, p_pgm, e_rel=1e-9, max_iter=7)
    yield "shard_pgm_accelerated", partial(sharded, pdist.nmf_pgm_sharded, p_pgm, accelerated=True, step_scale=0.5, e_rel=1e-9, max_iter=6)
    yield "shard_bsdmm", partial(sharded, pdist.nmf_bsdmm_sharded, problem(480, 640, 10, seed=8),
                                 proxs_g=[[ops.prox_plus, soft], [ops.prox_plus, soft]], e_rel=1e-9, max_iter=6)
    yield "_end", lambda: dist.destroy_process_group()


def main(argv):
    if len(argv) == 3 and argv[0] == "--compare":
        return compare(argv[1], argv[2])
    if len(argv) != 1:
        print(__doc__)
        return 2
    outdir = argv[0]
    os.makedirs(outdir, exist_ok=True)
    import torch  # noqa: F401      (before libpmx.so is loaded: the sharded routes need torch's HIP runtime to see the GPU)
    import __graft_entry__ as g
    if not os.environ.get("PMX_LIB"):
        g.build()
    n = 0
    for name, fn in routes():
        try:
            res = fn()
        except (NotImplementedError, AssertionError, TypeError, ValueError) as exc:     # refused on the host, nothing ran: its text is the result
            res = np.array("%s: %s" % (type(exc).__name__, exc))
            print("%-40s %s" % (name, res), flush=True)
        files = {}
        flatten(name, res, files)
        for key, arr in files.items():
            np.save(os.path.join(outdir, key + ".npy"), arr, allow_pickle=False)
        n += len(files)
        print("%-40s %d arrays" % (name, len(files)), flush=True)
    print("%d files in %s" % (n, outdir))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
