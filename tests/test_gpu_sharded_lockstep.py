"""GPU, world 3 / 4 / 8 in ONE process: the row-sharded solvers (pmx_adaprox_phase, pmx_pgm_phase, pmx_bsdmm_phase; k_shard_pack,
k_shard_post, k_shard_gram_in and their _split variants) against the fp64 oracle of the WHOLE problem.

tests/lockstep_world.py opens one context per rank and drives them in lockstep through the product's own drivers
(ShardedAdaproxDriver, ShardedLoop), the collective being a plain sum over the ranks' comm buffers: rank numbers above 1,
unequal shards (a zero-padded frame next to none, a tuned kernel next to a guarded one, fewer rows than K), column splits of
175 and 375, up to eight addends in every sum.  tests/test_gpu_distributed_world2.py runs two real processes with equal halves;
what is NOT covered by either is a real RCCL ring and timing.

  a. the comm buffer after the first phase 0 and its collective: gSt against fp64 residual_gradients of the whole problem (the
     tolerance of one GPU's gradient, __graft_entry__.smoke: rtol 2e-5, atol 2e-5 max|gS|); on an INTEGER family (entries 0..3:
     every local sum and every sum over ranks is exact in fp32) Gram(A), colsum(A), colsum(S) with array_equal, the padding
     exactly zero; pgm's step sizes against 1 / lmax of the fp64 global Gram matrices within test_gpu_step_rule.ACCEPT;
  b. trajectories after 5-9 iterations under the world-2 test's rule: per-entry bound 1e-5 + 1e-4 |want|; smooth back-ends in
     mode f32: every entry within it; otherwise a share >= 0.9999 (smooth) / 0.995 (amsgrad) within it and a hard envelope of
     50 x / 1000 x the bound.  Conditions, not measurements; tests/test_lockstep_world_cpu.py checks on the CPU that the
     oracle's own float32 run meets them with room to spare for every case below (a changed case must pass that first);
  d. stopping at the oracle's iteration (deferred test, _flush);
  e. the fp16 range guard's refusal on ONE rank of four.

KERNELS pins, per case and mode, the K1 kernel, frame and fused tail of every rank: a case that silently drops to another
kernel fails instead of passing."""
import ctypes as C
import functools
import os
import sys
from functools import partial

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import nmf_oracle as orc  # noqa: E402
from proxmin_amd.distributed import shard_rows  # noqa: E402
from test_gpu_step_rule import ACCEPT  # noqa: E402  (k_gram.hip's acceptance rule: imported, not copied)

MODES = ("f32", "bf16x3", "f16x2", "f16x2r")


def _even(M, W):
    return [(r * (M // W), (r + 1) * (M // W)) for r in range(W)]


# scheme: adaprox only; splits: S replicated (False) / S-split (True); its: 5-9 as in tests/test_gpu_distributed_world2.py
CASES = {
    # guarded kernels, N % 3 = 0, prox_unity_plus on S (its proximal loop takes more than two passes), replicated S
    "ada_unity_w3": dict(alg="adaprox", M=770, N=900, K=24, ranges=shard_rows(770, 3), schemes=("amsgrad",), unity=True, splits=(False,), its=9),
    # the tuned K = 64 kernel of every mode on 8 ranks of 128 rows; sncol = 160
    "ada_k64_w8": dict(alg="adaprox", M=1024, N=1280, K=64, ranges=_even(1024, 8), schemes=("amsgrad",), splits=(False, True), its=6),
    # 251 / 250 rows x 1500 columns: every rank on a zero-padded 256 x 1536 frame; sncol = 375
    "ada_ragged_w4": dict(alg="adaprox", M=1003, N=1500, K=64, ranges=shard_rows(1003, 4), schemes=("adam",), splits=(False, True), its=6),
    # a 5-row rank (fewer rows than K) between two tuned ones
    "ada_unequal_w3": dict(alg="adaprox", M=1285, N=768, K=64, ranges=[(0, 256), (256, 261), (261, 1285)], schemes=("adam", "amsgrad"),
                           splits=(False, True), its=6),
    "ada_k128_w4": dict(alg="adaprox", M=512, N=640, K=128, ranges=_even(512, 4), schemes=("adam",), splits=(True,), its=5, modes=("f32", "f16x2")),
    "ada_k32_w4": dict(alg="adaprox", M=512, N=1024, K=32, ranges=_even(512, 4), schemes=("amsgrad",), splits=(True,), its=6),
    # N % 3 != 0: replicated S only (s_split=True is refused)
    "pgm_w3": dict(alg="pgm", M=520, N=700, K=12, ranges=shard_rows(520, 3), splits=(False,), its=7),
    # sncol = 175: chunks of an odd number of floats
    "pgm_split_w4": dict(alg="pgm", M=520, N=700, K=12, ranges=shard_rows(520, 4), splits=(True,), its=7),
    "fista_split_w8": dict(alg="pgm", M=1024, N=1280, K=64, ranges=_even(1024, 8), splits=(True,), its=7, accelerated=True),
    "pgm_unequal_w3": dict(alg="pgm", M=1329, N=768, K=64, ranges=[(0, 300), (300, 305), (305, 1329)], splits=(True,), its=6),
    "bsdmm_w4": dict(alg="bsdmm", M=482, N=640, K=10, ranges=shard_rows(482, 4), splits=(False,), its=6),
    "bsdmm_w8": dict(alg="bsdmm", M=1024, N=1280, K=64, ranges=_even(1024, 8), splits=(False,), its=6),
}
# e. ada_k64_w8's shape on four ranks of 256 rows; rank 2's rows of A start 1e5 x above the data (tests/test_gpu_range.py)
REFUSED = dict(alg="adaprox", M=1024, N=1280, K=64, ranges=_even(1024, 4), schemes=("adam",), splits=(False,), its=5, modes=("f16x2",),
               far_rows=(512, 768, 1e5))
# d. loose e_rel: the oracle stops before max_iter (the shapes of ada_unity_w3 without the unity constraint, and of pgm_split_w4)
STOPPING = {
    "ada_stop_w3": dict(alg="adaprox", M=770, N=900, K=24, ranges=shard_rows(770, 3), schemes=("amsgrad",), splits=(False,), its=80, e_rel=5e-2,
                        check=True, modes=("f32",)),
    "pgm_stop_w4": dict(alg="pgm", M=520, N=700, K=12, ranges=shard_rows(520, 4), splits=(True,), its=300, e_rel=3e-2, modes=("f32",)),
}
ALL_CASES = dict(CASES, ada_refused_w4=REFUSED, **STOPPING)
assert CASES["ada_unity_w3"]["ranges"] == [(0, 257), (257, 514), (514, 770)]
assert [b - a for a, b in CASES["ada_ragged_w4"]["ranges"]] == [251, 251, 251, 250]
assert [b - a for a, b in CASES["bsdmm_w4"]["ranges"]] == [121, 121, 120, 120]

# K1 per arithmetic mode, as pmx_k1_info names it: the tuned kernels of K = 64 / 32 / 128 (whole 128-row blocks, on a zero-padded
# frame where the shape is ragged), the guarded ones of any shape, the fused small-problem kernel (K <= 16)
TUNED64 = {"f32": "k_grad_f32_pc", "bf16x3": "k_grad_bf16", "f16x2": "k_grad_f16_v8", "f16x2r": "k_grad_f16_v8_hh"}
TUNED32 = {"f32": "k_grad_f32_pc", "bf16x3": "k_grad_bf16", "f16x2": "k_grad_f16_k32", "f16x2r": "k_grad_f16_k32_r3"}
TUNED128 = {"f32": "k_grad_f32", "f16x2": "k_grad_f16_k128"}
GUARDED = {"f32": "k_grad_f32", "bf16x3": "k_grad_bf16", "f16x2": "k_grad_bf16", "f16x2r": "k_grad_bf16"}
SMALL = dict.fromkeys(MODES, "k_grad_small")


def _pin(fused, *groups, modes=MODES):
    """groups of equal neighbouring ranks: (ranks, kernel per mode, frame | {mode: frame}) -> {mode: [(ranks, kernel, frame, fused tail)]}"""
    return {m: [(n, ker[m], fr[m] if isinstance(fr, dict) else fr, fused) for n, ker, fr in groups] for m in modes}


# Pinned per case and mode: (ranks, K1 kernel, K1 frame (rows, columns), fused adaprox tail) in rank order, equal neighbours
# folded.  What each case was written to reach; recorded from pmx_k1_info / pmx_k1_frame on an MI355X.
KERNELS = {
    # K = 24: the 257-row ranks on guarded kernels; the 256-row rank on K = 32's tuned kernel, columns padded to 1024 (bf16x3 has none at K = 32)
    "ada_unity_w3": _pin(True, (2, GUARDED, (257, 900)), (1, TUNED32, {**dict.fromkeys(MODES, (256, 1024)), "bf16x3": (256, 900)})),
    "ada_k64_w8": _pin(True, (8, TUNED64, (128, 1280))),
    "ada_ragged_w4": _pin(True, (4, TUNED64, (256, 1536))),
    "ada_unequal_w3": _pin(True, (1, TUNED64, (256, 768)), (1, GUARDED, (5, 768)), (1, TUNED64, (1024, 768))),
    "ada_k128_w4": _pin(True, (4, TUNED128, (128, 640)), modes=("f32", "f16x2")),
    "ada_k32_w4": _pin(True, (4, TUNED32, (128, 1024))),
    "pgm_w3": _pin(False, (1, SMALL, (174, 700)), (2, SMALL, (173, 700))),
    "pgm_split_w4": _pin(False, (4, SMALL, (130, 700))),
    "fista_split_w8": _pin(False, (8, TUNED64, (128, 1280))),
    "pgm_unequal_w3": _pin(False, (1, GUARDED, (300, 768)), (1, GUARDED, (5, 768)), (1, TUNED64, (1024, 768))),
    "bsdmm_w4": _pin(False, (2, SMALL, (121, 640)), (2, SMALL, (120, 640))),
    "bsdmm_w8": _pin(False, (8, TUNED64, (128, 1280))),
}

BOUND_ATOL, BOUND_RTOL = 1e-5, 1e-4


def modes_of(c):
    return c.get("modes", MODES)


def is_smooth(c, scheme):
    """amsgrad's eps clamp turns rounding differences into visible ones on a few entries (tests/test_gpu_parity_strict.py)"""
    return c["alg"] != "adaprox" or scheme == "adam"


@functools.lru_cache(maxsize=None)
def problem(name):
    """(Y, A0, S0) of a case in float32, read-only, shared by every test of the case"""
    c = ALL_CASES[name]
    Y, A0, S0 = orc.synthetic_problem(c["M"], c["N"], c["K"], np.float32, unity_S=c.get("unity", False), seed=4)
    if c.get("far_rows"):
        r0, r1, f = c["far_rows"]
        A0[r0:r1] *= np.float32(f)
    for x in (Y, A0, S0):
        x.setflags(write=False)
    return Y, A0, S0


@functools.lru_cache(maxsize=None)
def oracle_run(name, scheme, dtype="float64", e_scale=1.0):
    """the unsharded oracle on the whole problem, arrays of `dtype` -> (A, S, iterations), read-only"""
    c = ALL_CASES[name]
    dt = np.dtype(dtype).type
    Y, A0, S0 = problem(name)
    Yd, A, S = Y.astype(dt), A0.astype(dt), S0.astype(dt)
    its = c["its"]
    if c["alg"] == "adaprox":
        ret = orc.adaprox_nmf(Yd, A, S, ("plus",), ("unity_plus", 0) if c.get("unity") else ("plus",), scheme=scheme, max_iter=its,
                              e_rel=c.get("e_rel", 1e-3) * e_scale, check_convergence=c.get("check", False))
        n = ret[4]
    elif c["alg"] == "pgm":
        okw = dict(accelerated=True, step=lambda a, s_, it, g: tuple(0.5 * x for x in orc.lipschitz_steps(a, s_))) if c.get("accelerated") else {}
        n = orc.pgm_nmf(Yd, A, S, max_iter=its, e_rel=c.get("e_rel", 1e-9) * e_scale, **okw)[3]
    else:
        n = orc.bsdmm_nmf(Yd, A, S, proxs_g=[[("plus",), ("soft", 0.01, "relative")]] * 2, max_iter=its, e_rel=1e-9)[1]
    A.setflags(write=False)
    S.setflags(write=False)
    return A, S, n


def parity(got, want, smooth, exact, what):
    """rule (b) for one array; prints the figures before it asserts -> (worst ratio, share within the bound)"""
    err = np.abs(got.astype(np.float64) - want)
    ratio = err / (BOUND_ATOL + BOUND_RTOL * np.abs(want))
    worst, share = float(ratio.max()), float((ratio <= 1.0).mean())
    print("%-40s worst %8.3f x the bound, %.6f within" % (what, worst, share))
    assert np.isfinite(got).all(), what
    if smooth and exact:
        assert worst <= 1.0, "%s: worst entry %.2f x the bound against the fp64 oracle" % (what, worst)
    else:
        assert share >= (0.9999 if smooth else 0.995), "%s: %.5f within the bound" % (what, share)
        env = 50.0 if smooth else 1000.0
        assert worst <= env, "%s: worst entry %.1f x the bound (envelope %g x)" % (what, worst, env)
    return worst, share


def variants(cases):
    out = []
    for name, c in cases.items():
        for scheme in c.get("schemes", (None,)):
            for split in c["splits"]:
                for mode in modes_of(c):
                    out.append(pytest.param(name, scheme, split, mode, id="-".join([name] + ([scheme] if scheme else []) + ["split" if split else "repl", mode])))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pm():
    import __graft_entry__ as g
    g.build()
    import proxmin_amd
    return proxmin_amd


def open_world(pm, name, scheme, split, mode, data=None):
    from lockstep_world import LockstepWorld
    ops = pm.operators
    c = ALL_CASES[name]
    Y, A0, S0 = data if data is not None else problem(name)
    if c["alg"] == "adaprox":
        pS = partial(ops.prox_unity_plus, axis=0) if c.get("unity") else ops.prox_plus
        e = c.get("e_rel", 1e-3)
        return LockstepWorld(Y, A0, S0, c["ranges"], "adaprox", mode, split, prox_A=ops.prox_plus, prox_S=pS, scheme=scheme,
                             check_convergence=c.get("check", False), e_rel=(e, e), prox_max_iter=1000)
    if c["alg"] == "pgm":
        e = c.get("e_rel", 1e-9)
        return LockstepWorld(Y, A0, S0, c["ranges"], "pgm", mode, split, accelerated=c.get("accelerated", False),
                             step_scale=0.5 if c.get("accelerated") else 1.0, e_rel=(e, e))
    pgl = [[ops.prox_plus, partial(ops.prox_soft, thresh=0.01)]] * 2
    return LockstepWorld(Y, A0, S0, c["ranges"], "bsdmm", mode, split, proxs_g=pgl, e_rel=(1e-9, 1e-9), e_abs=(0.0, 0.0))


def kernel_runs(world):
    """[(ranks, kernel, frame, tail_fused)] in rank order, equal neighbours folded"""
    out = []
    for info in world.k1_infos():
        item = (info["kernel"], tuple(int(v) for v in info["frame"]), bool(info["tail_fused"]))
        if out and out[-1][1:] == item:
            out[-1] = (out[-1][0] + 1,) + item
        else:
            out.append((1,) + item)
    return out


def pin_kernels(name, mode, world):
    got = kernel_runs(world)
    print("K1 of %s in mode %s: %r" % (name, mode, got))
    assert got == KERNELS[name][mode], "%s, mode %s: the ranks run %r, the case was written for %r" % (name, mode, got, KERNELS[name][mode])


def c_layout(eng):
    """offsets of the comm buffer as the C ABI reports them (pmx_comm_layout / pmx_comm_layout_split)"""
    lib, h = eng.dev.lib, eng.dev.h
    cnt = C.c_int64()
    if eng.s_split:
        chunk, offs = C.c_int64(), (C.c_int64 * 4)()
        assert lib.pmx_comm_layout_split(h, C.byref(cnt), C.byref(chunk), offs) == 0
        return dict(count=cnt.value, chunk=chunk.value, gst=offs[0], gram=offs[0], colsum_A=offs[1], colsum_S=offs[2], scalars=offs[3])
    offs = (C.c_int64 * 3)()
    assert lib.pmx_comm_layout(h, C.byref(cnt), offs) == 0
    return dict(count=cnt.value, chunk=cnt.value, gst=offs[0], gram=offs[0], colsum_A=offs[1], colsum_S=None, scalars=offs[2])


def first_gradient_point(c, Y, A0, S0):
    """fp64 gS of the first iteration.  pgm, FISTA and adaprox evaluate it at (A0, S0); bsdmm after its A step (Gauss-Seidel),
    which at the start (Z = X, U = 0) is A1 = prox_plus(A0 - step_A gA)."""
    Y64, A, S = Y.astype(np.float64), A0.astype(np.float64), S0.astype(np.float64)
    if c["alg"] == "bsdmm":
        sA = orc.lipschitz_steps(A, S)[0]
        A = orc.apply_prox(A - sA * orc.residual_gradients(A, S, Y64)[0], sA, ("plus",))
    return orc.residual_gradients(A, S, Y64)[1]


def assembled_gst(snap, lay, N, K, split, world):
    """the N x K block of gS^T as the ranks hold it after the collective; replicated: identical on every rank"""
    if not split:
        for b in snap[1:]:
            assert np.array_equal(b, snap[0]), "the all-reduced buffers differ between ranks"
        return snap[0][:N * K].reshape(N, K)
    sncol = N // world
    assert lay["gst"] == sncol * K
    return np.concatenate([snap[q][:sncol * K].reshape(sncol, K) for q in range(world)], axis=0)


@pytest.mark.gpu
@pytest.mark.parametrize("name,scheme,split,mode", variants(CASES))
def test_trajectory_and_first_gradient_match_the_fp64_oracle(pm, name, scheme, split, mode):
    c = CASES[name]
    Y, A0, S0 = problem(name)
    N, K, W = c["N"], c["K"], len(c["ranges"])
    snap, subs = [], [0]
    with open_world(pm, name, scheme, split, mode) as w:
        pin_kernels(name, mode, w)
        lay = c_layout(w.shards[0])

        def first_collective(what, *handles):
            if not snap:
                assert what == ("reduce_scatter" if split else "all_reduce")
                snap.extend(t.cpu().numpy().copy() for t in handles[0].tensors)
        w.dist.after.append(first_collective)
        more = w.engine.more_subs

        def counting_more_subs(t0, n):
            subs[0] += 1
            more(t0, n)
        w.engine.more_subs = counting_more_subs
        n, drv = w.run(c["its"])
        facs = w.factors()
        fused = w.engine.tail_fused()
        log = list(w.engine.status_log)
    # ---- a. gSt of the first iteration, every entry
    want = first_gradient_point(c, Y, A0, S0)
    gst = assembled_gst(snap, lay, N, K, split, W)
    tol = 2e-5 * np.abs(want).max()
    print("gSt: worst |err| %.3g (atol %.3g)" % (np.abs(gst - want.T).max(), tol))
    np.testing.assert_allclose(gst, want.T, rtol=2e-5, atol=tol)
    # ---- b. the trajectory
    Ao, So, n_ref = oracle_run(name, scheme)
    assert n == n_ref == c["its"]
    for st in log:
        assert len({s[2] for s in st}) == 1
    for A_r, S_r in facs[1:]:
        np.testing.assert_array_equal(S_r, facs[0][1])     # replicated S (S-split: after the gather) is bit-identical on all ranks
    if c.get("unity"):
        # prox_unity_plus: the proximal loop of S takes more than two passes -- decided on the device by the fused tail, else
        # continued through more_subs on all three ranks
        assert max(s[3][1] for st in log for s in st) > 2
        assert fused or subs[0] > 0
    smooth = is_smooth(c, scheme)
    for r, ((r0, r1), (A_r, S_r)) in enumerate(zip(c["ranges"], facs)):
        assert A_r.shape == (r1 - r0, K)
        parity(A_r, Ao[r0:r1], smooth, mode == "f32", "A rows of rank %d" % r)
        parity(S_r, So, smooth, mode == "f32", "S on rank %d" % r)


@pytest.mark.gpu
def test_proximal_passes_continue_through_more_subs_on_three_ranks(pm, monkeypatch):
    """ada_unity_w3 with the tail as a chain of kernels (PMX_TAIL_FUSED=0, read by pmx_adaprox_begin): the two passes enqueued
    with an iteration do not finish prox_unity_plus, every rank halts with HALT_NEED_SUB in the same iteration and the driver
    continues it through pmx_adaprox_more_subs on all three (the fused tail above decides its passes on the device)."""
    monkeypatch.setenv("PMX_TAIL_FUSED", "0")
    name, scheme = "ada_unity_w3", "amsgrad"
    c = CASES[name]
    calls = []
    with open_world(pm, name, scheme, False, "f32") as w:
        assert not any(i["tail_fused"] for i in w.k1_infos())
        more = w.engine.more_subs

        def counting_more_subs(t0, n):
            calls.append((t0, n))
            more(t0, n)
        w.engine.more_subs = counting_more_subs
        n, drv = w.run(c["its"])
        facs = w.factors()
        log = list(w.engine.status_log)
    assert calls, "no iteration ran out of proximal passes: more_subs was never driven"
    assert any(s[0] == 1 and s[1] == 2 for st in log for s in st)              # HALT_NEED_SUB was read ...
    assert all(len({s[:3] for s in st}) == 1 for st in log)                   # ... by all three ranks in the same iteration
    Ao, So, n_ref = oracle_run(name, scheme)
    assert n == n_ref == c["its"]
    for r, ((r0, r1), (A_r, S_r)) in enumerate(zip(c["ranges"], facs)):
        np.testing.assert_array_equal(S_r, facs[0][1])
        parity(A_r, Ao[r0:r1], False, True, "A rows of rank %d" % r)
        parity(S_r, So, False, True, "S on rank %d" % r)


def integer_problem(c, seed):
    """entries 0..3 in A and S, integer Y: every product, every local sum and every sum over ranks is exact in fp32.  bsdmm packs
    the Gram matrix of the A it has just UPDATED: with Y = A S exactly its gradient is zero and the A step is the identity."""
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 4, (c["M"], c["K"])).astype(np.float32)
    S = rng.integers(0, 4, (c["K"], c["N"])).astype(np.float32)
    Y = (A.astype(np.float64) @ S.astype(np.float64))
    if c["alg"] != "bsdmm":
        Y = Y + rng.integers(-3, 4, Y.shape)
    assert np.abs(Y).max() < 2 ** 24 and (Y == np.round(Y)).all()
    return Y.astype(np.float32), A, S


def int_variants():
    out = []
    for name, c in CASES.items():
        for split in c["splits"]:
            for mode in modes_of(c):
                out.append(pytest.param(name, split, mode, id="-".join([name, "split" if split else "repl", mode])))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,split,mode", int_variants())
def test_small_sums_of_the_comm_buffer_are_exact_on_integers(pm, name, split, mode):
    c = CASES[name]
    M, N, K, W = c["M"], c["N"], c["K"], len(c["ranges"])
    Y, A0, S0 = integer_problem(c, 1000 + M + K)
    G = A0.astype(np.float64).T @ A0.astype(np.float64)
    csA, csS = A0.astype(np.float64).sum(0), S0.astype(np.float64).sum(1)
    assert max(G.max(), csA.max(), csS.max()) < 2 ** 24
    scheme = c.get("schemes", (None,))[0]
    ada = c["alg"] == "adaprox"
    with open_world(pm, name, scheme, split, mode, data=(Y, A0, S0)) as w:
        lay = c_layout(w.shards[0])
        KP = w.shards[0].layout.KP
        assert lay["colsum_A"] - lay["gram"] == KP * KP
        drv = w.driver()
        args = (0.9, 0.9, 0) if ada else ()
        w.engine.phase(0, 0, *args)
        drv._allreduce()
        bufs = [t.cpu().numpy().copy() for t in (w.engine.comm_out if split else w.engine.comm).tensors]
        steps = None
        if c["alg"] == "pgm":
            w.engine.phase(1, 0)
            steps = [tuple(r.steps) for r in w.results()]
    small = [b[lay["gram"]:lay["scalars"]] for b in bufs]
    for q in range(1, W):
        assert np.array_equal(small[q], small[0]), "rank %d holds other small sums than rank 0" % q      # (S-split: every chunk carries them)
    ex = bufs[0]
    gram = ex[lay["gram"]:lay["colsum_A"]].reshape(KP, KP)
    if ada:
        assert not gram.any()                   # the layout's Gram section is unused by adaprox: zeros
        colA = ex[lay["colsum_A"]:lay["colsum_A"] + 128]
        assert np.array_equal(colA[:K], csA) and not colA[K:].any()
        if split:
            colS = ex[lay["colsum_S"]:lay["colsum_S"] + 128]
            assert np.array_equal(colS[:K], csS) and not colS[K:].any()
    else:
        assert np.array_equal(gram[:K, :K], G)
        assert not gram[K:].any() and not gram[:, K:].any()
    assert ex[lay["scalars"] + 31] == 0         # the collective halt flag: no rank is halted
    if steps is not None:
        scale = 0.5 if c.get("accelerated") else 1.0
        want = tuple(scale * s for s in orc.lipschitz_steps(A0.astype(np.float64), S0.astype(np.float64)))
        for r, st in enumerate(steps):
            assert st == steps[0], "rank %d derived other steps than rank 0: %r vs %r" % (r, st, steps[0])
        for j in range(2):
            e = abs(steps[0][j] / want[j] - 1.0)
            print("step[%d] %.9g, fp64 %.9g: off by %.3g (allowed %.3g)" % (j, steps[0][j], want[j], e, ACCEPT))
            assert e <= ACCEPT


@pytest.mark.gpu
def test_s_split_is_refused_where_the_ranks_do_not_divide_n(pm):
    with pytest.raises(NotImplementedError, match="divisible"):
        open_world(pm, "pgm_w3", None, True, "f32")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(STOPPING))
def test_lockstep_run_stops_at_the_oracles_iteration(pm, name):
    """check_convergence with a loose e_rel: the oracle stops before max_iter (and does so at the same iteration for an e_rel 0.1 %
    either side: tests/test_lockstep_world_cpu.py), every rank stops there -- the deferred test and, where the stop falls on the
    last iteration of a chunk, _flush."""
    c = STOPPING[name]
    scheme = c.get("schemes", (None,))[0]
    split = c["splits"][0]
    Ao, So, n_ref = oracle_run(name, scheme)
    assert n_ref < c["its"]
    with open_world(pm, name, scheme, split, "f32") as w:
        n, drv = w.run(c["its"])
        facs = w.factors()
        res = w.results()
        log = list(w.engine.status_log)
    assert n == n_ref and drv.stopped
    for r in res:
        assert tuple(r.converged) == (1, 1)
    assert all(s[2] == st[0][2] for st in log for s in st)
    for r, ((r0, r1), (A_r, S_r)) in enumerate(zip(c["ranges"], facs)):
        np.testing.assert_array_equal(S_r, facs[0][1])
        parity(A_r, Ao[r0:r1], is_smooth(c, scheme), True, "A rows of rank %d" % r)      # (mode f32)
        parity(S_r, So, is_smooth(c, scheme), True, "S on rank %d" % r)


@pytest.mark.gpu
def test_one_refused_rank_among_four(pm):
    """Mode f16x2: rank 2's rows of A start 1e5 x above the data, its first K1 launch is refused by the fp16 range guard (which
    writes nothing) and it goes on in exact fp32; ranks 0, 1 and 3 -- whose rows are ordinary -- are stopped at the same
    iteration through the collective halt flag (four addends), repeat it and stay on the fp16 kernel."""
    c = REFUSED
    name, scheme = "ada_refused_w4", "adam"
    with open_world(pm, name, scheme, False, "f16x2") as w:
        before = w.k1_infos()
        n, drv = w.run(c["its"])
        after = w.k1_infos()
        facs = w.factors()
        log = list(w.engine.status_log)
    assert [i["kernel"] for i in before] == ["k_grad_f16_v8"] * 4
    assert [i["range_faults"] for i in after] == [0, 0, 1, 0]
    assert [i["kernel"] for i in after] == ["k_grad_f16_v8", "k_grad_f16_v8", "k_grad_f32_pc", "k_grad_f16_v8"]
    assert log and all(len({s[2] for s in st}) == 1 for st in log)          # the same it_done on every rank, at every reading
    assert log[0][2][1] == 4 and {log[0][r][1] for r in (0, 1, 3)} == {5}   # HALT_RETRY where it was refused, HALT_PEER elsewhere
    Ao, So, n_ref = oracle_run(name, scheme)
    assert n == n_ref == c["its"]
    for r, ((r0, r1), (A_r, S_r)) in enumerate(zip(c["ranges"], facs)):
        np.testing.assert_array_equal(S_r, facs[0][1])
        parity(A_r, Ao[r0:r1], True, False, "A rows of rank %d" % r)
        parity(S_r, So, True, False, "S on rank %d" % r)
