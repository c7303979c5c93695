"""CPU: the lockstep harness of tests/lockstep_world.py proven without a GPU, and the precondition of the GPU cases.

1. The NumPy stand-in engines of tests/test_distributed_cpu.py (adaprox replicated and S-split, pgm / FISTA, bsdmm) behind ONE
   LockstepEngine and ONE LockstepDist, driven by the product's ShardedAdaproxDriver / ShardedLoop at world 3 and 8 with even and
   unequal row ranges (one-row ranks included): the result equals the unsharded fp64 oracle to what that file asserts at world 2.
2. For every case of tests/test_gpu_sharded_lockstep.py: the oracle run on float32 arrays against the oracle on float64 meets the
   caps the device is held to, with room to spare -- a case whose float32 ORACLE cannot stay inside them says nothing about a
   kernel.  Room to spare, from the caps themselves: in every case a share of 0.9999 within the bound (the smooth cap, also for
   amsgrad) and a worst entry at a tenth of the smooth envelope, 5 x; every entry within the bound where a smooth back-end runs
   in mode f32 (the device's cap there).
   The stopping cases stop at the same iteration with e_rel 0.1 % either side (0.2 % of the test's ratio: a hundred times what float32
   factors can move it), in float32 as in float64."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import nmf_oracle as orc  # noqa: E402
from proxmin_amd.distributed import ShardedAdaproxDriver, ShardedLoop, shard_rows  # noqa: E402
from lockstep_world import LockstepDist, LockstepEngine, PerRank  # noqa: E402
import test_distributed_cpu as w2  # noqa: E402
import test_gpu_sharded_lockstep as gl  # noqa: E402


def row_ranges(M, world, how):
    if how == "even":
        return shard_rows(M, world)
    # unequal: one-row ranks between larger ones, the last rank takes the rest
    sizes = {3: [M // 2, 1], 8: [1, 2, 1, 3, 1, 2, 1]}[world]
    edges = np.concatenate([[0], np.cumsum(sizes), [M]])
    assert edges[-2] < M
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


def _n96(case):
    """the world-2 S-split cases with N = 96, which 3 and 8 divide"""
    return (case[0], case[1], 96) + tuple(case[3:])


ADA_CASES = [c if c[0] != "split" else _n96(c) for c in w2.CASES]


@pytest.mark.parametrize("how", ["even", "unequal"])
@pytest.mark.parametrize("world", [3, 8])
@pytest.mark.parametrize("case", ADA_CASES, ids=lambda c: "-".join(str(x) for x in c[:4]))
def test_lockstep_adaprox_standins_match_unsharded_oracle(case, world, how):
    split = case[0] == "split"
    M, N, K, unity, scheme, pS, check, e_rel, its = case[1:] if split else case
    Y, A0, S0 = orc.synthetic_problem(M, N, K, np.float64, unity_S=unity, seed=3)
    ranges = row_ranges(M, world, how)
    shards = [(A0[r0:r1].copy(), S0.copy()) for r0, r1 in ranges]
    if split:
        engines = [w2.NumpySplitShardEngine(r, world, Y[r0:r1], A_l, S, M, ("plus",), pS, scheme, check, e_rel) for r, ((r0, r1), (A_l, S)) in enumerate(zip(ranges, shards))]
    else:
        engines = [w2.NumpyShardEngine(Y[r0:r1], A_l, S, M, ("plus",), pS, scheme, check, e_rel) for (r0, r1), (A_l, S) in zip(ranges, shards)]
    eng = LockstepEngine(engines)
    assert eng.s_split == split
    drv = ShardedAdaproxDriver(eng, None, check, True, 1000, chunk=3, dist_module=LockstepDist(world))
    n = drv.run(its, np.full(its, 0.9))
    Ao, So = A0.copy(), S0.copy()
    conv, _, _, _, n_ref, _ = orc.adaprox_nmf(Y, Ao, So, ("plus",), pS, scheme=scheme, max_iter=its, e_rel=e_rel, check_convergence=check)
    assert n == n_ref
    if check:
        assert drv.stopped == all(conv)
    S_ranks = [np.ascontiguousarray(e.St.T) if split else e.S for e in engines]
    for S in S_ranks:
        np.testing.assert_allclose(S, So, rtol=1e-9, atol=1e-12)
        np.testing.assert_array_equal(S, S_ranks[0])                      # bitwise identical replicas
    np.testing.assert_allclose(np.concatenate([a for a, _ in shards]), Ao, rtol=1e-9, atol=1e-12)
    assert all(len({s[:3] for s in st}) == 1 for st in eng.status_log)


@pytest.mark.parametrize("how", ["even", "unequal"])
@pytest.mark.parametrize("world", [3, 8])
@pytest.mark.parametrize("case", w2.PB_CASES, ids=lambda c: "-".join(str(x) for x in c[:5]))
def test_lockstep_pgm_bsdmm_standins_match_unsharded_oracle(case, world, how):
    alg, M, N, K, opt, e_rel, its = case
    Y, A0, S0 = orc.synthetic_problem(M, N, K, np.float64, seed=3)
    ranges = row_ranges(M, world, how)
    shards = [(A0[r0:r1].copy(), S0.copy()) for r0, r1 in ranges]
    make = w2.NumpyPgmShardEngine if alg == "pgm" else w2.NumpyBsdmmShardEngine
    engines = [make(Y[r0:r1], A_l, S, M, opt, e_rel) for (r0, r1), (A_l, S) in zip(ranges, shards)]
    loop = ShardedLoop(LockstepEngine(engines), None, deferred_test=(alg == "pgm"), chunk=3, dist_module=LockstepDist(world))
    n = loop.run(its)
    Ao, So = A0.copy(), S0.copy()
    if alg == "pgm":
        conv, _, _, n_ref = orc.pgm_nmf(Y, Ao, So, accelerated=opt, max_iter=its, e_rel=e_rel)
    else:
        conv, n_ref = orc.bsdmm_nmf(Y, Ao, So, proxs_g=[[("plus",), ("soft", opt, "relative")]] * 2, max_iter=its, e_rel=e_rel)
    assert n == n_ref, (n, n_ref)
    assert loop.stopped == all(conv)
    for _, S in shards:
        np.testing.assert_allclose(S, So, rtol=1e-8, atol=1e-11)
        np.testing.assert_array_equal(S, shards[0][1])
    np.testing.assert_allclose(np.concatenate([a for a, _ in shards]), Ao, rtol=1e-8, atol=1e-11)


def test_the_early_stopping_standin_cases_do_stop_early():
    """(otherwise the deferred test and _flush above would go unexercised)"""
    for case in ADA_CASES:
        c = case[1:] if case[0] == "split" else case
        if c[7] > 1e-3:
            Y, A, S = orc.synthetic_problem(c[0], c[1], c[2], np.float64, unity_S=c[3], seed=3)
            assert orc.adaprox_nmf(Y, A, S, ("plus",), c[5], scheme=c[4], max_iter=c[8], e_rel=c[7], check_convergence=True)[4] < c[8]


def test_lockstep_collectives_on_known_numbers():
    """three ranks, chunks of two: every collective against sums worked out by hand; chunk 2 is reduced like chunk 0"""
    import torch
    W = 3
    d = LockstepDist(W)
    seen = []
    d.after.append(lambda name, *h: seen.append(name))
    bufs = [torch.arange(6, dtype=torch.float32) + 10.0 * r for r in range(W)]             # rank r: 10 r + (0 .. 5)
    outs = [torch.zeros(2) for _ in range(W)]
    d.reduce_scatter_tensor(PerRank(outs), PerRank(bufs))
    for q in range(W):
        assert outs[q].tolist() == [30.0 + 3 * (2 * q), 30.0 + 3 * (2 * q + 1)]
    full = [torch.full((6,), -1.0) for _ in range(W)]
    for q in range(W):
        full[q][2 * q:2 * q + 2] = torch.tensor([q + 0.5, q + 0.75])
    d.all_gather_into_tensor(PerRank(full))
    for r in range(W):
        assert full[r].tolist() == [0.5, 0.75, 1.5, 1.75, 2.5, 2.75]
    d.all_reduce(PerRank(bufs))
    for r in range(W):
        assert bufs[r].tolist() == [30.0 + 3 * i for i in range(6)]
    # fp32, rank order: (1 + 2^-24) + 2^-24 rounds to 1 twice, 2^-24 + 2^-24 + 1 does not
    a = [torch.tensor([1.0]), torch.tensor([2.0 ** -24]), torch.tensor([2.0 ** -24])]
    d.all_reduce(PerRank(a))
    assert a[0].item() == 1.0
    b = [torch.tensor([2.0 ** -24]), torch.tensor([2.0 ** -24]), torch.tensor([1.0])]
    d.all_reduce(PerRank(b))
    assert b[0].item() == 1.0 + 2.0 ** -23
    assert seen == ["reduce_scatter", "all_gather", "all_reduce", "all_reduce", "all_reduce"]


def test_lockstep_engine_insists_on_agreement():
    class Fake:
        def __init__(self, st):
            self.st = st

        def chain_status(self):
            return self.st
    ok = LockstepEngine([Fake((1, 4, 2, (2, 3))), Fake((1, 5, 2, (2, 7))), Fake((1, 5, 2, (4, 1)))])     # HALT_RETRY on one rank, HALT_PEER on its peers
    assert ok.chain_status() == (1, 4, 2, (4, 7))
    for bad in ((1, 5, 3, (0, 0)), (0, 0, 2, (0, 0)), (1, 1, 2, (0, 0))):
        with pytest.raises(AssertionError):
            LockstepEngine([Fake((1, 5, 2, (0, 0))), Fake(bad)]).chain_status()


# ---- 2. the precondition of the GPU cases ---------------------------------------------------------------------------------
def _scheme_variants():
    return [(name, scheme) for name, c in gl.ALL_CASES.items() for scheme in c.get("schemes", (None,))]


@pytest.mark.parametrize("name,scheme", _scheme_variants(), ids=lambda v: str(v))
def test_float32_oracle_meets_the_caps_with_room_to_spare(name, scheme):
    c = gl.ALL_CASES[name]
    A64, S64, n64 = gl.oracle_run(name, scheme)
    A32, S32, n32 = gl.oracle_run(name, scheme, "float32")
    assert A32.dtype == np.float32 and n32 == n64
    smooth = gl.is_smooth(c, scheme)
    for got, want, what in ((A32, A64, "A"), (S32, S64, "S")):
        ratio = np.abs(got.astype(np.float64) - want) / (gl.BOUND_ATOL + gl.BOUND_RTOL * np.abs(want))
        worst, share = float(ratio.max()), float((ratio <= 1.0).mean())
        print("%s %s %s: float32 oracle worst %.3f x the bound, %.6f within" % (name, scheme, what, worst, share))
        assert share >= 0.9999 and worst <= 5.0
        if smooth and "f32" in gl.modes_of(c):       # the device's cap there: every entry within the bound
            assert worst <= 1.0


@pytest.mark.parametrize("name", sorted(gl.STOPPING))
def test_stopping_cases_stop_early_and_not_on_the_edge(name):
    c = gl.STOPPING[name]
    scheme = c.get("schemes", (None,))[0]
    n = gl.oracle_run(name, scheme)[2]
    assert 2 <= n < c["its"]
    for dtype in ("float64", "float32"):
        for e_scale in (0.999, 1.0, 1.001):
            assert gl.oracle_run(name, scheme, dtype, e_scale)[2] == n, (dtype, e_scale)


def test_cases_are_what_the_issue_lists():
    rows = {name: [b - a for a, b in c["ranges"]] for name, c in gl.ALL_CASES.items()}
    assert rows["ada_k64_w8"] == [128] * 8 and rows["ada_unequal_w3"] == [256, 5, 1024] and rows["pgm_unequal_w3"] == [300, 5, 1024]
    for name, c in gl.ALL_CASES.items():
        assert sum(rows[name]) == c["M"] and c["ranges"][0][0] == 0
        for split in c["splits"]:
            assert not split or c["N"] % len(c["ranges"]) == 0
    assert gl.CASES["pgm_w3"]["N"] % 3 != 0
    assert {c["N"] // len(c["ranges"]) for c in gl.CASES.values() if True in c["splits"]} >= {160, 175, 375}
    assert set(gl.KERNELS) == set(gl.CASES) and all(set(gl.KERNELS[n]) == set(gl.modes_of(c)) for n, c in gl.CASES.items())
