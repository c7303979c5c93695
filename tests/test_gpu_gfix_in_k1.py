"""GPU: mode f16x2r at K1's K = 64 -- the K x K correction of the high x high residual (k_gfix.hip) rides on K1's own idle waves
(k_grad_f16_v8<.., HH, RS, .., GF>: gram shares on the consumers before their first block, reduce shares on the producers behind their
last, the apply tasks on all eight waves at the end) wherever a pass wants both gradients, and runs as the three stand-alone launches
(k_gfix_gram / _reduce / _apply) everywhere else and under PMX_K1_GFIX=0.

Both run the same device code in the same order (k_gfix_dev.h), so everything a pass writes must be BITWISE the same either way, and both
stay within K1's tolerance of the fp64 oracle (tests/test_gpu_frame.py::_check_grad: rtol 2e-5, atol 2e-5 max|g|).  DeviceNMF.gfix_info()
says who formed the correction.  Shapes: 128 x 256 (ONE workgroup loops over all 256 gram shares, all 256 reduce shares and the apply
tasks of both blocks), 384 x 512 (three panels, two column regions: six workgroups, odd panel count), 4096 x 4096 (the chained instance
the benchmark runs, 256 workgroups: one share of each stage per workgroup).

K1's planner gives every row region at least one panel (gridX = ceil(panels / RP)) and the frame's columns are whole regions, so no shape
reaches the host's "a region of the plan is empty" exclusion; the ragged case below checks the ride on a zero-padded frame instead
(the stages see the factors' own row counts, K1 the frame's)."""
import os
from contextlib import contextmanager
from functools import partial

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 64
MODE = "f16x2r"
SHAPES = [(128, 256), (384, 512), (4096, 4096)]


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as g
    g.build()
    from proxmin_amd import engine
    return engine


@pytest.fixture(scope="module")
def orc():
    from oracle import nmf_oracle
    return nmf_oracle


@pytest.fixture(scope="module")
def problems(orc):
    """(M, N) -> Y, two sets of factors and their fp64 gradients: computed once, shared, never written to"""
    out = {}
    for (M, N) in SHAPES:
        Y, A, S = orc.synthetic_problem(M, N, K, np.float32, seed=M + N)
        A2 = (A * 3.0 + 0.25).astype(np.float32)
        S2 = (S * 0.5 + 0.125).astype(np.float32)
        Y64 = Y.astype(np.float64)
        refs = [orc.residual_gradients(a.astype(np.float64), s.astype(np.float64), Y64) for (a, s) in ((A, S), (A2, S2))]
        for x in (Y, A, S, A2, S2) + tuple(refs[0]) + tuple(refs[1]):
            x.setflags(write=False)
        out[(M, N)] = (Y, ((A, S), (A2, S2)), refs)
    return out


@contextmanager
def env(name, value):
    assert name not in os.environ
    os.environ[name] = value
    try:
        yield
    finally:
        del os.environ[name]


def stand_alone_launches():
    """PMX_K1_GFIX=0 (read at every K1 launch): the three correction launches behind K1"""
    return env("PMX_K1_GFIX", "0")


def _close_to_oracle(g, ref):
    for got, want in zip(g, ref):
        assert got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-5 * np.abs(want).max())


def _same_bits(g, h):
    assert np.array_equal(g[0], h[0]) and np.array_equal(g[1], h[1])


def _counted(dev, what, n=1):
    """run the block, then: exactly n more corrections of kind `what` ("in_k1" / "launches"), none of the other kind, no fault"""
    @contextmanager
    def cm():
        before = dev.gfix_info()
        yield
        after = dev.gfix_info()
        other = "launches" if what == "in_k1" else "in_k1"
        assert after[what] - before[what] == n and after[other] == before[other], (what, before, after)
        assert after["faults"] == before["faults"] and after["fell_back"] == before["fell_back"], (before, after)
    return cm()


@pytest.mark.parametrize("M,N", SHAPES)
def test_gradients_bitwise_equal_to_the_stand_alone_launches(eng, problems, M, N):
    Y, factors, refs = problems[(M, N)]
    with eng.DeviceNMF(M, N, K, mode=MODE) as dev:
        info = dev.k1_info()
        assert info["kernel"] == "k_grad_f16_v8_hh" and info["frame"] == (M, N), info
        if (M, N) == (4096, 4096):
            assert info["chain"] > 0, info            # the headline's chained instance
        if (M, N) == (128, 256):
            assert info["row_regions"] * info["col_regions"] == 1, info
        dev.set_Y(Y)
        for (A, S), ref in zip(factors, refs):        # the second pair: other factors in the same context
            dev.set_factors(A, S)
            with _counted(dev, "in_k1"):
                g1 = dev.grad()
            with stand_alone_launches(), _counted(dev, "launches"):
                g0 = dev.grad()
            _same_bits(g1, g0)
            _close_to_oracle(g1, ref)
            _close_to_oracle(g0, ref)
            with _counted(dev, "in_k1"):
                _same_bits(dev.grad(), g1)            # and back again
        assert dev.k1_info()["kernel"] == "k_grad_f16_v8_hh" and dev.k1_info()["chain_faults"] == 0, dev.k1_info()
        assert not dev.gfix_info()["fell_back"]


def _run_adaprox(eng, Y, A, S, iters=12, Kc=K):
    from proxmin_amd import operators as ops
    M, N = Y.shape
    with eng.DeviceNMF(M, N, Kc, mode=MODE) as dev:
        dev.set_Y(Y)
        dev.set_factors(A, S)
        pA = ops.device_proxseq(ops.prox_plus, 0)
        pS = ops.device_proxseq(partial(ops.prox_unity_plus, axis=0), 1)
        dev.adaprox_begin([pA, pS], scheme="amsgrad", check_convergence=False, prox_max_iter=1000, e_rel=(1e-3, 1e-3))
        dev.adaprox_run(np.full(iters, 0.9), 0.9)
        return dev.get_factors(), dev.k1_info(), dev.gfix_info()


def _run_pgm(eng, Y, A, S, iters=12):
    from proxmin_amd import operators as ops
    M, N = Y.shape
    with eng.DeviceNMF(M, N, K, mode=MODE) as dev:
        dev.set_Y(Y)
        dev.set_factors(A, S)
        pA = ops.device_proxseq(ops.prox_plus, 0)
        pS = ops.device_proxseq(partial(ops.prox_unity_plus, axis=0), 1)
        dev.pgm_begin([pA, pS], e_rel=(1e-12, 1e-12))
        dev.pgm_run(iters)
        return dev.get_factors(), dev.k1_info(), dev.gfix_info()


def _run_bsdmm(eng, Y, A, S, iters=3):
    from proxmin_amd import operators as ops
    M, N = Y.shape
    with eng.DeviceNMF(M, N, K, mode=MODE) as dev:
        dev.set_Y(Y)
        dev.set_factors(A, S)
        pA = ops.device_proxseq(ops.prox_plus, 0)
        pS = ops.device_proxseq(ops.prox_plus, 1)
        pg = [ops.device_proxseq(ops.prox_plus, 0), ops.device_proxseq(partial(ops.prox_soft, thresh=1e-3), 0)]
        dev.bsdmm_begin([pA, pS], [pg, pg], e_rel=(1e-12, 1e-12), e_abs=(0.0, 0.0))
        dev.bsdmm_run(iters)                          # one-gradient passes: the row split's instance for gA, <ONLYS> for gSt
        return dev.get_factors(), dev.k1_info(), dev.gfix_info()


def _ran(f, A, S):
    assert np.isfinite(f[0]).all() and np.isfinite(f[1]).all()
    assert not np.array_equal(f[0], A) and not np.array_equal(f[1], S)


@pytest.mark.parametrize("run,shape", [(_run_adaprox, (384, 512)), (_run_adaprox, (4096, 4096)), (_run_pgm, (384, 512))],
                         ids=["adaprox-384x512", "adaprox-4096x4096", "pgm-384x512"])
def test_solver_factors_bitwise_equal_to_the_stand_alone_launches(eng, problems, run, shape):
    Y, factors, _ = problems[shape]
    A, S = factors[0]
    f1, k1, c1 = run(eng, Y, A, S)
    with stand_alone_launches():
        f0, k0, c0 = run(eng, Y, A, S)
    _ran(f1, A, S)
    _same_bits(f1, f0)
    for k in (k1, k0):
        assert k["kernel"] == "k_grad_f16_v8_hh" and k["chain_faults"] == 0 and k["tail_faults"] == 0, k
    if run is _run_adaprox and shape == (4096, 4096):
        assert k1["tail_fused"] and k0["tail_fused"], (k1, k0)     # the fused tail folds the correction slab K1 left
    assert c1["in_k1"] >= 12 and c1["launches"] == 0 and not c1["fell_back"] and c1["faults"] == 0, c1
    assert c0["launches"] >= 12 and c0["in_k1"] == 0 and not c0["fell_back"], c0


def test_bsdmm_keeps_the_launches(eng, problems):
    """one gradient per pass: nothing rides, and the switch changes nothing"""
    Y, factors, _ = problems[(384, 512)]
    A, S = factors[0]
    f1, k1, c1 = _run_bsdmm(eng, Y, A, S)
    with stand_alone_launches():
        f0, k0, c0 = _run_bsdmm(eng, Y, A, S)
    _ran(f1, A, S)
    _same_bits(f1, f0)
    assert k1["kernel"] == "k_grad_f16_v8_hh", k1
    assert c1["in_k1"] == 0 and c1["launches"] > 0 and c1 == c0, (c1, c0)


def test_K_48_on_the_K_64_frame(eng, orc):
    """K1 runs K = 64 on zero-padded copies of the factors: the stages read the copies K1 reads"""
    M, N, Kc = 384, 512, 48
    Y, A, S = orc.synthetic_problem(M, N, Kc, np.float32, seed=48)
    rA, rS = orc.residual_gradients(A.astype(np.float64), S.astype(np.float64), Y.astype(np.float64))
    with eng.DeviceNMF(M, N, Kc, mode=MODE) as dev:
        info = dev.k1_info()
        assert info["kernel"] == "k_grad_f16_v8_hh" and info["frame_K"] == 64, info
        dev.set_Y(Y)
        dev.set_factors(A, S)
        with _counted(dev, "in_k1"):
            g1 = dev.grad()
        with stand_alone_launches(), _counted(dev, "launches"):
            g0 = dev.grad()
    _same_bits(g1, g0)
    _close_to_oracle(g1, (rA, rS))


def test_ragged_shape_on_a_frame(eng, orc):
    """1000 x 1500 on its zero-padded frame (1024 x 1536): the stages guard the factors' own rows (1000 / 1500: a gram share and an apply
    task end inside a tile), K1 the frame's.  Whichever path the host takes, the result is the stand-alone launches'."""
    M, N = 1000, 1500
    Y, A, S = orc.synthetic_problem(M, N, K, np.float32, seed=5)
    rA, rS = orc.residual_gradients(A.astype(np.float64), S.astype(np.float64), Y.astype(np.float64))
    with eng.DeviceNMF(M, N, K, mode=MODE) as dev:
        info = dev.k1_info()
        assert info["kernel"] == "k_grad_f16_v8_hh" and info["frame"] != (M, N) and info["frame"][0] % 128 == 0, info
        dev.set_Y(Y)
        dev.set_factors(A, S)
        before = dev.gfix_info()
        g1 = dev.grad()
        after = dev.gfix_info()
        # every region of a plan holds a panel (module docstring), so the pass carries the correction
        assert (info["row_regions"] - 1) * info["panels_per_region"] * 128 < info["frame"][0], info
        assert (after["launches"] - before["launches"], after["in_k1"] - before["in_k1"]) == (0, 1), (info, before, after)
        with stand_alone_launches(), _counted(dev, "launches"):
            g0 = dev.grad()
    _same_bits(g1, g0)
    _close_to_oracle(g1, (rA, rS))


def test_forty_passes_in_one_context(eng, problems):
    """the arrival words carry the launch's number: a base that is off by one launch shows as a stale or a missing correction"""
    M, N = 384, 512
    Y, factors, _ = problems[(M, N)]
    A, S = factors[0]
    with eng.DeviceNMF(M, N, K, mode=MODE) as dev:
        dev.set_Y(Y)
        with _counted(dev, "in_k1", 40):
            for i in range(40):
                Ai = (A * (1.0 + 0.03 * i) + 0.001 * i).astype(np.float32)
                Si = (S * (1.0 - 0.01 * i)).astype(np.float32)
                dev.set_factors(Ai, Si)
                g = dev.grad()
        with stand_alone_launches(), _counted(dev, "launches"):
            g0 = dev.grad()
    _same_bits(g, g0)


def test_reported_fault_repeats_the_pass_with_the_launches(eng, problems):
    """PMX_INJECT_GFIX_FAULT=2 (read when the context is created): the second pass that carries the correction REPORTS the ride's fault
    code -- one workgroup writes the status word and carries on; no wait is lengthened, nothing traps.  The host repeats the pass with the
    stand-alone launches, which the context keeps from then on; gradients are those of an undisturbed context."""
    M, N = 384, 512
    Y, factors, refs = problems[(M, N)]
    (A, S), (A2, S2) = factors
    with eng.DeviceNMF(M, N, K, mode=MODE) as dev:
        dev.set_Y(Y)
        dev.set_factors(A, S)
        want1 = dev.grad()
        dev.set_factors(A2, S2)
        want2 = dev.grad()
    with env("PMX_INJECT_GFIX_FAULT", "2"):
        dev = eng.DeviceNMF(M, N, K, mode=MODE)
    with dev:
        dev.set_Y(Y)
        dev.set_factors(A, S)
        with _counted(dev, "in_k1"):
            g1 = dev.grad()
        dev.set_factors(A2, S2)
        g2 = dev.grad()                               # carried, reported, repeated
        c = dev.gfix_info()
        assert c == {"in_k1": 2, "launches": 1, "fell_back": True, "faults": 1}, c
        g3 = dev.grad()                               # stays on the launches
        c = dev.gfix_info()
        assert c == {"in_k1": 2, "launches": 2, "fell_back": True, "faults": 1}, c
        assert dev.k1_info()["kernel"] == "k_grad_f16_v8_hh" and dev.k1_info()["chain_faults"] == 0, dev.k1_info()
    _same_bits(g1, want1)
    _same_bits(g2, want2)
    _same_bits(g3, want2)
    _close_to_oracle(g2, refs[1])


def test_reported_fault_inside_a_solver_run(eng, problems):
    """the same report from the fifth iteration of an adaprox run: the iteration is repeated from the factors it started with, the run ends
    on the factors of an undisturbed one"""
    Y, factors, _ = problems[(384, 512)]
    A, S = factors[0]
    f1, k1, c1 = _run_adaprox(eng, Y, A, S)
    with env("PMX_INJECT_GFIX_FAULT", "5"):
        f2, k2, c2 = _run_adaprox(eng, Y, A, S)
    _same_bits(f1, f2)
    # (iterations are enqueued ahead of the status read: the launches behind the fifth carried the correction too and were skipped on the device)
    assert c2["fell_back"] and c2["faults"] == 1 and 5 <= c2["in_k1"] <= 12 and c2["launches"] >= 8, c2
    assert k2["chain_faults"] == 0 and k2["tail_faults"] == 0, k2
