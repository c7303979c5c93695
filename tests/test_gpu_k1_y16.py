"""GPU: K1 at K = 64 in mode f16x2r fetches Y sixteen bytes per lane (k_grad_f16_v8<.., HH, .., Y16>) where Y's pitch is a multiple of
four floats and its base 16-byte aligned, and eight bytes per lane (the instances without Y16) everywhere else and under PMX_K1_Y16=0.

The two fetches put every Y value into the subtraction it always went into, so everything K1 writes must be BITWISE the same with either,
and both stay within K1's tolerance of the fp64 oracle (tests/test_gpu_frame.py::_check_grad: rtol 2e-5, atol 2e-5 max|g|).  Shapes:
128 x 256 (one workgroup, one panel: the producers' prefetch runs past the region's end and is clamped), 384 x 512 (three panels, two
column regions: the clamp on an odd panel count), 4096 x 4096 (the chained instance the benchmark runs)."""
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
def eight_byte_fetch():
    """PMX_K1_Y16=0 (read at every K1 launch): the instances that fetch Y eight bytes per lane"""
    assert "PMX_K1_Y16" not in os.environ
    os.environ["PMX_K1_Y16"] = "0"
    try:
        yield
    finally:
        del os.environ["PMX_K1_Y16"]


def _close_to_oracle(g, ref):
    for got, want in zip(g, ref):
        assert got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-5 * np.abs(want).max())


def _same_bits(g, h):
    assert np.array_equal(g[0], h[0]) and np.array_equal(g[1], h[1])


@pytest.mark.parametrize("M,N", SHAPES)
def test_gradients_bitwise_equal_to_the_8_byte_fetch(eng, problems, M, N):
    Y, factors, refs = problems[(M, N)]
    with eng.DeviceNMF(M, N, K, mode=MODE) as dev:
        info = dev.k1_info()
        assert info["kernel"] == "k_grad_f16_v8_hh" and info["frame"] == (M, N), info
        if (M, N) == (4096, 4096):
            assert info["chain"] > 0, info            # the headline's chained instance
        dev.set_Y(Y)
        for (A, S), ref in zip(factors, refs):        # the second pair: other factors in the same context
            dev.set_factors(A, S)
            g16 = dev.grad()
            with eight_byte_fetch():
                g8 = dev.grad()
            _same_bits(g16, g8)
            _close_to_oracle(g16, ref)
            _same_bits(dev.grad(), g16)               # and back again
        assert dev.k1_info()["kernel"] == "k_grad_f16_v8_hh" and dev.k1_info()["chain_faults"] == 0, dev.k1_info()


@pytest.mark.parametrize("pad,shift", [(4, 0), (2, 0), (4, 2)], ids=["ld=N+4", "ld=N+2:8-byte", "ld=N+4,base+2:8-byte"])
def test_device_y_pitch_and_alignment(eng, problems, pad, shift):
    """A device Y adopted in place: pitch N + 4 keeps the 16-byte fetch, pitch N + 2 or a base two floats off must fall back to 8 bytes."""
    import torch
    M, N = 384, 512
    Y, factors, refs = problems[(M, N)]
    (A, S), ref = factors[0], refs[0]
    with eng.DeviceNMF(M, N, K, mode=MODE) as dev:
        dev.set_Y(Y)
        dev.set_factors(A, S)
        g0 = dev.grad()
    _close_to_oracle(g0, ref)
    ld = N + pad
    flat = torch.full((M * ld + 8,), 7.0, dtype=torch.float32, device="cuda:0")      # (garbage between and behind the rows: must not be used)
    assert flat.data_ptr() % 16 == 0
    view = flat[shift:shift + M * ld].view(M, ld)
    view[:, :N] = torch.from_numpy(Y.copy()).to("cuda:0")
    torch.cuda.synchronize()
    assert view.data_ptr() % 16 == 4 * shift
    with eng.DeviceNMF(M, N, K, mode=MODE) as dev:
        dev.set_Y_device(view.data_ptr(), ld=ld, copy=False, keepalive=flat)
        dev.set_factors(A, S)
        g = dev.grad()
        assert dev.k1_info()["kernel"] == "k_grad_f16_v8_hh", dev.k1_info()
        with eight_byte_fetch():
            g8 = dev.grad()
    _same_bits(g, g0)
    _same_bits(g8, g0)
    _close_to_oracle(g, ref)


def _run_adaprox(eng, Y, A, S):
    from proxmin_amd import operators as ops
    M, N = Y.shape
    with eng.DeviceNMF(M, N, K, mode=MODE) as dev:
        dev.set_Y(Y)
        dev.set_factors(A, S)
        pA = ops.device_proxseq(ops.prox_plus, 0)
        pS = ops.device_proxseq(partial(ops.prox_unity_plus, axis=0), 1)
        dev.adaprox_begin([pA, pS], scheme="amsgrad", check_convergence=False, prox_max_iter=1000, e_rel=(1e-3, 1e-3))
        dev.adaprox_run(np.full(3, 0.9), 0.9)
        assert dev.k1_info()["kernel"] == "k_grad_f16_v8_hh", dev.k1_info()
        return dev.get_factors()


def _run_bsdmm(eng, Y, A, S):
    from proxmin_amd import operators as ops
    M, N = Y.shape
    with eng.DeviceNMF(M, N, K, mode=MODE) as dev:
        dev.set_Y(Y)
        dev.set_factors(A, S)
        pA = ops.device_proxseq(ops.prox_plus, 0)
        pS = ops.device_proxseq(ops.prox_plus, 1)
        pg = [ops.device_proxseq(ops.prox_plus, 0), ops.device_proxseq(partial(ops.prox_soft, thresh=1e-3), 0)]
        dev.bsdmm_begin([pA, pS], [pg, pg], e_rel=(1e-12, 1e-12), e_abs=(0.0, 0.0))
        dev.bsdmm_run(3)                              # one-gradient passes: the row split's instance for gA, <ONLYS> for gSt
        assert dev.k1_info()["kernel"] == "k_grad_f16_v8_hh", dev.k1_info()
        return dev.get_factors()


@pytest.mark.parametrize("run", [_run_adaprox, _run_bsdmm], ids=["adaprox", "bsdmm"])
def test_solver_factors_bitwise_equal_to_the_8_byte_fetch(eng, problems, run):
    Y, factors, _ = problems[(384, 512)]
    A, S = factors[0]
    f16 = run(eng, Y, A, S)
    with eight_byte_fetch():
        f8 = run(eng, Y, A, S)
    assert np.isfinite(f16[0]).all() and np.isfinite(f16[1]).all()
    assert not np.array_equal(f16[0], A) and not np.array_equal(f16[1], S)           # (the iterations ran)
    _same_bits(f16, f8)
