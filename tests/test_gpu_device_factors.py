"""GPU: A and S that live in HBM (torch tensors) are read and updated there, in place.

The yardstick everywhere is the same call with host (NumPy) factors: it runs the same kernels on the same bits, so every
comparison is exact -- no tolerance.  Group 1 pins the transfer kernel alone (csrc/k_xfer.hip) through the C ABI, bit for bit;
the others the solvers, the helpers and the refusals on top of it."""
import ctypes as C
from functools import partial

import numpy as np
import pytest

import proxmin_amd as pm
from proxmin_amd import _lib
from proxmin_amd.engine import DeviceNMF, as_device_factor
from oracle import nmf_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import __graft_entry__ as g
    g.build()
    import torch as t
    assert t.cuda.is_available()
    return t


# ---- 1. the kernel alone ---------------------------------------------------------------------------
# (rows, K) of a context buffer.  Block 0's view is rows x K, block 1's K x rows (the same two numbers, K <= 128 on the
# component axis): one context with M = N = rows serves both.
XFER_SHAPES = [(1, 1), (5, 3), (33, 7), (63, 64), (65, 64), (130, 100), (257, 128)]
SPECIAL32 = [0x7fc00001, 0xffc12345, 0x7f800001, 0xff8abcde, 0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0x00000000]
SPECIAL64 = [0x7ff8000000000001, 0xfff8123456789abc, 0x7ff0000000000001, 0xfff0000000abcdef, 0x8000000000000000, 0x0000000000000001,
             0x800fffffffffffff, 0x7ff0000000000000, 0x0000000000000000]


def _bits(rng, n, f64):
    """n random bit patterns with NaNs (quiet and signalling, with payloads), -0.0, denormals and infinities planted"""
    ut = np.uint64 if f64 else np.uint32
    b = rng.integers(0, np.iinfo(ut).max, size=n, dtype=ut, endpoint=True)
    sp = np.array(SPECIAL64 if f64 else SPECIAL32, dtype=ut)
    pos = rng.permutation(n)[: min(n, len(sp))]
    b[pos] = sp[: len(pos)]
    return b


def _geometry(shape, colmajor, pad, off):
    """-> (element strides, flat length) of a view of `shape` that starts `off` elements into a flat array, 7 elements behind it"""
    n0, n1 = shape
    st = (1, n0 + pad) if colmajor else (n1 + pad, 1)
    return st, off + (n0 - 1) * st[0] + (n1 - 1) * st[1] + 1 + 7


def _positions(shape, st, off):
    i, j = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    return off + i * st[0] + j * st[1]


def _to_gpu(torch, bits):
    it = np.int64 if bits.dtype == np.uint64 else np.int32
    return torch.from_numpy(bits.view(it).copy()).cuda()


def _view(torch, flat_int, shape, st, off, f64):
    return torch.as_strided(flat_int.view(torch.float64 if f64 else torch.float32), shape, st, off)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("rows,K", XFER_SHAPES)
def test_transfer_kernel_is_bit_exact_and_writes_nothing_else(torch, rows, K, f64):
    """pmx_factor_from_device into BUF_A / BUF_ST against pmx_download; pmx_factor_to_device into a flat tensor full of a
    sentinel pattern: the logical elements arrive, every other element (in front of the view, pitch padding, behind it) keeps
    its bits; in -> out reproduces the source.  Both blocks, row- and column-major, dense and pitch + 3, view offset 0 and 1
    (the base then misaligned for 8- / 16-byte accesses)."""
    rng = np.random.default_rng(rows * 1000 + K + (7 if f64 else 0))
    ut, ft = (np.uint64, np.float64) if f64 else (np.uint32, np.float32)
    with DeviceNMF(rows, rows, K, mode="f64" if f64 else "f32") as dev:
        lib = dev.lib

        def call(fn, buf, view):
            ref = as_device_factor(view)
            _lib.check(fn(dev.h, buf, C.c_void_p(ref.ptr), ref.strides[0], ref.strides[1], int(f64)))

        for block, buf in ((0, _lib.BUF_A), (1, _lib.BUF_ST)):
            shape = (rows, K) if block == 0 else (K, rows)
            for colmajor in (False, True):
                for pad in (0, 3):
                    for off in (0, 1):
                        what = "block %d %s pad %d off %d" % (block, "col-major" if colmajor else "row-major", pad, off)
                        st, n = _geometry(shape, colmajor, pad, off)
                        pos = _positions(shape, st, off)
                        # in: caller's view -> context
                        flat = _bits(rng, n, f64)
                        logical = flat[pos]
                        src = _to_gpu(torch, flat)
                        call(lib.pmx_factor_from_device, buf, _view(torch, src, shape, st, off, f64))
                        got = dev._download(buf, rows).view(ut)
                        want = logical if block == 0 else logical.T
                        assert np.array_equal(got, want), "in: " + what
                        assert np.array_equal(src.cpu().numpy().view(ut), flat), "in changed its source: " + what
                        # round trip: context -> a second view of the same geometry in a sentinel-filled flat tensor
                        sentinel = (np.arange(n, dtype=ut) * ut(2654435761) + ut(0x5a5a5a5a)).astype(ut)
                        dst = _to_gpu(torch, sentinel)
                        call(lib.pmx_factor_to_device, buf, _view(torch, dst, shape, st, off, f64))
                        expect = sentinel.copy()
                        expect[pos] = logical
                        assert np.array_equal(dst.cpu().numpy().view(ut), expect), "round trip: " + what
                        # out alone: what pmx_upload put there
                        up = _bits(rng, rows * K, f64).reshape(rows, K)
                        dev._upload(buf, up.view(ft))
                        dst = _to_gpu(torch, sentinel)
                        call(lib.pmx_factor_to_device, buf, _view(torch, dst, shape, st, off, f64))
                        expect = sentinel.copy()
                        expect[pos] = up if block == 0 else up.T
                        assert np.array_equal(dst.cpu().numpy().view(ut), expect), "out: " + what


def test_transfer_argument_checks(torch):
    with DeviceNMF(8, 12, 4, mode="f32") as dev:
        t = torch.zeros(200, device="cuda")
        p = C.c_void_p(t.data_ptr())
        f = dev.lib.pmx_factor_from_device
        assert f(dev.h, _lib.BUF_A, p, 4, 1, 0) == 0
        assert f(dev.h, _lib.BUF_ST, p, 12, 1, 0) == 0
        assert f(dev.h, _lib.BUF_A, None, 4, 1, 0) == -1                 # PMX_E_INVALID
        assert f(dev.h, _lib.BUF_A, p, 2, 2, 0) == -1                    # no unit stride
        assert f(dev.h, _lib.BUF_A, p, 3, 1, 0) == -1                    # pitch 3 < K = 4
        assert f(dev.h, _lib.BUF_ST, p, 1, 3, 0) == -1                   # column pitch 3 < K = 4 rows of S
        assert f(dev.h, _lib.BUF_A, p, 4, 1, 1) == -4                    # PMX_E_UNSUPPORTED: float64 into an fp32 context
        assert dev.lib.pmx_factor_to_device(dev.h, _lib.BUF_A, p, 1, 7, 0) == -1
        assert float(t.abs().sum()) == 0.0


# ---- 2. end to end -----------------------------------------------------------------------------------
def _same(a, b, path="ret"):
    """exact equality of two return values: structure, types, dtypes, bits"""
    if isinstance(a, (tuple, list)):
        assert type(a) is type(b) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (path, i))
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, path
        assert a.tobytes() == b.tobytes(), path
    else:
        assert type(a) is type(b), path
        assert a == b or (a != a and b != b), path


def _unity_S(S):
    return S / S.sum(0, keepdims=True)


ROUTES = {
    "pgm": lambda Y, W: dict(),
    "fista": lambda Y, W: dict(accelerated=True, step=pm.nmf.scaled_step_pgm(0.5)),
    "linesearch": lambda Y, W: dict(backtracking=True, f=partial(pm.nmf.log_likelihood, Y=Y)),
    "bb": lambda Y, W: dict(step=pm.utils.BarzilaiBorweinStepper(type=1, init_r=0.1)),
    "unity_long_A": lambda Y, W: dict(prox_A=partial(pm.operators.prox_unity_plus, axis=0)),
    "amsgrad_unity": lambda Y, W: dict(algorithm=pm.adaprox, scheme="amsgrad", prox_S=partial(pm.operators.prox_unity_plus, axis=0)),
    "adam_b1_array": lambda Y, W: dict(algorithm=pm.adaprox, scheme="adam", b1=np.linspace(0.9, 0.5, ITERS)),
    "bsdmm_g": lambda Y, W: dict(algorithm=pm.bsdmm, proxs_g=[[pm.operators.prox_plus, partial(pm.operators.prox_soft, thresh=0.01)]] * 2),
    "weighted": lambda Y, W: dict(W=W, step=pm.nmf.scaled_step_pgm(0.9)),
}
ITERS = 6
SHAPES = [(33, 47, 3), (64, 96, 8), (200, 1000, 5), (256, 512, 64)]


def _problem(shape, dtype=np.float32):
    M, N, K = shape
    Y, A0, S0 = orc.synthetic_problem(M, N, K, dtype, seed=M + K)
    W = (0.5 + np.random.default_rng(N).random((M, N))).astype(dtype)
    return Y, A0, _unity_S(S0).astype(dtype), W


def _run(torch, route, Y, A0, S0, W, on_device, Y_on_device, **extra):
    """one nmf() call -> (return value, A, S as NumPy)"""
    Yc = torch.from_numpy(Y).cuda() if Y_on_device else Y
    kw = dict(max_iter=ITERS, e_rel=1e-9)
    kw.update(ROUTES[route](Yc, W))
    kw.update(extra)
    if on_device:
        A, S = torch.from_numpy(A0).cuda(), torch.from_numpy(S0).cuda()
        ret = pm.nmf.nmf(Yc, A, S, **kw)
        return ret, A.cpu().numpy(), S.cpu().numpy()
    A, S = A0.copy(), S0.copy()
    ret = pm.nmf.nmf(Yc, A, S, **kw)
    return ret, A, S


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_torch_factors_equal_host_factors(torch, route, shape):
    """library default mode and exact fp32, Y on the host and in HBM: factors and return values equal the host run's, bit for bit"""
    Y, A0, S0, W = _problem(shape)
    before = pm.get_default_mode()
    try:
        for mode in (None, "f32"):
            pm.set_default_mode(mode)
            for Y_on_device in (False, True):
                ret_h, A_h, S_h = _run(torch, route, Y, A0, S0, W, False, Y_on_device)
                ret_d, A_d, S_d = _run(torch, route, Y, A0, S0, W, True, Y_on_device)
                what = "mode %s, Y %s" % (mode, "in HBM" if Y_on_device else "on the host")
                assert not np.array_equal(A_h, A0), what          # (the run moved the factors at all)
                assert A_d.tobytes() == A_h.tobytes() and S_d.tobytes() == S_h.tobytes(), what
                _same(ret_d, ret_h)
    finally:
        pm.set_default_mode(before)


@pytest.mark.parametrize("shape", [(33, 47, 3), (48, 72, 40)], ids=["small-problem", "matrix-core"])
@pytest.mark.parametrize("route", ["pgm", "fista", "amsgrad_unity", "adam_b1_array"])
def test_float64_torch_factors_equal_host_factors(torch, route, shape):
    Y, A0, S0, W = _problem(shape, np.float64)
    for Y_on_device in (False, True):
        ret_h, A_h, S_h = _run(torch, route, Y, A0, S0, W, False, Y_on_device)
        ret_d, A_d, S_d = _run(torch, route, Y, A0, S0, W, True, Y_on_device)
        assert A_h.dtype == np.float64 and A_d.dtype == np.float64
        assert not np.array_equal(A_h, A0)
        assert A_d.tobytes() == A_h.tobytes() and S_d.tobytes() == S_h.tobytes()
        _same(ret_d, ret_h)
        if route in ("pgm", "fista"):
            assert ret_d[1][0].dtype == np.float64                 # gradients in the factors' NumPy dtype


def test_direct_solver_calls_take_torch_factors(torch):
    """algorithms.pgm / adaprox / bsdmm called without nmf()"""
    Y, A0, S0, _ = _problem((33, 47, 3))
    prox = [pm.operators.prox_plus] * 2

    def calls(A, S):
        grad = partial(pm.nmf.grad_likelihood, Y=Y)
        r1 = pm.pgm([A, S], grad, pm.nmf.step_pgm, prox=prox, max_iter=ITERS, e_rel=1e-9)
        r2 = pm.adaprox([A, S], grad, pm.nmf.step_adaprox, prox=prox, scheme="padam", max_iter=ITERS, e_rel=1e-9)
        pf, sf = pm.nmf.bsdmm_closures(Y, prox)
        r3 = pm.bsdmm([A, S], pf, sf, max_iter=ITERS, e_rel=1e-9)
        return r1, r2, r3
    A, S = A0.copy(), S0.copy()
    want = calls(A, S)
    At, St = torch.from_numpy(A0).cuda(), torch.from_numpy(S0).cuda()
    got = calls(At, St)
    _same(got, want)
    assert At.cpu().numpy().tobytes() == A.tobytes() and St.cpu().numpy().tobytes() == S.tobytes()


def test_warm_started_moments_stay_host_arrays(torch):
    Y, A0, S0, _ = _problem((64, 96, 8))
    outs = []
    for on_device in (False, True):
        Mm = [np.full(A0.shape, 0.01, np.float32), np.full(S0.shape, 0.02, np.float32)]
        Vv = [np.full(A0.shape, 0.03, np.float32), np.full(S0.shape, 0.04, np.float32)]
        Vh = [np.full(A0.shape, 0.05, np.float32), np.full(S0.shape, 0.06, np.float32)]
        outs.append(_run(torch, "amsgrad_unity", Y, A0, S0, None, on_device, False, M=Mm, V=Vv, Vhat=Vh) + (Mm, Vv, Vh))
    _same(list(outs[1]), list(outs[0]))


# ---- 3. views ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["pgm", "amsgrad_unity"])
def test_views_give_the_same_bits_and_keep_their_surroundings(torch, route):
    Y, A0, S0, W = _problem((200, 1000, 5))
    M, N, K = 200, 1000, 5
    ret_h, A_h, S_h = _run(torch, route, Y, A0, S0, W, False, False)
    kw = dict(max_iter=ITERS, e_rel=1e-9)
    kw.update(ROUTES[route](Y, W))
    wide = torch.full((M, K + 5), 7.25, device="cuda")
    wide[:, :K] = torch.from_numpy(A0).cuda()
    St = torch.from_numpy(np.ascontiguousarray(S0.T)).cuda()          # contiguous N x K
    A, S = wide[:, :K], St.T
    assert not A.is_contiguous() and not S.is_contiguous()
    ret_d = pm.nmf.nmf(Y, A, S, **kw)
    assert A.cpu().numpy().tobytes() == A_h.tobytes()
    assert St.cpu().numpy().tobytes() == np.ascontiguousarray(S_h.T).tobytes()
    assert bool((wide[:, K:] == 7.25).all())                          # the 5 spare columns
    _same(ret_d, ret_h)


# ---- 4. callback ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["pgm", "amsgrad_unity", "bsdmm_g"])
def test_callback_sees_the_callers_own_tensors(torch, route):
    Y, A0, S0, W = _problem((64, 96, 8))
    trace_h, trace_d = [], []
    _run(torch, route, Y, A0, S0, W, False, False, callback=lambda A, S, it=None: trace_h.append((it, A.copy(), S.copy())))
    At, St = torch.from_numpy(A0).cuda(), torch.from_numpy(S0).cuda()

    def cb(A, S, it=None):
        assert A is At and S is St
        trace_d.append((it, A.cpu().numpy(), S.cpu().numpy()))
    kw = dict(max_iter=ITERS, e_rel=1e-9)
    kw.update(ROUTES[route](Y, W))
    pm.nmf.nmf(Y, At, St, callback=cb, **kw)
    assert len(trace_h) == ITERS
    _same(trace_d, trace_h)


@pytest.mark.parametrize("route", ["pgm", "amsgrad_unity"])
def test_stop_iteration_leaves_the_host_runs_factors(torch, route):
    Y, A0, S0, W = _problem((64, 96, 8))

    def stop(A, S, it=None):
        if it == 2:
            raise StopIteration
    ret_h, A_h, S_h = _run(torch, route, Y, A0, S0, W, False, False, callback=stop)
    ret_d, A_d, S_d = _run(torch, route, Y, A0, S0, W, True, False, callback=stop)
    assert A_d.tobytes() == A_h.tobytes() and S_d.tobytes() == S_h.tobytes()
    _same(ret_d, ret_h)


# ---- 5. the helpers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_helpers_equal_their_host_values(torch, dtype):
    Y, A0, S0, W = _problem((33, 47, 3), dtype)
    At, St = torch.from_numpy(A0).cuda(), torch.from_numpy(S0).cuda()
    Yt = torch.from_numpy(Y).cuda()
    _same(pm.nmf.log_likelihood(At, St, Y=Y), pm.nmf.log_likelihood(A0, S0, Y=Y))
    _same(pm.nmf.log_likelihood(At, St, Y=Yt), pm.nmf.log_likelihood(A0, S0, Y=Yt))
    _same(pm.nmf.log_likelihood(At, St, Y=Y, W=W), pm.nmf.log_likelihood(A0, S0, Y=Y, W=W))
    _same(pm.nmf.step_pgm(At, St), pm.nmf.step_pgm(A0, S0))
    if dtype == np.float32:
        _same(pm.nmf.step_adaprox(At, St), pm.nmf.step_adaprox(A0, S0))
    assert At.cpu().numpy().tobytes() == A0.tobytes() and St.cpu().numpy().tobytes() == S0.tobytes()


# ---- 6. refusals that need the device ------------------------------------------------------------------
def test_refusals_leave_the_tensors_alone(torch):
    Y, A0, S0, _ = _problem((33, 47, 3))
    cases = [
        (np.float64, dict(), "float64"),                                                              # a float32 Y: the call computes in fp32
        (np.float32, dict(algorithm=pm.adaprox, prox_A=partial(pm.operators.prox_unity_plus, axis=0)), "axis"),
        (np.float32, dict(step=lambda *X, it=None: (1e-3, 1e-3)), "step"),
    ]
    for dtype, kw, word in cases:
        At, St = torch.from_numpy(A0.astype(dtype)).cuda(), torch.from_numpy(S0.astype(dtype)).cuda()
        with pytest.raises(NotImplementedError, match=word):
            pm.nmf.nmf(Y, At, St, max_iter=3, **kw)
        assert At.cpu().numpy().tobytes() == A0.astype(dtype).tobytes() and St.cpu().numpy().tobytes() == S0.astype(dtype).tobytes()
    At = torch.from_numpy(A0).cuda()
    with pytest.raises(TypeError, match="both"):
        pm.nmf.nmf(Y, At, S0.copy(), max_iter=3)
    with pytest.raises(NotImplementedError, match="grad_likelihood"):
        pm.nmf.grad_likelihood(At, torch.from_numpy(S0).cuda(), Y=Y)
    assert At.cpu().numpy().tobytes() == A0.tobytes()


# ---- 7. ordering ---------------------------------------------------------------------------------------
def test_factors_produced_on_a_side_stream(torch):
    """The factors are written on a side stream directly behind a few large matmuls and nmf() is called without any
    synchronisation: pmx_factor_from_device must wait for that stream (its hipDeviceSynchronize -- an array interface carries
    no stream, and the context's stream is non-blocking).  A race cannot be made to fail deterministically: this is a guard
    that costs little, the review of that synchronise is the check."""
    Y, A0, S0, W = _problem((256, 512, 64))
    ret_h, A_h, S_h = _run(torch, "pgm", Y, A0, S0, W, False, False)
    srcA, srcS = torch.from_numpy(A0).cuda(), torch.from_numpy(S0).cuda()
    a = torch.rand(4096, 4096, device="cuda")
    A, S = torch.zeros_like(srcA), torch.zeros_like(srcS)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        keep = [a @ a for _ in range(6)]
        A.copy_(srcA, non_blocking=True)
        S.copy_(srcS, non_blocking=True)
    ret_d = pm.nmf.nmf(Y, A, S, max_iter=ITERS, e_rel=1e-9)
    torch.cuda.synchronize()
    del keep
    assert A.cpu().numpy().tobytes() == A_h.tobytes() and S.cpu().numpy().tobytes() == S_h.tobytes()
    _same(ret_d, ret_h)
