"""CPU: nmf.nmf_batch's host side -- what it refuses (before a GPU is touched and before any array is written), the packer, the
empty batch, the ABI mirrors, and that a valid call without a GPU fails loudly."""
import ctypes
from functools import partial

import numpy as np
import pytest


@pytest.fixture(scope="module")
def pm():
    import __graft_entry__ as g
    g.build()
    import proxmin_amd
    return proxmin_amd


def _batch(shapes=((6, 9, 2), (4, 12, 3)), dtype=np.float32, seed=0):
    rng = np.random.default_rng(seed)
    Ys = [rng.random((m, n)).astype(dtype) for m, n, k in shapes]
    As = [rng.random((m, k)).astype(dtype) for m, n, k in shapes]
    Ss = [rng.random((k, n)).astype(dtype) for m, n, k in shapes]
    return Ys, As, Ss


@pytest.fixture()
def no_device(pm, monkeypatch):
    """the loader, the GPU probe and the entry point fail the test if a refused call reaches them"""
    from proxmin_amd import _lib, batch

    def reached(*a, **k):
        raise AssertionError("a refused call reached the device layer")
    monkeypatch.setattr(batch, "_entry_point", reached)
    monkeypatch.setattr(_lib, "require_gpu", reached)
    monkeypatch.setattr(_lib, "load", reached)


def _refused(pm, exc, Ys, As, Ss, **kw):
    keep = [[x.copy() if isinstance(x, np.ndarray) else x for x in seq] for seq in (Ys, As, Ss)]
    with pytest.raises(exc) as info:
        pm.nmf.nmf_batch(Ys, As, Ss, **kw)
    for seq, old in zip((Ys, As, Ss), keep):
        for x, o in zip(seq, old):
            if isinstance(x, np.ndarray):
                np.testing.assert_array_equal(x, o)
    return str(info.value)


class _OnGpu:
    def __init__(self, shape):
        self.__cuda_array_interface__ = {"typestr": "<f4", "shape": shape, "strides": None, "data": (4096, False), "version": 3}
        self.shape = shape


def test_dtypes_and_device_arrays_are_refused(pm, no_device):
    Ys, As, Ss = _batch(dtype=np.float64)
    assert "float64" in _refused(pm, NotImplementedError, Ys, As, Ss)
    Ys, As, Ss = _batch()
    As[1] = As[1].astype(np.float64)
    assert "As[1]" in _refused(pm, NotImplementedError, Ys, As, Ss)
    Ys, As, Ss = _batch()
    Ys[0] = Ys[0].astype(np.float16)
    _refused(pm, NotImplementedError, Ys, As, Ss)
    Ys, As, Ss = _batch()
    Ss[0] = (Ss[0] * 10).astype(np.int32)
    _refused(pm, NotImplementedError, Ys, As, Ss)
    for which in range(3):
        seqs = list(_batch())
        seqs[which][1] = _OnGpu(seqs[which][1].shape)
        assert "[1]" in _refused(pm, NotImplementedError, *seqs)


def test_user_callables_and_operators_outside_the_kernel_are_refused(pm, no_device):
    ops, nmf, utils = pm.operators, pm.nmf, pm.utils
    Ys, As, Ss = _batch()
    for kw in (dict(prox_A=lambda X, step: X),
               dict(prox_S=partial(lambda X, step, q=1: X, q=2)),
               dict(step=lambda *X, it=None: (0.1, 0.1)),
               dict(step=utils.BarzilaiBorweinStepper().step),
               dict(prox_A=partial(ops.prox_max_entropy, gamma=0.5)),
               dict(prox_S=ops.AlternatingProjections([ops.prox_plus, partial(ops.prox_max_entropy, gamma=0.5)])),
               dict(prox_A=partial(ops.prox_soft, thresh=np.array([0.1, 0.2]))),
               dict(prox_S=partial(ops.prox_components, prox=[ops.prox_plus, ops.prox_id], axis=0)),
               dict(prox_A=partial(ops.prox_unity, axis=0)),                 # the long axis of A
               dict(prox_S=partial(ops.prox_unity_plus, axis=1)),            # the long axis of S
               dict(prox_A=ops.AlternatingProjections([partial(ops.prox_unity_plus, axis=0), ops.prox_plus]))):
        _refused(pm, NotImplementedError, Ys, As, Ss, **kw)


def test_keywords_of_the_single_call_that_a_batch_does_not_take(pm, no_device):
    Ys, As, Ss = _batch()
    for kw in (dict(W=1), dict(backtracking=True), dict(callback=lambda *X, it=None: None), dict(algorithm=pm.algorithms.pgm)):
        assert "unexpected" in _refused(pm, TypeError, Ys, As, Ss, **kw)


def test_sizes_and_shapes_are_refused_with_the_problem_index(pm, no_device):
    f = np.float32
    for shape in ((4, 8, 17), (4097, 8, 2), (8, 8193, 2), (2048, 1024, 2)):
        m, n, k = shape
        Ys, As, Ss = _batch()
        Ys.append(np.zeros((m, n), f)); As.append(np.zeros((m, k), f)); Ss.append(np.zeros((k, n), f))
        assert "problem 2" in _refused(pm, ValueError, Ys, As, Ss)
    Ys, As, Ss = _batch()
    Ss[1] = Ss[1][:, :-1]
    assert "problem 1" in _refused(pm, ValueError, Ys, As, Ss)
    Ys, As, Ss = _batch()
    As[0] = As[0][:-1]
    assert "problem 0" in _refused(pm, ValueError, Ys, As, Ss)
    Ys, As, Ss = _batch()
    As[0] = np.ones((6, 3), f)                            # K of A and S differ
    _refused(pm, ValueError, Ys, As, Ss)
    Ys, As, Ss = _batch()
    _refused(pm, ValueError, Ys, As[:1], Ss)
    _refused(pm, ValueError, Ys, As, Ss + [Ss[0]])
    Ys, As, Ss = _batch()
    Ys[0] = Ys[0][0]                                      # 1-D
    _refused(pm, ValueError, Ys, As, Ss)


def test_accepted_operators_and_step_rules_build_their_parameters(pm):
    from proxmin_amd import batch, _lib
    ops, nmf = pm.operators, pm.nmf
    accepted = [ops.prox_id, ops.prox_zero, ops.prox_plus, partial(ops.prox_min, thresh=0.1), partial(ops.prox_max, thresh=2.0),
                partial(ops.prox_hard, thresh=0.1), partial(ops.prox_hard_plus, thresh=0.1, type="absolute"), partial(ops.prox_soft, thresh=0.01),
                partial(ops.prox_soft_plus, thresh=0.01)]
    for q in accepted:
        p = batch.batch_params(q, q, None, False, 10, 1e-3)
        assert p.prox[0].n == 1 and p.prox[1].n == 1 and p.use_fixed_steps == 0 and p.step_scale == 1.0
    p = batch.batch_params(partial(ops.prox_unity, axis=1), partial(ops.prox_unity_plus, axis=0), nmf.step_pgm, True, 7, (1e-2, 1e-3))
    assert p.prox[0].seq[0].op == _lib.PROX["unity"] and p.prox[0].seq[0].unit == 0
    assert p.prox[1].seq[0].op == _lib.PROX["unity_plus"] and p.prox[1].seq[0].unit == 0
    assert p.accelerated == 1 and p.max_iter == 7 and tuple(p.e_rel) == (1e-2, 1e-3)
    ap = ops.AlternatingProjections([partial(ops.prox_unity, axis=1), ops.prox_plus], repeat=2)
    p = batch.batch_params(ap, None, partial(nmf.step_pgm, W=1), False, 1, 0.0)
    assert p.prox[0].n == 2 and p.prox[0].repeat == 2 and p.prox[1].n == 1 and p.prox[1].seq[0].op == _lib.PROX["id"]
    p = batch.batch_params(ops.prox_plus, ops.prox_plus, nmf.scaled_step_pgm(0.5), True, 1, 1e-3, max_workgroups=3)
    assert p.step_scale == 0.5 and p.use_fixed_steps == 0 and p.max_workgroups == 3
    p = batch.batch_params(ops.prox_plus, ops.prox_plus, nmf.constant_step(1e-3, 2e-3), False, 1, 1e-3)
    assert p.use_fixed_steps == 1 and tuple(p.fixed_steps) == (1e-3, 2e-3)
    with pytest.raises(ValueError):
        batch.batch_params(ops.prox_plus, ops.prox_plus, partial(nmf.step_pgm, W=np.ones((2, 2))), False, 1, 1e-3)
    with pytest.raises(TypeError):
        batch.batch_params(ops.prox_plus, ops.prox_plus, 0.5, False, 1, 1e-3)


def test_packer_round_trips_ragged_strided_and_3d_inputs(pm):
    from proxmin_amd import batch
    rng = np.random.default_rng(3)
    f = np.float32
    wide = rng.random((7, 22)).astype(f)
    Ys = [rng.random((5, 9)).astype(f), wide[:, ::2], np.asfortranarray(rng.random((3, 4)).astype(f))]
    tall = rng.random((10, 8)).astype(f)
    As = [rng.random((5, 2)).astype(f), tall[:7, ::2], rng.random((3, 1)).astype(f)]
    Ss = [np.asfortranarray(rng.random((2, 9)).astype(f)), rng.random((11, 8)).astype(f).T[::2, :][:, :11], rng.random((1, 4)).astype(f)]
    assert As[1].shape == (7, 4) and Ss[1].shape == (4, 11) and not As[1].flags.c_contiguous and not Ss[1].flags.c_contiguous
    assert Ss[0].flags.f_contiguous and not Ss[0].flags.c_contiguous
    Yl, Al, Sl = batch.check_batch(Ys, As, Ss)
    items, Y, A, S = batch.pack(Yl, Al, Sl)
    oy = oa = os_ = 0
    for b in range(3):
        it = items[b]
        M, N = Ys[b].shape
        K = As[b].shape[1]
        assert (it.M, it.N, it.K, it.ldY, it.offY, it.offA, it.offS) == (M, N, K, N, oy, oa, os_)
        np.testing.assert_array_equal(Y[oy:oy + M * N].reshape(M, N), Ys[b])
        np.testing.assert_array_equal(A[oa:oa + M * K].reshape(M, K), As[b])
        np.testing.assert_array_equal(S[os_:os_ + K * N].reshape(K, N), Ss[b])
        oy, oa, os_ = oy + M * N, oa + M * K, os_ + K * N
    assert (Y.size, A.size, S.size) == (oy, oa, os_) and Y.dtype == A.dtype == S.dtype == f
    # scatter: new values arrive in the caller's own memory, through the views, and nothing beside them moves
    before_wide, before_tall = wide.copy(), tall.copy()
    A2, S2 = A + 1, S * 2
    batch.unpack(items, A2, S2, Al, Sl)
    for b in range(3):
        it = items[b]
        np.testing.assert_array_equal(As[b], A2[it.offA:it.offA + it.M * it.K].reshape(it.M, it.K))
        np.testing.assert_array_equal(Ss[b], S2[it.offS:it.offS + it.K * it.N].reshape(it.K, it.N))
    np.testing.assert_array_equal(wide, before_wide)
    np.testing.assert_array_equal(tall[:, 1::2], before_tall[:, 1::2])
    np.testing.assert_array_equal(tall[7:], before_tall[7:])
    assert not np.array_equal(tall[:7, ::2], before_tall[:7, ::2])
    # three 3-D arrays are sequences of views
    Y3, A3, S3 = rng.random((4, 6, 5)).astype(f), rng.random((4, 6, 2)).astype(f), rng.random((4, 2, 5)).astype(f)
    Yl, Al, Sl = batch.check_batch(Y3, A3, S3)
    items, Y, A, S = batch.pack(Yl, Al, Sl)
    np.testing.assert_array_equal(Y, Y3.reshape(-1))
    np.testing.assert_array_equal(A, A3.reshape(-1))
    np.testing.assert_array_equal(S, S3.reshape(-1))
    batch.unpack(items, -A, -S, Al, Sl)
    np.testing.assert_array_equal(A3.reshape(-1), -A)
    np.testing.assert_array_equal(S3.reshape(-1), -S)


def test_empty_batch(pm, no_device):
    res = pm.nmf_batch([], [], [])
    assert res.converged.shape == (0, 2) and res.converged.dtype == bool
    assert res.iterations.shape == (0,) and res.steps.shape == (0, 2) and res.steps.dtype == np.float64
    f = np.float32
    res = pm.nmf.nmf_batch(np.zeros((0, 4, 5), f), np.zeros((0, 4, 2), f), np.zeros((0, 2, 5), f), accelerated=True)
    assert len(res) == 0


def test_batch_abi_sizes_equal_the_ctypes_mirrors(pm):
    from proxmin_amd import _lib
    sizes = (ctypes.c_int * 3)()
    assert _lib.load().pmx_batch_abi_sizes(sizes) == 0
    assert list(sizes) == [ctypes.sizeof(t) for t in (_lib.BatchItem, _lib.BatchResult, _lib.BatchParams)]
    assert ctypes.sizeof(_lib.BatchItem) == 56 and ctypes.sizeof(_lib.BatchResult) == 64
    assert ctypes.sizeof(_lib.BatchParams) == 2 * ctypes.sizeof(_lib.ProxSeq) + 16 + 8 + 16 + 16
    assert pm.nmf_batch is pm.nmf.nmf_batch


def test_the_entry_point_refuses_what_the_python_layer_refuses(pm):
    """pmx_nmf_batch_pgm itself: sizes and bad arguments PMX_E_INVALID (-1), long-axis unity and ops 11 / 12 PMX_E_UNSUPPORTED (-4), all
    before the device is touched (this runs without a GPU) and with the arrays untouched"""
    from proxmin_amd import _lib, batch
    lib = _lib.load()
    ops = pm.operators
    Ys, As, Ss = _batch()
    items, Y, A, S = batch.pack(*batch.check_batch(Ys, As, Ss))
    A0, S0 = A.copy(), S.copy()
    out = (_lib.BatchResult * 2)()

    def call(p, items=items, B=2):
        vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        return lib.pmx_nmf_batch_pgm(0, B, items, vp(Y), vp(A), vp(S), ctypes.byref(p), out)

    good = batch.batch_params(ops.prox_plus, ops.prox_plus, None, False, 2, 1e-3)
    for op, unit, want in ((_lib.PROX["unity"], 1, -4), (_lib.PROX["unity_plus"], 1, -4), (_lib.PROX["max_entropy"], 0, -4),
                           (_lib.PROX["components"], 0, -4), (13, 0, -1)):
        p = batch.batch_params(ops.prox_plus, ops.prox_plus, None, False, 2, 1e-3)
        p.prox[1].seq[0].op, p.prox[1].seq[0].unit, p.prox[1].seq[0].reserved = op, unit, 1 if op == 12 else 0
        assert call(p) == want and lib.pmx_last_error()
    for field, value in (("K", 17), ("M", 4097), ("N", 8193), ("ldY", 3), ("offA", -1)):
        bad = (_lib.BatchItem * 2)()
        ctypes.memmove(bad, items, ctypes.sizeof(bad))
        setattr(bad[1], field, value)
        assert call(good, items=bad) == -1
        assert b"problem 1" in lib.pmx_last_error()
    assert call(good, B=-1) == -1
    assert lib.pmx_nmf_batch_pgm(0, 2, items, None, None, None, ctypes.byref(good), out) == -1
    assert lib.pmx_nmf_batch_pgm(0, 0, None, None, None, None, ctypes.byref(good), None) == 0      # B == 0 does nothing
    np.testing.assert_array_equal(A, A0)
    np.testing.assert_array_equal(S, S0)


def test_without_a_gpu_a_valid_call_fails_loudly(pm):
    """no silent CPU path (as tests/test_abi.py: test_no_gpu_fails_loudly)"""
    from proxmin_amd import _lib
    if _lib.load().pmx_device_count() > 0:
        pytest.skip("a GPU is visible")
    Ys, As, Ss = _batch()
    keep = [a.copy() for a in As + Ss]
    with pytest.raises(_lib.PmxError):
        pm.nmf.nmf_batch(Ys, As, Ss, max_iter=2)
    for a, o in zip(As + Ss, keep):
        np.testing.assert_array_equal(a, o)
