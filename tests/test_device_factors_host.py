"""CPU: how a device-resident A / S is recognised and what is refused before anything touches a GPU.

engine.as_device_factor on objects that only LOOK like device arrays (a `__cuda_array_interface__` dict around an address that is
never dereferenced), and the refusals of nmf() and its helpers that need no device: they must come with the arrays untouched."""
import numpy as np
import pytest

import proxmin_amd as pm
from proxmin_amd import _lib
from proxmin_amd.engine import as_device_factor, DeviceFactorRef, as_device_array


class _Dev:
    def __init__(self, index):
        self.index = index


class Fake:
    """a device array as torch presents it: the interface dict, a .device with an index, no host data"""

    def __init__(self, typestr="<f4", shape=(6, 8), strides=None, readonly=False, device=0, ptr=4096):
        self.__cuda_array_interface__ = {"typestr": typestr, "shape": shape, "strides": strides, "data": (ptr, readonly), "version": 3}
        self.shape = shape
        self.ndim = len(shape)
        if device is not None:
            self.device = _Dev(device) if device != "int" else 3

    def __array__(self, *a, **k):                    # what np.asarray does to a torch tensor on the GPU
        raise TypeError("can't convert a device tensor to numpy")


def test_layouts_that_are_taken():
    r = as_device_factor(Fake())
    assert isinstance(r, DeviceFactorRef) and r.shape == (6, 8) and r.strides == (8, 1) and r.ptr == 4096 and r.dtype == np.dtype(np.float32)
    assert r.ndim == 2 and r.device == 0 and r.owner is not None
    assert as_device_factor(Fake(strides=(32, 4))).strides == (8, 1)               # dense, strides spelt out
    assert as_device_factor(Fake(strides=(44, 4))).strides == (11, 1)              # pitched row-major: the first 8 columns of 11
    assert as_device_factor(Fake(strides=(4, 24))).strides == (1, 6)               # column-major (St.T of a contiguous 8 x 6)
    assert as_device_factor(Fake(strides=(4, 36))).strides == (1, 9)               # ... with a pitch
    r8 = as_device_factor(Fake(typestr="<f8", strides=(96, 8)))
    assert r8.dtype == np.dtype(np.float64) and r8.strides == (12, 1)
    assert as_device_factor(Fake(typestr="<f8", strides=(8, 48))).strides == (1, 6)
    # an axis of extent 1 is never stepped along: torch gives a 1 x 1 tensor the strides (1, 1) and a 1 x n row (n, 1)
    assert as_device_factor(Fake(shape=(1, 1), strides=(4, 4))).shape == (1, 1)
    assert as_device_factor(Fake(shape=(1, 7), strides=(28, 4))).strides == (7, 1)
    assert as_device_factor(Fake(shape=(5, 1), strides=(4, 4))).shape == (5, 1)
    assert as_device_factor(r) is r
    assert as_device_factor(Fake(device=2)).device == 2
    assert as_device_factor(Fake(device="int")).device == 3

    class Cupy(Fake):
        class device:
            id = 1
    assert as_device_factor(Cupy(device=None)).device == 1


def test_host_data_is_not_a_device_factor():
    assert as_device_factor(np.zeros((3, 4), np.float32)) is None
    assert as_device_factor([[1.0, 2.0]]) is None
    host = Fake()
    host.is_cuda = False                              # a torch tensor on the host
    assert as_device_factor(host) is None


@pytest.mark.parametrize("bad", [
    dict(readonly=True),
    dict(typestr="<f2"), dict(typestr="<i4"), dict(typestr=">f4"),
    dict(shape=(6,)), dict(shape=(2, 3, 4)),
    dict(strides=(64, 8)),                            # neither stride is the unit stride (every other column)
    dict(strides=(16, 4)),                            # rows overlap: pitch 4 < 8 columns
    dict(strides=(4, 16)),                            # columns overlap
    dict(strides=(-32, 4)),                           # a flipped view
    dict(strides=(34, 4)),                            # not whole elements
    dict(typestr="<f8", strides=(48, 4)),
    dict(device=None),                                # no way to tell the GPU
])
def test_refused_layouts(bad):
    with pytest.raises(TypeError):
        as_device_factor(Fake(**bad))


def test_a_ref_is_never_copied_to_the_host():
    with pytest.raises(TypeError):
        np.asarray(as_device_factor(Fake()))


def test_Y_detection_is_untouched():
    """as_device_array keeps its own, narrower rule (row-major only; read-only is fine for Y)"""
    assert as_device_array(Fake(readonly=True)).ld == 8
    with pytest.raises(TypeError):
        as_device_array(Fake(strides=(4, 24)))


M, N, K = 6, 9, 2


def _fakes(dtype="<f4"):
    return Fake(dtype, (M, K), ptr=1 << 20), Fake(dtype, (K, N), ptr=1 << 21)


def test_no_gpu_fails_loudly_and_dereferences_nothing():
    import __graft_entry__ as g
    g.build()
    if _lib.load().pmx_device_count() > 0:
        pytest.skip("a GPU is visible")
    A, S = _fakes()
    Y = np.ones((M, N), np.float32)
    for algorithm in (pm.pgm, pm.adaprox, pm.bsdmm):
        with pytest.raises(_lib.PmxError):
            pm.nmf.nmf(Y, A, S, algorithm=algorithm, max_iter=1)
    with pytest.raises(_lib.PmxError):
        pm.nmf.log_likelihood(A, S, Y=Y)
    with pytest.raises(_lib.PmxError):
        pm.nmf.step_pgm(A, S)
    with pytest.raises(_lib.PmxError):
        pm.nmf.step_adaprox(A, S)


def test_mixed_host_and_device_factors():
    A, S = _fakes()
    Y = np.ones((M, N), np.float32)
    hA, hS = np.ones((M, K), np.float32), np.ones((K, N), np.float32)
    for algorithm in (pm.pgm, pm.adaprox, pm.bsdmm):
        with pytest.raises(TypeError, match="both"):
            pm.nmf.nmf(Y, A, hS, algorithm=algorithm, max_iter=1)
        with pytest.raises(TypeError, match="both"):
            pm.nmf.nmf(Y, hA, S, algorithm=algorithm, max_iter=1)
    with pytest.raises(TypeError, match="both"):
        pm.nmf.log_likelihood(hA, S, Y=Y)
    with pytest.raises(TypeError, match="both"):
        pm.nmf.step_pgm(A, hS)
    assert (hA == 1).all() and (hS == 1).all()


def test_user_callables_take_host_arrays():
    from functools import partial
    A, S = _fakes()
    Y = np.ones((M, N), np.float32)
    called = []

    def prox(X, step):
        called.append("prox")
        return X

    def step(*X, it=None):
        called.append("step")
        return 1.0, 1.0

    def grad(*X):
        called.append("grad")
        return X

    with pytest.raises(NotImplementedError, match="prox"):
        pm.nmf.nmf(Y, A, S, prox_A=prox, max_iter=1)
    with pytest.raises(NotImplementedError, match="prox"):
        pm.nmf.nmf(Y, A, S, prox_S=prox, algorithm=pm.adaprox, max_iter=1)
    with pytest.raises(NotImplementedError, match="prox"):
        pm.nmf.nmf(Y, A, S, algorithm=pm.bsdmm, proxs_g=[[prox], None], max_iter=1)
    with pytest.raises(NotImplementedError, match="step"):
        pm.nmf.nmf(Y, A, S, step=step, max_iter=1)
    with pytest.raises(NotImplementedError, match="step"):
        pm.nmf.nmf(Y, A, S, step=step, algorithm=pm.adaprox, max_iter=1)
    with pytest.raises(NotImplementedError, match="grad"):
        pm.pgm([A, S], grad, pm.nmf.constant_step(1.0), prox=[pm.operators.prox_plus] * 2, max_iter=1)
    with pytest.raises(NotImplementedError, match="closures"):
        pm.bsdmm([A, S], lambda X, step, j=None, Xs=None: X, lambda Xs, j=None: 1.0, max_iter=1)
    # prox_unity* along a factor's long axis is a host prox wherever it is not fused
    long_A = partial(pm.operators.prox_unity_plus, axis=0)
    with pytest.raises(NotImplementedError, match="axis"):
        pm.nmf.nmf(Y, A, S, prox_A=long_A, algorithm=pm.adaprox, max_iter=1)
    with pytest.raises(NotImplementedError, match="axis"):
        pm.nmf.nmf(Y, A, S, prox_A=long_A, algorithm=pm.bsdmm, max_iter=1)
    with pytest.raises(NotImplementedError, match="axis"):
        pm.nmf.nmf(Y, A, S, prox_A=long_A, backtracking=True, f=partial(pm.nmf.log_likelihood, Y=Y), max_iter=1)
    assert called == []


def test_sharded_runs_and_grad_likelihood_take_host_factors():
    A, S = _fakes()
    Y = np.ones((M, N), np.float32)
    with pytest.raises(NotImplementedError, match="M_global"):
        pm.nmf.nmf(Y, A, S, M_global=2 * M, max_iter=1)
    with pytest.raises(NotImplementedError, match="grad_likelihood"):
        pm.nmf.grad_likelihood(A, S, Y=Y)


def test_factors_and_Y_on_two_gpus():
    A, S = Fake("<f4", (M, K), device=1), Fake("<f4", (K, N), device=1)
    Y = Fake("<f4", (M, N), device=0)
    with pytest.raises(ValueError, match="GPU"):
        pm.nmf.nmf(Y, A, S, max_iter=1)
    with pytest.raises(ValueError, match="GPU"):
        pm.nmf.nmf(np.ones((M, N), np.float32), A, Fake("<f4", (K, N), device=0), max_iter=1)
