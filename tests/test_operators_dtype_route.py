"""CPU: operators called on arrays -- how the argument is parsed, which view of it reaches the library, and what is refused before
the library is asked for a GPU.

Device arrays are objects that only LOOK like them (a `__cuda_array_interface__` dict around an address that is never dereferenced,
as in tests/test_device_factors_host.py).  `_lib.require_gpu` is replaced by a function that fails the test, and the two calls
that carry an argument to the library (operators._call_view / _call_flat) by recorders: every test below sees what WOULD be
launched without touching a device."""
import ctypes as C
from functools import partial

import numpy as np
import pytest

from proxmin_amd import _lib, operators as ops
from proxmin_amd.engine import DeviceOperandRef, as_device_operand, as_device_array

PTR = 1 << 20
ELEMENTWISE = [ops.prox_zero, ops.prox_plus, ops.prox_min, ops.prox_max, ops.prox_hard, ops.prox_hard_plus, ops.prox_soft, ops.prox_soft_plus,
               ops.prox_max_entropy]


class _Dev:
    def __init__(self, index):
        self.index = index


class Fake:
    """a device array as torch presents it: the interface dict, a .device with an index, no host data"""

    def __init__(self, typestr="<f4", shape=(6, 8), strides=None, readonly=False, ptr=PTR):
        self.__cuda_array_interface__ = {"typestr": typestr, "shape": shape, "strides": strides, "data": (ptr, readonly), "version": 3}
        self.shape = shape
        self.ndim = len(shape)
        self.device = _Dev(0)

    def __array__(self, *a, **k):                    # what np.asarray does to a torch tensor on the GPU
        raise TypeError("can't convert a device tensor to numpy")


@pytest.fixture
def calls(monkeypatch):
    """no GPU may be asked for; the calls that would reach the library are recorded as tuples"""
    def no_gpu():
        pytest.fail("the library was asked for a GPU")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    rec = []

    def view(ptr, on_device, dtype, rows, K, s0, s1, ps, step_k):
        rec.append(("view", ptr, bool(on_device), np.dtype(dtype).name, rows, K, s0, s1, ps.seq[0].op, ps.seq[0].unit,
                    tuple(np.broadcast_to(np.asarray(step_k, np.float64).reshape(-1), (K,)))))

    def flat(ptr, on_device, dtype, n, ps, step):
        rec.append(("flat", ptr, bool(on_device), np.dtype(dtype).name, n, ps.seq[0].op, float(step)))
    monkeypatch.setattr(ops, "_call_view", view)
    monkeypatch.setattr(ops, "_call_flat", flat)
    return rec


# ---- parsing ---------------------------------------------------------------------------------------------------------------------
def test_operand_layouts():
    r = as_device_operand(Fake())
    assert isinstance(r, DeviceOperandRef) and r.shape == (6, 8) and r.strides == (8, 1) and r.flat and r.size == 48 and r.dtype == np.float32
    assert as_device_operand(Fake(strides=(44, 4))).flat is False                        # the first 8 columns of 11
    assert as_device_operand(Fake(strides=(44, 4))).strides == (11, 1)
    c = as_device_operand(Fake(strides=(4, 24)))                                         # column-major, dense: St.T
    assert c.strides == (1, 6) and c.flat
    assert as_device_operand(Fake(strides=(4, 36))).flat is False                        # column-major with a pitch
    r8 = as_device_operand(Fake(typestr="<f8", strides=(96, 8)))
    assert r8.dtype == np.float64 and r8.strides == (12, 1) and not r8.flat
    for shape, strides in (((7,), None), ((7,), (4,)), ((2, 3, 4), None), ((2, 3, 4), (48, 16, 4)), ((2, 3, 4), (4, 8, 24)), ((2, 1, 4), (16, 4, 4))):
        o = as_device_operand(Fake(shape=shape, strides=strides))
        assert o.flat and o.strides is None and o.size == int(np.prod(shape)) and o.ndim == len(shape)
    # an axis of extent 1 makes a view one contiguous run only if the OTHER axis has unit stride
    col = as_device_operand(Fake(shape=(100, 1), strides=(32, 4)))                       # column 0 of a 100 x 8 tensor
    assert col.flat is False and col.strides == (8, 1)
    row = as_device_operand(Fake(shape=(1, 8), strides=(4, 24)))                         # row 0 of a column-major 6 x 8 tensor
    assert row.flat is False and row.strides == (1, 6)
    assert as_device_operand(Fake(shape=(100, 1), strides=(4, 4))).flat                  # a dense column
    assert as_device_operand(Fake(shape=(1, 8), strides=(32, 4))).flat                   # a dense row
    assert as_device_operand(Fake(shape=(1, 1), strides=(400, 36))).flat
    assert as_device_operand(np.zeros((3, 4))) is None and as_device_operand([[1.0]]) is None
    host = Fake()
    host.is_cuda = False
    assert as_device_operand(host) is None
    nodev = Fake()
    del nodev.device                                  # the library takes the GPU from the pointer: nothing is asked of the object
    assert as_device_operand(nodev).ptr == PTR


def test_device_of_a_cupy_like_Y_is_read_from_id():
    """engine.DeviceArrayRef used to read .device.index only: a CuPy array (.device.id) on GPU n > 0 was taken to be on GPU 0"""
    class Cupy(Fake):
        class device:
            id = 2
    y = Cupy()
    del y.device                                      # (the instance's torch-like .device: the class's CuPy-like one shows)
    assert as_device_array(y).device == 2
    plain = Fake()
    del plain.device
    assert as_device_array(plain).device == 0


@pytest.mark.parametrize("bad, exc", [
    (dict(readonly=True), TypeError),
    (dict(typestr="<f2"), TypeError), (dict(typestr="<i4"), TypeError), (dict(typestr=">f8"), TypeError),
    (dict(shape=(7,), typestr="<f2"), TypeError), (dict(shape=(7,), readonly=True), TypeError),
    (dict(strides=(64, 8)), TypeError),               # neither stride is 1
    (dict(strides=(-32, 4)), TypeError),              # a flipped view
    (dict(strides=(16, 4)), TypeError),               # rows overlap
    (dict(strides=(34, 4)), TypeError),               # not whole elements
    (dict(shape=(7,), strides=(8,)), NotImplementedError),                 # every other element
    (dict(shape=(7,), strides=(-4,)), NotImplementedError),
    (dict(shape=(2, 3, 4), strides=(96, 16, 4)), NotImplementedError),     # a 3-D view with a pitch
])
@pytest.mark.parametrize("prox", [ops.prox_plus, partial(ops.prox_soft, thresh=0.5), ops.prox_max_entropy,
                                  partial(ops.prox_components, prox=ops.prox_plus, axis=0)])
def test_refused_arguments_name_the_cause(calls, bad, exc, prox):
    with pytest.raises(exc) as e:
        prox(Fake(**bad), 1.0)
    assert "device-resident operator argument" in str(e.value) or "axis" in str(e.value)
    assert calls == []


def test_refusals_that_depend_on_the_call(calls):
    X3 = Fake(shape=(2, 3, 4))
    with pytest.raises(NotImplementedError, match="thresh of shape"):
        ops.prox_soft(X3, 1.0, thresh=np.array([0.1, 0.2, 0.3, 0.4]))
    with pytest.raises(NotImplementedError, match="does not broadcast per component"):
        ops.prox_soft(X3, np.array([0.1, 0.2, 0.3, 0.4]), thresh=0.5)
    with pytest.raises(NotImplementedError, match="2-D array"):
        ops.prox_unity(X3, 1.0, axis=0)
    with pytest.raises(NotImplementedError, match="no host view"):
        ops.prox_components(Fake(), 1.0, prox=[ops.prox_plus] * 5 + [lambda X, step: X], axis=0)
    with pytest.raises(NotImplementedError, match="no host view"):
        ops.prox_components(X3, 1.0, prox=ops.prox_plus, axis=0)
    with pytest.raises(NotImplementedError, match="at most 128"):
        ops.prox_soft(Fake(shape=(4, 200)), 1.0, thresh=np.ones(200))
    with pytest.raises(ValueError, match="7 operators for 6 components"):
        ops.prox_components(Fake(), 1.0, prox=[ops.prox_plus] * 7, axis=0)
    assert calls == []


# ---- what reaches the library --------------------------------------------------------------------------------------------------------
def test_dtype_is_the_arrays_own(calls):
    for dt, name in ((np.float32, "float32"), (np.float64, "float64"), (np.float16, "float32"), (np.int32, "float32")):
        X = np.ones((5, 7), dt)
        assert ops.prox_plus(X, 1.0) is X
        assert calls[-1][:5] == ("flat", calls[-1][1], False, name, 35)
        assert ops.prox_unity(X, 1.0, axis=1) is X
        assert calls[-1][2:8] == (False, name, 5, 7, 7, 1)
    X = np.ones((5, 7))
    ops.prox_plus(X, 1.0)
    assert calls[-1][1] == X.ctypes.data                                  # a dense float64 array is worked on in place: no padded copy
    F = np.asfortranarray(np.ones((5, 7)))
    ops.prox_plus(F, 1.0)
    assert calls[-1][1] == F.ctypes.data and calls[-1][4] == 35


def test_flat_form_on_device_arrays(calls):
    for prox in ELEMENTWISE:
        for fake in (Fake(shape=(133,)), Fake("<f8", shape=(2, 3, 4)), Fake("<f8", strides=(8, 48)), Fake(shape=(300, 260))):
            assert prox(fake, 0.5) is fake
            kind, ptr, on_device, name, n, op, step = calls[-1]
            assert (kind, ptr, on_device, n, step) == ("flat", PTR, True, int(np.prod(fake.shape)), 0.5)
            assert name == ("float64" if fake.__cuda_array_interface__["typestr"] == "<f8" else "float32")
    calls.clear()
    # a pitched view wider than 128: groups of at most 128 columns of its row-major orientation, as views
    wide = Fake("<f8", shape=(300, 260), strides=(8 * 300, 8))
    ops.prox_soft(wide, 0.5, thresh=0.1)
    assert [c[:8] for c in calls] == [("view", PTR, True, "float64", 300, 128, 300, 1), ("view", PTR + 8 * 128, True, "float64", 300, 128, 300, 1),
                                      ("view", PTR + 8 * 256, True, "float64", 300, 4, 300, 1)]
    calls.clear()
    tall = Fake(shape=(260, 30), strides=(4, 4 * 270))                     # column-major with a pitch: its transpose is the row-major view
    ops.prox_plus(tall, 0.5)
    assert [c[:8] for c in calls] == [("view", PTR, True, "float32", 30, 128, 270, 1), ("view", PTR + 4 * 128, True, "float32", 30, 128, 270, 1),
                                      ("view", PTR + 4 * 256, True, "float32", 30, 4, 270, 1)]


def test_single_column_and_single_row_of_a_pitched_tensor(calls):
    """element-wise operators with a scalar step on a (M, 1) / (1, N) view whose one long axis is NOT the unit stride: a view call
    with the pitch, never the flat form (which would rewrite the first M elements of the parent instead of the column)"""
    col = Fake(shape=(100, 1), strides=(32, 4))                                        # At[:, 0:1] of a 100 x 8 float32 tensor
    row = Fake("<f8", shape=(1, 8), strides=(8, 48))                                   # P.T[0:1] of an 8 x 6 float64 tensor
    for prox in ELEMENTWISE:
        calls.clear()
        assert prox(col, 0.5) is col
        assert [c[:8] for c in calls] == [("view", PTR, True, "float32", 100, 1, 8, 1)], prox
        calls.clear()
        assert prox(row, 0.5) is row
        assert [c[:8] for c in calls] == [("view", PTR, True, "float64", 8, 1, 6, 1)], prox


def test_read_only_host_arrays_are_refused(calls):
    """dense float32 / float64 host arrays are worked on through their address: NumPy's writeable flag is checked by hand"""
    for X in (np.ones((4, 5)), np.ones(7, np.float32), np.asfortranarray(np.ones((4, 5))), np.ones((4, 5), np.float16), np.ones((6, 8))[:, :3]):
        X.setflags(write=False)
        for prox in (ops.prox_plus, partial(ops.prox_soft, thresh=0.5)) + ((partial(ops.prox_unity, axis=1),) if X.ndim == 2 else ()):
            with pytest.raises(ValueError, match="read-only"):
                prox(X, 1.0)
    assert calls == []


def test_views_where_components_matter(calls):
    T = Fake("<f8", shape=(50, 33), strides=(8 * 70, 8), ptr=PTR + 3 * 70 * 8)         # rows 3.., the first 33 columns of a 70-wide tensor
    ops.prox_unity_plus(T, 1.0, axis=1)
    assert calls[-1][:10] == ("view", PTR + 3 * 70 * 8, True, "float64", 50, 33, 70, 1, _lib.PROX["unity_plus"], 0)
    ops.prox_unity(T, 1.0, axis=0)                                                     # the other axis, still short: the transposed view
    assert calls[-1][:10] == ("view", PTR + 3 * 70 * 8, True, "float64", 33, 50, 1, 70, _lib.PROX["unity"], 0)
    S = Fake(shape=(7, 400))                                                           # K x N: axis=1 is the long axis -> sums over the view's rows
    ops.prox_unity_plus(S, 1.0, axis=1)
    assert calls[-1][:10] == ("view", PTR, True, "float32", 400, 7, 1, 400, _lib.PROX["unity_plus"], 1)
    calls.clear()
    W = Fake(shape=(300, 260))                                                         # long axis AND wider than 128: column groups through views
    ops.prox_unity(W, 1.0, axis=0)
    assert [c[:10] for c in calls] == [("view", PTR + 4 * c0, True, "float32", 300, min(128, 260 - c0), 260, 1, _lib.PROX["unity"], 1) for c0 in (0, 128, 256)]
    # per-component thresholds and steps
    ops.prox_soft(S, 0.5, thresh=np.arange(7.0).reshape(7, 1))
    assert calls[-1][:9] == ("view", PTR, True, "float32", 400, 7, 1, 400, _lib.PROX["components"])
    ops.prox_soft(S, np.arange(7.0).reshape(7, 1), thresh=0.25)
    assert calls[-1][:9] == ("view", PTR, True, "float32", 400, 7, 1, 400, _lib.PROX["soft"]) and calls[-1][10] == tuple(np.arange(7.0))
    ops.prox_components(Fake(), 0.5, prox=[ops.prox_plus, partial(ops.prox_soft, thresh=0.5)] * 4, axis=1)
    assert calls[-1][:9] == ("view", PTR, True, "float32", 6, 8, 8, 1, _lib.PROX["components"])


def test_alternating_projections_call_their_members(calls):
    X = Fake("<f8", shape=(9, 5))
    ap = ops.AlternatingProjections([partial(ops.prox_unity, axis=1), ops.prox_plus], repeat=2)
    assert ap(X, 1.0) is X
    assert [c[0] for c in calls] == ["flat", "view", "flat", "view"] and all(c[1] == PTR and c[2] for c in calls)


def test_host_arrays_go_to_PMX_DEVICE(monkeypatch):
    """_run_rows used to pass a literal 0"""
    monkeypatch.delenv("PMX_DEVICE", raising=False)
    assert ops._host_device() == 0
    monkeypatch.setenv("PMX_DEVICE", "3")
    assert ops._host_device() == 3


# ---- the library's own refusals: before anything is launched, so they need no GPU either ---------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.load()


def _seq(op="plus", unit=0):
    return ops._seq([(op, unit, 0.0, 0)])


def test_pmx_prox_view_refusals(lib):
    X = np.zeros((4, 8))
    sk = (C.c_double * 128)()
    ps = _seq()
    ptr = C.c_void_p(X.ctypes.data)
    view = lambda p=ptr, dev=0, f64=1, rows=4, K=8, s0=8, s1=1, q=ps, s=sk, tab=None, nt=0: lib.pmx_prox_view(p, dev, f64, rows, K, s0, s1, C.byref(q) if q is not None else None, s, tab, nt, 0)
    assert view(p=None) == -1 and view(q=None) == -1 and view(s=None) == -1
    assert view(K=129, s0=129) == -1 and view(K=0) == -1 and view(rows=0) == -1
    assert b"K <= 128" in lib.pmx_last_error()
    for s0, s1 in ((16, 2), (7, 1), (1, 3), (-8, 1), (0, 0)):
        assert view(dev=1, s0=s0, s1=s1) == -1, (s0, s1)
        assert b"one of them must be 1" in lib.pmx_last_error()
    assert view(s0=9) == -1                                                # a host array is dense
    assert view(p=C.c_void_p(X.ctypes.data + 4)) == -1 and b"not aligned" in lib.pmx_last_error()
    assert view(p=C.c_void_p(X.ctypes.data + 2), f64=0) == -1
    tab = (_lib.Prox * 8)()
    for k in range(8):
        tab[k].op = _lib.PROX["plus"]
    tab[5].op = _lib.PROX["unity"]
    comp = ops._seq([("components", 0, [("plus", 0.0, 0)] * 8, 0)])
    assert view(q=comp, tab=tab, nt=1) == -1 and b"not an element-wise operator" in lib.pmx_last_error()
    assert view(q=comp) == -1                                              # names a table that was not given


def test_pmx_prox_flat_refusals(lib):
    X = np.zeros(16)
    ptr = C.c_void_p(X.ctypes.data)
    assert lib.pmx_prox_flat(None, 0, 1, 16, C.byref(_seq()), 1.0, 0) == -1
    assert lib.pmx_prox_flat(ptr, 0, 1, 16, None, 1.0, 0) == -1
    assert lib.pmx_prox_flat(ptr, 0, 1, 0, C.byref(_seq()), 1.0, 0) == -1
    assert lib.pmx_prox_flat(C.c_void_p(X.ctypes.data + 4), 0, 1, 8, C.byref(_seq()), 1.0, 0) == -1
    assert lib.pmx_prox_flat(ptr, 0, 1, 16, C.byref(_seq("unity", 0)), 1.0, 0) == -1 and b"not an element-wise operator" in lib.pmx_last_error()
    comp = ops._seq([("components", 0, [("plus", 0.0, 0)] * 8, 0)])
    assert lib.pmx_prox_flat(ptr, 0, 1, 16, C.byref(comp), 1.0, 0) == -1
    dev = C.c_int(-1)
    assert lib.pmx_pointer_device(None, C.byref(dev)) == -1 and lib.pmx_pointer_device(ptr, None) == -1
