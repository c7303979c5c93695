"""Thin object wrapper around one libpmx context: device residency of Y / A / S^T for the
duration of an `nmf()` call, uploads/downloads with the S <-> S^T transposition, and the solver
entry points.  Pure plumbing -- every number is produced by the HIP kernels behind the C ABI.
"""
from __future__ import annotations

import ctypes as C
import logging
import os

import numpy as np

from . import _lib

logger = logging.getLogger("proxmin")
_noticed = set()


def _notice(key, msg):
    """one line per distinct situation on logger "proxmin" (INFO): which K1 a context really got"""
    if key not in _noticed:
        _noticed.add(key)
        logger.info(msg)


# Arithmetic of the three contractions inside the fused residual-gradient kernel:
#   "f32"    exact fp32 MFMA (v_mfma_f32_32x32x2_f32)
#   "bf16x3" split-bf16 MFMA with fp32-class accuracy (3-term split for A@S, 2-term for the gradients);
#            K <= 64, larger K runs the fp32 kernel
#   "f16x2"  as "bf16x3", but shapes with K = 64, M % 128 = 0, N % 256 = 0 run the two-term fp16 kernel (operands scaled
#            by powers of two from the factor maxima: 9 instead of 12 MFMA products per multiply-add), and so do shapes
#            with K = 128, M % 128 = 0, N % 128 = 0 (k_grad_f16_k128; no weights there)
#   "f16x2r" "f16x2" with the RESIDUAL in exact fp32's class (include/pmx.h: PMX_MODE_F16X2R).  K1's K = 64 / 128 without weights: the
#            residual from the high x high fp16 product alone, the rest restored exactly through K x K matrices (k_gfix.hip) -- 7 instead
#            of 9 MFMA products per multiply-add; K = 32: third fp16 terms of A and S in a second accumulator (11 products)
# [r6] The library's default IS the benchmarked arithmetic: f16x2r is in exact fp32's error class, falls back to the
# exact-fp32 kernel by itself where it has no kernel of its own (off-shape weighted contexts: open_weighted) or where one fp16 scale cannot
# carry the residual (the range guard, tests/test_gpu_range.py), and runs the tuned kernels on zero-padded frames for ragged shapes.
LIBRARY_DEFAULT_MODE = "f16x2r"
_DEFAULT_MODE = os.environ.get("PMX_MODE", LIBRARY_DEFAULT_MODE)
assert _DEFAULT_MODE in ("f32", "bf16x3", "f16x2", "f16x2r"), "PMX_MODE must be one of f32, bf16x3, f16x2, f16x2r"


def set_default_mode(mode=None):
    """Select the contraction arithmetic used by nmf() and friends ("f32", "bf16x3", "f16x2" or "f16x2r"); None: back to the
    library's default (LIBRARY_DEFAULT_MODE, or PMX_MODE from the environment)."""
    global _DEFAULT_MODE
    if mode is None:
        mode = os.environ.get("PMX_MODE", LIBRARY_DEFAULT_MODE)
    assert mode in ("f32", "bf16x3", "f16x2", "f16x2r")
    _DEFAULT_MODE = mode


def get_default_mode():
    return _DEFAULT_MODE


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def f64_applies(M, N, K, weighted=False):
    """Shapes the fp64 kernels take (include/pmx.h: PMX_MODE_F64 -- the fused small-problem kernels for the reference's own examples
    and BASELINE cfg1, the MFMA passes of k_big_f64.hip for the rest up to K = 128); PMX_F64=0 switches the mode off (fp64 inputs are
    then computed in fp32 and cast back, with a warning)."""
    def off(name):                      # the library reads these with atoi(): anything that is not a non-zero number switches off
        v = os.environ.get(name)
        if v is None:
            return False
        try:
            return int(v.strip() or 0) == 0
        except ValueError:
            return True
    if off("PMX_F64"):
        return False
    small = not weighted and not off("PMX_K1_SMALL") and K <= 16 and M <= 4096 and N <= 8192 and M * N <= (1 << 20)
    # [r6] everything else up to K = 128 -- and every weighted likelihood -- : one MFMA pass per gradient (k_big_f64.hip);
    # PMX_F64_BIG=0 keeps the small kernels only
    return small or (not off("PMX_F64_BIG") and K <= 128 and 8.0 * M * N * (2 if weighted else 1) <= 160e9)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class DeviceArrayRef:
    """[r6] Y (or W) that is ALREADY in HBM: anything that speaks `__cuda_array_interface__` (a torch tensor on the GPU, a
    CuPy array): float32 (or float64: [r6] copied into the fp64 context's own array), row-major, unit stride along the rows.  nmf() and the solvers adopt float32 zero-copy (pmx_set_Y_device)
    instead of uploading a host array -- the reference's Y lives in host RAM (nmf.py:96), ours may live where the kernels read it.
    The owner must keep its memory alive and unchanged for the duration of the call (the context holds a reference)."""

    def __init__(self, obj):
        cai = obj.__cuda_array_interface__
        ts = cai.get("typestr")
        if ts not in ("<f4", "=f4", "|f4", "<f8", "=f8", "|f8"):
            raise TypeError("a device-resident Y must be float32 or float64 (got %r)" % (ts,))
        es = 8 if ts.endswith("8") else 4
        shape = tuple(int(v) for v in cai["shape"])
        if len(shape) != 2:
            raise TypeError("a device-resident Y must be two-dimensional")
        strides = cai.get("strides")
        if strides is None:
            ld = shape[1]
        else:
            if int(strides[1]) != es or int(strides[0]) % es or int(strides[0]) < es * shape[1]:
                raise TypeError("a device-resident Y must be row-major with unit stride along its rows")
            ld = int(strides[0]) // es
        self.ptr, self.shape, self.ld, self.owner = int(cai["data"][0]), shape, ld, obj
        self.dtype = np.dtype(np.float64 if es == 8 else np.float32)
        self.ndim = 2
        # the GPU: from the pointer where the runtime knows it, else .device.index (torch) / .device.id (CuPy) / an integer .device;
        # an object that says nothing about its device is taken to be on GPU 0
        dev = pointer_device(self.ptr)
        self.device = dev if dev is not None else (_device_index(obj) if getattr(obj, "device", None) is not None else 0)

    def __array__(self, *a, **k):
        raise TypeError("this array lives on the GPU; proxmin_amd adopts it in place")


def as_device_array(obj):
    """DeviceArrayRef for an object that lives on the GPU, None for host data"""
    if isinstance(obj, DeviceArrayRef):
        return obj
    if isinstance(obj, np.ndarray) or not hasattr(obj, "__cuda_array_interface__"):
        return None
    if getattr(obj, "is_cuda", True) is False:       # a torch tensor on the host
        return None
    return DeviceArrayRef(obj)


class DeviceFactorRef:
    """A factor (A: M x K, S: K x N) that is ALREADY in HBM and is updated there, in place: anything that speaks
    `__cuda_array_interface__`, writable, two-dimensional, float32 or float64, row- or column-major with any pitch (one of the two
    strides is the unit stride; the stride of an axis of extent 1 does not count).  Unlike Y it is not adopted by the kernels: the
    context keeps its own copies (S as S^T) and moves the block device to device at entry, at exit and before every callback
    (include/pmx.h: pmx_factor_from_device / pmx_factor_to_device; csrc/k_xfer.hip).  `strides` are in ELEMENTS, `dtype` is the NumPy
    dtype the solvers compute their return values in, `owner` the caller's object."""

    def __init__(self, obj):
        self.ptr, self.shape, self.strides, self.dtype = _parse_view(obj.__cuda_array_interface__, "a device-resident factor")
        self.owner = obj
        self.ndim = 2
        self.device = _device_index(obj, self.ptr)

    def __array__(self, *a, **k):
        raise TypeError("this array lives on the GPU; proxmin_amd updates it in place")


def _parse_header(cai, what):
    """-> (pointer, shape, element size, element strides or None for a C-contiguous array) of a WRITABLE float32 / float64 array
    interface; TypeError naming the cause otherwise"""
    ts = cai.get("typestr")
    if ts not in ("<f4", "=f4", "|f4", "<f8", "=f8", "|f8"):
        raise TypeError("%s must be float32 or float64 (got %r)" % (what, ts))
    es = 8 if ts.endswith("8") else 4
    shape = tuple(int(v) for v in cai["shape"])
    data = cai["data"]
    if bool(data[1]):
        raise TypeError("%s is updated in place: a read-only array cannot be one" % what)
    strides = cai.get("strides")
    if strides is not None:
        if len(strides) != len(shape) or any(int(s) % es for s in strides):
            raise TypeError("%s's strides %r are not whole elements" % (what, tuple(strides)))
        strides = tuple(int(s) // es for s in strides)
    return int(data[0]), shape, es, strides


def _parse_view(cai, what):
    """-> (pointer, shape, element strides, dtype) of a two-dimensional row- or column-major view with any pitch (the rule of
    include/pmx.h: pmx_factor_from_device); TypeError naming the cause for anything else"""
    shape = tuple(int(v) for v in cai["shape"])
    if len(shape) != 2:
        ts = cai.get("typestr")
        if ts not in ("<f4", "=f4", "|f4", "<f8", "=f8", "|f8"):
            raise TypeError("%s must be float32 or float64 (got %r)" % (what, ts))
        raise TypeError("%s must be two-dimensional (got shape %r)" % (what, shape))
    ptr, shape, es, st = _parse_header(cai, what)
    if st is None:
        st = (shape[1], 1)
    # one unit stride, the other axis stepping over at least that axis's extent (an axis of extent 1 is never stepped along)
    rowmajor = (st[1] == 1 or shape[1] == 1) and (st[0] >= shape[1] or shape[0] == 1)
    colmajor = (st[0] == 1 or shape[0] == 1) and (st[1] >= shape[0] or shape[1] == 1)
    if not (rowmajor or colmajor):
        if 1 not in st:
            raise TypeError("%s needs unit stride along one of its axes (element strides %r)" % (what, st))
        raise TypeError("%s's rows overlap (shape %r, element strides %r)" % (what, shape, st))
    if rowmajor:
        st = (st[0] if shape[0] > 1 else max(shape[1], 1), 1)
    else:
        st = (1, st[1] if shape[1] > 1 else max(shape[0], 1))
    return ptr, shape, st, np.dtype(np.float64 if es == 8 else np.float32)


def pointer_device(ptr):
    """the GPU a device pointer lives on, as the runtime knows it (pmx_pointer_device: hipPointerGetAttributes); None where it cannot
    say -- the library is not built, no GPU, or an address it does not know as device memory"""
    if not os.path.exists(_lib.LIB_PATH):       # not built: nobody to ask (a stale or mismatched library raises in load(), loudly)
        return None
    lib = _lib.load()
    if lib.pmx_device_count() < 1:
        return None
    dev = C.c_int(-1)
    return int(dev.value) if lib.pmx_pointer_device(C.c_void_p(int(ptr)), C.byref(dev)) == 0 else None


def _device_index(obj, ptr=None):
    """the HIP device an array lives on: the pointer's own (a CuPy array carries .device.id, other producers nothing torch-like: the
    runtime knows), else obj.device.index (torch), obj.device.id (CuPy) or an int"""
    if ptr is not None:
        dev = pointer_device(ptr)
        if dev is not None:
            return dev
    dev = getattr(obj, "device", None)
    for v in (getattr(dev, "index", None), getattr(dev, "id", None), dev):
        if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
            return int(v)
    raise TypeError("cannot tell which GPU this device-resident factor lives on (no .device.index, .device.id or integer .device)")


class DeviceOperandRef:
    """The argument of an operator of proxmin_amd.operators that lives in HBM and is updated there: anything that speaks
    `__cuda_array_interface__`, writable, float32 or float64.  Two-dimensional: a row- or column-major view with any pitch
    (`strides` in elements, DeviceFactorRef's rule).  `flat`: the array is one contiguous run of `size` elements (1-D with unit
    stride, C- or F-contiguous n-D), which is all an element-wise operator with a scalar step needs; arrays of other dimensions
    than two must be that.  The GPU is not asked here: the library takes it from the pointer."""

    def __init__(self, obj):
        what = "a device-resident operator argument"
        cai = obj.__cuda_array_interface__
        shape = tuple(int(v) for v in cai["shape"])
        if len(shape) == 2:
            self.ptr, self.shape, self.strides, self.dtype = _parse_view(cai, what)
            # one contiguous run?  Judged on the interface's own strides: _parse_view's normalisation replaces the stride of an axis of
            # extent 1, and a single column (M, 1) of a wider tensor is a run only if its rows are 1 element apart
            raw = cai.get("strides")
            raw = (shape[1], 1) if raw is None else tuple(int(v) // self.dtype.itemsize for v in raw)
            self.flat = _contiguous(shape, raw)
        else:
            self.ptr, self.shape, es, st = _parse_header(cai, what)
            self.dtype = np.dtype(np.float64 if es == 8 else np.float32)
            self.strides = None
            if st is not None and not _contiguous(self.shape, st):
                raise NotImplementedError("%s of %d dimensions must be C- or F-contiguous (shape %r, element strides %r): only "
                                          "two-dimensional arrays are taken as row- or column-major views" % (what, len(shape), shape, st))
            self.flat = True
        self.size = int(np.prod(self.shape, dtype=np.int64)) if self.shape else 1
        self.ndim = len(self.shape)
        self.owner = obj


def _contiguous(shape, st):
    """do these element strides lay `shape` out as one run, in C or in Fortran order?  (axes of extent 1 do not count)"""
    for order in (range(len(shape) - 1, -1, -1), range(len(shape))):
        want, good = 1, True
        for ax in order:
            if shape[ax] != 1 and st[ax] != want:
                good = False
                break
            want *= shape[ax]
        if good:
            return True
    return False


def as_device_operand(obj):
    """DeviceOperandRef for an operator argument that lives on the GPU, None for host data"""
    if isinstance(obj, np.ndarray) or not hasattr(obj, "__cuda_array_interface__"):
        return None
    if getattr(obj, "is_cuda", True) is False:       # a torch tensor on the host
        return None
    return DeviceOperandRef(obj)


def as_device_factor(obj):
    """DeviceFactorRef for a factor that lives on the GPU, None for host data"""
    if isinstance(obj, DeviceFactorRef):
        return obj
    if isinstance(obj, np.ndarray) or not hasattr(obj, "__cuda_array_interface__"):
        return None
    if getattr(obj, "is_cuda", True) is False:       # a torch tensor on the host
        return None
    return DeviceFactorRef(obj)


def factor_pair(A, S):
    """-> (A, S) as they are for host factors, (DeviceFactorRef, DeviceFactorRef) for factors in HBM; one of each is refused"""
    rA, rS = as_device_factor(A), as_device_factor(S)
    if (rA is None) != (rS is None):
        raise TypeError("A and S must both be host arrays or both live on the GPU (A is %s, S is %s)"
                        % tuple("on the device" if r is not None else "on the host" for r in (rA, rS)))
    if rA is None:
        return A, S
    if rA.device != rS.device:
        raise ValueError("A lives on GPU %d and S on GPU %d" % (rA.device, rS.device))
    return rA, rS


def factor_owner(X):
    """what the caller passed: the callback's argument"""
    return X.owner if isinstance(X, DeviceFactorRef) else X


def device_of(Y, A, default=0):
    """The GPU a call runs on: where its device-resident arrays are (Y and the factors must agree), else `default`."""
    dY = Y.device if isinstance(Y, DeviceArrayRef) else None
    dA = A.device if isinstance(A, DeviceFactorRef) else None
    if dY is not None and dA is not None and dY != dA:
        raise ValueError("Y lives on GPU %d and the factors on GPU %d" % (dY, dA))
    return dA if dA is not None else (dY if dY is not None else default)


_F64_FACTORS_IN_F32 = ("float64 device-resident factors are taken by the fp64 kernels only (float64 Y, library operators and step rules, no "
                       "Barzilai-Borwein, K <= 128); this call computes in float32: hand it float32 arrays")


def refuse_f64_factors(*X):
    """float64 factors in HBM on a call that computes in fp32 (they could only be rounded into the caller's own array)"""
    if any(isinstance(x, DeviceFactorRef) and x.dtype == np.float64 for x in X):
        raise NotImplementedError(_F64_FACTORS_IN_F32)


class DeviceNMF:
    """Device state for one factorisation problem Y (M x N) ~ A (M x K) @ S (K x N)."""

    def __init__(self, M, N, K, device=0, mode=None, stream=None):
        self.lib = _lib.require_gpu()
        self.M, self.N, self.K = int(M), int(N), int(K)
        self.device = device
        mode = mode or _DEFAULT_MODE
        self.mode = mode
        self.f64 = mode in ("f64", "f64mfma")          # fp64 operands, products and sums (small problems, the fused loops of the three back-ends: k_small_f64.hip)
        mode_id = {"f32": _lib.MODE_F32, "bf16x3": _lib.MODE_BF16X3, "f16x2": _lib.MODE_F16X2, "f16x2r": _lib.MODE_F16X2R, "f64": _lib.MODE_F64, "f64mfma": _lib.MODE_F64_MFMA}[mode]
        h = C.c_void_p()
        _lib.check(self.lib.pmx_ctx_create(C.byref(h), device, self.M, self.N, self.K, mode_id,
                                           C.c_void_p(stream) if stream else None))
        self.h = h
        self._keep, self._kept_for = [], {}
        # a split-precision context that fell off its fast kernel says so once (pmx_k1_info knows): ragged shapes and
        # K outside {64, 128} run the generic split-bf16 kernels or the exact-fp32 one, 1.5-3 x slower per pass
        if mode not in ("f32", "f64", "f64mfma"):
            k = self.k1_info()["kernel"]
            fast = {"f16x2": ("k_grad_f16_v8", "k_grad_f16_k128", "k_grad_f16_k32", "k_grad_small"), "bf16x3": ("k_grad_bf16", "k_grad_small"),
                    "f16x2r": ("k_grad_f16_v8_r3", "k_grad_f16_k32_r3", "k_grad_f16_v8_hh", "k_grad_f16_k128_hh", "k_grad_f16_k128", "k_grad_small")}[mode]
            generic_bf16 = k == "k_grad_bf16" and not (self.K == 64 and self.M % 128 == 0 and self.N % 256 == 0)
            if k not in fast or generic_bf16 or (mode in ("f16x2", "f16x2r") and k == "k_grad_bf16"):
                _notice((mode, k, self.K, self.M % 128 == 0, self.N % 256 == 0),
                        "proxmin_amd: mode %s at %d x %d x %d runs %s, not the tuned kernel (those take K = 64 with M %% 128 = 0 and "
                        "N %% 256 = 0, or K = 128 with M %% 128 = 0 and N %% 128 = 0)" % (mode, self.M, self.N, self.K, k))

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            try:
                if self.mode in ("f16x2", "f16x2r") and self.k1_info()["range_faults"]:
                    _notice(("range", self.M, self.N, self.K),
                            "proxmin_amd: mode %s at %d x %d x %d: the factors ran away from the data (K max|A| max|S| > 2^16 max|Y|: one fp16 "
                            "scale cannot carry that residual); the run went on with the exact-fp32 kernel" % (self.mode, self.M, self.N, self.K))
            except Exception:
                pass
            self.lib.pmx_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sync(self):
        _lib.check(self.lib.pmx_ctx_sync(self.h))

    # -- data -------------------------------------------------------------------------------
    def set_Y(self, Y):
        ref = as_device_array(Y)
        if ref is not None:               # already in HBM: float32 adopted in place; float64 copied into the fp64 context's own (padded) array
            assert ref.shape == (self.M, self.N), "Y must be M x N"
            if ref.dtype == np.float64:
                if not self.f64:
                    raise NotImplementedError("a float64 device-resident Y is taken by the fp64 kernels only (library operators and step rules, K <= 128); "
                                              "this call computes in float32: hand it a float32 array")
                _lib.check(self.lib.pmx_set_Y_device_f64(self.h, C.c_void_p(int(ref.ptr)), int(ref.ld)))
                return
            if self.f64:
                raise NotImplementedError("an fp64 context takes a float64 Y")
            self.set_Y_device(ref.ptr, ld=ref.ld, copy=False, keepalive=ref.owner)
            return
        Y = np.asarray(Y)
        assert Y.shape == (self.M, self.N), "Y must be M x N"
        if self.f64:
            Yd = np.ascontiguousarray(Y, dtype=np.float64)
            _lib.check(self.lib.pmx_set_Y_host_f64(self.h, _vp(Yd), self.N))
            return
        Yf = _f32(Y)
        _lib.check(self.lib.pmx_set_Y_host(self.h, _vp(Yf), self.N))

    def set_Y_device(self, dptr, ld=None, copy=False, keepalive=None):
        """Adopt (or copy) a float32 row-major device array, e.g. a torch tensor's data_ptr()."""
        if keepalive is not None:
            self._keep.append(keepalive)
        _lib.check(self.lib.pmx_set_Y_device(self.h, C.c_void_p(int(dptr)), int(ld or self.N), int(bool(copy))))
        if not copy and not self.f64:
            fr = self.k1_info()["frame"]
            if tuple(fr) != (self.M, self.N):
                _notice(("frame-copy", self.M, self.N, self.K),
                        "proxmin_amd: %d x %d x %d runs on the zero-padded frame %d x %d of its tuned kernel: the device array handed over with copy=False is "
                        "COPIED into a frame-sized buffer (%.2f GiB more device memory; PMX_FRAME=0 keeps the caller's array and the guarded kernels)"
                        % (self.M, self.N, self.K, fr[0], fr[1], fr[0] * fr[1] * 4 / 2.0 ** 30))

    def set_W(self, W):
        """Weights of the likelihood (nmf.py:13-41), an M x N array; None goes back to W == 1.  Mode "f32" takes any
        shape; the split-bf16 mode only those of its default kernel (K = 64, M % 128 = 0, N % 256 = 0) and raises
        NotImplementedError otherwise -- see open_weighted()."""
        if W is None:
            _lib.check((self.lib.pmx_set_W_host_f64 if self.f64 else self.lib.pmx_set_W_host)(self.h, None, 0))
            return
        W = np.asarray(W)
        assert W.shape == (self.M, self.N), "W must be M x N"
        if self.f64:                     # [r6] the fp64 matrix-core kernels take weights (mode "f64mfma" forces them on a small problem)
            Wd = np.ascontiguousarray(W, dtype=np.float64)
            _lib.check(self.lib.pmx_set_W_host_f64(self.h, _vp(Wd), self.N))
            return
        Wf = _f32(W)
        _lib.check(self.lib.pmx_set_W_host(self.h, _vp(Wf), self.N))

    def set_W_device(self, dptr, ld=None, copy=False, keepalive=None):
        if keepalive is not None:
            self._keep.append(keepalive)
        _lib.check(self.lib.pmx_set_W_device(self.h, C.c_void_p(int(dptr)), int(ld or self.N), int(bool(copy))))

    def _upload(self, buf, arr2d):
        if self.f64:
            a = np.ascontiguousarray(arr2d, dtype=np.float64)
            _lib.check(self.lib.pmx_upload_f64(self.h, buf, _vp(a), a.size))
            return
        a = _f32(arr2d)
        _lib.check(self.lib.pmx_upload(self.h, buf, _vp(a), a.size))

    def _download(self, buf, rows):
        if self.f64:
            out = np.empty((rows, self.K), dtype=np.float64)
            _lib.check(self.lib.pmx_download_f64(self.h, buf, _vp(out), out.size))
            return out
        out = np.empty((rows, self.K), dtype=np.float32)
        _lib.check(self.lib.pmx_download(self.h, buf, _vp(out), out.size))
        return out

    def _check_ref(self, ref, j):
        want = (self.M, self.K) if j == 0 else (self.K, self.N)
        assert ref.shape == want, "A must be M x K and S K x N"
        if ref.device != self.device:
            raise ValueError("the array lives on GPU %d, this context on GPU %d" % (ref.device, self.device))
        if (ref.dtype == np.float64) != self.f64:
            raise NotImplementedError(_F64_FACTORS_IN_F32 if not self.f64 else "an fp64 context takes float64 device-resident factors")

    def _from_device(self, buf, ref, j=None):
        """block j (default `buf & 1`) from the caller's array in HBM, device to device (include/pmx.h: pmx_factor_from_device: it waits for
        everything the caller enqueued on the device before the call)"""
        self._check_ref(ref, buf & 1 if j is None else j)
        old = self._kept_for.get(buf)            # one owner per buffer: a context that serves many calls (nmf._factors_only) lets go of the last one
        if old is not None:
            self._keep[:] = [o for o in self._keep if o is not old]
        self._kept_for[buf] = ref.owner
        self._keep.append(ref.owner)
        _lib.check(self.lib.pmx_factor_from_device(self.h, buf, C.c_void_p(ref.ptr), ref.strides[0], ref.strides[1], int(self.f64)))

    def _to_device(self, buf, ref, j=None):
        """block j (default `buf & 1`) into the caller's array in HBM: its logical elements only, complete when the call returns"""
        self._check_ref(ref, buf & 1 if j is None else j)
        _lib.check(self.lib.pmx_factor_to_device(self.h, buf, C.c_void_p(ref.ptr), ref.strides[0], ref.strides[1], int(self.f64)))

    def set_factors(self, A, S):
        if isinstance(A, DeviceFactorRef) or isinstance(S, DeviceFactorRef):
            A, S = factor_pair(A, S)
            self._check_ref(A, 0)                      # (both checked before either is copied)
            self._check_ref(S, 1)
            self._from_device(_lib.BUF_A, A)
            self._from_device(_lib.BUF_ST, S)
            return
        assert A.shape == (self.M, self.K) and S.shape == (self.K, self.N), "A must be M x K and S K x N"
        self._upload(_lib.BUF_A, A)
        self._upload(_lib.BUF_ST, np.asarray(S).T)

    def get_factors(self):
        return self._download(_lib.BUF_A, self.M), self._download(_lib.BUF_ST, self.N).T

    def write_factors(self, A, S):
        """the current factors into the caller's device-resident arrays (DeviceFactorRef), device to device"""
        self._check_ref(A, 0)
        self._check_ref(S, 1)
        self._to_device(_lib.BUF_A, A)
        self._to_device(_lib.BUF_ST, S)

    def put(self, base, j, arr):
        """upload block j (0: M x K array, 1: K x N array) of a two-block state (moments, Z/U, ...)."""
        if isinstance(arr, DeviceFactorRef):
            self._from_device(base + j, arr, j)
            return
        self._upload(base + j, arr if j == 0 else np.asarray(arr).T)

    def get(self, base, j):
        out = self._download(base + j, self.M if j == 0 else self.N)
        return out if j == 0 else out.T

    # -- measurement --------------------------------------------------------------------------
    def set_timing(self, on=True, every=1):
        """Bracket K1 launches with HIP events on the launch stream (every `every`-th launch)."""
        _lib.check(self.lib.pmx_set_timing(self.h, int(every) if on else 0))

    def get_timing(self):
        """(summed K1 duration in ms, number of bracketed K1 launches) since set_timing(True)."""
        ms, n = C.c_double(), C.c_int()
        _lib.check(self.lib.pmx_get_timing(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    PHASES = ("k1_with_prologue", "pack", "collective", "post", "update", "after_update_to_next_k1")

    def set_phase_timing(self, every=4):
        """Row-sharded runs: HIP-event timeline of every `every`-th iteration's phases (include/pmx.h: pmx_set_phase_timing); 0: off."""
        _lib.check(self.lib.pmx_set_phase_timing(self.h, int(every)))

    def get_phase_timing(self):
        """({phase: mean ms}, iterations averaged) since set_phase_timing."""
        ms, n = (C.c_double * 6)(), C.c_int()
        _lib.check(self.lib.pmx_get_phase_timing(self.h, ms, C.byref(n)))
        return {k: ms[i] for i, k in enumerate(self.PHASES)}, n.value

    def time_grad(self, do_A=True, do_S=True, reps=10):
        """average K1 duration in ms (kernel ablation helper, includes the presplit kernel in bf16x3 mode)"""
        ms = C.c_double()
        _lib.check(self.lib.pmx_time_grad(self.h, int(do_A), int(do_S), int(reps), C.byref(ms)))
        return ms.value

    def k1_info(self):
        """Layout of this context's fused residual-gradient kernel (include/pmx.h: pmx_k1_info)."""
        v = (C.c_int * 8)()
        _lib.check(self.lib.pmx_k1_info(self.h, v))
        keys = ("kernel", "chain", "slabs_A", "slabs_S", "row_regions", "col_regions", "panels_per_region", "chain_faults")
        d = dict(zip(keys, list(v)))
        d["kernel"] = ("k_grad_f32", "k_grad_bf16", "k_grad_f16_v8", "k_grad_f16_v9", "k_grad_small", "k_grad_f16_k128", "k_grad_f32_pc", "k64_front", "k_grad_f16_k32", "k_grad_f16_v8_r3", "k_grad_f16_k32_r3", "k_grad_f16_v8_hh", "k_grad_f16_k128_hh", "k64_grad_pass")[d["kernel"]]
        v7 = d.pop("chain_faults")
        d["chain_faults"], d["tail_faults"], d["tail_fused"] = v7 % 1000, (v7 // 1000) % 1000, bool((v7 // 1000000) % 10)
        d["range_faults"] = v7 // 10000000   # 1: a two-term fp16 K1 refused the residual's range, the context went on in exact fp32 (f16_range_fault)
        fr = (C.c_int64 * 3)()
        _lib.check(self.lib.pmx_k1_frame(self.h, fr))
        d["frame"] = (fr[0], fr[1])          # != (M, N): a ragged shape on a zero-padded frame (include/pmx.h: pmx_k1_frame)
        d["frame_K"] = fr[2]                 # != K: K1 runs the next tuned K on zero-padded copies of the factors
        return d

    def gfix_info(self):
        """Who formed mode f16x2r's K x K correction in this context so far (include/pmx.h: pmx_gfix_info): K1 launches that carried it,
        stand-alone triples of launches, and whether a carried correction faulted and the context fell back to the launches."""
        v = (C.c_int * 4)()
        _lib.check(self.lib.pmx_gfix_info(self.h, v))
        return {"in_k1": v[0], "launches": v[1], "fell_back": bool(v[2]), "faults": v[3]}

    # -- single operations --------------------------------------------------------------------
    def grad(self):
        """nmf.grad_likelihood at the current device factors -> (gA (M x K), gS (K x N))."""
        _lib.check(self.lib.pmx_grad(self.h))
        return self._download(_lib.BUF_GA, self.M), self._download(_lib.BUF_GST, self.N).T

    def loglike(self):
        out = C.c_double()
        _lib.check(self.lib.pmx_loglike(self.h, C.byref(out)))
        return out.value

    def step_pgm(self):
        out = (C.c_double * 2)()
        _lib.check(self.lib.pmx_step_pgm(self.h, out))
        return out[0], out[1]

    def step_adaprox(self):
        out = np.empty(2 * self.K, dtype=np.float32)
        _lib.check(self.lib.pmx_step_adaprox(self.h, _vp(out)))
        return out[: self.K].copy(), out[self.K:].copy()

    # -- per-component operator tables (include/pmx.h: pmx_prox_table) --------------------------
    def _stamp_tables(self, seqs, first=0):
        """Upload the tables that device operator sequences carry (operators._seq: `seq.tables`) into this context's slots
        first, first + 1, .. and return copies of the sequences whose PMX_PROX_COMPONENTS entries name those slots.  Every
        table is checked before the first is written: ValueError for one without K rows, NotImplementedError for more tables
        than the context has slots."""
        from . import operators
        operators.check_tables(seqs, self.K)
        if first + sum(len(operators.seq_tables(q)) for q in seqs) > _lib.MAX_TABLES:
            raise NotImplementedError("more than %d per-component operator tables in one call" % _lib.MAX_TABLES)
        out, nxt = [], first
        for q in seqs:
            tables = operators.seq_tables(q)
            if not tables:
                out.append(q)
                continue
            c = _lib.ProxSeq.from_buffer_copy(q)
            for i in range(c.n):
                if c.seq[i].op == _lib.PROX["components"]:
                    tab = tables[c.seq[i].reserved - 1]
                    _lib.check(self.lib.pmx_prox_table(self.h, nxt, tab, len(tab)))
                    c.seq[i].reserved = nxt + 1
                    nxt += 1
            out.append(c)
        self._ntab = nxt
        return out

    def prox_apply(self, buf, seq, step_k):
        """One operator sequence on a device buffer of the context in place (include/pmx.h: pmx_prox_apply); step_k: the K
        per-component steps.  Tables go into the slots behind those of the running solver."""
        seq, = self._stamp_tables([seq], first=getattr(self, "_ntab_solver", 0))
        sk = np.ascontiguousarray(np.broadcast_to(np.asarray(step_k, dtype=np.float32).reshape(-1), (self.K,)))
        _lib.check(self.lib.pmx_prox_apply(self.h, int(buf), C.byref(seq), _vp(sk)))

    # -- solvers ------------------------------------------------------------------------------
    def pgm_begin(self, prox, accelerated=False, step_scale=1.0, fixed_steps=None, e_rel=(1e-6, 1e-6), bb=None, backtracking=False,
                  host_prox=(False, False), unweighted_rule=False):
        p = _lib.PgmParams()
        p.prox[0], p.prox[1] = self._stamp_tables(list(prox))
        self._ntab_solver = self._ntab
        p.accelerated = int(bool(accelerated))
        p.step_scale = float(step_scale)
        p.use_fixed_steps = int(fixed_steps is not None)
        p.unweighted_rule = int(bool(unweighted_rule))    # step_pgm(*X) without its W on a weighted problem (include/pmx.h)
        if fixed_steps is not None:
            p.fixed_steps[0], p.fixed_steps[1] = float(fixed_steps[0]), float(fixed_steps[1])
        p.e_rel[0], p.e_rel[1] = float(e_rel[0]), float(e_rel[1])
        if bb is not None:
            p.bb_type, p.bb_init_r = int(bb[0]), float(bb[1])
        p.backtracking = int(bool(backtracking))
        p.host_prox[0], p.host_prox[1] = int(bool(host_prox[0])), int(bool(host_prox[1]))
        _lib.check(self.lib.pmx_pgm_begin(self.h, C.byref(p)))

    def pgm_split(self, phase, steps=None):
        """One piece of ONE iteration (include/pmx.h: pmx_pgm_split): 0 gradient, 1 argument of the user prox, 2 update."""
        r = _lib.Result()
        st = (C.c_double * 2)(float(steps[0]), float(steps[1])) if steps is not None else None
        _lib.check(self.lib.pmx_pgm_split(self.h, int(phase), st, C.byref(r)))
        return r

    def pgm_bt_split(self, phase):
        """One piece of ONE pgm iteration with the line search when a block's prox is a user callable (include/pmx.h:
        pmx_pgm_bt_split) -> (mask of the blocks whose prox is owed, (T_A s_A, T_S s_S), result)."""
        r = _lib.Result()
        need, eff = C.c_int(), (C.c_double * 2)()
        _lib.check(self.lib.pmx_pgm_bt_split(self.h, int(phase), C.byref(need), eff, C.byref(r)))
        return need.value, (eff[0], eff[1]), r

    def pgm_set_fixed_steps(self, steps):
        """new step constants of a context begun with fixed steps (include/pmx.h: pmx_pgm_set_fixed_steps)"""
        _lib.check(self.lib.pmx_pgm_set_fixed_steps(self.h, (C.c_double * 2)(float(steps[0]), float(steps[1]))))

    def pgm_step_arrays(self, arrays):
        """arrays[j]: None (block j keeps its scalar step) or an array that broadcasts against block j (A: M x K, S: K x N) --
        uploaded element by element for the split phases that follow (include/pmx.h: pmx_pgm_step_arrays)."""
        mask = 0
        for j, a in enumerate(arrays):
            if a is None:
                continue
            shape = (self.M, self.K) if j == 0 else (self.K, self.N)
            self.put(_lib.BUF_STEP_A, j, np.broadcast_to(np.asarray(a, dtype=np.float32), shape))
            mask |= 1 << j
        _lib.check(self.lib.pmx_pgm_step_arrays(self.h, mask))

    def pgm_run(self, n_iter):
        r = _lib.Result()
        _lib.check(self.lib.pmx_pgm_run(self.h, int(n_iter), C.byref(r)))
        return r

    def adaprox_begin(self, prox, scheme="adam", b2=0.999, eps=1e-8, p=0.25, check_convergence=True,
                      prox_max_iter=1000, warm_moments=False, warm_vhat=False, fixed_alpha=None, e_rel=(1e-6, 1e-6),
                      host_step=False, host_prox=(False, False)):
        q = _lib.AdaproxParams()
        q.prox[0], q.prox[1] = self._stamp_tables(list(prox))
        self._ntab_solver = self._ntab
        q.scheme = _lib.SCHEME[scheme]
        q.b2, q.eps, q.p = float(b2), float(eps), float(p)
        q.check_convergence = int(bool(check_convergence))
        q.prox_max_iter = int(prox_max_iter)
        q.warm_vhat = int(bool(warm_vhat))
        q.use_fixed_steps = 2 if host_step else int(fixed_alpha is not None)
        q.host_prox[0], q.host_prox[1] = int(bool(host_prox[0])), int(bool(host_prox[1]))
        if fixed_alpha is not None:
            q.fixed_alpha[0], q.fixed_alpha[1] = float(fixed_alpha[0]), float(fixed_alpha[1])
        q.e_rel[0], q.e_rel[1] = float(e_rel[0]), float(e_rel[1])
        _lib.check(self.lib.pmx_adaprox_begin(self.h, C.byref(q), int(bool(warm_moments))))

    def adaprox_run(self, b1_slice, b1_prev):
        b1 = np.ascontiguousarray(b1_slice, dtype=np.float64)
        r = _lib.Result()
        _lib.check(self.lib.pmx_adaprox_run(self.h, int(b1.size), b1.ctypes.data_as(C.POINTER(C.c_double)),
                                            float(b1_prev), C.byref(r)))
        return r

    def adaprox_set_alpha(self, alpha_A, alpha_S):
        """per-component step sizes of the next iteration (a user `step` callable's return value, K values per block)"""
        a = np.ascontiguousarray(np.concatenate([np.asarray(alpha_A, np.float32).ravel(), np.asarray(alpha_S, np.float32).ravel()]))
        assert a.size == 2 * self.K
        _lib.check(self.lib.pmx_adaprox_set_alpha(self.h, _vp(a)))

    def adaprox_split(self, phase, it, b1_it, b1_prev, host_tau=(0, 0)):
        """One half of ONE iteration (include/pmx.h: pmx_adaprox_split).  Returns (Result, (maxpsi_A, maxpsi_S))."""
        r = _lib.Result()
        tau = (C.c_int * 2)(int(host_tau[0]), int(host_tau[1]))
        mp = (C.c_double * 2)()
        _lib.check(self.lib.pmx_adaprox_split(self.h, int(phase), int(it), float(b1_it), float(b1_prev), tau, mp, C.byref(r)))
        return r, (mp[0], mp[1])

    def bsdmm_begin(self, prox_f, proxs_g, e_rel=(1e-6, 1e-6), e_abs=(0.0, 0.0), update_order=None):
        p = _lib.BsdmmParams()
        if update_order is not None:
            order = [int(j) for j in update_order]
            if len(order) > 8:
                raise NotImplementedError("update_order with more than 8 entries")
            p.n_order = len(order)
            for i, j in enumerate(order):
                p.order[i] = j
        for j in range(2):
            if len(proxs_g[j] or []) > _lib.MAX_G:
                raise NotImplementedError("at most %d constraints per factor on the device" % _lib.MAX_G)
        flat = self._stamp_tables(list(prox_f) + [ps for j in range(2) for ps in (proxs_g[j] or [])])
        self._ntab_solver = self._ntab
        p.prox_f[0], p.prox_f[1] = flat[:2]
        at = 2
        for j in range(2):
            g = proxs_g[j] or []
            p.n_g[j] = len(g)
            for i in range(len(g)):
                p.prox_g[j][i] = flat[at]
                at += 1
            p.e_rel[j], p.e_abs[j] = float(e_rel[j]), float(e_abs[j])
        _lib.check(self.lib.pmx_bsdmm_begin(self.h, C.byref(p)))

    def set_host_grad(self, on=True):
        """The gradient of every iteration is what the caller uploads into BUF_GA / BUF_GST (a user `grad` callable);
        the context needs no Y (include/pmx.h: pmx_set_host_grad)."""
        _lib.check(self.lib.pmx_set_host_grad(self.h, int(bool(on))))

    def bsdmm_split(self, j, phase, host_f=False, host_g=0, last_block=False, step_f=0.0):
        """One piece of one block update (include/pmx.h: pmx_bsdmm_split)."""
        r = _lib.Result()
        _lib.check(self.lib.pmx_bsdmm_split(self.h, int(j), int(phase), int(bool(host_f)), int(host_g), int(bool(last_block)), float(step_f), C.byref(r)))
        return r

    def bsdmm_run(self, n_iter):
        r = _lib.Result()
        _lib.check(self.lib.pmx_bsdmm_run(self.h, int(n_iter), C.byref(r)))
        return r

    def iter_norms(self):
        """((d2_A, x2_A), (d2_S, x2_S)): the sums of each block's last outer / Boyd test (include/pmx.h: pmx_iter_norms)."""
        v = (C.c_double * 4)()
        _lib.check(self.lib.pmx_iter_norms(self.h, v))
        return (v[0], v[1]), (v[2], v[3])


def open_weighted(M, N, K, W, **kw):
    """Context for a weighted likelihood: the default arithmetic mode where its kernel takes weights, exact fp32
    otherwise (never a CPU path: both are device kernels)."""
    dev = DeviceNMF(M, N, K, **kw)
    if W is None:
        return dev
    try:
        dev.set_W(W)
        return dev
    except NotImplementedError:
        mode = dev.mode
        dev.close()
    _notice(("weighted", mode, K), "proxmin_amd: a weighted likelihood at %d x %d x %d has no kernel in mode %s (its weighted kernels take "
            "K = 64, M %% 128 = 0, N %% 256 = 0): this context computes in exact fp32 (k_grad_f32)" % (M, N, K, mode))
    dev = DeviceNMF(M, N, K, **dict(kw, mode="f32"))
    dev.set_W(W)
    return dev
