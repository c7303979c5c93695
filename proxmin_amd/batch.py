"""Host side of `nmf.nmf_batch`: many small factorisations in one launch (include/pmx.h: pmx_nmf_batch_pgm, csrc/k_batch.hip).

The batch is packed into one contiguous Y, one A and one S buffer with an item table (shape and offsets per problem), handed to the
entry point on PMX_DEVICE's GPU, and the factors are scattered back into the caller's arrays.  Everything that is refused is
refused here, before a GPU is touched and before any array is written.
"""
from __future__ import annotations

import ctypes as C
import os
from functools import partial

import numpy as np

from . import _lib, operators, utils

# where both small-problem device bodies apply (csrc/k_grad.hip: grad_small_applies, csrc/pmx_api.hip: eig_small_applies)
K_MAX, M_MAX, N_MAX, MN_MAX = 16, 4096, 8192, 1 << 20


class BatchResult:
    """Per problem what pgm's own return and log line carry (algorithms.py:140-144), without the gradients:
    converged (B, 2) bool, iterations (B,) int, steps (B, 2) float64 (the float32 steps of the single call); norms (B, 2, 2) holds
    the two sums [block][diff^2, norm^2] of each problem's last stopping test."""

    def __init__(self, B):
        self.converged = np.zeros((B, 2), dtype=bool)
        self.iterations = np.zeros((B,), dtype=np.int64)
        self.steps = np.zeros((B, 2), dtype=np.float64)
        self.norms = np.zeros((B, 2, 2), dtype=np.float64)
        self.launch_ms = 0.0

    def __len__(self):
        return len(self.iterations)

    def __repr__(self):
        return "BatchResult(B=%d, converged=%d, iterations=%d..%d)" % (
            len(self), int(self.converged.all(axis=1).sum()), int(self.iterations.min()) if len(self) else 0, int(self.iterations.max()) if len(self) else 0)


def _host_f32(x, what, b):
    if hasattr(x, "__cuda_array_interface__"):
        raise NotImplementedError("nmf_batch: %s[%d] lives on a GPU: a batch takes host arrays (device-resident batches are not built)" % (what, b))
    if what != "Ys" and not isinstance(x, np.ndarray):
        raise TypeError("nmf_batch: %s[%d] must be a numpy array (it is updated in place), not %s" % (what, b, type(x).__name__))
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise NotImplementedError("nmf_batch: %s[%d] is %s: a batch computes in float32 (loop over nmf() for float64)" % (what, b, x.dtype))
    if x.ndim != 2:
        raise ValueError("nmf_batch: %s[%d] has %d dimensions: every problem is 2-D" % (what, b, x.ndim))
    return x


def check_batch(Ys, As, Ss):
    """-> three lists of 2-D float32 host arrays (views of the caller's), every shape checked; raises what nmf_batch raises."""
    for name, seq in (("Ys", Ys), ("As", As), ("Ss", Ss)):
        if hasattr(seq, "__cuda_array_interface__"):
            raise NotImplementedError("nmf_batch: %s lives on a GPU: a batch takes host arrays (device-resident batches are not built)" % name)
    try:
        B = len(Ys)
        same = len(As) == B and len(Ss) == B
    except TypeError:
        raise ValueError("nmf_batch: Ys, As and Ss are sequences of equal length")
    if not same:
        raise ValueError("nmf_batch: %d Ys, %d As and %d Ss: the three sequences must have equal length" % (len(Ys), len(As), len(Ss)))
    Yl = [_host_f32(Ys[b], "Ys", b) for b in range(B)]
    Al = [_host_f32(As[b], "As", b) for b in range(B)]
    Sl = [_host_f32(Ss[b], "Ss", b) for b in range(B)]
    for b in range(B):
        (M, N), (Ma, K), (Ks, Ns) = Yl[b].shape, Al[b].shape, Sl[b].shape
        if Ma != M or Ns != N or Ks != K:
            raise ValueError("nmf_batch: problem %d: Y is %d x %d, A %d x %d and S %d x %d (A must be M x K and S K x N)" % (b, M, N, Ma, K, Ks, Ns))
        if not (1 <= K <= K_MAX and 1 <= M <= M_MAX and 1 <= N <= N_MAX and M * N <= MN_MAX):
            raise ValueError("nmf_batch: problem %d is %d x %d x %d: a batch takes K <= %d, M <= %d, N <= %d, M N <= 2^20 (use nmf() for it)"
                             % (b, M, N, K, K_MAX, M_MAX, N_MAX))
    return Yl, Al, Sl


def pack(Yl, Al, Sl):
    """-> (item table, Y, A, S): the batch in three contiguous float32 buffers.  Y rows lose their own pitch (ldY = N); A is M x K and
    S K x N, dense, whatever strides the caller's arrays have."""
    B = len(Yl)
    items = (_lib.BatchItem * max(B, 1))()
    oy = oa = os_ = 0
    for b in range(B):
        (M, N), K = Yl[b].shape, Al[b].shape[1]
        it = items[b]
        it.M, it.N, it.K, it.ldY, it.offY, it.offA, it.offS = M, N, K, N, oy, oa, os_
        oy += M * N
        oa += M * K
        os_ += K * N
    Y, A, S = np.empty(oy, np.float32), np.empty(oa, np.float32), np.empty(os_, np.float32)
    for b in range(B):
        it = items[b]
        np.copyto(Y[it.offY:it.offY + it.M * it.N].reshape(it.M, it.N), Yl[b])
        np.copyto(A[it.offA:it.offA + it.M * it.K].reshape(it.M, it.K), Al[b])
        np.copyto(S[it.offS:it.offS + it.K * it.N].reshape(it.K, it.N), Sl[b])
    return items, Y, A, S


def unpack(items, A, S, Al, Sl):
    """the packed factors back into the caller's arrays, through `arr[...] = ...` (any strides)"""
    for b in range(len(Al)):
        it = items[b]
        Al[b][...] = A[it.offA:it.offA + it.M * it.K].reshape(it.M, it.K)
        Sl[b][...] = S[it.offS:it.offS + it.K * it.N].reshape(it.K, it.N)


def _batch_seq(prox, j):
    """the device sequence of block j's operator, or what nmf_batch raises for it"""
    name = "prox_S" if j else "prox_A"
    if prox is None:
        prox = operators.prox_id                      # pgm: prox=None is prox_id (algorithms.py:63-64)
    try:
        seq = operators.device_proxseq(prox, j, for_solver=True)
    except operators.NotFusable as exc:
        raise NotImplementedError("nmf_batch: %s: %s; a batch takes prox_unity* along the short axis only (axis=1 on A, axis=0 on S)" % (name, exc))
    except NotImplementedError as exc:
        raise NotImplementedError("nmf_batch: %s: %s (a batch takes this library's operators only)" % (name, exc))
    ops = [seq.seq[i].op for i in range(seq.n)]
    if _lib.PROX["max_entropy"] in ops:
        raise NotImplementedError("nmf_batch: %s: prox_max_entropy is not in the batch kernel (loop over nmf())" % name)
    if _lib.PROX["components"] in ops or operators.seq_tables(seq):
        raise NotImplementedError("nmf_batch: %s: per-component parameters / prox_components are not in the batch kernel (loop over nmf())" % name)
    return seq


def batch_params(prox_A, prox_S, step, accelerated, max_iter, e_rel, max_workgroups=0):
    """pmx_batch_params for the call, or what nmf_batch raises for its operators and step rule"""
    from . import nmf as _nmf
    from .algorithms import _e_rel_pair
    p = _lib.BatchParams()
    p.prox[0], p.prox[1] = _batch_seq(prox_A, 0), _batch_seq(prox_S, 1)
    scale, fixed = 1.0, None
    if isinstance(getattr(step, "__self__", step), utils.BarzilaiBorweinStepper):
        raise NotImplementedError("nmf_batch: Barzilai-Borwein steps are not in the batch kernel (loop over nmf())")
    if step is None or step is _nmf.step_pgm:
        pass
    elif isinstance(step, partial) and step.func is _nmf.step_pgm and not step.args:
        sW = step.keywords.get("W", 1)
        if not np.isscalar(sW):
            raise ValueError(_nmf._AMBIGUOUS)
        if sW != 1 or set(step.keywords) - {"W"}:
            raise NotImplementedError("nmf_batch: the Lipschitz rule with W = 1 only")
    elif isinstance(step, _nmf.scaled_step_pgm):
        scale = step.scale
    elif isinstance(step, _nmf.constant_step):
        fixed = step.steps
    elif callable(step):
        raise NotImplementedError("nmf_batch: step %r is a user callable: a batch takes nmf.step_pgm, nmf.scaled_step_pgm(c) or "
                                  "nmf.constant_step(a, b) (loop over nmf() for anything else)" % (step,))
    else:
        raise TypeError("step must be callable")
    e_rel = _e_rel_pair(e_rel)
    max_iter = int(max_iter)
    if max_iter < 0:
        raise ValueError("nmf_batch: max_iter < 0")
    p.e_rel[0], p.e_rel[1] = e_rel
    p.step_scale = float(scale)
    p.use_fixed_steps = int(fixed is not None)
    if fixed is not None:
        p.fixed_steps[0], p.fixed_steps[1] = float(fixed[0]), float(fixed[1])
    p.accelerated = int(bool(accelerated))
    p.max_iter = max_iter
    p.max_workgroups = int(max_workgroups)
    return p


def _entry_point():
    """the library with a GPU behind it (no GPU: _lib.PmxError -- there is no CPU path) and the device host arrays are sent to"""
    return _lib.require_gpu(), int(os.environ.get("PMX_DEVICE", "0"))


def run(Ys, As, Ss, prox_A, prox_S, step, accelerated, max_iter, e_rel, max_workgroups=0):
    Yl, Al, Sl = check_batch(Ys, As, Ss)
    p = batch_params(prox_A, prox_S, step, accelerated, max_iter, e_rel, max_workgroups)
    B = len(Yl)
    res = BatchResult(B)
    if B == 0:
        return res
    lib, device = _entry_point()
    items, Y, A, S = pack(Yl, Al, Sl)
    out = (_lib.BatchResult * B)()
    _lib.check(lib.pmx_nmf_batch_pgm(device, B, items, Y.ctypes.data_as(C.c_void_p), A.ctypes.data_as(C.c_void_p), S.ctypes.data_as(C.c_void_p),
                                     C.byref(p), out))
    unpack(items, A, S, Al, Sl)
    raw = np.frombuffer(out, dtype=np.dtype([("it_done", "<i4"), ("stopped", "<i4"), ("conv", "<i4", (2,)), ("step", "<f8", (2,)), ("norms", "<f8", (2, 2))]))
    res.iterations[:] = raw["it_done"]
    res.converged[:] = raw["conv"] != 0
    res.steps[:] = raw["step"].astype(np.float32)          # pgm returns its steps in the factors' dtype (algorithms.py:144)
    res.norms[:] = raw["norms"]
    ms = C.c_double()
    lib.pmx_batch_last_launch_ms(C.byref(ms))
    res.launch_ms = ms.value
    return res
