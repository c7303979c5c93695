"""Proximal operators of the nmf() path -- same names, arguments and in-place behaviour as
proxmin/operators.py:20-184 -- backed by the HIP operator kernel (csrc/k_update.hip, prox_one).

Two uses:
  * passed to `nmf.nmf()` as `prox_A` / `prox_S` / `proxs_g` (bare, or wrapped in
    `functools.partial` for `axis=` / `thresh=` / `type=`, or combined with `AlternatingProjections`),
    they are recognised by identity -- the same test as AlternatingProjections.find,
    operators.py:213-224 -- and run FUSED inside the solver kernels; the Python bodies below are
    never called on that path;
  * called directly on an array they run the same operator code on that array, in the array's own element type like the
    reference (operators.py:33-38, :138-160): float64 arrays in fp64, float32 arrays in fp32 (every other dtype is computed in
    float32).  A host array goes to the GPU `PMX_DEVICE` names (default 0) and comes back (`pmx_prox_view` / `pmx_prox_flat`);
    an array that lives in HBM -- anything with `__cuda_array_interface__`, float32 or float64: a torch tensor on the GPU, a
    CuPy array -- is updated in place on its own GPU, nothing copied, and the object passed in is returned.  Element-wise
    operators with a scalar step take 1-D and C- or F-contiguous n-D arrays; wherever components, axes or per-component
    steps matter the array is a 2-D row- or column-major view with any pitch (e.g. `T[3:, :33]`, `St.T`).  `step`, `thresh`
    and `gamma` are host scalars or host arrays.  There is no NumPy implementation in this package.

Per-component parameters: `thresh` (`gamma`) of the threshold operators may be an array with one value per component, and
`prox_components` gives every component an operator of its own.  Both become one device entry PMX_PROX_COMPONENTS whose
table holds one (op, thresh, relative) row per component (include/pmx.h: pmx_prox_table).
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from . import _lib, engine

__all__ = ["prox_id", "prox_zero", "prox_plus", "prox_unity", "prox_unity_plus", "prox_min", "prox_max",
           "prox_hard", "prox_hard_plus", "prox_soft", "prox_soft_plus", "prox_max_entropy", "prox_components",
           "AlternatingProjections"]


# ---------------------------------------------------------------------------------------------
# direct application on arrays (host, or in HBM)
# ---------------------------------------------------------------------------------------------
# operators that work entry by entry: what a row of a per-component table may be (include/pmx.h: pmx_prox_table)
ELEMENTWISE = ("id", "zero", "plus", "min", "max", "hard", "hard_plus", "soft", "soft_plus", "max_entropy")


def _seq(entries, repeat=1):
    """entries: (op, unit, thresh, relative), or ("components", 0, rows, 0) with rows = [(op, thresh, relative)] * K: the rows
    go into `ps.tables` (a Python attribute: a list of K-row _lib.Prox arrays) and the entry's `reserved` is 1 + its index there.
    The engine uploads the tables and re-stamps `reserved` with the context's own index (engine.DeviceNMF._stamp_tables)."""
    ps = _lib.ProxSeq()
    ps.n = len(entries)
    ps.repeat = repeat
    ps.tables = []
    for i, (op, unit, thresh, relative) in enumerate(entries):
        if op == "components":
            tab = (_lib.Prox * len(thresh))()
            for k, (rop, rth, rrel) in enumerate(thresh):
                assert rop in ELEMENTWISE
                tab[k].op, tab[k].thresh, tab[k].relative = _lib.PROX[rop], float(rth), int(rrel)
            ps.tables.append(tab)
            ps.seq[i].op, ps.seq[i].reserved = _lib.PROX["components"], len(ps.tables)
            continue
        ps.seq[i].op, ps.seq[i].unit, ps.seq[i].thresh, ps.seq[i].relative = _lib.PROX[op], unit, float(thresh), int(relative)
    return ps


def seq_tables(seq):
    """the per-component tables a device operator sequence carries (a list of K-row _lib.Prox arrays; [] for none)"""
    return list(getattr(seq, "tables", None) or [])


def table_rows(tab):
    """one table as [(op code, thresh, relative)] * K"""
    return [(int(r.op), float(r.thresh), int(r.relative)) for r in tab]


def check_tables(seqs, K):
    """Every per-component table of these sequences has one row per component of the problem: ValueError otherwise (where the
    reference's broadcast of the thresholds against the factor would fail)."""
    for seq in seqs:
        for tab in seq_tables(seq):
            if len(tab) != K:
                raise ValueError("per-component operator parameters: %d values for a factorisation with K = %d components" % (len(tab), K))


def _work_dtype(dtype):
    """the element type an array of this dtype is computed in: its own for float32 and float64, float32 for every other"""
    return np.dtype(dtype) if np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.float64)) else np.dtype(np.float32)


def _host_device():
    """the GPU host arrays are sent to: PMX_DEVICE from the environment, else 0 (utils.BarzilaiBorweinStepper's rule); an array that
    lives on a GPU is worked on where it is"""
    return int(os.environ.get("PMX_DEVICE", "0"))


def _call_view(ptr, on_device, dtype, rows, K, s0, s1, ps, step_k):
    """pmx_prox_view: `ps` on rows x K elements of `dtype` (float32 / float64), element (r, k) at ptr + r * s0 + k * s1 elements"""
    lib = _lib.require_gpu()
    sk = np.ascontiguousarray(np.broadcast_to(np.asarray(step_k, dtype=np.float64).reshape(-1), (K,)))
    tables = seq_tables(ps)
    flat = None
    if tables:                           # per-component rows travel next to the sequence: ntables x K of them
        check_tables([ps], K)
        flat = (_lib.Prox * (len(tables) * K))()
        for t, tab in enumerate(tables):
            C.memmove(C.byref(flat, t * K * C.sizeof(_lib.Prox)), tab, C.sizeof(tab))
    _lib.check(lib.pmx_prox_view(C.c_void_p(ptr), int(on_device), int(np.dtype(dtype) == np.float64), rows, K, s0, s1, C.byref(ps),
                                 sk.ctypes.data_as(C.POINTER(C.c_double)), flat, len(tables), _host_device()))


def _call_flat(ptr, on_device, dtype, n, ps, step):
    """pmx_prox_flat: element-wise `ps` with one step on n contiguous elements"""
    lib = _lib.require_gpu()
    _lib.check(lib.pmx_prox_flat(C.c_void_p(ptr), int(on_device), int(np.dtype(dtype) == np.float64), n, C.byref(ps), float(step), _host_device()))


def _run_rows(rows2d, ps, step_k):
    """The one place HOST data meets the device.  `ps` on a two-dimensional host array seen as rows of components (step_k: one
    step, or one per component), or -- a one-dimensional array -- on its elements with the one step `step_k` (the flat form:
    element-wise operators only).  -> the result in the dtype it was computed in: the argument itself, updated in place, where it
    is a dense row-major float32 / float64 array, else a new array."""
    buf = np.ascontiguousarray(rows2d, dtype=_work_dtype(rows2d.dtype))
    if buf.ndim == 1:
        if buf.size:
            _call_flat(buf.ctypes.data, False, buf.dtype, buf.size, ps, step_k)
        return buf
    _call_view(buf.ctypes.data, False, buf.dtype, buf.shape[0], buf.shape[1], buf.shape[1], 1, ps, step_k)
    return buf


class _Operand:
    """What an operator was called on.  A host array (anything np.asarray takes) is computed in its own dtype when that is float32
    or float64 -- in place where its layout allows, else through a contiguous copy -- and in float32 otherwise.  An array in HBM
    (engine.DeviceOperandRef: `__cuda_array_interface__`, float32 / float64) is updated where it lives; nothing is copied.
    `X` is what the operator returns: the caller's own object (the ndarray made of it for host data that was not one)."""

    def __init__(self, X):
        self.ref = engine.as_device_operand(X)
        if self.ref is not None:
            self.X, self.shape, self.dtype = X, self.ref.shape, self.ref.dtype
        else:
            self.X = X if isinstance(X, np.ndarray) else np.asarray(X)
            if not self.X.flags.writeable:       # (dense arrays are updated through their address: NumPy's own check would be bypassed)
                raise ValueError("assignment destination is read-only")
            self.shape, self.dtype = self.X.shape, self.X.dtype
        self.ndim = len(self.shape)
        self.on_device = self.ref is not None

    def run_rows(self, axis, ps, step_k, c0=0, c1=None):
        """`ps` on the two-dimensional array seen as rows of components, the components running along `axis` (1: the array as it
        is, 0: its transpose), on components [c0, c1) of that view only"""
        if self.on_device:
            st = self.ref.strides if axis == 1 else self.ref.strides[::-1]
            rows, ncol = self.shape if axis == 1 else self.shape[::-1]
            c1 = ncol if c1 is None else min(c1, ncol)
            _call_view(self.ref.ptr + c0 * st[1] * self.dtype.itemsize, True, self.dtype, rows, c1 - c0, st[0], st[1], ps, step_k)
            return
        V = self.X if axis == 1 else self.X.T
        if c0 != 0 or (c1 is not None and c1 < V.shape[1]):
            V = V[:, c0:c1]
        out = _run_rows(V, ps, step_k)
        if out is not V:
            V[...] = out

    def run_flat(self, ps, step):
        """element-wise `ps` with the scalar `step` on every element"""
        if self.on_device:
            if self.ref.flat:
                if self.ref.size:
                    _call_flat(self.ref.ptr, True, self.dtype, self.ref.size, ps, step)
                return
            # a pitched two-dimensional view: its row-major orientation in groups of at most MAXK columns
            axis = 1 if self.ref.strides[1] == 1 else 0
            for c0 in range(0, self.shape[axis], _lib.MAXK):
                self.run_rows(axis, ps, step, c0, c0 + _lib.MAXK)
            return
        Xw = self.X.T if self.X.flags.f_contiguous and not self.X.flags.c_contiguous else self.X
        out = _run_rows(Xw.reshape(-1), ps, step)            # (a view of a contiguous array, a copy of any other)
        if not np.may_share_memory(out, Xw):
            Xw[...] = out.reshape(Xw.shape)


def _scalar_or_array(thresh):
    """-> (float, None) for a scalar or a size-1 array, (None, float64 array) for anything larger"""
    if np.ndim(thresh) == 0:
        return float(thresh), None
    arr = np.asarray(thresh, dtype=np.float64)
    if arr.size == 1:
        return float(arr.reshape(-1)[0]), None
    return None, arr


def _component_axis(shape, X_shape):
    """Which axis of a 2-D X an array of this shape indexes when it broadcasts one value per component: 1 for (K,) / (1, K) with
    K = X.shape[1] (how A holds its components), 0 for (K, 1) with K = X.shape[0] (S); None: it does not."""
    if len(X_shape) != 2:
        return None
    if shape in ((X_shape[1],), (1, X_shape[1])):
        return 1
    if shape == (X_shape[0], 1):
        return 0
    return None


def _apply_rows(A, step, rows, axis):
    """One per-component table (rows[k] = (op, thresh, relative) of component k along `axis` of the 2-D operand A) on A in place."""
    K = A.shape[axis]
    if K > _lib.MAXK:
        raise NotImplementedError("per-component operator parameters for %d components (at most %d)" % (K, _lib.MAXK))
    if len(rows) != K:
        raise ValueError("per-component operator parameters: %d values for %d components along axis %d of X %s" % (len(rows), K, axis, A.shape))
    step_arr = np.asarray(step, dtype=np.float64)
    if step_arr.ndim == 0 or step_arr.size == 1:
        sk = float(step_arr.reshape(-1)[0]) if step_arr.size else 0.0
    elif _component_axis(step_arr.shape, A.shape) == axis:
        sk = step_arr.reshape(-1)
    else:
        raise NotImplementedError("step of shape %s next to per-component parameters along axis %d of X %s" % (step_arr.shape, axis, A.shape))
    A.run_rows(axis, _seq([("components", 0, rows, 0)]), sk)
    return A.X


def _apply(X, step, op, axis=None, thresh=0.0, kind="relative"):
    """Run one operator on X in place, in X's own element type (float32 and float64; any other dtype is computed in float32):
    a host array, or an array in HBM (`__cuda_array_interface__`), which is updated where it lives.  Returns the caller's object."""
    assert kind in ["relative", "absolute"]
    A = _Operand(X)
    rel = kind == "relative"
    step_arr = np.asarray(step, dtype=np.float64)
    if op in ("unity", "unity_plus"):
        if A.ndim != 2 or axis not in (0, 1):
            raise NotImplementedError("prox_unity on the device needs a 2-D array and axis in (0, 1)")
        if A.shape[axis] <= _lib.MAXK:
            A.run_rows(axis, _seq([(op, 0, 0.0, 0)]), 0.0)
            return A.X
        # long normalised axis: sums over the ROWS of the view whose components run along the other axis (column sums folded
        # across the grid), that axis in groups of at most MAXK independent columns
        for c0 in range(0, A.shape[1 - axis], _lib.MAXK):
            A.run_rows(1 - axis, _seq([(op, 1, 0.0, 0)]), 0.0, c0, c0 + _lib.MAXK)
        return A.X
    thresh, per_k = _scalar_or_array(thresh)
    if per_k is not None:               # one threshold per component: the shapes that broadcast along X's components
        axis = _component_axis(per_k.shape, A.shape)
        if axis is None:
            raise NotImplementedError("thresh of shape %s on X of shape %s: per-component thresholds only ((K,) / (1, K) along axis 1, "
                                      "(K, 1) along axis 0); per-row and per-element thresholds are not built" % (per_k.shape, A.shape))
        return _apply_rows(A, step, [(op, t, rel) for t in per_k.reshape(-1)], axis)
    ps = _seq([(op, 0, thresh, rel)])
    if step_arr.ndim == 0 or step_arr.size == 1 or not rel or op in ("id", "zero", "plus"):
        A.run_flat(ps, float(step_arr.reshape(-1)[0]) if step_arr.size else 0.0)
        return A.X
    # per-component step (what adaprox passes: shape (K,) for A, (K,1) for S -- nmf.py:93)
    if A.ndim == 2 and step_arr.shape in ((A.shape[1],), (1, A.shape[1])) and A.shape[1] <= _lib.MAXK:
        A.run_rows(1, ps, step_arr.reshape(-1))
        return A.X
    if A.ndim == 2 and step_arr.shape == (A.shape[0], 1) and A.shape[0] <= _lib.MAXK:
        A.run_rows(0, ps, step_arr.reshape(-1))
        return A.X
    raise NotImplementedError("step of shape %s does not broadcast per component over X of shape %s" % (step_arr.shape, A.shape))


def prox_id(X, step):
    """Identity proximal operator (operators.py:20-23)."""
    return X


def prox_zero(X, step):
    """Projection onto zero (operators.py:26-30)."""
    return _apply(X, step, "zero")


def prox_plus(X, step):
    """Projection onto non-negative numbers (operators.py:33-38)."""
    return _apply(X, step, "plus")


def prox_unity(X, step, axis=0):
    """Projection onto sum=1 along an axis (operators.py:41-45).  Along a factor's long axis (axis=0 on A, axis=1 on S) it
    runs fused inside pgm / FISTA (one more launch per application); adaprox and bsdmm apply it between kernel launches."""
    return _apply(X, step, "unity", axis=axis)


def prox_unity_plus(X, step, axis=0):
    """Non-negative projection onto sum=1 along an axis (operators.py:48-52).  Long axis: see prox_unity."""
    return _apply(X, step, "unity_plus", axis=axis)


def prox_min(X, step, thresh=0, type="relative"):
    """Projection onto numbers above `thresh` (operators.py:55-68).
    `thresh` may be an array with one value per component ((K,) / (1, K) next to an M x K array, (K, 1) next to a K x N one):
    component k is projected onto numbers above thresh[k] -- the evident broadcast; the reference raises on an array here
    (boolean-index assignment of an array).  Arrays per row or per element raise NotImplementedError."""
    return _apply(X, step, "min", thresh=thresh, kind=type)


def prox_max(X, step, thresh=0, type="relative"):
    """Projection onto numbers below `thresh` (operators.py:71-84).
    `thresh` may be an array with one value per component, as for prox_min: component k is projected onto numbers below
    thresh[k] (the reference raises on an array here).  Arrays per row or per element raise NotImplementedError."""
    return _apply(X, step, "max", thresh=thresh, kind=type)


def prox_hard(X, step, thresh=0, type="relative"):
    """Hard thresholding (operators.py:109-124).
    `thresh` may be an array with one value per component ((K,) / (1, K) next to an M x K array, (K, 1) next to a K x N one),
    as in the reference, where it broadcasts; arrays per row or per element raise NotImplementedError (not built)."""
    return _apply(X, step, "hard", thresh=thresh, kind=type)


def prox_hard_plus(X, step, thresh=0, type="relative"):
    """Hard thresholding with projection onto non-negative numbers (operators.py:127-135).
    `thresh` may be an array with one value per component ((K,) / (1, K) next to an M x K array, (K, 1) next to a K x N one),
    as in the reference, where it broadcasts; arrays per row or per element raise NotImplementedError (not built)."""
    return _apply(X, step, "hard_plus", thresh=thresh, kind=type)


def prox_soft(X, step, thresh=0, type="relative"):
    """Soft thresholding (operators.py:138-150).
    `thresh` may be an array with one value per component ((K,) / (1, K) next to an M x K array, (K, 1) next to a K x N one),
    as in the reference, where it broadcasts; arrays per row or per element raise NotImplementedError (not built)."""
    return _apply(X, step, "soft", thresh=thresh, kind=type)


def prox_soft_plus(X, step, thresh=0, type="relative"):
    """Soft thresholding with projection onto non-negative numbers (operators.py:153-160).
    `thresh` may be an array with one value per component ((K,) / (1, K) next to an M x K array, (K, 1) next to a K x N one),
    as in the reference, where it broadcasts; arrays per row or per element raise NotImplementedError (not built)."""
    return _apply(X, step, "soft_plus", thresh=thresh, kind=type)


def prox_max_entropy(X, step, gamma=1, type="relative"):
    """Proximal operator of the entropy regulariser g(x) = gamma sum x ln x (operators.py:163-184), in place:
    with gamma_ = gamma * step ("relative") or gamma ("absolute"), every entry x > 0 becomes the y > 0 with
    y + gamma_ ln y = x - gamma_, i.e. gamma_ W(exp(x / gamma_ - 1) / gamma_) with the principal Lambert W.
    Entries <= 0, NaN and -inf keep their value, +inf stays +inf (so the operator jumps at 0, as the reference's does).

    `gamma` may be an array with one value per component ((K,) / (1, K) next to an M x K array, (K, 1) next to a K x N one):
    component k is regularised with gamma[k] -- the evident broadcast, on which the reference raises (a broadcast error); arrays
    per row or per element raise NotImplementedError.

    Three more differences from the reference, all of them where the reference has no usable answer:
      * the equation is solved in the log domain, so the result is finite for every finite x > 0 -- the reference's
        exp(x / gamma_ - 1) overflows to inf above 88.7 (float32 arrays) / 709 (float64);
      * a per-component or per-element `step` with type="relative" (what adaprox passes; step arrays in pgm) applies
        gamma * step element by element -- the broadcasting the reference intends and raises on (ValueError / TypeError);
      * where gamma_ is <= 0 or NaN the entries > 0 become NaN (the reference writes NaN at 0 and numbers without
        meaning below 0)."""
    if isinstance(X, np.ndarray) and _work_dtype(X.dtype) != X.dtype:
        # a dtype that is computed in float32 (neither float32 nor float64): the entries the operator does not touch keep their
        # own value, not its float32 rounding -- "only entries > 0 change"
        keep = ~(X > 0)
        kept = X[keep]
        _apply(X, step, "max_entropy", thresh=gamma, kind=type)
        X[keep] = kept
        return X
    return _apply(X, step, "max_entropy", thresh=gamma, kind=type)


def _component_rows(prox, K, block=None):
    """The table of prox_components(prox=...) over K components, [(op, thresh, relative)] * K -- or None when a member is not
    an element-wise operator of this module with scalar parameters (bare or a keyword-only partial)."""
    members = list(prox) if isinstance(prox, (list, tuple)) else [prox] * K
    rows = []
    for q in members:
        try:
            e = _one_entry(q, 0 if block is None else block)
        except NotImplementedError:
            return None
        if e is None or e[0] not in ELEMENTWISE:
            return None
        rows.append((e[0], e[2], e[3]))
    return rows


def prox_components(X, step, prox=None, axis=0):
    """Component k of X along `axis` (X[k] for axis=0, X[:, k] for axis=1) gets its own operator prox[k](., step), in place
    (the contract of operators.py:87-103, whose body reads an undefined name and cannot run).  `prox` is one callable -- every
    component gets it -- or a list with one callable per component (ValueError for another length).

    Members that are element-wise operators of this module with scalar parameters run as ONE device kernel with a
    per-component table (2-D X, at most 128 components); any other callable is called on its component's host view -- for an X
    that lives on the GPU there is no such view: NotImplementedError.
    Difference from the reference's contract: a per-component `step` -- shape (K,) / (1, K) with axis=1, (K, 1) with axis=0,
    what adaprox passes -- reaches member k as component k's own step; the reference would hand every member the whole array."""
    A = _Operand(X)
    if axis not in (0, 1) or A.ndim <= axis:
        raise NotImplementedError("prox_components: axis %r of an array of shape %s" % (axis, A.shape))
    K = A.shape[axis]
    members = list(prox) if isinstance(prox, (list, tuple)) else [prox] * K
    if len(members) != K:
        raise ValueError("prox_components: %d operators for %d components along axis %d of X %s" % (len(members), K, axis, A.shape))
    if A.ndim == 2 and K <= _lib.MAXK:
        rows = _component_rows(members, K)
        if rows is not None:
            return _apply_rows(A, step, rows, axis)
    if A.on_device:
        raise NotImplementedError("prox_components on an array that lives on the GPU runs as one device kernel with a per-component table: a 2-D "
                                  "array, at most %d components, every member an element-wise operator of proxmin_amd.operators with scalar "
                                  "parameters (got shape %s, axis %d, members %r); there is no host view to hand another callable"
                                  % (_lib.MAXK, A.shape, axis, members))
    X = A.X
    step_arr = np.asarray(step)
    per_k = step_arr.size > 1 and _component_axis(step_arr.shape, X.shape) == axis
    for k in range(K):
        Xk = X[k] if axis == 0 else X[:, k]
        Xk[...] = members[k](Xk, step_arr.reshape(-1)[k] if per_k else step)
    return X


class AlternatingProjections(object):
    """POCS composition of several operators (operators.py:187-224): the list is applied
    last-to-first, `repeat` times.  Inside nmf() a list of built-ins becomes one fused device
    operator sequence; called directly it applies the members one after the other."""

    def __init__(self, prox_list=None, repeat=1):
        self.operators = []
        self.repeat = repeat
        if prox_list is not None:
            self.operators += prox_list

    def __call__(self, X, step):
        for _ in range(self.repeat):
            for prox in self.operators[::-1]:
                X = prox(X, step)
        return X

    def find(self, cls):
        for i, prox in enumerate(self.operators):
            if isinstance(prox, functools.partial):
                if prox.func is cls:
                    return i
            elif prox is cls:
                return i
        return -1


# ---------------------------------------------------------------------------------------------
# recognition of built-ins (used by nmf(): callable -> device operator sequence)
# ---------------------------------------------------------------------------------------------
_BY_FUNC = {prox_id: "id", prox_zero: "zero", prox_plus: "plus", prox_unity: "unity", prox_unity_plus: "unity_plus",
            prox_min: "min", prox_max: "max", prox_hard: "hard", prox_hard_plus: "hard_plus",
            prox_soft: "soft", prox_soft_plus: "soft_plus", prox_max_entropy: "max_entropy", prox_components: "components"}


def _one_entry(prox, block):
    func, kw = prox, {}
    if isinstance(prox, functools.partial):
        if prox.args:
            return None
        func, kw = prox.func, dict(prox.keywords)
    op = _BY_FUNC.get(func)
    if op is None:
        return None
    if op in ("unity", "unity_plus"):
        axis = kw.pop("axis", 0)
        if kw or axis not in (0, 1):
            return None
        # device layout: A is M x K, S is held as S^T (N x K).  unit 0 = along the K components.
        unit = 0 if (block == 0 and axis == 1) or (block == 1 and axis == 0) else 1
        return (op, unit, 0.0, 0)
    if op in ("id", "zero", "plus"):
        return None if kw else (op, 0, 0.0, 0)
    if op == "components":
        # fused when `axis` is the block's component axis (1 for A, 0 for S: unit == 0 above) and every member is an element-wise
        # operator with scalar parameters; everything else is a user prox (plain NotImplementedError: the host route)
        members, axis = kw.pop("prox", None), kw.pop("axis", 0)
        if kw or members is None:
            return None
        if axis != (1 if block == 0 else 0):
            raise NotImplementedError("prox_components along axis %r of block %d: fused along the component axis only (axis=1 on A, "
                                      "axis=0 on S)" % (axis, block))
        if not isinstance(members, (list, tuple)):             # one callable for every component: the operator itself
            rows = _component_rows(members, 1, block)
            if rows is None:
                raise NotImplementedError("prox_components of %r: not an element-wise operator of proxmin_amd.operators" % (members,))
            return (rows[0][0], 0, rows[0][1], rows[0][2])
        rows = _component_rows(members, len(members), block)
        if rows is None or not rows:
            raise NotImplementedError("prox_components with a member that is not an element-wise operator of proxmin_amd.operators "
                                      "with scalar parameters: %r" % (members,))
        return ("components", 0, rows, 0)
    thresh = kw.pop("gamma", 1) if op == "max_entropy" else kw.pop("thresh", 0)
    kind = kw.pop("type", "relative")
    if kw:
        return None
    assert kind in ["relative", "absolute"]
    thresh, per_k = _scalar_or_array(thresh)
    if per_k is not None:
        # one value per component: (K,) / (1, K) on A (M x K), (K, 1) on S (K x N); the reference would also broadcast per-row
        # and per-element shapes, which are not built
        ok = per_k.ndim == 2 and per_k.shape[1] == 1 if block == 1 else (per_k.ndim == 1 or (per_k.ndim == 2 and per_k.shape[0] == 1))
        if not ok:
            raise NotImplementedError("%s of shape %s on block %d: per-component values only ((K,) or (1, K) on A, (K, 1) on S); "
                                      "per-row and per-element shapes are not built" % ("gamma" if op == "max_entropy" else "thresh", per_k.shape, block))
        return ("components", 0, [(op, t, kind == "relative") for t in per_k.reshape(-1)], 0)
    return (op, 0, thresh, kind == "relative")


class NotFusable(NotImplementedError):
    """An operator of this module that the solver asked about does not contain: prox_unity* along the long axis, a
    grid-wide sum per application.  pgm / FISTA run it on the device (the update becomes a chain of launches, one more per
    application: for_solver="pgm") unless the call has a line search, a user grad / step / prox or fp64 kernels; adaprox,
    bsdmm and those pgm calls apply it between kernel launches by calling it on the host copy of its argument -- which
    runs the stand-alone device operator kernel -- one iteration per call."""


def has_tables(seq):
    """Does a device operator sequence hold a per-component entry (PMX_PROX_COMPONENTS)?"""
    return any(seq.seq[i].op == _lib.PROX["components"] for i in range(seq.n))


def is_components(prox):
    """prox_components, bare or as a partial (whatever its members)"""
    return (prox.func if isinstance(prox, functools.partial) else prox) is prox_components


def has_long_axis(seq):
    """Does a device operator sequence hold prox_unity* along the long axis of its block (pmx_prox.unit != 0)?"""
    return any(seq.seq[i].unit != 0 for i in range(seq.n))


def device_proxseq(prox, block, for_solver=False):
    """Translate a prox callable into a device operator sequence for factor `block` (0 = A, 1 = S).
    Returns a _lib.ProxSeq (n == 0 for prox=None) or raises NotImplementedError for callables that
    are not (compositions of) this module's operators.  for_solver: also raise (NotFusable) for operators that the
    solver's kernels do not contain -- True: adaprox, bsdmm and every host-driven route; "pgm": the fused pgm / FISTA
    chain, which takes prox_unity* along the long axis."""
    if for_solver and prox is not None:
        seq = device_proxseq(prox, block)
        if for_solver != "pgm" and has_long_axis(seq):
            raise NotFusable("prox_unity along the long axis of block %d is applied between kernel launches" % block)
        return seq
    if prox is None:
        return _seq([])
    if isinstance(prox, AlternatingProjections):
        entries = [_one_entry(q, block) for q in prox.operators[::-1]]
        if any(e is None for e in entries) or len(entries) > _lib.MAX_SEQ:
            raise NotImplementedError("AlternatingProjections of user-defined operators (or more than %d) cannot run on the device" % _lib.MAX_SEQ)
        return _seq(entries, repeat=int(prox.repeat))
    e = _one_entry(prox, block)
    if e is None:
        raise NotImplementedError(
            "prox %r is not one of proxmin_amd.operators (bare, functools.partial or AlternatingProjections): "
            "user-defined Python prox callables are not supported on the device path" % (prox,))
    return _seq([e])
