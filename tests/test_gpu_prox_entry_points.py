"""GPU: the stand-alone operator entry points of the C ABI give the same bits on the same float32 input.

One operator sequence on one rows x K float32 array through
  (a) pmx_prox_view on the dense host array (strides (K, 1)),
  (b) pmx_prox_array_tables (pmx_prox_array where the sequence names no table),
  (c) pmx_prox_apply on a context's buffer (DeviceNMF.prox_apply): the array as A (BUF_A) and as S^T (BUF_ST),
compared with np.testing.assert_array_equal.  (b) and (c) are float32 wrappers of what (a) runs: this is their regression test.

Shapes: the smallest that reach every instance and loop boundary of the kernel -- (7, 5): fewer rows than a workgroup's 32, one
value per lane, ragged K; (700, 33): two values per lane, ragged; (8225, 64): a second sweep of the 8192-row grid; (300, 128):
four values per lane.  Inputs are 0.25 + random, column sums far from zero, except where a case says otherwise.
"""
import ctypes as C

import numpy as np
import pytest

SHAPES = [(7, 5), (700, 33), (8225, 64), (300, 128)]
OTHER = 40                       # the other dimension of the context that holds the array as a factor


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _mixed_rows(K):
    """a per-component table with mixed rows, one kind of them prox_max_entropy"""
    kinds = [("soft", 0.3, 1), ("max_entropy", 0.4, 1), ("hard", 0.6, 0), ("plus", 0.0, 0), ("soft_plus", 0.2, 0)]
    return [kinds[k % len(kinds)] for k in range(K)]


def _cases(rows, K):
    """name -> (entries of operators._seq in the device layout (unit 1: along the rows), repeat, one all-negative column)"""
    return {
        "soft relative": ([("soft", 0, 0.3, 1)], 1, False),
        "max_entropy": ([("max_entropy", 0, 0.3, 1)], 1, False),
        "components, mixed rows": ([("components", 0, _mixed_rows(K), 0)], 1, False),
        "(unity rows, unity components, plus) x 2": ([("unity", 1, 0.0, 0), ("unity", 0, 0.0, 0), ("plus", 0, 0.0, 0)], 2, False),
        # (threshold: the mean entry of a column that sums to one)
        "unity_plus rows, hard absolute": ([("unity_plus", 1, 0.0, 0), ("hard", 0, 1.0 / rows, 0)], 1, False),
        "unity_plus rows, a column that sums to zero": ([("unity_plus", 1, 0.0, 0)], 1, True),
    }


def _flat_tables(_lib, tables, K):
    if not tables:
        return None
    flat = (_lib.Prox * (len(tables) * K))()
    for t, tab in enumerate(tables):
        C.memmove(C.byref(flat, t * K * C.sizeof(_lib.Prox)), tab, C.sizeof(tab))
    return flat


@pytest.mark.gpu
@pytest.mark.parametrize("rows,K", SHAPES, ids=lambda v: str(v))
def test_legacy_entry_points_give_the_bits_of_prox_view(rows, K):
    from proxmin_amd import _lib, operators
    from proxmin_amd.engine import DeviceNMF
    lib = _lib.require_gpu()
    rng = np.random.default_rng(rows + K)
    X0 = (0.25 + rng.random((rows, K))).astype(np.float32)
    Xneg = X0.copy()
    Xneg[:, K // 2] = -Xneg[:, K // 2]                   # plus empties the column: its total is 0 and 0 / 0 is NaN on every route
    other_A = np.ones((OTHER, K), np.float32)
    other_S = np.ones((K, OTHER), np.float32)
    steps = [np.full(K, 0.7, np.float32), np.linspace(0.5, 2.0, K).astype(np.float32)]
    with DeviceNMF(rows, OTHER, K, mode="f32") as as_A, DeviceNMF(OTHER, rows, K, mode="f32") as as_St:
        for name, (entries, repeat, negative) in _cases(rows, K).items():
            X = Xneg if negative else X0
            for sk in steps:
                what = "%s, steps %g .. %g" % (name, sk[0], sk[-1])
                ps = operators._seq(entries, repeat)
                tables = operators.seq_tables(ps)
                flat = _flat_tables(_lib, tables, K)
                # (a)
                view = X.copy()
                sk64 = sk.astype(np.float64)
                _lib.check(lib.pmx_prox_view(_vp(view), 0, 0, rows, K, K, 1, C.byref(ps), sk64.ctypes.data_as(C.POINTER(C.c_double)),
                                             flat, len(tables), 0))
                assert not np.array_equal(view, X, equal_nan=True), what
                # (b)
                arr = X.copy()
                if tables:
                    _lib.check(lib.pmx_prox_array_tables(0, _vp(arr), rows, K, C.byref(ps), _vp(sk), flat, len(tables)))
                else:
                    _lib.check(lib.pmx_prox_array(0, _vp(arr), rows, K, C.byref(ps), _vp(sk)))
                np.testing.assert_array_equal(arr, view, err_msg="pmx_prox_array*: " + what)
                # (c)
                as_A.set_factors(X, other_S)
                as_A.prox_apply(_lib.BUF_A, ps, sk)
                np.testing.assert_array_equal(as_A.get_factors()[0], view, err_msg="pmx_prox_apply on BUF_A: " + what)
                as_St.set_factors(other_A, np.ascontiguousarray(X.T))
                as_St.prox_apply(_lib.BUF_ST, ps, sk)
                np.testing.assert_array_equal(as_St.get_factors()[1].T, view, err_msg="pmx_prox_apply on BUF_ST: " + what)
                if negative:
                    nan = np.isnan(view)
                    assert nan[:, K // 2].all() and nan.sum() == rows, what
                else:
                    assert np.isfinite(view).all(), what
