"""GPU: operators called on arrays work in the array's own element type, and on arrays that live in HBM in place.

1. float64 against the outputs recorded from the reference (tests/golden/operators.npz): bit for bit where every output entry is an
   input entry, 0 or the one product thresh * step; soft thresholding within two roundings and a contraction; prox_unity* against a
   long-double evaluation within the summation bound that holds for any order.
2. float64 values that float32 cannot hold (1e300, 1e-310), and a threshold of 1e-9 on values of order 1.
3. prox_max_entropy in float64: the optimality condition to the bound the fp64 solver kernels meet.
4. a torch tensor on the GPU and its host copy give the same bytes: every operator, both types, scalar and per-component
   parameters, prox_components, AlternatingProjections.
5. views (pitch, a start at row 3, column-major, the long axis): the same bytes as the host call on the NumPy view, and every
   byte of the parent tensor outside the view (a NaN payload pattern) stays.
6. a tensor produced on a side stream without synchronisation.    7. which GPU.

Shapes are the smallest that reach each path: K = 3 / 33 / 100 (1 / 2 / 4 values per lane), 8225 rows (second sweep of the row
loop), n = 5 and 128 * 7 + 5 (flat tails), 300 x 260 (wider than 128 components), 37 x 7 and 8225 x 40 (column-major tile edges)."""
import importlib.util
import json
import os
from functools import partial

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from proxmin_amd import operators as ops

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_max_entropy_golden", os.path.join(GOLDEN, "make_max_entropy_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)                       # (imports the reference only inside its main())
EPS64 = 2.0 ** -53
DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]


@pytest.fixture(scope="module")
def torch():
    import __graft_entry__ as g
    g.build()
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ---- 1. float64 against the reference's recorded outputs -----------------------------------------------------------------------------
def _fixture_fn(spec):
    fn = getattr(ops, "prox_" + spec[0])
    if spec[0] in ("unity", "unity_plus"):
        return partial(fn, axis=spec[1])
    return partial(fn, thresh=spec[1], type=spec[2]) if len(spec) > 1 else fn


def test_float64_fixture(built):
    z, meta = load_golden("operators.npz")
    seen = set()
    for e in meta["entries"]:
        k, spec = e["key"], e["spec"]
        if z[k + "/X"].dtype != np.float64:
            continue
        X, step, want = z[k + "/X"].copy(), z[k + "/step"], z[k + "/out"]
        inp = X.copy()
        step = float(step) if step.ndim == 0 else step
        out = _fixture_fn(spec)(X, step)
        assert out is X and X.dtype == np.float64
        seen.add(spec[0])
        if spec[0] in ("id", "zero", "plus", "min", "max", "hard", "hard_plus"):
            assert np.array_equal(_bits(X), _bits(want)), e
        elif spec[0] in ("soft", "soft_plus"):
            t = np.abs(np.asarray(spec[1]) * (np.asarray(step) if spec[2] == "relative" else 1.0))
            bound = 2.0 * 2.0 ** -52 * np.maximum(np.abs(inp), t)
            err = np.abs(X - want)
            print("%s %s: worst error / bound %.3f" % (k, spec, (err / bound).max()))
            assert (err <= bound).all(), e
        else:
            axis = spec[1]
            x = inp.astype(np.longdouble)
            if spec[0] == "unity_plus":
                x = np.where(x < 0, np.longdouble(0), x)
            s = x.sum(axis=axis, keepdims=True)
            ref = x / s
            n = inp.shape[axis]
            bound = (n + 2) * 2.0 ** -53 * np.asarray(np.abs(x).sum(axis=axis, keepdims=True) / np.abs(s), dtype=np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                rel = np.asarray(np.abs(X.astype(np.longdouble) - ref) / np.abs(ref), dtype=np.float64)
            rel = np.where(ref == 0, np.abs(X), rel)                # (a clamped entry: 0 / s is exactly 0)
            print("%s %s: worst error / bound %.3f" % (k, spec, (rel / np.broadcast_to(bound, rel.shape)).max()))
            assert (rel <= bound).all(), e
    assert seen == {"id", "zero", "plus", "min", "max", "hard", "hard_plus", "soft", "soft_plus", "unity", "unity_plus"}


# ---- 2. float64 beyond float32 -------------------------------------------------------------------------------------------------------
def test_float64_beyond_float32_range(built):
    rng = np.random.default_rng(11)
    n = 128 * 7 + 5
    special = np.array([1e300, -1e300, 1e-310, -1e-310, 0.0, -0.0, np.nan, np.inf, -np.inf, 3e-39, -2e39, 0.21, -0.21])
    x = np.concatenate([special, rng.standard_normal(n - special.size) * 10.0 ** rng.integers(-300, 300, n - special.size)])
    thresh, step = 0.3, 0.7
    with np.errstate(invalid="ignore"):
        # the reference's formulas (operators.py:33-38, :55-68, :109-125) in NumPy's float64
        plus = x.copy()
        plus[plus < 0] = 0
        low = x.copy()
        low[low - thresh * step < 0] = thresh * step
        hard = x.copy()
        hard[np.abs(hard) < thresh * step] = 0
    for prox, want in ((ops.prox_plus, plus), (partial(ops.prox_min, thresh=thresh), low), (partial(ops.prox_hard, thresh=thresh), hard)):
        X = x.copy()
        assert prox(X, step) is X
        assert np.array_equal(_bits(X), _bits(want)), prox
    assert hard[0] == 1e300 and hard[1] == -1e300 and hard[2] == 0 and np.isnan(hard[6]) and hard[7] == np.inf and hard[8] == -np.inf
    assert plus[2] == 1e-310 and low[3] == thresh * step


def test_float64_small_threshold(built):
    """thresh = 1e-9 on values of order 1: the float32 round trip loses it altogether (2^-24 = 6e-8 relative)"""
    rng = np.random.default_rng(12)
    x = rng.standard_normal(128 * 7 + 5)
    thresh, step = 1e-9, 0.75
    X = x.copy()
    ops.prox_soft(X, step, thresh=thresh)
    t = np.longdouble(thresh) * np.longdouble(step)
    xl = x.astype(np.longdouble)
    ref = np.sign(xl) * np.maximum(np.abs(xl) - t, np.longdouble(0))
    err = np.asarray(np.abs(X.astype(np.longdouble) - ref), dtype=np.float64)
    bound = 2.0 * 2.0 ** -52 * np.maximum(np.abs(x), thresh * step)
    print("soft 1e-9: worst error / bound %.3f" % (err / bound).max())
    assert (err <= bound).all()
    assert (X != x).all()                                               # (the threshold did act)


# ---- 3. prox_max_entropy in float64 --------------------------------------------------------------------------------------------------
_ME = json.loads(str(np.load(os.path.join(GOLDEN, "max_entropy.npz"), allow_pickle=False)["meta"]))["op"]


def _residual_error(y, x, g_):
    """|dy| / y of a result y for input x from the optimality condition, in extended precision (tests/test_gpu_max_entropy.py)"""
    y, x, g_ = (np.asarray(v, dtype=np.longdouble) for v in (y, x, g_))
    F = y + g_ * np.log(y) - x + g_
    return np.asarray(np.abs(F) / (y + g_), dtype=np.float64)


@pytest.mark.parametrize("name", sorted(_ME))
def test_max_entropy_float64(built, name):
    c = _ME[name]
    g_ = gen.gamma_eff(c["gamma"], c["type"], c["step"])
    X = gen.operator_inputs(tuple(c["shape"]), g_, c["seed"])
    inp = X.copy()
    assert ops.prox_max_entropy(X, c["step"], gamma=c["gamma"], type=c["type"]) is X
    want = np.load(os.path.join(GOLDEN, "max_entropy.npz"), allow_pickle=False)[name + "/ref64"]
    touched = inp > 0
    assert np.array_equal(_bits(X[~touched]), _bits(inp[~touched])) and (~touched).sum() >= 8       # <= 0, -0.0, NaN, -inf: their own bits
    inf = touched & np.isinf(inp)
    assert inf.sum() == 1 and (X[inf] == np.inf).all()
    fin = touched & ~inf
    assert np.isfinite(X[fin]).all() and (X[fin] > 0).all()
    rel = _residual_error(X[fin], inp[fin], g_)
    bd = gen.bound(want[fin], inp[fin], g_, EPS64)
    print("%s: worst error / bound %.3f over %d entries" % (name, (rel / bd).max(), fin.sum()))
    assert (rel <= bd).all(), float((rel / bd).max())


# ---- 4. device-resident == host, bit for bit -----------------------------------------------------------------------------------------
THRESH_OPS = [ops.prox_min, ops.prox_max, ops.prox_hard, ops.prox_hard_plus, ops.prox_soft, ops.prox_soft_plus]


def _operators(K):
    """every operator with the components along axis 1 of a rows x K array: scalar and per-component parameters"""
    rng = np.random.default_rng(K)
    th = rng.uniform(0.05, 0.6, K)
    L = [ops.prox_zero, ops.prox_plus, partial(ops.prox_unity, axis=1), partial(ops.prox_unity_plus, axis=1), partial(ops.prox_unity, axis=0),
         partial(ops.prox_unity_plus, axis=0)]
    for f in THRESH_OPS:
        L += [partial(f, thresh=0.3), partial(f, thresh=th), partial(f, thresh=0.2, type="absolute")]
    L += [partial(ops.prox_max_entropy, gamma=0.7), partial(ops.prox_max_entropy, gamma=th)]
    members = [ops.prox_plus, partial(ops.prox_soft, thresh=0.1), partial(ops.prox_hard, thresh=0.4, type="absolute"), ops.prox_id,
               partial(ops.prox_max_entropy, gamma=0.5), partial(ops.prox_min, thresh=-0.2)]
    L += [partial(ops.prox_components, prox=[members[k % len(members)] for k in range(K)], axis=1),
          ops.AlternatingProjections([partial(ops.prox_unity, axis=1), ops.prox_plus], repeat=2)]
    return L


def _same_on_device(torch, prox, host, step):
    """prox on a copy of the host array and on its copy in HBM -> the same bytes, and the tensor itself comes back"""
    t = torch.from_numpy(host.copy()).cuda()
    h = host.copy()
    assert prox(t, step) is t
    prox(h, step)
    assert t.cpu().numpy().tobytes() == h.tobytes(), prox


@pytest.mark.parametrize("per_component_step", [False, True], ids=["scalar-step", "step-per-component"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(37, 3), (8225, 33), (41, 100)], ids=lambda s: "%dx%d" % s)
def test_device_resident_equals_host(torch, shape, dtype, per_component_step):
    rng = np.random.default_rng(shape[0])
    X = rng.standard_normal(shape).astype(dtype)
    step = rng.uniform(0.25, 1.0, shape[1]) if per_component_step else 0.5
    for prox in _operators(shape[1]):
        _same_on_device(torch, prox, X, step)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(5,), (128 * 7 + 5,), (3, 5, 7)], ids=["n5", "n901", "3x5x7"])
def test_flat_form_on_the_device(torch, shape, dtype):
    X = np.random.default_rng(5).standard_normal(shape).astype(dtype)
    for prox in [ops.prox_zero, ops.prox_plus, partial(ops.prox_max_entropy, gamma=0.7)] + [partial(f, thresh=0.3) for f in THRESH_OPS]:
        _same_on_device(torch, prox, X, 0.5)
    want = np.sign(X) * np.maximum(np.abs(X) - dtype(0.3) * dtype(0.5), 0)          # (and the tail is computed, not just equal)
    got = torch.from_numpy(X.copy()).cuda()
    ops.prox_soft(got, 0.5, thresh=0.3)
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=8 * np.finfo(dtype).eps)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_wider_than_128(torch, dtype):
    X = (np.random.default_rng(6).random((300, 260)) + 0.1).astype(dtype)
    for prox in (partial(ops.prox_unity, axis=0), partial(ops.prox_unity_plus, axis=1), partial(ops.prox_soft, thresh=0.3)):
        _same_on_device(torch, prox, X, 0.5)
    t = torch.from_numpy(X.copy()).cuda()
    ops.prox_unity(t, 0.5, axis=0)
    np.testing.assert_allclose(t.cpu().numpy().sum(axis=0, dtype=np.float64), 1.0, rtol=300 * np.finfo(dtype).eps)


# ---- 5. views ------------------------------------------------------------------------------------------------------------------------
def _payload(shape, dtype):
    """a parent tensor whose every element is a NaN with its own payload"""
    n = int(np.prod(shape))
    if dtype == np.float64:
        b = np.uint64(0x7ff8000000000000) | (np.arange(n, dtype=np.uint64) + np.uint64(1))
    else:
        b = np.uint32(0x7fc00000) | (np.arange(n, dtype=np.uint32) % np.uint32(0x3ffff0) + np.uint32(1))
    return b.view(dtype).reshape(shape).copy()


K40 = np.random.default_rng(40).uniform(0.05, 0.6, (40, 1))
K7 = np.random.default_rng(7).uniform(0.05, 0.6, (7, 1))
VIEWS = {
    # name: (parent shape, view of the parent, operator)
    "first-33-columns-soft": ((8225, 70), lambda P: P[:, :33], partial(ops.prox_soft, thresh=0.3)),
    "first-33-columns-unity": ((8225, 70), lambda P: P[:, :33], partial(ops.prox_unity_plus, axis=1)),
    "first-33-columns-long-axis": ((8225, 70), lambda P: P[:, :33], partial(ops.prox_unity, axis=0)),
    "transposed-NxK-thresholds": ((8225, 40), lambda P: P.T, partial(ops.prox_soft, thresh=K40)),
    "row-3-and-column-1": ((45, 70), lambda P: P[3:, 1:34], partial(ops.prox_unity_plus, axis=1)),
    # an axis of extent 1 whose other axis is not the unit stride: not one contiguous run
    "single-column-soft": ((100, 8), lambda P: P[:, 0:1], partial(ops.prox_soft, thresh=0.3)),
    "single-column-3-plus": ((8225, 8), lambda P: P[:, 3:4], ops.prox_plus),
    "single-row-of-transpose-hard": ((37, 6), lambda P: P.T[0:1], partial(ops.prox_hard, thresh=0.4)),
    "single-row-of-transpose-max-entropy": ((37, 6), lambda P: P.T[2:3], partial(ops.prox_max_entropy, gamma=0.7)),
    "row-3-flat": ((45, 33), lambda P: P[3:], partial(ops.prox_hard, thresh=0.4)),
    "KxN-thresholds-37x7": ((7, 37), lambda P: P, partial(ops.prox_soft, thresh=K7)),
    "KxN-thresholds-8225x40": ((40, 8300), lambda P: P[:, :8225], partial(ops.prox_soft_plus, thresh=K40)),
    "KxN-unity-axis-1-37x7": ((7, 40), lambda P: P[:, 3:], partial(ops.prox_unity_plus, axis=1)),
    "KxN-unity-long-axis-8225x40": ((40, 8300), lambda P: P[:, :8225], partial(ops.prox_unity_plus, axis=1)),
    "KxN-unity-axis-0-37x7": ((7, 40), lambda P: P[:, 3:], partial(ops.prox_unity_plus, axis=0)),
    "KxN-unity-short-axis-8225x40": ((40, 8300), lambda P: P[:, :8225], partial(ops.prox_unity_plus, axis=0)),
    "KxN-max-entropy-8225x40": ((40, 8300), lambda P: P[:, :8225], partial(ops.prox_max_entropy, gamma=K40)),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(VIEWS))
def test_views(torch, name, dtype):
    shape, view, prox = VIEWS[name]
    parent = _payload(shape, dtype)
    v = view(parent)
    v[...] = np.random.default_rng(len(name)).standard_normal(v.shape)
    inside = np.zeros(shape, bool)
    view(inside)[...] = True
    before = parent.copy()
    t = torch.from_numpy(parent.copy()).cuda()
    tv = view(t)
    assert prox(tv, 0.5) is tv
    prox(view(parent), 0.5)                                             # the host call on the corresponding NumPy view
    got = t.cpu().numpy()
    assert np.array_equal(_bits(got)[~inside], _bits(before)[~inside])  # pitch padding, rows and columns outside: every byte stays
    assert got.tobytes() == parent.tobytes()
    assert not np.array_equal(_bits(got)[inside], _bits(before)[inside])


# ---- 6. ordering ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_tensor_produced_on_a_side_stream(torch, dtype):
    """The tensor is written on a side stream directly behind a few large matmuls and the operator is called without any
    synchronisation: the call must wait for that stream (its hipDeviceSynchronize -- an array interface carries no stream).  A race
    cannot be made to fail deterministically: a guard, as tests/test_gpu_device_factors.py::test_factors_produced_on_a_side_stream."""
    X = np.random.default_rng(9).standard_normal((8225, 33)).astype(dtype)
    prox = ops.AlternatingProjections([partial(ops.prox_unity, axis=1), partial(ops.prox_soft_plus, thresh=0.1)], repeat=2)
    h = X.copy()
    prox(h, 0.5)
    src = torch.from_numpy(X).cuda()
    a = torch.rand(4096, 4096, device="cuda")
    t = torch.zeros_like(src)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        keep = [a @ a for _ in range(6)]
        t.copy_(src, non_blocking=True)
    prox(t, 0.5)
    torch.cuda.synchronize()
    del keep
    assert t.cpu().numpy().tobytes() == h.tobytes()


# ---- 7. device choice ----------------------------------------------------------------------------------------------------------------
def test_default_device(torch, monkeypatch):
    monkeypatch.delenv("PMX_DEVICE", raising=False)
    X = np.array([[-1.0, 2.0, 3.0]])
    np.testing.assert_array_equal(ops.prox_plus(X, 1.0), [[0.0, 2.0, 3.0]])
    t = torch.tensor([[-1.0, 2.0, 3.0]], device="cuda:0")
    ops.prox_unity_plus(t, 1.0, axis=1)
    np.testing.assert_allclose(t.cpu().numpy(), [[0.0, 0.4, 0.6]], rtol=1e-6)


def test_tensor_on_the_second_gpu(torch, monkeypatch):
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU visible: a tensor on device 1 needs two (the device is taken from the pointer, hipPointerGetAttributes)")
    monkeypatch.delenv("PMX_DEVICE", raising=False)
    torch.cuda.set_device(0)
    X = np.random.default_rng(1).standard_normal((8225, 33))
    h = X.copy()
    ops.prox_soft(h, 0.5, thresh=0.3)
    t = torch.from_numpy(X).to("cuda:1")
    assert ops.prox_soft(t, 0.5, thresh=0.3) is t and t.device.index == 1
    assert torch.cuda.current_device() == 0 and torch.empty(1, device="cuda").device.index == 0      # the caller's current device stays
    assert t.cpu().numpy().tobytes() == h.tobytes()
    monkeypatch.setenv("PMX_DEVICE", "1")                               # host arrays go where PMX_DEVICE says
    h2 = X.copy()
    ops.prox_soft(h2, 0.5, thresh=0.3)
    assert h2.tobytes() == h.tobytes()
