"""GPU: prox_max_entropy (operators.py:163-184), fused in every update kernel in fp32 and fp64.

oracle/nmf_oracle.py does not know the operator: expected values are the real reference's, recorded by
tests/golden/make_max_entropy_golden.py (max_entropy*.npz; inputs regenerated here from the seeds with that module's own
recipes and checked against the stored sums), and -- beyond the range in which the reference's exp() overflows -- the
operator's own optimality condition  y + gamma_ ln y = x - gamma_  evaluated in extended precision.

The bound on a single application, for the exact value y of an input x, w = y / gamma_ and eps = 2^-24 (fp32 arithmetic) or 2^-53:

    |dy| / y  <=  8 eps (1 + (|x / gamma_| + |ln gamma_| + 1) / (1 + w))

The second term is the rounding of L = x / gamma_ - 1 - ln gamma_ carried through dw / w = dL / (1 + w); the factor 8 covers the
iteration's own arithmetic and the final product.  The reference's own fp32 output stays inside it on the fixture's inputs
(asserted by the generator).  Solver runs are held to the tolerances the existing suites use for the same route and shape class,
imported from them: RTOL of test_gpu_f64.py (1e-10, small fp64 kernels), _close of test_gpu_f64_big.py (1e-9, matrix-core fp64
kernels), and for fp32 every entry to rtol 1e-4 with no absolute allowance, next to test_gpu_nmf.py's own rule for fp32 factors,
assert_factors_close, as that file has it (rtol 2e-4 / atol 2e-5; the weaker of the two here).  The fp32 cases' worst relative
error measured on an MI355X: 8.4e-6.

Measured on an MI355X (worst error / bound): stand-alone against the reference 0.39, fp32 beyond its range 0.27, fp64 beyond its
range 0.20, per-component steps 0.28.
"""
import ctypes
import importlib.util
import json
import logging
import os
import re
from functools import partial

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_f64 import RTOL as RTOL_SMALL
from test_gpu_f64_big import _close as _close_big
import test_gpu_nmf as tgn

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_max_entropy_golden", os.path.join(GOLDEN, "make_max_entropy_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)                       # (imports the reference only inside its main())

EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53
_Z = {}


def _npz(name):
    if name not in _Z:
        _Z[name] = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    return _Z[name]


META = json.loads(str(_npz("max_entropy.npz")["meta"]))


def _final(name, which):
    return _npz("max_entropy_%d.npz" % META["volumes"][name])[name + "/" + which]


@pytest.fixture(scope="module")
def pm():
    import __graft_entry__ as g
    g.build()
    import proxmin_amd
    return proxmin_amd


def residual_error(y, x, g_):
    """|dy| / y of a result y for input x from the optimality condition, in extended precision: F(y) = y + g ln y - x + g,
    dF / dy = 1 + g / y"""
    y, x, g_ = (np.asarray(v, dtype=np.longdouble) for v in (y, x, g_))
    F = y + g_ * np.log(y) - x + g_
    return np.asarray(np.abs(F) / (y + g_), dtype=np.float64)


# ---- 1. the operator alone -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(META["op"]))
def test_standalone_operator_against_the_reference(pm, name, dtype):
    c = META["op"][name]
    g_ = gen.gamma_eff(c["gamma"], c["type"], c["step"])
    X64 = gen.operator_inputs(tuple(c["shape"]), g_, c["seed"])
    assert float(np.nansum(np.where(np.isfinite(X64), X64, 0.0))) == c["sum64"]           # the generator's inputs
    X = X64.astype(dtype)
    inp = X.copy()
    out = pm.operators.prox_max_entropy(X, c["step"], gamma=c["gamma"], type=c["type"])
    assert out is X
    z = _npz("max_entropy.npz")
    want = z[name + "/ref64of32"] if dtype == np.float32 else z[name + "/ref64"]
    touched = inp > 0
    ut = np.uint32 if dtype == np.float32 else np.uint64
    assert np.array_equal(X[~touched].view(ut), inp[~touched].view(ut))                     # <= 0, -0.0, NaN, -inf: their own bits
    assert (~touched).sum() >= 8 and np.isnan(inp[~touched]).any() and (inp[~touched] == 0).sum() >= 2
    inf = touched & np.isinf(inp)
    assert inf.sum() == 1 and (X[inf] == np.inf).all()
    fin = touched & ~inf
    # (float64 arrays are computed in float32, as for every operator called on an array: the fp32 bound)
    x = inp[fin].astype(np.float64)
    rel = np.abs(X[fin].astype(np.float64) - want[fin]) / want[fin]
    bd = gen.bound(want[fin], x, g_, EPS32)
    print("%s %s: worst error / bound %.3f over %d entries" % (name, np.dtype(dtype).name, (rel / bd).max(), fin.sum()))
    assert np.isfinite(X[fin]).all()
    assert (rel <= bd).all(), (name, float((rel / bd).max()))


@pytest.mark.parametrize("gamma,kind,step", [(0.05, "absolute", 1.0), (1.0, "absolute", 1.0), (3.0, "relative", 0.25), (1e30, "absolute", 1.0),
                                             (2.0, "relative", 2.0 ** 113)])
def test_fp32_beyond_the_references_range(pm, gamma, kind, step):
    """x / gamma_ up to 1e4 -- the reference's fp32 exp() overflows above 88.7 -- and L down to -80 (only a large gamma_ gets
    there: L >= -1 - ln gamma_): finite, and the optimality condition holds to the bound"""
    g_ = float(np.float32(gamma) * np.float32(step)) if kind == "relative" else float(np.float32(gamma))
    lmin = -1.0 - np.log(g_)
    lo = max(-80.0, lmin + 1e-3)
    q = np.concatenate([np.linspace(lo, 100.0, 3300) + 1.0 + np.log(g_), np.geomspace(60.0, 1e4, 3300)])
    x = (q * g_).astype(np.float32)
    x = x[(x > 0) & np.isfinite(x)]
    X = x[: x.size // 200 * 200].reshape(-1, 200).copy()          # (wider than MAXK)
    inp = X.copy()
    out = pm.operators.prox_max_entropy(X, step, gamma=gamma, type=kind)
    assert out is X and np.isfinite(X).all() and (X > 0).all()
    x = inp.astype(np.float64)
    L = x / g_ - 1.0 - np.log(g_)
    assert (x / g_).max() >= 0.97e4
    if lmin < -80:
        assert L.min() < -79.0
    rel = residual_error(X, x, g_)
    bd = gen.bound(X.astype(np.float64), x, g_, EPS32)
    print("gamma_ %g: L %.1f .. %.3g, worst error / bound %.3f" % (g_, L.min(), L.max(), (rel / bd).max()))
    assert (rel <= bd).all(), float((rel / bd).max())


@pytest.mark.parametrize("mode,M,K", [("f64", 33, 3), ("f64mfma", 40, 20), ("f64mfma", 48, 40), ("f64mfma", 128, 100)])
@pytest.mark.parametrize("gamma,kind,step", [(0.05, "absolute", 0.5), (4.0, "relative", 0.25), (1e36, "relative", 0.5)])
def test_fp64_beyond_the_references_range(pm, mode, M, K, gamma, kind, step):
    """the fp64 kernels' operator, reached through one pgm iteration whose gradient is exactly zero (Y = 0, S = 0, constant
    steps): A <- prox(A, step).  x / gamma_ up to 1e6 (the reference's fp64 exp() overflows above 709), L down to -80."""
    from proxmin_amd.engine import DeviceNMF
    ops = pm.operators
    N = 56
    g_ = gamma * step if kind == "relative" else gamma
    lmin = -1.0 - np.log(g_)
    lo = max(-80.0, lmin + 1e-3)
    n = M * K
    q = np.concatenate([np.linspace(lo, 700.0, n // 2) + 1.0 + np.log(g_), np.geomspace(500.0, 1e6, n - n // 2)])
    A0 = np.random.default_rng(M + K).permutation(q * g_).reshape(M, K)
    A0[0, 0], A0[1, 0], A0[2, 0] = -1.0, 0.0, -0.0
    assert np.isfinite(A0).all()
    with DeviceNMF(M, N, K, mode=mode) as dev:
        dev.set_Y(np.zeros((M, N)))
        dev.set_factors(A0, np.zeros((K, N)))
        dev.pgm_begin([ops.device_proxseq(partial(ops.prox_max_entropy, gamma=gamma, type=kind), 0), ops.device_proxseq(ops.prox_plus, 1)],
                      fixed_steps=(step, step), e_rel=(0.0, 0.0))
        dev.pgm_run(1)
        A, S = dev.get_factors()
    assert A.dtype == np.float64 and (S == 0).all()
    touched = A0 > 0
    assert np.array_equal(A[~touched].view(np.uint64), A0[~touched].view(np.uint64)) and (~touched).sum() >= 3
    y, x = A[touched], A0[touched]
    assert np.isfinite(y).all() and (y > 0).all()
    L = x / g_ - 1.0 - np.log(g_)
    assert (x / g_).max() >= 0.99e6 and (lmin > -80 or L.min() < -79.0)
    rel = residual_error(y, x, g_)
    bd = gen.bound(y, x, g_, EPS64)
    print("%s K %d gamma_ %g: L %.1f .. %.3g, worst error / bound %.3f" % (mode, K, g_, L.min(), L.max(), (rel / bd).max()))
    assert (rel <= bd).all(), float((rel / bd).max())


@pytest.mark.parametrize("block", [0, 1], ids=["A", "S"])
def test_per_component_steps_relative_type(pm, block):
    """what adaprox passes (algorithms.py:384-387): (K,) next to an M x K array, (K, 1) next to a K x N array.  The reference
    raises on both; here gamma * step is formed element by element, the scalar formula column by column (row by row of S)."""
    rng = np.random.default_rng(5 + block)
    M, N, K, gamma = 37, 45, 7, 0.8
    step = rng.uniform(0.02, 3.0, K)
    if block == 0:
        X = rng.uniform(-0.5, 8.0, (M, K)).astype(np.float32)
        st, G = step, np.broadcast_to(step[None, :], (M, K))
    else:
        X = rng.uniform(-0.5, 8.0, (K, N)).astype(np.float32)
        st, G = step[:, None], np.broadcast_to(step[:, None], (K, N))
    inp = X.copy()
    out = pm.operators.prox_max_entropy(X, st, gamma=gamma, type="relative")
    assert out is X
    g_ = (np.float32(gamma) * G.astype(np.float32)).astype(np.float64)          # the product the kernel forms
    touched = inp > 0
    assert 0 < (~touched).sum() < touched.sum()
    assert np.array_equal(X[~touched].view(np.uint32), inp[~touched].view(np.uint32))
    x, y, gg = inp[touched].astype(np.float64), X[touched].astype(np.float64), g_[touched]
    rel = residual_error(y, x, gg)
    bd = 8.0 * EPS32 * (1.0 + (np.abs(x / gg) + np.abs(np.log(gg)) + 1.0) / (1.0 + y / gg))
    print("block %d: worst error / bound %.3f" % (block, (rel / bd).max()))
    assert (rel <= bd).all(), float((rel / bd).max())
    # an absolute gamma ignores the step array
    X2 = inp.copy()
    pm.operators.prox_max_entropy(X2, st, gamma=gamma, type="absolute")
    X3 = inp.copy()
    pm.operators.prox_max_entropy(X3, 1.0, gamma=gamma, type="absolute")
    assert np.array_equal(X2, X3)


def test_gamma_that_is_not_positive_gives_nan_where_the_operator_acts(pm):
    for gamma in (0.0, -1.0, np.nan):
        X = np.array([[-1.0, 0.0, 0.5, 2.0, np.nan, -np.inf]], dtype=np.float32)
        inp = X.copy()
        pm.operators.prox_max_entropy(X, 1.0, gamma=gamma, type="absolute")
        assert np.isnan(X[0, 2]) and np.isnan(X[0, 3])
        keep = [0, 1, 4, 5]
        assert np.array_equal(X[0, keep].view(np.uint32), inp[0, keep].view(np.uint32))


# ---- 2. the solvers against the reference's finals ---------------------------------------------------------------------
SHAPES = ["%s_%dx%dx%d" % ("f64" if dt == "float64" else "f32", M, N, K) for dt, M, N, K in gen.SOLVER_SHAPES]
SMALL64 = ("f64_33x47x3", "f64_40x56x12")


def _call_kw(pm, c, Y):
    ops = pm.operators
    me = partial(ops.prox_max_entropy, gamma=c["gamma"], type=c["type"])
    route, j = c["route"], c["block"]
    kw = dict(max_iter=META["iterations"], e_rel=c["e_rel"])
    prox = [ops.prox_plus, ops.prox_plus]
    if route == "pgm_ap":
        prox[j] = ops.AlternatingProjections([ops.prox_plus, me])
    elif route != "bsdmm_g":
        prox[j] = me
    if route == "fista":
        kw.update(accelerated=True, step=pm.nmf.scaled_step_pgm(0.5))
    if route == "pgm_bt":
        kw.update(backtracking=True, f=partial(pm.nmf.log_likelihood, Y=Y))
    if route == "bsdmm_g":
        kw["proxs_g"] = [[me], None] if j == 0 else [None, [me]]
    if route in ("bsdmm_prox", "bsdmm_g"):
        kw["algorithm"] = pm.bsdmm
    if route == "adam_abs":
        kw.update(algorithm=pm.adaprox, scheme="adam")
    kw.update(prox_A=prox[0], prox_S=prox[1])
    return kw


def _problem(c):
    Y, A0, S0 = gen.solver_problem(c["M"], c["N"], c["K"], c["dtype"], c["seed"])
    sums = [float(v.astype(np.float64).sum()) for v in (Y, A0, S0)]
    assert sums == c["sums"], "the regenerated inputs are not the generator's"
    return Y, A0, S0


def _compare(shape, mode, got, want, what):
    if shape in SMALL64:
        np.testing.assert_allclose(got, want, rtol=RTOL_SMALL, atol=1e-14, err_msg=what)      # test_gpu_f64.py
    elif shape.startswith("f64"):
        _close_big(got, want, name=what)                                                        # test_gpu_f64_big.py
    else:
        rel = np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(np.abs(want), 1e-300)
        print("%s: worst relative error %.3g" % (what, rel.max()))
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=0, err_msg=what)                  # every entry, no absolute allowance
        old = tgn.MODE["name"]
        tgn.MODE["name"] = mode
        try:
            tgn.assert_factors_close(got, want, np.float32, what)                               # test_gpu_nmf.py
        finally:
            tgn.MODE["name"] = old


@pytest.mark.parametrize("route", gen.SOLVER_ROUTES)
@pytest.mark.parametrize("shape", SHAPES)
def test_solver_routes_against_the_reference(pm, caplog, shape, route):
    """the operator once on A and once on S (prox_plus on the other block), 8 iterations: the reference's final factors at the
    existing suites' tolerances for the route and shape class; fp32 in the library's default arithmetic and in exact fp32; the
    same call with A and S as torch tensors in HBM gives the host call's bits; adaprox's sub-iteration counts are the reference's"""
    import torch
    for block in "AS":
        name = "%s/%s/%s" % (shape, route, block)
        c = META["solver"][name]
        Y, A0, S0 = _problem(c)
        for mode in ((None, "f32") if shape.startswith("f32") else (None,)):
            pm.set_default_mode(mode)
            try:
                mname = pm.get_default_mode()
                A, S = A0.copy(), S0.copy()
                caplog.clear()
                with caplog.at_level(logging.INFO, logger="proxmin"):
                    pm.nmf.nmf(Y, A, S, **_call_kw(pm, c, Y))
                text = " | ".join(r.getMessage() for r in caplog.records)
                assert "one iteration per call" not in text and "user-defined Python callable" not in text, text
                assert not (shape.startswith("f64") and "computed in float32" in text), text       # the fp64 kernels ran
                what = "%s (%s)" % (name, mname)
                assert A.dtype == A0.dtype
                _compare(shape, mname, A, _final(name, "A"), what + " A")
                _compare(shape, mname, S, _final(name, "S"), what + " S")
                if route == "adam_abs":
                    m = re.search(r"Completed (\d+) iterations and \[(\d+), (\d+)\] sub-iterations", text)
                    sub = [c["calls_me"], c["calls_plus"]] if c["block"] == 0 else [c["calls_plus"], c["calls_me"]]
                    assert m and [int(m.group(2)), int(m.group(3))] == sub, (text, sub)
                At, St = torch.from_numpy(A0).cuda(), torch.from_numpy(S0).cuda()
                pm.nmf.nmf(Y, At, St, **_call_kw(pm, c, Y))
                assert np.array_equal(At.cpu().numpy(), A) and np.array_equal(St.cpu().numpy(), S), what + ": device-resident factors"
            finally:
                pm.set_default_mode(None)


# ---- 3. which kernels ran, and that nothing went through the host ------------------------------------------------------
def test_adaprox_leaves_the_fused_tail_to_sequences_without_the_operator(pm):
    from proxmin_amd.engine import DeviceNMF
    ops = pm.operators
    c = META["solver"]["f32_64x96x8/adam_abs/S"]
    Y, A0, S0 = _problem(c)
    me = partial(ops.prox_max_entropy, gamma=c["gamma"], type="absolute")
    fused = {}
    for tag, pS in (("max_entropy", me), ("plus", ops.prox_plus), ("seq", ops.AlternatingProjections([ops.prox_plus, me]))):
        with DeviceNMF(c["M"], c["N"], c["K"]) as dev:
            dev.set_Y(Y)
            dev.set_factors(A0, S0)
            dev.adaprox_begin([ops.device_proxseq(ops.prox_plus, 0), ops.device_proxseq(pS, 1)], scheme="adam", e_rel=(1e-4, 1e-4))
            res = dev.adaprox_run(np.full(2, 0.9), 0.9)
            assert res.iterations == 2
            v = (ctypes.c_int * 8)()
            assert dev.lib.pmx_k1_info(dev.h, v) == 0
            fused[tag] = v[7] >= 1000000
            assert fused[tag] == bool(dev.k1_info()["tail_fused"])
    assert fused == {"max_entropy": False, "plus": True, "seq": False}, fused


@pytest.mark.parametrize("route", ["pgm", "adam_abs", "bsdmm_g"])
def test_no_host_route(pm, monkeypatch, caplog, route):
    """no per-iteration download: DeviceNMF.get is called as often after 8 iterations as after 2 (what the solver returns), and
    nothing warns about a host path"""
    from proxmin_amd import engine
    c = META["solver"]["f32_64x96x8/%s/S" % route]
    Y, A0, S0 = _problem(c)
    calls = []
    real_get = engine.DeviceNMF.get

    def get(self, base, j):
        calls.append(("get", base, j))
        return real_get(self, base, j)
    monkeypatch.setattr(engine.DeviceNMF, "get", get)
    counts = []
    for iters in (2, 8):
        del calls[:]
        kw = _call_kw(pm, c, Y)
        kw["max_iter"] = iters
        with caplog.at_level(logging.INFO, logger="proxmin"):
            pm.nmf.nmf(Y, A0.copy(), S0.copy(), **kw)
        counts.append(len(calls))
    text = " | ".join(r.getMessage() for r in caplog.records)
    assert "one iteration per call" not in text and "user-defined Python callable" not in text, text
    assert counts[0] == counts[1] and counts[0] <= 6, counts
