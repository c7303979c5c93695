"""pgm / FISTA with prox_unity / prox_unity_plus ALONG A FACTOR'S LONG AXIS (axis=0 on A, axis=1 on S) fused into the update
chain (csrc/k_update.hip: k_pgm_unity -- head, middle and finish launches around the grid-wide column sums).

Against the fp64 oracle.  oracle.nmf_oracle.pgm_nmf runs 4 to 6 iterations with e_rel = 1e-9 (nothing stops) on every case
of CASES; one more case stops early with its stopping quantity d / (e^2 n) outside [0.5, 2], so the iteration count and
`converged` are asserted EQUAL.  Tolerance, after tests/test_gpu_update_step.py: the oracle was run in float32 and in float64
on the very inputs of every case (`python tests/test_gpu_unity_long_axis.py`, CPU only, prints the table); REF_ERR_* is the
largest float32-versus-float64 difference over the case list in units of 2^-23 x the array's largest magnitude, and the
device is allowed 4 x that.  These comparisons run the exact-fp32 gradient kernels (mode "f32"): the bound is the rounding of
float32 arithmetic, which is what the update chain computes in; the split-precision gradient kernels carry their own,
separately tested error.  The library's default arithmetic is covered by the bit-for-bit comparison below.

Bit for bit.  The same call with the operator wrapped in a Python function is the host route -- T = Xe - s G downloaded, the
stand-alone k_prox_view (its `sum` and `div` launches) on a fresh upload, the result uploaded again -- and must give IDENTICAL factors.

Shapes are the smallest that reach each path: the small front (260 x 380 x 6), NC = 2 with a ragged K (700 x 96 x 33), a
second row sweep of the 8192-row grid on A (8225 x 64 x 64) and on S with K = 40 (96 x 8232 x 40: a K without a tuned gradient
kernel, which runs on the frame of the next tuned K), NC = 4 (300 x 200 x 128), and 2048 x 3072 x 32, where both factors have <= 4096 rows and K1 is not
k_grad_small: the update leaves the Gram partials of the next step rule.
"""
import logging
import os
import sys
from functools import partial

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ULP = 2.0 ** -23
# largest float32-oracle vs float64-oracle difference over CASES + STOP_CASE, in units of 2^-23 x max |array|
# (`python tests/test_gpu_unity_long_axis.py`), and the device's allowance: 4 x
# -- one pair for the Barzilai-Borwein cases (the rule divides two sums that the rounding of X and G moves), one for the rest
REF_ERR = {"bb": (6.61, 2.74), "rest": (47.4, 8.15)}
TOL = {k: (4 * a, 4 * s) for k, (a, s) in REF_ERR.items()}
TOL_A, TOL_S = TOL["rest"]
HARD_T = 1.5e-3                # threshold of the astro example's prox_hard (absolute)
HARD_GUARD = 1e-4            # no |argument| of the hard threshold within this (relative) of it
BAND = (0.5, 2.0)            # no stopping decision with d / (e^2 n) in here

SMALL, RAGGED, TALL_A, TALL_S, WIDE_K, GRAM = (260, 380, 6), (700, 96, 33), (8225, 64, 64), (96, 8232, 40), (300, 200, 128), (2048, 3072, 32)

UPA, UPS = ("unity_plus", 0), ("unity_plus", 1)
UA, US = ("unity", 0), ("unity", 1)
ASTRO_S = ("seq", (UPS, ("hard", HARD_T, "absolute")), 1)                 # examples/astro_unmixing.py's proxS
MIX_A = ("seq", (UA, ("unity", 1), ("plus",)), 2)                         # short and long axes, two long-axis applications
PLUS = ("plus",)


def _case(shape, pA, pS, step="default", acc=False, iters=5, **kw):
    c = dict(shape=shape, pA=pA, pS=pS, step=step, acc=acc, iters=iters, e_rel=1e-9, weighted=False, callback=False, seed=11)
    c.update(kw)
    c["id"] = "%dx%dx%d-" % shape + "-".join([_name(pA), _name(pS), step, "fista" if acc else "pgm", "it%d" % iters] +
                                             ["w"] * c["weighted"] + ["cb"] * c["callback"])
    return c


def _name(p):
    if p[0] == "seq":
        return "seq(%s)x%d" % ("+".join(_name(q) for q in p[1]), p[2])
    return p[0] + ("%d" % p[1] if p[0].startswith("unity") else "")


CASES = [
    _case(SMALL, UPA, PLUS),
    _case(SMALL, UPA, PLUS, step="scaled", acc=True, iters=6),
    _case(SMALL, UPA, PLUS, callback=True, iters=4),
    _case(SMALL, UA, US, step="bb", iters=4),
    _case(RAGGED, UPA, PLUS, step="scaled", acc=True),
    _case(RAGGED, PLUS, US),
    _case(RAGGED, MIX_A, PLUS, iters=4),
    _case(RAGGED, MIX_A, UPS, step="constant", acc=True, iters=4),            # L = 2 next to L = 1: S idles in the middle launch
    _case(TALL_A, UPA, PLUS),
    _case(TALL_A, UA, PLUS, step="constant", acc=True),
    _case(TALL_A, UPA, PLUS, step="constant", weighted=True, iters=4),
    _case(TALL_S, PLUS, UPS),
    _case(TALL_S, PLUS, US, step="scaled", acc=True, iters=4),
    _case(SMALL, PLUS, ASTRO_S, step="scaled", iters=4, seed=16),     # (few entries: a seed exists for which nothing comes near the threshold)
    _case(WIDE_K, UPA, PLUS, step="bb"),
    _case(WIDE_K, UPA, UPS, step="scaled", acc=True, iters=4),
    _case(GRAM, UPA, PLUS),
    _case(GRAM, PLUS, UPS, step="scaled", acc=True, iters=4),
    _case(GRAM, UA, US, iters=4),
]
# the stopping test fires at iteration 2 of 8 (d / n falls 24 x and 200 x there, by 1.4 x per iteration afterwards): per-block
# e_rel in the geometric middle of the oracle's own d / n before and after (printed by __main__)
STOP_E_REL = (0.164, 0.283)
STOP_AT = 2
STOP_CASE = _case(SMALL, UPA, PLUS, iters=8, e_rel=STOP_E_REL)
assert len({c["id"] for c in CASES}) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------------
# inputs and the oracle
# ---------------------------------------------------------------------------------------------------------------------
def make_problem(c):
    """Factors that start feasible: the normalised block sums to one along its long axis, the other block takes the scale."""
    from oracle import nmf_oracle as orc
    M, N, K = c["shape"]
    Y, A0, S0 = orc.synthetic_problem(M, N, K, np.float32, seed=c["seed"])
    A0 = A0.astype(np.float64) + 0.25
    S0 = S0.astype(np.float64) + 0.25
    longA = _has_long(c["pA"], 0)
    longS = _has_long(c["pS"], 1)
    if longA:
        f = A0.sum(0, keepdims=True)
        A0, S0 = A0 / f, S0 * f.T
    if longS:
        f = S0.sum(1, keepdims=True)
        S0 = S0 / f
        if not longA:
            A0 = A0 * f.T
    W = None
    if c["weighted"]:
        W = (0.5 + np.random.default_rng(c["seed"] + 1).random((M, N))).astype(np.float32)
    return Y, A0.astype(np.float32), S0.astype(np.float32), W


def _has_long(spec, block):
    if spec[0] == "seq":
        return any(_has_long(q, block) for q in spec[1])
    return spec[0] in ("unity", "unity_plus") and spec[1] == (0 if block == 0 else 1)


def constant_steps(c, A0, S0):
    from oracle import nmf_oracle as orc
    sA, sS = orc.lipschitz_steps(A0.astype(np.float64), S0.astype(np.float64))
    return float(np.float32(0.6 * sA)), float(np.float32(0.6 * sS))


def run_oracle(c, dtype, trace=None, iters=None):
    from oracle import nmf_oracle as orc
    Y, A0, S0, W = make_problem(c)
    A, S = A0.astype(dtype), S0.astype(dtype)
    step = None
    if c["step"] == "scaled":
        step = lambda A_, S_, it, G: tuple(dtype(0.5) * s for s in orc.lipschitz_steps(A_, S_))
    elif c["step"] == "constant":
        cs = constant_steps(c, A0, S0)
        step = lambda A_, S_, it, G: (dtype(cs[0]), dtype(cs[1]))
    elif c["step"] == "bb":
        bb = orc.BBStepper(1, 0.1)
        step = lambda A_, S_, it, G: bb.step([A_, S_], it, list(G))
    conv, G, St, n = orc.pgm_nmf(Y.astype(dtype), A, S, prox_A=c["pA"], prox_S=c["pS"], step=step, accelerated=c["acc"],
                                 max_iter=iters or c["iters"], e_rel=c["e_rel"], trace=trace, W=None if W is None else W.astype(dtype))
    return A, S, conv, n


def to_prox(ops, spec):
    if spec[0] == "seq":
        return ops.AlternatingProjections([to_prox(ops, q) for q in spec[1]], repeat=spec[2])
    if spec[0] in ("unity", "unity_plus"):
        return partial(getattr(ops, "prox_" + spec[0]), axis=spec[1])
    if spec[0] == "plus":
        return ops.prox_plus
    assert spec[0] == "hard"
    return partial(ops.prox_hard, thresh=spec[1], type=spec[2])


def wrap_long(ops, spec):
    """the same operator as a Python function: the host route through the stand-alone kernels"""
    assert spec[0] in ("unity", "unity_plus")
    fn, ax = getattr(ops, "prox_" + spec[0]), spec[1]
    return lambda X, s: fn(X, s, axis=ax)


def run_device(pm, c, wrap=False, callback=None, iters=None):
    Y, A0, S0, W = make_problem(c)
    A, S = A0.copy(), S0.copy()
    ops = pm.operators
    pA = wrap_long(ops, c["pA"]) if wrap and _has_long(c["pA"], 0) else to_prox(ops, c["pA"])
    pS = wrap_long(ops, c["pS"]) if wrap and _has_long(c["pS"], 1) else to_prox(ops, c["pS"])
    step = {"default": None, "scaled": pm.nmf.scaled_step_pgm(0.5), "constant": None, "bb": None}[c["step"]]
    if c["step"] == "constant":
        step = pm.nmf.constant_step(*constant_steps(c, A0, S0))
    elif c["step"] == "bb":
        step = pm.utils.BarzilaiBorweinStepper(1, 0.1).step
    conv, G, steps = pm.nmf.nmf(Y, A, S, W=1 if W is None else W, prox_A=pA, prox_S=pS, step=step, accelerated=c["acc"],
                                max_iter=iters or c["iters"], e_rel=c["e_rel"], callback=callback)
    return A, S, conv


def in_units(got, ref):
    scale = np.abs(ref).max()
    return np.abs(got.astype(np.float64) - ref).max() / (ULP * scale)


def assert_close(got, ref, tol, what):
    assert np.isfinite(got).all() and np.isfinite(ref).all(), what
    u = in_units(got, ref)
    print("%s: %.2f units (tolerance %.1f)" % (what, u, tol))
    assert u <= tol, "%s: %.2f units of 2^-23 x max|.| > %.1f" % (what, u, tol)


# ---------------------------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pm_any():
    import __graft_entry__ as g
    g.build()
    import proxmin_amd
    yield proxmin_amd
    proxmin_amd.set_default_mode(None)


@pytest.fixture()
def pm(pm_any):
    pm_any.set_default_mode("f32")
    return pm_any


@pytest.fixture(params=["library-default", "f32"])
def pm_modes(pm_any, request):
    pm_any.set_default_mode(None if request.param == "library-default" else request.param)
    return pm_any


_ORACLE = {}


def oracle64(c):
    """computed once per case, shared, never modified"""
    if c["id"] not in _ORACLE:
        trace = []
        A, S, conv, n = run_oracle(c, np.float64, trace=trace)
        for x in (A, S):
            x.setflags(write=False)
        _ORACLE[c["id"]] = (A, S, conv, n, trace)
    return _ORACLE[c["id"]]


# ---------------------------------------------------------------------------------------------------------------------
# 0. what keeps the comparison honest, on the oracle alone (no GPU)
# ---------------------------------------------------------------------------------------------------------------------
def _stop_ratios(c):
    """d / (e^2 n) per block and iteration of the float64 oracle with nothing stopping"""
    trace = []
    A, S, _, _ = run_oracle(dict(c, e_rel=1e-30), np.float64, trace=trace)
    its = trace[1:] + [(A, S)]
    out = []
    for (Ap, Sp), (An, Sn) in zip(trace, its):
        out.append(tuple(((Xn - Xp) ** 2).sum() / (e ** 2 * (Xn ** 2).sum()) for Xp, Xn, e in ((Ap, An, c["e_rel"][0]), (Sp, Sn, c["e_rel"][1]))))
    return out


def _hard_margin(c):
    from oracle import nmf_oracle as orc
    worst = [np.inf]
    real = orc.apply_prox

    def spy(X, step, spec):
        if spec is not None and spec[0] == "hard":
            worst[0] = min(worst[0], np.abs(np.abs(X) / spec[1] - 1.0).min())
        return real(X, step, spec)
    orc.apply_prox = spy
    try:
        run_oracle(c, np.float64)
    finally:
        orc.apply_prox = real
    return worst[0]


def test_reference_preconditions():
    r = _stop_ratios(STOP_CASE)
    for it, (ra, rs) in enumerate(r[:STOP_AT]):
        assert not (BAND[0] <= ra <= BAND[1]) and not (BAND[0] <= rs <= BAND[1]), (it, ra, rs)
    fired = [it for it, (ra, rs) in enumerate(r) if ra <= 1 and rs <= 1]
    assert fired and fired[0] == STOP_AT - 1, r
    for c in CASES:
        if c["pS"] is ASTRO_S:
            assert _hard_margin(c) > HARD_GUARD
        if "unity" in (c["pA"][0], c["pS"][0]):          # prox_unity without plus: column sums well away from zero
            trace = oracle64(c)[4]
            for A, S in trace:
                if c["pA"][0] == "unity":
                    assert (np.abs(A.sum(0)) > 0.1).all()
                if c["pS"][0] == "unity":
                    assert (np.abs(S.sum(1)) > 0.1).all()


# ---------------------------------------------------------------------------------------------------------------------
# 1. fails without the fused chain
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pgm_begin_takes_the_long_axis_and_runs_a_chunk(pm, caplog):
    from proxmin_amd.engine import DeviceNMF
    ops = pm.operators
    c = _case(SMALL, UPA, PLUS, iters=6)
    Y, A0, S0, _ = make_problem(c)
    with DeviceNMF(*c["shape"], mode="f32") as dev:
        dev.set_Y(Y)
        dev.set_factors(A0, S0)
        dev.pgm_begin([ops.device_proxseq(partial(ops.prox_unity_plus, axis=0), 0), ops.device_proxseq(ops.prox_plus, 1)], e_rel=(1e-9, 1e-9))
        res = dev.pgm_run(6)
        assert res.iterations == 6 and res.total_iterations == 6 and not res.stopped
        A, S = dev.get_factors()
    Ao, So, _, _, _ = oracle64(c)
    assert_close(A, Ao, TOL_A, "A")
    assert_close(S, So, TOL_S, "S")
    from proxmin_amd import algorithms
    saved = set(algorithms._warned)
    algorithms._warned.clear()
    try:
        with caplog.at_level(logging.WARNING, logger="proxmin"):
            A, S = A0.copy(), S0.copy()
            pm.nmf.nmf(Y, A, S, prox_A=partial(ops.prox_unity_plus, axis=0), max_iter=6, e_rel=1e-9)
        bad = [r.getMessage() for r in caplog.records if "one iteration per call" in r.getMessage() or "goes through the host" in r.getMessage()]
        assert not bad, bad
    finally:
        algorithms._warned.clear()
        algorithms._warned.update(saved)
    assert_close(A, Ao, TOL_A, "A (nmf)")


# ---------------------------------------------------------------------------------------------------------------------
# 2. against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_against_the_fp64_oracle(pm, c):
    Ao, So, conv_o, n_o, trace = oracle64(c)
    if c["shape"] == GRAM:
        from proxmin_amd.engine import DeviceNMF
        with DeviceNMF(*c["shape"]) as dev:
            assert dev.k1_info()["kernel"] != "k_grad_small"
    seen = []
    cb = (lambda A, S, it=None: seen.append((A.copy(), S.copy()))) if c["callback"] else None
    A, S, conv = run_device(pm, c, callback=cb)
    tol_A, tol_S = TOL["bb" if c["step"] == "bb" else "rest"]
    assert_close(A, Ao, tol_A, "A")
    assert_close(S, So, tol_S, "S")
    assert tuple(conv) == tuple(conv_o) == (False, False)
    if c["callback"]:
        assert len(seen) == len(trace) == c["iters"]
        for it, ((Ad, Sd), (At, St)) in enumerate(zip(seen, trace)):
            assert_close(Ad, At, tol_A, "A seen at it=%d" % it)
            assert_close(Sd, St, tol_S, "S seen at it=%d" % it)


@pytest.mark.gpu
def test_stops_where_the_oracle_stops(pm):
    from proxmin_amd.engine import DeviceNMF
    c = STOP_CASE
    Ao, So, conv_o, n_o, _ = oracle64(c)
    assert n_o == STOP_AT and tuple(conv_o) == (True, True)
    ops = pm.operators
    Y, A0, S0, _ = make_problem(c)
    with DeviceNMF(*c["shape"], mode="f32") as dev:
        dev.set_Y(Y)
        dev.set_factors(A0, S0)
        dev.pgm_begin([ops.device_proxseq(to_prox(ops, c["pA"]), 0), ops.device_proxseq(to_prox(ops, c["pS"]), 1)], e_rel=c["e_rel"])
        res = dev.pgm_run(c["iters"])
        A, S = dev.get_factors()
    assert res.total_iterations == n_o and res.stopped and tuple(bool(x) for x in res.converged) == (True, True)
    assert_close(A, Ao, TOL_A, "A")
    assert_close(S, So, TOL_S, "S")
    A, S, conv = run_device(pm, c)
    assert tuple(conv) == (True, True)
    assert_close(A, Ao, TOL_A, "A (nmf)")


# ---------------------------------------------------------------------------------------------------------------------
# 3. bit for bit what the stand-alone operator gives between the launches
# ---------------------------------------------------------------------------------------------------------------------
BITWISE = [_case(sh, pA, pS, step=st, acc=acc, iters=4)
           for sh, pA, pS in ((TALL_A, UPA, PLUS), (GRAM, UPA, PLUS), (GRAM, PLUS, UPS))
           for st, acc in (("default", False), ("constant", True), ("constant", False), ("scaled", True))]


@pytest.mark.gpu
@pytest.mark.parametrize("c", BITWISE, ids=[c["id"] for c in BITWISE])
def test_bit_for_bit_with_the_host_route(pm_modes, c, caplog):
    from proxmin_amd import algorithms
    saved = set(algorithms._warned)
    algorithms._warned.clear()
    try:
        with caplog.at_level(logging.WARNING, logger="proxmin"):
            A, S, _ = run_device(pm_modes, c)
        host = [r.getMessage() for r in caplog.records if "one iteration per call" in r.getMessage() or "applied on the host" in r.getMessage()]
        assert not host, "the first of the two runs must be the fused one: %r" % host
        Ah, Sh, _ = run_device(pm_modes, c, wrap=True)
    finally:
        algorithms._warned.clear()
        algorithms._warned.update(saved)
    assert np.isfinite(A).all() and np.isfinite(S).all()
    assert not np.array_equal(A, make_problem(c)[1])
    np.testing.assert_array_equal(A, Ah)
    np.testing.assert_array_equal(S, Sh)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the reference's surprises
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_non_positive_column_becomes_nan_like_the_reference(pm):
    c = _case(RAGGED, UPA, PLUS, iters=1)
    Y, A0, S0, _ = make_problem(c)
    Y = (0.1 * Y).astype(np.float32)              # A S - Y > 0: the gradient of an all-zero column is positive, the step makes it negative
    kz = 17
    A0[:, kz] = 0.0
    Ao, So = A0.astype(np.float64), S0.astype(np.float64)
    from oracle import nmf_oracle as orc
    with np.errstate(invalid="ignore", divide="ignore"):
        orc.pgm_nmf(Y.astype(np.float64), Ao, So, prox_A=UPA, prox_S=PLUS, max_iter=1, e_rel=1e-9)
    assert np.isnan(Ao[:, kz]).all() and np.isnan(Ao).sum() == Ao.shape[0] and not np.isnan(So).any()
    A, S = A0.copy(), S0.copy()
    pm.nmf.nmf(Y, A, S, prox_A=partial(pm.operators.prox_unity_plus, axis=0), max_iter=1, e_rel=1e-9)
    np.testing.assert_array_equal(np.isnan(A), np.isnan(Ao))
    assert not np.isnan(S).any()
    keep = ~np.isnan(Ao)
    assert np.abs(A[keep] - Ao[keep]).max() <= TOL_A * ULP * np.abs(Ao[keep]).max()
    assert_close(S, So, TOL_S, "S")


@pytest.mark.gpu
def test_components_behind_K_on_a_padded_frame(pm_any):
    """K = 40 has no tuned gradient kernel in the library's default arithmetic (k1_info()["frame_K"] says which K runs): the
    update chain divides components < 40 only (the others would be 0 / 0), and everything read back is K = 40 wide and finite."""
    from proxmin_amd import _lib
    from proxmin_amd.engine import DeviceNMF
    pm_any.set_default_mode(None)
    ops = pm_any.operators
    c = _case(TALL_S, UPA, UPS, iters=3)
    Y, A0, S0, _ = make_problem(c)
    with DeviceNMF(*c["shape"]) as dev:
        info = dev.k1_info()
        dev.set_Y(Y)
        dev.set_factors(A0, S0)
        dev.pgm_begin([ops.device_proxseq(to_prox(ops, c["pA"]), 0), ops.device_proxseq(to_prox(ops, c["pS"]), 1)], e_rel=(1e-9, 1e-9))
        res = dev.pgm_run(3)
        A, S = dev.get_factors()
        got = [dev.get(b, j) for b in (_lib.BUF_A, _lib.BUF_EVAL_A, _lib.BUF_GA) for j in (0, 1)]
    assert info["frame_K"] >= 40 and res.total_iterations == 3
    for x in got:
        assert np.isfinite(x).all() and 40 in x.shape
    np.testing.assert_allclose(A.sum(0), 1.0, rtol=2e-5)
    np.testing.assert_allclose(S.sum(1), 1.0, rtol=2e-5)
    Ao, So, _, _, _ = oracle64(c)
    np.testing.assert_allclose(A, Ao, rtol=2e-4, atol=2e-5 * np.abs(Ao).max())      # (split-precision gradients: smoke()'s bound)
    np.testing.assert_allclose(S, So, rtol=2e-4, atol=2e-5 * np.abs(So).max())


# ---------------------------------------------------------------------------------------------------------------------
# 5. the routes that did not change
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_other_solvers_and_the_line_search_keep_the_host_route(pm, caplog):
    from oracle import nmf_oracle as orc
    from proxmin_amd import algorithms
    ops = pm.operators
    c = _case(SMALL, UPA, PLUS, iters=4)
    Y, A0, S0, _ = make_problem(c)
    uA = partial(ops.prox_unity_plus, axis=0)
    runs = (
        ("adaprox", dict(algorithm=pm.adaprox, scheme="adam"), lambda A, S: orc.adaprox_nmf(Y.astype(np.float64), A, S, UPA, PLUS, scheme="adam", max_iter=4, e_rel=1e-9)),
        ("bsdmm", dict(algorithm=pm.bsdmm), lambda A, S: orc.bsdmm_nmf(Y.astype(np.float64), A, S, prox_A=UPA, max_iter=4, e_rel=1e-9)),
        ("line search", dict(backtracking=True, f=partial(pm.nmf.log_likelihood, Y=Y)),
         lambda A, S: orc.pgm_nmf(Y.astype(np.float64), A, S, prox_A=UPA, backtracking=True, max_iter=4, e_rel=1e-9)),
    )
    saved = set(algorithms._warned)
    try:
        for name, kw, ref in runs:
            algorithms._warned.clear()
            caplog.clear()
            A, S = A0.copy(), S0.copy()
            with caplog.at_level(logging.WARNING, logger="proxmin"):
                pm.nmf.nmf(Y, A, S, prox_A=uA, max_iter=4, e_rel=1e-9, **kw)
            msgs = [r.getMessage() for r in caplog.records if "one iteration per call" in r.getMessage()]
            assert len(msgs) == 1, (name, msgs)
            Ao, So = A0.astype(np.float64), S0.astype(np.float64)
            ref(Ao, So)
            np.testing.assert_allclose(A, Ao, rtol=2e-4, atol=2e-5 * np.abs(Ao).max(), err_msg=name)
            np.testing.assert_allclose(S, So, rtol=2e-4, atol=2e-5 * np.abs(So).max(), err_msg=name)
    finally:
        algorithms._warned.clear()
        algorithms._warned.update(saved)


# ---------------------------------------------------------------------------------------------------------------------
if __name__ == "__main__":
    worst, worst_bb = [0.0, 0.0], [0.0, 0.0]
    for c in CASES:
        A64, S64, _, _ = run_oracle(c, np.float64)
        A32, S32, _, _ = run_oracle(c, np.float32)
        u = (in_units(A32, A64), in_units(S32, S64))
        w = worst_bb if c["step"] == "bb" else worst
        w[:] = [max(a, x) for a, x in zip(w, u)]
        print("%-70s A %8.2f  S %8.2f" % (c["id"], u[0], u[1]))
    print("stop case, d / n per iteration (float64 oracle):")
    rat = _stop_ratios(dict(STOP_CASE, e_rel=(1.0, 1.0)))
    for it, r in enumerate(rat):
        print("  it %d: A %.4e  S %.4e" % (it, r[0], r[1]))
    e = tuple(float("%.3g" % np.sqrt(np.sqrt(rat[STOP_AT - 1][j] * rat[STOP_AT - 2][j]))) for j in range(2))
    print("STOP_E_REL = %r   (geometric middle of iterations %d and %d)" % (e, STOP_AT - 2, STOP_AT - 1))
    c = dict(STOP_CASE, e_rel=e)
    A64, S64, conv, n = run_oracle(c, np.float64)
    A32, S32, conv32, n32 = run_oracle(c, np.float32)
    u = (in_units(A32, A64), in_units(S32, S64))
    worst = [max(w, x) for w, x in zip(worst, u)]
    print("stop case: n = %d / %d, conv %r / %r, A %.2f S %.2f; ratios %r" % (n, n32, conv, conv32, u[0], u[1], _stop_ratios(c)))
    print('REF_ERR = {"bb": (%.3g, %.3g), "rest": (%.3g, %.3g)}' % (worst_bb[0], worst_bb[1], worst[0], worst[1]))
