"""Every host-driven route of algorithms.pgm / adaprox / bsdmm and of the two sharded drivers, pinned as a transcript: the
complete sequence of device calls and user-callable invocations, the return value, the caller's arrays, the log records and
the `_warned` keys.  No GPU, no libpmx.so: the solvers reach the device through one seam, `algorithms._open_device`, which
is replaced by a recording stand-in engine that answers from a small script; the sharded drivers take their engine and
their collectives as parameters.  The expected transcripts (tests/golden/host_routes.json) were recorded with
`python tests/test_host_routes.py --record` BEFORE the host loops were folded into one driver; a difference is a change of
behaviour.  Arrays appear as dtype, shape and a digest of their bytes; the stand-in's arrays differ by buffer, block and
call count, so what a host prox returned must be what `put` receives."""
import hashlib
import json
import logging
import os
import re
import sys
from functools import partial

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from proxmin_amd import _lib, algorithms, distributed, nmf as dnmf, operators, utils  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "host_routes.json")
M, K, N = 6, 2, 5
MAX_ITER, STOP_AT = 5, 3


# -- summaries ------------------------------------------------------------------------------------
def summ(x):
    if isinstance(x, np.ndarray):
        return "%s%s#%s" % (x.dtype.str[1:], list(x.shape), hashlib.sha1(np.ascontiguousarray(x).tobytes()).hexdigest()[:8])
    if isinstance(x, np.generic):
        return "%s:%r" % (x.dtype.str[1:], x.item())
    if isinstance(x, _lib.ProxSeq):
        return "seq(%d,%d;%s)" % (x.n, x.repeat, ",".join("%d/%d/%r/%d" % (x.seq[i].op, x.seq[i].unit, x.seq[i].thresh, x.seq[i].relative) for i in range(x.n)))
    if isinstance(x, tuple):
        return "(" + ", ".join(summ(v) for v in x) + ")"
    if isinstance(x, list):
        return "[" + ", ".join(summ(v) for v in x) + "]"
    if isinstance(x, dict):
        return "{" + ", ".join("%s=%s" % (k, summ(x[k])) for k in sorted(x)) + "}"
    return re.sub(r" at 0x[0-9a-fA-F]+", "", repr(x))


def call_line(name, args, kw):
    return "%s %s%s" % (name, summ(tuple(args)), (" " + summ(kw)) if kw else "")


class Rec:
    """a user callable whose every invocation goes into the transcript"""

    def __init__(self, T, name, fn):
        self.T, self.name, self.fn = T, name, fn

    def __call__(self, *a, **k):
        self.T.append(call_line("call " + self.name, a, k))
        return self.fn(*a, **k)

    def __repr__(self):
        return "<user %s>" % self.name


# -- the stand-in engine --------------------------------------------------------------------------
class Res:
    def __init__(self, eng, stopped=False):
        self.iterations = 1
        self.total_iterations = eng.iters
        self.stopped = int(bool(stopped))
        self.converged = eng.script.get("converged", (1, 1)) if stopped else (0, 0)
        self.steps = (0.125, 0.25)
        self.sub_iterations = (2 * eng.iters, eng.iters)


class RecEngine:
    """DeviceNMF's methods as the solvers use them: every call recorded, answered from `script`."""

    def __init__(self, T, script, f64):
        self.T, self.script = T, script
        self.M, self.N, self.K = M, N, K
        self.dt = np.float64 if f64 else np.float32
        self.iters, self.n = 0, 0
        self.mask, self.left = 0, 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.T.append("close")

    def _arr(self, rows, tag):
        self.n += 1
        v = ((np.arange(rows * K) * 7 + tag * 3 + self.n * 5) % 17 - 4) / 8.0
        return v.astype(self.dt).reshape(rows, K)

    def _advance(self, n=1):
        self.iters += max(0, min(int(n), self.script.get("stop_at", STOP_AT) - self.iters))
        return Res(self, self.iters >= self.script.get("stop_at", STOP_AT))

    # data
    def get(self, base, j):
        self.T.append(call_line("get", (base, j), {}))
        out = self._arr(M if j == 0 else N, base + j)
        return out if j == 0 else out.T

    def put(self, base, j, arr):
        self.T.append(call_line("put", (base, j, np.asarray(arr)), {}))

    def _download(self, buf, rows):
        self.T.append(call_line("_download", (buf, rows), {}))
        return self._arr(rows, buf)

    def _upload(self, buf, arr):
        self.T.append(call_line("_upload", (buf, np.asarray(arr)), {}))

    def get_factors(self):
        self.T.append("get_factors")
        return self._arr(M, 0), self._arr(N, 1).T

    def step_adaprox(self):
        self.T.append("step_adaprox")
        return np.array([0.5, 0.25], np.float32), np.array([0.125, 0.5], np.float32)

    # everything that only takes arguments
    def __getattr__(self, name):
        if name not in ("pgm_begin", "adaprox_begin", "bsdmm_begin", "pgm_set_fixed_steps", "pgm_step_arrays", "adaprox_set_alpha"):
            raise AttributeError(name)

        def method(*a, **k):
            if name == "pgm_begin":
                self.mask = sum(1 << j for j, h in enumerate(k.get("host_prox", (0, 0))) if h)
            self.T.append(call_line(name, a, k))
        return method

    # solvers
    def pgm_run(self, n):
        self.T.append(call_line("pgm_run", (n,), {}))
        return self._advance(n)

    def pgm_split(self, phase, steps=None):
        self.T.append(call_line("pgm_split", (phase, steps), {}))
        return self._advance(1) if phase == 2 else Res(self)

    def pgm_bt_split(self, phase):
        self.T.append(call_line("pgm_bt_split", (phase,), {}))
        if phase == 0:
            trials = self.script.get("bt_trials", [2, 1, 1, 1, 1])
            self.left = trials[self.iters] if self.mask else 0
            self.trial = 0
        else:
            self.left -= 1
        self.trial += 1
        eff = (0.5 / self.trial, 0.25 / self.trial)
        if self.left > 0:
            return self.mask, eff, Res(self)
        return 0, eff, self._advance(1)

    def adaprox_run(self, b1, b1_prev):
        self.T.append(call_line("adaprox_run", (np.asarray(b1), b1_prev), {}))
        return self._advance(len(b1))

    def adaprox_split(self, phase, it, b1_it, b1_prev, taus=(0, 0)):
        self.T.append(call_line("adaprox_split", (phase, it, b1_it, b1_prev, list(taus)), {}))
        return (self._advance(1), (0.0, 0.0)) if phase == 1 else (Res(self), (2.0, 4.0))

    def bsdmm_run(self, n):
        self.T.append(call_line("bsdmm_run", (n,), {}))
        return self._advance(n)

    def bsdmm_split(self, j, phase, host_f=False, host_g=0, last_block=False, step_f=0.0):
        self.T.append(call_line("bsdmm_split", (j, phase, host_f, host_g, last_block, step_f), {}))
        return self._advance(1) if (phase == 2 and last_block) else Res(self)


class Ctx:
    """one route: fresh arrays, the transcript, the wrapped user callables"""

    def __init__(self, dtype=np.float32, script=None):
        self.T = []
        self.script = dict(script or {})
        r = np.arange(M * N).reshape(M, N)
        self.Y = ((r * 5) % 13 / 4.0).astype(dtype)
        self.A = ((np.arange(M * K).reshape(M, K) * 3) % 7 / 4.0 + 0.25).astype(dtype)
        self.S = ((np.arange(K * N).reshape(K, N) * 5) % 11 / 8.0 + 0.125).astype(dtype)
        self.grad = partial(dnmf.grad_likelihood, Y=self.Y, W=1)
        self.X = [self.A, self.S]

    def rec(self, name, fn):
        return Rec(self.T, name, fn)

    def open_device(self, Y, A, S, W, f64=False, f64_mfma=False):
        self.T.append(call_line("open", (Y, A, S, W), {"f64": f64, "f64_mfma": f64_mfma}))
        return RecEngine(self.T, self.script, f64)

    # user callables
    def callback(self, stop=None):
        def cb(*X, it=None):
            if it == stop:
                raise StopIteration
        return self.rec("callback", cb)

    def prox(self, name="prox"):
        return self.rec(name, lambda X, step: np.maximum(X, 0))

    def step(self):
        return self.rec("step", lambda *X, it=None: (0.25 / (it + 1), 0.5))

    def step_grads(self):
        return self.rec("step_grads", lambda *X, it=None, grads=None: (0.5, 0.125 * (it + 1)))

    def step_arrays(self):
        def st(*X, it=None):
            if it == 0:
                return (np.array([0.25, 0.5]), 0.5)                              # one block
            if it == 1:
                return (np.full((M, K), 0.125), np.array([[0.5], [0.25]]))       # both blocks
            return (0.25, 0.5)                                                   # scalars again
        return self.rec("step_arrays", st)

    def user_grad(self):
        return self.rec("grad", lambda A, S: (A * 0.5, S * 0.25))

    def f(self):
        return partial(dnmf.log_likelihood, Y=self.Y)


DEFAULT_PGM_STEP = partial(dnmf.step_pgm, W=1)
UNITY_LONG_A = partial(operators.prox_unity, axis=0)
PLUS = operators.prox_plus


def pgm(c, step=DEFAULT_PGM_STEP, grad=None, **kw):
    return algorithms.pgm(c.X, grad or c.grad, step, max_iter=kw.pop("max_iter", MAX_ITER), **kw)


def ada(c, step=dnmf.step_adaprox, grad=None, **kw):
    return algorithms.adaprox(c.X, grad or c.grad, step, max_iter=kw.pop("max_iter", MAX_ITER), **kw)


def bsd(c, prox=(PLUS, PLUS), closures=None, **kw):
    pf, sf = closures or dnmf.bsdmm_closures(c.Y, list(prox))
    return algorithms.bsdmm(c.X, pf, sf, max_iter=kw.pop("max_iter", MAX_ITER), **kw)


def generic(c, step=0.5):
    return (c.rec("proxs_f", lambda X, s, j=None, Xs=None: np.maximum(X - s * 0.125, 0)), c.rec("steps_f_cb", lambda Xs, j=None: step * (j + 1)))


F64 = dict(dtype=np.float64)
F64_SWITCHES = ("PMX_F64", "PMX_F64_BIG", "PMX_K1_SMALL")      # engine.f64_applies reads them

# name -> (callable(ctx), Ctx keywords)
ROUTES = {
    # ---- pgm ----
    "pgm_fused": (lambda c: pgm(c, prox=[PLUS, PLUS]), {}),
    "pgm_fused_not_converged": (lambda c: pgm(c, accelerated=True), {"script": {"converged": (1, 0)}}),
    "pgm_fused_max_iter0": (lambda c: pgm(c, max_iter=0), {}),
    "pgm_callback": (lambda c: pgm(c, callback=c.callback()), {}),
    "pgm_null_callback": (lambda c: pgm(c, callback=utils.NullCallback()), {}),
    "pgm_callback_max_iter0": (lambda c: pgm(c, callback=c.callback(), max_iter=0), {}),
    "pgm_callback_stop": (lambda c: pgm(c, callback=c.callback(2)), {}),
    "pgm_callback_stop_at0": (lambda c: pgm(c, callback=c.callback(0)), {}),
    "pgm_slow_callback_stop": (lambda c: pgm(c, step=c.step(), callback=c.callback(2)), {}),
    "pgm_bt_step_callback_stop": (lambda c: pgm(c, step=c.step(), backtracking=True, f=c.f(), callback=c.callback(2)), {}),
    "pgm_bt_prox_callback_stop": (lambda c: pgm(c, prox=[c.prox(), PLUS], backtracking=True, f=c.f(), callback=c.callback(2)), {}),
    "pgm_step_grads": (lambda c: pgm(c, step=c.step_grads(), prox=[PLUS, PLUS]), {}),
    "pgm_step_nograds": (lambda c: pgm(c, step=c.step(), prox=[PLUS, PLUS], callback=c.callback()), {}),
    "pgm_step_arrays": (lambda c: pgm(c, step=c.step_arrays()), {}),
    "pgm_step_arrays_prox": (lambda c: pgm(c, step=c.step_arrays(), prox=[c.prox("prox_A"), c.prox("prox_S")]), {}),
    "pgm_step_arrays_end": (lambda c: pgm(c, step=c.step_arrays()), {"script": {"stop_at": 2}}),
    "pgm_prox_A": (lambda c: pgm(c, prox=[c.prox(), PLUS]), {}),
    "pgm_prox_S": (lambda c: pgm(c, prox=[None, c.prox()]), {}),
    "pgm_prox_both": (lambda c: pgm(c, prox=[c.prox("prox_A"), c.prox("prox_S")], accelerated=True, callback=c.callback()), {}),
    "pgm_prox_shared": (lambda c: pgm(c, prox=c.prox()), {}),
    "pgm_step_prox": (lambda c: pgm(c, step=c.step_grads(), prox=[PLUS, c.prox()]), {}),
    "pgm_grad": (lambda c: pgm(c, grad=c.user_grad()), {}),
    "pgm_grad_prox": (lambda c: pgm(c, grad=c.user_grad(), prox=[c.prox(), PLUS]), {}),
    "pgm_grad_step": (lambda c: pgm(c, grad=c.user_grad(), step=c.step_grads()), {}),
    "pgm_bb_fused": (lambda c: pgm(c, step=utils.BarzilaiBorweinStepper(2, 0.25)), {}),
    "pgm_bb_prox": (lambda c: pgm(c, step=utils.BarzilaiBorweinStepper().step, prox=[c.prox(), PLUS]), {}),
    "pgm_bt_fused": (lambda c: pgm(c, backtracking=True, f=c.f()), {}),
    "pgm_bt_step": (lambda c: pgm(c, step=c.step(), backtracking=True, f=c.f()), {}),
    "pgm_bt_step_grads": (lambda c: pgm(c, step=c.step_grads(), backtracking=True, f=c.f()), {}),
    "pgm_bt_prox": (lambda c: pgm(c, prox=[c.prox(), PLUS], backtracking=True, f=c.f()), {}),
    "pgm_bt_prox_both": (lambda c: pgm(c, prox=[c.prox("prox_A"), c.prox("prox_S")], backtracking=True, f=c.f()), {"script": {"bt_trials": [1, 3, 1, 1, 1]}}),
    "pgm_bt_step_prox": (lambda c: pgm(c, step=c.step(), prox=[PLUS, c.prox()], backtracking=True, f=c.f()), {}),
    "pgm_bt_step_grads_prox": (lambda c: pgm(c, step=c.step_grads(), prox=[c.prox(), PLUS], backtracking=True, f=c.f()), {}),
    "pgm_unity_long_fused": (lambda c: pgm(c, prox=[UNITY_LONG_A, PLUS]), {}),
    "pgm_unity_long_callback": (lambda c: pgm(c, prox=[UNITY_LONG_A, partial(operators.prox_unity_plus, axis=1)], callback=c.callback()), {}),
    "pgm_unity_long_user_step": (lambda c: pgm(c, prox=[UNITY_LONG_A, PLUS], step=c.step()), {}),
    "pgm_unity_long_user_prox": (lambda c: pgm(c, prox=[UNITY_LONG_A, c.prox()]), {}),
    "pgm_unity_long_bt": (lambda c: pgm(c, prox=[UNITY_LONG_A, PLUS], backtracking=True, f=c.f()), {}),
    "pgm_constant_step": (lambda c: pgm(c, step=dnmf.constant_step(0.25, 0.5)), {}),
    "pgm_scaled_step": (lambda c: pgm(c, step=dnmf.scaled_step_pgm(0.5), accelerated=True), {}),
    "pgm_bare_step": (lambda c: pgm(c, step=dnmf.step_pgm, e_rel=(1e-3, 1e-4)), {}),
    "pgm_weighted": (lambda c: pgm(c, grad=partial(dnmf.grad_likelihood, Y=c.Y, W=np.ones((M, N), np.float32))), {}),
    "pgm_weighted_user_step": (lambda c: pgm(c, grad=partial(dnmf.grad_likelihood, Y=c.Y, W=np.ones((M, N), np.float32)), step=c.step()), {}),
    # ---- pgm, refusals ----
    "pgm_refuse_bt_user_grad": (lambda c: pgm(c, grad=c.user_grad(), backtracking=True, f=c.f()), {}),
    "pgm_refuse_bt_arrays": (lambda c: pgm(c, step=c.step_arrays(), backtracking=True, f=c.f()), {}),
    "pgm_refuse_bt_arrays_prox": (lambda c: pgm(c, step=c.step_arrays(), prox=[c.prox(), PLUS], backtracking=True, f=c.f()), {}),
    "pgm_refuse_bt_other_f": (lambda c: pgm(c, backtracking=True, f=c.rec("f", lambda *X: 0.0)), {}),
    "pgm_refuse_bt_other_W": (lambda c: pgm(c, backtracking=True, f=partial(dnmf.log_likelihood, Y=c.Y, W=2)), {}),
    "pgm_refuse_bt_bb_prox": (lambda c: pgm(c, step=utils.BarzilaiBorweinStepper(), prox=[c.prox(), PLUS], backtracking=True, f=c.f()), {}),
    "pgm_refuse_step_W_array": (lambda c: pgm(c, step=partial(dnmf.step_pgm, W=np.ones((M, N)))), {}),
    "pgm_refuse_step_W_2": (lambda c: pgm(c, step=partial(dnmf.step_pgm, W=2)), {}),
    "pgm_refuse_step_not_callable": (lambda c: pgm(c, step=0.5), {}),
    "pgm_refuse_grad_not_callable": (lambda c: pgm(c, grad=0.5), {}),
    # ---- pgm, float64 ----
    "pgm_f64_fused": (lambda c: pgm(c), F64),
    "pgm_f64_bt": (lambda c: pgm(c, backtracking=True, f=c.f()), F64),
    "pgm_f64_weighted": (lambda c: pgm(c, grad=partial(dnmf.grad_likelihood, Y=c.Y, W=np.ones((M, N))), step=dnmf.constant_step(0.25)), F64),
    "pgm_f64_callback": (lambda c: pgm(c, callback=c.callback()), F64),
    "pgm_f64_user_step": (lambda c: pgm(c, step=c.step()), F64),
    "pgm_f64_bb": (lambda c: pgm(c, step=utils.BarzilaiBorweinStepper()), F64),
    "pgm_f64_unity_long": (lambda c: pgm(c, prox=[UNITY_LONG_A, PLUS]), F64),
    "pgm_f64_mixed": (lambda c: algorithms.pgm([c.A.astype(np.float32), c.S], c.grad, DEFAULT_PGM_STEP, max_iter=MAX_ITER), F64),
    # ---- adaprox ----
    "ada_fused": (lambda c: ada(c, prox=[PLUS, PLUS]), {}),
    "ada_fused_noprox_nocheck": (lambda c: ada(c, check_convergence=False, scheme="AMSGrad", b1=np.linspace(0.9, 0.5, MAX_ITER)), {}),
    "ada_fused_not_converged": (lambda c: ada(c, prox=[PLUS, PLUS]), {"script": {"converged": (0, 1)}}),
    "ada_callback": (lambda c: ada(c, prox=[PLUS, PLUS], callback=c.callback(), b1=np.linspace(0.9, 0.5, MAX_ITER)), {}),
    "ada_callback_stop": (lambda c: ada(c, callback=c.callback(2)), {}),
    "ada_callback_stop_at0": (lambda c: ada(c, callback=c.callback(0)), {}),
    "ada_user_step": (lambda c: ada(c, step=c.rec("step", lambda *X, it=None: (0.5, np.array([[0.25], [0.125]]))), prox=[PLUS, PLUS], b1=np.linspace(0.9, 0.5, MAX_ITER)), {}),
    "ada_user_step_callback_stop": (lambda c: ada(c, step=c.rec("step", lambda *X, it=None: (np.array([0.5, 0.25]), 0.125)), callback=c.callback(2)), {}),
    "ada_user_step_bad_shape": (lambda c: ada(c, step=c.rec("step", lambda *X, it=None: (np.ones(3), 0.125))), {}),
    "ada_prox_default_rule": (lambda c: ada(c, prox=[c.prox(), PLUS], prox_max_iter=3), {}),
    "ada_prox_S_callback": (lambda c: ada(c, prox=[PLUS, c.prox()], prox_max_iter=3, callback=c.callback(2), b1=np.linspace(0.9, 0.5, MAX_ITER)), {}),
    "ada_prox_both": (lambda c: ada(c, prox=[c.prox("prox_A"), c.prox("prox_S")], prox_max_iter=2), {}),
    "ada_prox_constant_step": (lambda c: ada(c, step=dnmf.constant_step(0.25, 0.5), prox=[c.prox(), PLUS], prox_max_iter=3), {}),
    "ada_prox_user_step": (lambda c: ada(c, step=c.rec("step", lambda *X, it=None: (0.5, np.array([[0.25], [0.125]]))), prox=[c.prox("prox_A"), c.prox("prox_S")], prox_max_iter=3), {}),
    "ada_constant_step": (lambda c: ada(c, step=dnmf.constant_step(0.25)), {}),
    "ada_grad": (lambda c: ada(c, grad=c.user_grad(), prox=[PLUS, PLUS]), {}),
    "ada_grad_prox": (lambda c: ada(c, grad=c.user_grad(), prox=[c.prox(), None], prox_max_iter=2), {}),
    "ada_unity_long": (lambda c: ada(c, prox=[UNITY_LONG_A, PLUS], prox_max_iter=2), {}),
    "ada_warm": (lambda c: ada(c, prox=[PLUS, PLUS], M=[c.A * 0.5, c.S * 0.5], V=[c.A * 0.25, c.S * 0.25], Vhat=[c.A * 2, c.S * 2], scheme="amsgrad"), {}),
    "ada_warm_M_only": (lambda c: ada(c, M=[c.A * 0.5, c.S * 0.5], callback=c.callback()), {}),
    "ada_max_iter0": (lambda c: ada(c, max_iter=0), {}),
    "ada_max_iter0_user_step": (lambda c: ada(c, max_iter=0, step=c.step()), {}),
    "ada_refuse_step_not_callable": (lambda c: ada(c, step=0.5), {}),
    "ada_f64_fused": (lambda c: ada(c, prox=[PLUS, PLUS]), F64),
    "ada_f64_weighted": (lambda c: ada(c, grad=partial(dnmf.grad_likelihood, Y=c.Y, W=np.ones((M, N)))), F64),
    "ada_f64_callback": (lambda c: ada(c, callback=c.callback()), F64),
    "ada_f64_user_prox": (lambda c: ada(c, prox=[c.prox(), PLUS], prox_max_iter=2), F64),
    # ---- bsdmm ----
    "bsdmm_fused": (lambda c: bsd(c), {}),
    "bsdmm_fused_proxs_g": (lambda c: bsd(c, proxs_g=[[PLUS, partial(operators.prox_soft, thresh=0.125)], None], e_rel=(1e-3, 1e-4), e_abs=1e-6), {}),
    "bsdmm_fused_not_converged": (lambda c: bsd(c), {"script": {"converged": (0, 0)}}),
    "bsdmm_callback": (lambda c: bsd(c, callback=c.callback()), {}),
    "bsdmm_callback_stop": (lambda c: bsd(c, callback=c.callback(2)), {}),
    "bsdmm_user_prox_f": (lambda c: bsd(c, prox=(c.prox(), PLUS)), {}),
    "bsdmm_user_prox_f_callback_stop": (lambda c: bsd(c, prox=(PLUS, c.prox()), callback=c.callback(2)), {}),
    "bsdmm_user_g_block0": (lambda c: bsd(c, proxs_g=[[c.prox("g0"), PLUS], None]), {}),
    "bsdmm_user_g_block1": (lambda c: bsd(c, proxs_g=[None, c.prox("g1")], callback=c.callback()), {}),
    "bsdmm_user_g_both": (lambda c: bsd(c, prox=(c.prox("prox_A"), PLUS), proxs_g=[[PLUS, c.prox("g0b")], [c.prox("g1a"), c.prox("g1b")]]), {}),
    "bsdmm_unity_long": (lambda c: bsd(c, prox=(UNITY_LONG_A, PLUS), proxs_g=[None, [partial(operators.prox_unity_plus, axis=1)]]), {}),
    "bsdmm_generic": (lambda c: bsd(c, closures=generic(c)), {}),
    "bsdmm_generic_callback_g": (lambda c: bsd(c, closures=generic(c), proxs_g=[[c.prox("g0")], None], callback=c.callback()), {}),
    "bsdmm_generic_step_zero": (lambda c: bsd(c, closures=generic(c, step=0.0)), {}),
    "bsdmm_generic_three_blocks": (lambda c: algorithms.bsdmm([c.A, c.S, c.S], *generic(c), max_iter=MAX_ITER), {}),
    "bsdmm_order_10": (lambda c: bsd(c, update_order=[1, 0]), {}),
    "bsdmm_order_10_user_prox": (lambda c: bsd(c, prox=(c.prox(), PLUS), update_order=[1, 0]), {}),
    "bsdmm_order_0": (lambda c: bsd(c, update_order=[0]), {}),
    "bsdmm_order_0_generic": (lambda c: bsd(c, closures=generic(c), update_order=[0]), {}),
    "bsdmm_order_empty": (lambda c: bsd(c, update_order=[], callback=c.callback()), {}),
    "bsdmm_order_empty_callback_stop": (lambda c: bsd(c, update_order=[], callback=c.callback(2)), {}),
    "bsdmm_refuse_fixed_steps_g": (lambda c: bsd(c, steps_g_update="fixed", steps_g=[[1.0], None]), {}),
    "bsdmm_refuse_Ls": (lambda c: bsd(c, Ls=[[np.eye(2)], None]), {}),
    "bsdmm_refuse_weighted": (lambda c: bsd(c, closures=dnmf.bsdmm_closures(c.Y, [PLUS, PLUS], W=np.ones((M, N)))), {}),
    "bsdmm_max_iter0_callback": (lambda c: bsd(c, max_iter=0, callback=c.callback()), {}),
    "bsdmm_f64_fused": (lambda c: bsd(c), F64),
    "bsdmm_f64_callback": (lambda c: bsd(c, callback=c.callback()), F64),
    "bsdmm_f64_user_prox": (lambda c: bsd(c, prox=(c.prox(), PLUS)), F64),
}


def _strip(s):
    return re.sub(r" at 0x[0-9a-fA-F]+", "", s)


class _Logs(logging.Handler):
    def __init__(self, T):
        super().__init__(logging.DEBUG)
        self.T = T

    def emit(self, record):
        self.T.append("log %s %s" % (record.levelname, _strip(record.getMessage())))


def run_route(name, patch):
    """-> the route's transcript, a list of lines"""
    fn, kw = ROUTES[name]
    c = Ctx(**kw)
    patch(algorithms, "_open_device", c.open_device)

    def run_rows(rows2d, ps, step_k):              # operators called on a host copy run a device kernel: recorded, identity
        c.T.append(call_line("operators._run_rows", (np.asarray(rows2d), ps, np.asarray(step_k)), {}))
        return np.ascontiguousarray(rows2d, dtype=np.float32)
    patch(operators, "_run_rows", run_rows)
    algorithms._warned.clear()
    log = logging.getLogger("proxmin")
    handler, level = _Logs(c.T), log.level
    log.addHandler(handler)
    log.setLevel(logging.DEBUG)
    try:
        try:
            c.T.append("return " + summ(fn(c)))
        except Exception as exc:                   # noqa: BLE001 -- the exception IS the recorded outcome
            c.T.append("raise %s: %s" % (type(exc).__name__, _strip(str(exc))))
    finally:
        log.removeHandler(handler)
        log.setLevel(level)
    c.T.append("A " + summ(c.A))
    c.T.append("S " + summ(c.S))
    c.T.append("warned " + summ(sorted(algorithms._warned)))
    algorithms._warned.clear()
    return c.T


# -- the sharded drivers --------------------------------------------------------------------------
class FakeTensor:
    """what reduce_scatter_sum / all_gather_chunks touch of a tensor; slices and clones keep a readable name"""

    class device:
        type = "cpu"

    def __init__(self, name, n):
        self.name, self.n = name, int(n)

    def numel(self):
        return self.n

    def view(self, *shape):
        return self

    def clone(self):
        return FakeTensor(self.name + ".clone", self.n)

    def __getitem__(self, s):
        return FakeTensor("%s[%d:%d]" % (self.name, s.start, s.stop), s.stop - s.start)

    def __repr__(self):
        return self.name


class RecDist:
    class ReduceOp:
        SUM = "SUM"

    def __init__(self, T, rank=1, world=2):
        self.T, self.rank, self.world = T, rank, world

    def all_reduce(self, t, op=None, group=None):
        self.T.append("all_reduce %r op=%s group=%r" % (t, op, group))

    def reduce_scatter_tensor(self, out, inp, op=None, group=None):
        self.T.append("reduce_scatter_tensor %r %r op=%s group=%r" % (out, inp, op, group))

    def all_gather_into_tensor(self, out, inp, group=None):
        self.T.append("all_gather_into_tensor %r %r group=%r" % (out, inp, group))

    def get_rank(self, group=None):
        return self.rank

    def get_world_size(self, group=None):
        return self.world


class RecShardEngine:
    """phase / chain_status / more_subs / tail_fused, recorded; chain_status answers from `status` (then: nothing halted,
    every enqueued iteration done)"""

    def __init__(self, T, status=(), s_split=False, st_iterate=False, fused=(True,)):
        self.T, self.status, self.fused = T, list(status), list(fused)
        self.comm = FakeTensor("comm", 32)
        self.last = 0
        if s_split:
            self.s_split = True
            self.comm_out = FakeTensor("comm_out", 16)
            self.st_full = FakeTensor("st_full", 2 * N * K)
            self.st_iterate = FakeTensor("st_iterate", 2 * N * K) if st_iterate else None

    def tail_fused(self):
        v = self.fused.pop(0) if len(self.fused) > 1 else self.fused[0]
        self.T.append("tail_fused -> %r" % v)
        return v

    def phase(self, *a):
        self.T.append("phase " + summ(a))
        if a[0] == 1:
            self.last = a[1] + 1

    def chain_status(self):
        st = self.status.pop(0) if self.status else (0, 0, self.last, (2, 2))
        self.T.append("chain_status -> " + summ(st))
        return st

    def more_subs(self, t0, n):
        self.T.append("more_subs %d %d" % (t0, n))


def _drive(T, make, run):
    try:
        drv = make()
        T.append("chunk %r nsub %r" % (drv.chunk, getattr(drv, "nsub", None)))
        try:
            T.append("return %r" % (run(drv),))
        finally:
            T.append("it %r stopped %r chunk %r nsub %r" % (drv.it, drv.stopped, drv.chunk, getattr(drv, "nsub", None)))
    except Exception as exc:                       # noqa: BLE001
        T.append("raise %s: %s" % (type(exc).__name__, _strip(str(exc))))


CONV, NEED, ERR = distributed.HALT_CONVERGED, distributed.HALT_NEED_SUB, distributed.HALT_ERROR
B1 = np.linspace(0.9, 0.5, 100)


def loop_case(status=(), n=4, chunk=2, deferred=True, runs=1, **eng):
    def case(T):
        e = RecShardEngine(T, status, **eng)
        _drive(T, lambda: distributed.ShardedLoop(e, "grp", deferred_test=deferred, chunk=chunk, dist_module=RecDist(T)),
               lambda d: [d.run(n) for _ in range(runs)])
    return case


def ada_case(status=(), n=4, chunk=2, check=True, any_prox=True, prox_max_iter=1000, runs=1, **eng):
    def case(T):
        e = RecShardEngine(T, status, **eng)
        _drive(T, lambda: distributed.ShardedAdaproxDriver(e, "grp", check, any_prox, prox_max_iter, chunk=chunk, dist_module=RecDist(T)),
               lambda d: [d.run(n, B1) for _ in range(runs)])
    return case


SHARDED = {
    "loop_two_chunks_flush_deferred": loop_case(),
    "loop_two_chunks_flush_converges": loop_case(status=[(0, 0, 2, (0, 0)), (0, 0, 4, (0, 0)), (1, CONV, 4, (0, 0))]),
    "loop_not_deferred": loop_case(deferred=False),
    "loop_converged_mid_chunk": loop_case(status=[(1, CONV, 3, (0, 0))], n=8, chunk=4),
    "loop_halt_error": loop_case(status=[(0, 0, 2, (0, 0)), (1, ERR, 3, (0, 0))]),
    "loop_halt_retry": loop_case(status=[(1, distributed.HALT_RETRY, 1, (0, 0))], n=3),
    "loop_run_zero": loop_case(n=0),
    "loop_two_runs": loop_case(n=2, runs=2),
    "loop_s_split": loop_case(n=3, s_split=True),
    "loop_s_split_fista": loop_case(n=3, s_split=True, st_iterate=True),
    "loop_s_split_fista_run_zero": loop_case(n=0, s_split=True, st_iterate=True),
    "ada_two_chunks_flush": ada_case(),
    "ada_two_chunks_flush_converges": ada_case(status=[(0, 0, 2, (3, 1)), (0, 0, 4, (1, 7)), (1, CONV, 4, (1, 7))]),
    "ada_no_check": ada_case(check=False),
    "ada_no_prox_keeps_nsub": ada_case(status=[(0, 0, 2, (5, 5))], n=2, any_prox=False),
    "ada_prox_max_iter_caps_nsub": ada_case(status=[(0, 0, 2, (9, 5))], n=2, prox_max_iter=4),
    "ada_converged_mid_chunk": ada_case(status=[(1, CONV, 3, (2, 2))], n=8, chunk=4),
    "ada_need_sub_resume": ada_case(status=[(1, NEED, 1, (2, 2)), (1, NEED, 1, (6, 2)), (0, 0, 4, (9, 3))], n=4, chunk=4),
    "ada_need_sub_progress": ada_case(status=[(1, NEED, 0, (2, 2)), (1, NEED, 2, (5, 2)), (0, 0, 4, (3, 3))], n=4, chunk=4),
    "ada_halt_error": ada_case(status=[(1, ERR, 1, (2, 2))]),
    "ada_halt_peer": ada_case(status=[(1, distributed.HALT_PEER, 1, (2, 2))], n=3, chunk=4),
    "ada_run_zero": ada_case(n=0),
    "ada_two_runs": ada_case(n=2, runs=2),
    "ada_s_split": ada_case(n=3, s_split=True),
    "ada_s_split_refuses_need_sub": ada_case(status=[(1, NEED, 1, (2, 2))], s_split=True),
    "ada_chunk_64_then_16": ada_case(n=82, chunk=None, fused=(True, True, False)),
    "ada_chunk_clamped_unfused": ada_case(n=70, chunk=100, fused=(True, False)),
    "ada_chunk_no_tail_fused_attr": lambda T: _drive(
        T, lambda: distributed.ShardedAdaproxDriver(type("E", (), {"phase": None})(), dist_module=RecDist(T)), lambda d: None),
}


def run_sharded(name):
    T = []
    SHARDED[name](T)
    return T


# -- golden file: one table of distinct lines, every route a list of indices into it ----------------
def record_all(patch):
    table, index, routes = [], {}, {}
    for name in list(ROUTES) + list(SHARDED):
        T = run_route(name, patch) if name in ROUTES else run_sharded(name)
        routes[name] = [index.setdefault(line, len(index)) for line in T]
        table.extend(line for line in T if index[line] == len(table))
    return {"lines": table, "routes": routes}


def dumps(gold):
    body = ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in gold["routes"].items())
    lines = ",\n".join("  " + json.dumps(line) for line in gold["lines"])
    return '{"lines": [\n%s\n],\n"routes": {\n%s\n}}\n' % (lines, body)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        g = json.load(fh)
    return {name: [g["lines"][i] for i in idx] for name, idx in g["routes"].items()}


def test_golden_lists_every_route(golden):
    assert sorted(golden) == sorted(list(ROUTES) + list(SHARDED))


@pytest.mark.parametrize("name", list(ROUTES))
def test_solver_route(name, golden, monkeypatch):
    for v in F64_SWITCHES:
        monkeypatch.delenv(v, raising=False)
    got = run_route(name, monkeypatch.setattr)
    assert got == golden[name]


@pytest.mark.parametrize("name", list(SHARDED))
def test_sharded_route(name, golden):
    assert run_sharded(name) == golden[name]


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_host_routes.py --record   (writes tests/golden/host_routes.json)")
    for v in F64_SWITCHES:
        os.environ.pop(v, None)
    gold = record_all(lambda obj, attr, value: setattr(obj, attr, value))
    with open(GOLDEN, "w") as fh:
        fh.write(dumps(gold))
    print("%d routes, %d transcript lines (%d distinct) -> %s" % (
        len(gold["routes"]), sum(len(v) for v in gold["routes"].values()), len(gold["lines"]), GOLDEN))
