"""Single-step parity of the update kernels behind pgm() and adaprox() (csrc/k_update.hip: k_pgm_update, k_ada_moment,
k_ada_sub, k_ada_finish, the fused k_ada_tail) with the fp64 oracle, on EVERY entry.

The gradient comes from a table -- a list of (GA, GS) float32 pairs, one per iteration, served by a closure with a counter
to the device (`pm.pgm([A, S], grad, ...)` / `pm.adaprox([A, S], grad, ...)` take any callable as `grad`) and to the oracle
(`grad=` of oracle.nmf_oracle.pgm_nmf / adaprox_nmf).  It does not depend on X: K1, Y and their summation-order noise are out
of the picture and nothing feeds a rounding difference back, so what is left -- element-wise arithmetic, the row / column
mapping of the element-wise grid, a handful of reductions -- must agree with the fp64 oracle entry by entry.  There is no
in-tolerance fraction and no envelope here.

Tolerances.  For every compared quantity the oracle was run in float32 and in float64 on the very inputs of every case
below (`python tests/test_gpu_update_step.py`, CPU only, prints the table) and the element-wise difference expressed in
units of 2^-23 times the entry's natural scale: the entry's own magnitude for M, V, Vhat and the returned steps,
max(|x|, largest |alpha Phi / Psi| (adaprox) or |step g| (pgm) the entry saw) for the factors.  REF_ERR_* are the largest
values over the case list, the device is allowed TOL_* = 4 x that: its evaluation order differs in equally valid ways (M
formed in fp64 and rounded once, fma contraction, the ulp of sqrtf / powf, unity's row sum in another order).

What keeps the comparison honest is checked on the oracle alone, without a GPU (test_reference_preconditions): no argument
of a hard threshold within 1e-4 (relative) of the threshold in any pass, and every stopping decision the reference takes
-- proximal sub-iteration loops and the outer test -- has its quantity d / (e^2 n) outside [0.5, 2], so that the
sub-iteration counts, `converged` and the iteration count can be asserted EQUAL.

Where the reference's own behaviour is the surprising one, the reference wins: a cold start returns Vhat = [None, None]
also for amsgrad / padam / adamx and never accumulates a running maximum (algorithms.py:176-177: a local name is rebound);
adamx reads b1[-1] at iteration 0 (:213); a NaN in Psi poisons the whole block through gamma = Alpha / np.max(Psi) (:384).
"""
import contextlib
import functools
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

ULP = 2.0 ** -23

# Largest float32-oracle vs float64-oracle difference over ALL cases below, in units of 2^-23 x natural scale (see the
# module docstring; reproduce with `python tests/test_gpu_update_step.py`), and the device's allowance: 4 x.
REF_ERR_ADA_X, REF_ERR_ADA_M, REF_ERR_ADA_V, REF_ERR_ADA_VHAT = 88.9, 231.3, 6.23, 4.46
REF_ERR_PGM_X, REF_ERR_PGM_STEP = 19.7, 0.716
TOL_ADA_X, TOL_ADA_M, TOL_ADA_V, TOL_ADA_VHAT = 4 * REF_ERR_ADA_X, 4 * REF_ERR_ADA_M, 4 * REF_ERR_ADA_V, 4 * REF_ERR_ADA_VHAT
TOL_PGM_X, TOL_PGM_STEP = 4 * REF_ERR_PGM_X, 4 * REF_ERR_PGM_STEP

HARD_GUARD = 1e-4            # no |argument| of a hard threshold within this (relative) of the threshold
BAND = (0.5, 2.0)            # no stopping decision with d / (e^2 n) in here

# (M, N, K): one call covers two row counts, M rows of A and N rows of S^T.  K covers the NC = 1..4 instantiations and their
# ragged last 32-column group; the rows the 8192-row sweep of the element-wise grid (256 workgroups x 1024 threads, one
# half-wave per row), k_pgm_update's Gram side-output switch at 4096 rows and the tail's ceil(rows / 8192) row slots.
# Every K that is no multiple of 32 meets a row count >= 8192.
SHAPES = [
    (1, 8192, 1), (31, 8193, 2), (33, 8192, 31), (4096, 1, 32), (8193, 33, 33), (16385, 31, 63), (4097, 4096, 64),
    (8191, 8193, 65), (1, 4097, 96), (16385, 33, 97), (8192, 31, 127), (31, 16385, 128), (8193, 1, 97), (33, 8191, 127),
    (4096, 8193, 31), (16385, 4097, 33),
]
# the axes below are element-wise arithmetic, orthogonal to the row / column mapping: a ragged K with two row sweeps, a
# ragged K below one sweep, a full K at the 4096-row switch, and a tiny one
SUBSET = [(8193, 33, 33), (33, 8191, 127), (4097, 4096, 64), (31, 33, 2)]
SUBSET2 = [(8193, 33, 33), (31, 33, 2)]
# hard thresholding is discontinuous: few entries, so that a seed exists for which nothing comes near the threshold
HARD_SHAPES = [(8193, 33, 2), (31, 33, 65)]

SCHEMES = ("adam", "nadam", "amsgrad", "padam", "adamx", "radam")
ADA_ITERS, PGM_ITERS = 8, 6

PROX_PAIRS = {
    "plus_plus": (("plus",), ("plus",)),
    "plus_unity": (("plus",), ("unity_plus", 0)),
    "none_soft": (None, ("soft", 5.0, "relative")),
    "softplus_minmax": (("soft_plus", 1e-3, "absolute"), ("seq", (("min", 0.3, "absolute"), ("max", 0.8, "absolute")), 1)),
    "ap_unity": (("plus",), ("seq", (("unity", 0), ("plus",)), 2)),
    "hard": (("hard", "T", "relative"), ("hard", "T", "relative")),        # "T": set per case so that the threshold is ~0.12
}
PGM_PROX_PAIRS = dict(PROX_PAIRS, none_soft=(None, ("soft", 0.5, "relative")))


# ---------------------------------------------------------------------------------------------------------------------
# the case list
# ---------------------------------------------------------------------------------------------------------------------
ADA_DEFAULTS = dict(backend="ada", scheme="adam", iters=ADA_ITERS, b1=0.9, b2=0.999, eps=1e-8, p=0.25, prox="plus_unity", warm=False,
                    check=True, pmi=3, e_rel=1e-7, table="full", step=(0.01, 0.02), nan=False, seed=7, hard_T=None,
                    stop_at=None, hits_pmi=False, shrink_from=4)
PGM_DEFAULTS = dict(backend="pgm", accelerated=False, iters=PGM_ITERS, prox="plus_unity", e_rel=1e-6, table="full", step=(4e-5, 2e-5),
                    seed=7, hard_T=None, stop_at=None, nan=False, shrink_from=3)


def _mk(defaults, shape, **kw):
    c = dict(defaults, shape=tuple(shape), **kw)
    tag = [c["backend"], "%dx%dx%d" % c["shape"]]
    for k in sorted(kw):
        v = kw[k]
        if k == "hard_T":
            continue
        tag.append("%s=%s" % (k, v if not isinstance(v, tuple) else "_".join(str(x) for x in v)))
    c["id"] = "-".join(tag)
    return c


def _ada_cases():
    """The reference's proximal loop contracts entry by entry with 1 - Psi / max(Psi): with Psi spread over nine decades its
    stopping quantity falls by less than 2x per pass, so a loop that ends by its own test always passes through [0.5, 2].
    The cases therefore end their loops in the two ways that leave a margin: `plus` is met exactly at pass 2 (d = 0), and
    every other operator runs with e_rel = 1e-7 into prox_max_iter = 3 -- three full passes of the loop's arithmetic."""
    out = []
    a = partial(_mk, ADA_DEFAULTS)
    nat = dict(prox="plus_plus", pmi=1000, e_rel=1e-3)      # loops that end by their own test
    for scheme in SCHEMES:                                  # all six schemes on every shape (radam's switch inside the window)
        out += [a(s, scheme=scheme, **({"prox": "plus_plus"} if s[2] == 1 else {})) for s in SHAPES]   # (unity over K = 1 pins S at 1)
    for s in SUBSET:                                        # warm M, V, Vhat (above and below V); adamx with a b1 schedule
        out += [a(s, scheme=sc, warm=True, seed=9, b1="sched" if sc == "adamx" else 0.9) for sc in ("amsgrad", "padam", "adamx")]
        out += [a(s, scheme="adam", warm=True, seed=12)]
        out += [a(s, scheme=sc, **nat) for sc in ("nadam", "adam")]
    for s in SUBSET2:
        for eps, table in ((1e-3, "full"), (0.0, "nozero")):
            out += [a(s, scheme="adam", eps=eps, table=table), a(s, scheme="radam", eps=eps, table=table),
                    a(s, scheme="amsgrad", eps=eps, table=table, warm=True), a(s, scheme="padam", eps=eps, table=table)]
        out += [a(s, scheme="padam", p=p, warm=True) for p in (0.125, 0.5)]
        out += [a(s, scheme="adamx", b1="sched")]          # cold: iteration 0 reads b1[-1], Vhat stays None
        out += [a(s, scheme="nadam", check=False), a(s, scheme="amsgrad", warm=True, check=False, **nat)]
        out += [a(s, scheme="adam", prox="ap_unity", hits_pmi=True)]                          # the loop runs into prox_max_iter = 3
        # loops longer than one launch / round of 4 passes: S ends inside the second one (k_ada_finish replays from a later launch's
        # input, the tail redoes the passes that count); at 18 the 16-pass sum ring wraps and the chain asks the host for more passes
        out += [a(s, scheme="adam", prox="ap_unity", hits_pmi=True, pmi=pmi) for pmi in (6, 18)]
        out += [a(s, scheme="adam", step="rule"), a(s, scheme="amsgrad", warm=True, step="rule")]   # nmf.step_adaprox on the device
        out += [a(s, scheme="adam", table="shrink", b1=0.0, eps=1e-3, stop_at=5, **dict(nat, e_rel=3e-3))]    # the outer test fires at a known iteration
    for s in SUBSET:
        out += [a(s, scheme="adam" if i % 2 else "amsgrad", prox=p) for i, p in enumerate(("none_soft", "softplus_minmax", "ap_unity"))]
    out += [a(s, scheme="adam", prox="hard", hard_T=0.12, step=(0.002, 0.002), seed=11) for s in HARD_SHAPES]
    out += [a((8193, 33, 33), scheme="adam", nan=True)]
    return out


ACC_STOP_E_REL = {(8193, 33, 33): (7.63e-3, 7.67e-2), (31, 33, 2): (7.11e-3, 6.26e-6)}


def _pgm_cases():
    out = []
    for acc in (False, True):
        g = partial(_mk, PGM_DEFAULTS, accelerated=acc)
        out += [g(s, **({"prox": "plus_plus"} if s[2] == 1 else {})) for s in SHAPES]
        for s in SUBSET2:
            out += [g(s, prox=p) for p in ("none_soft", "softplus_minmax", "ap_unity")]
            out += [g(s, step="rule", prox="plus_plus")]                                     # nmf.step_pgm: the Lipschitz rule
            if not acc:                                                                      # e_rel met at a known iteration
                out += [g(s, table="shrink", e_rel=1e-4, stop_at=4)]
            else:       # FISTA keeps moving by omega (X - X_prev) after the gradient is gone: d falls by omega^2 = 0.08 in the second
                        # iteration, and a per-block e_rel puts d / (e^2 n) at ~3.5 before and ~0.28 after that fall
                out += [g(s, table="shrink", shrink_from=1, e_rel=ACC_STOP_E_REL[s], stop_at=2)]
        out += [g(s, prox="hard", hard_T=0.12, seed=11) for s in HARD_SHAPES]
    return out


ADA_CASES = _ada_cases()
PGM_CASES = _pgm_cases()
ALL_CASES = ADA_CASES + PGM_CASES
assert len({c["id"] for c in ALL_CASES}) == len(ALL_CASES)


# ---------------------------------------------------------------------------------------------------------------------
# inputs: seeded and fixed
# ---------------------------------------------------------------------------------------------------------------------
def _grad_block(rng, shape, kind):
    """ordinary values in +-1, exact zeros, |g| ~ 1e-6 (V below eps = 1e-8: the clamp is active), |g| ~ 1e3"""
    u = rng.random(shape)
    g = rng.uniform(-1.0, 1.0, shape)
    sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    mag = 0.5 + rng.random(shape)
    g = np.where(u < 0.25, sign * 1e3 * mag, g)
    g = np.where(u < 0.20, sign * 1e-6 * mag, g)
    if kind != "nozero":
        g = np.where(u < 0.10, 0.0, g)
    else:
        g = np.where(g == 0.0, 0.5, g)
    return g.astype(np.float32)


def make_table(c):
    M, N, K = c["shape"]
    rng = np.random.default_rng(1000 + c["seed"])
    base = [(_grad_block(rng, (M, K), c["table"]), _grad_block(rng, (K, N), c["table"])) for _ in range(2)]
    # every entry keeps its sign over the iterations: M = (1 - b1) g + b1 M then never cancels, and "the entry's own magnitude"
    # stays a meaningful scale for it (with free signs the float32 reference itself is off by more than M's magnitude on the
    # handful of entries in a million where the two terms cancel to 1e-7)
    sgn = [np.where(rng.random(s) < 0.5, np.float32(-1), np.float32(1)) for s in ((M, K), (K, N))]
    zc = K // 2
    table = []
    for it in range(c["iters"]):
        GA, GS = base[it % 2]
        # other rows' magnitudes in later iterations: every entry meets several of them
        GA = np.abs(np.roll(GA, 13 * it, axis=0)) * sgn[0]
        GS = np.abs(np.roll(GS, 13 * it, axis=1)) * sgn[1]
        if c["table"] == "shrink" and it >= c["shrink_from"]:      # later entries shrink: the outer test fires at a known iteration
            f = np.float32(1e-6 ** (it - c["shrink_from"] + 1))
            GA, GS = GA * f, GS * f
        if c["table"] != "nozero" and K >= 2:            # one component that is zero in every iteration
            GA[:, zc] = 0
            GS[zc, :] = 0
        table.append((np.ascontiguousarray(GA, dtype=np.float32), np.ascontiguousarray(GS, dtype=np.float32)))
    if c["nan"]:
        table[1][0][M // 2, K - 1] = np.nan
    return table


def make_inputs(c):
    M, N, K = c["shape"]
    rng = np.random.default_rng(c["seed"])
    if c["prox"] == "hard":      # nothing between 0.02 and 0.8: the threshold (~0.12, moving with max(Psi) in adaprox) sits in the gap
        def draw(shape):
            return np.where(rng.random(shape) < 0.5, 0.01 + 0.01 * rng.random(shape), 0.8 + 0.2 * rng.random(shape)).astype(np.float32)
    else:
        def draw(shape):
            return (0.2 + 0.8 * rng.random(shape)).astype(np.float32)
    A0, S0 = draw((M, K)), draw((K, N))
    pS = _prox_pairs(c)[1]
    if pS is not None and ("unity" in pS[0] or pS[0] == "seq" and any("unity" in q[0] for q in pS[1])):
        S0 = (S0 / S0.sum(0, keepdims=True)).astype(np.float32)
    inp = dict(A0=A0, S0=S0, table=make_table(c))
    if c["backend"] == "ada":
        b1 = c["b1"]
        inp["b1"] = 0.9 * 0.9 ** np.arange(c["iters"]) if isinstance(b1, str) else b1          # b1[it-1] != b1[it]; b1[-1] != b1[0]
        if c["warm"]:
            shapes = ((M, K), (K, N))
            inp["M"] = [rng.uniform(-0.05, 0.05, s).astype(np.float32) for s in shapes]
            inp["V"] = [np.where(rng.random(s) < 0.1, 0.0, 1e-2 * rng.random(s)).astype(np.float32) for s in shapes]
            inp["Vhat"] = [(v * np.where(rng.random(v.shape) < 0.5, 0.5, 2.0)).astype(np.float32) for v in inp["V"]]   # below and above V
    return inp


def _prox_pairs(c):
    return (PROX_PAIRS if c["backend"] == "ada" else PGM_PROX_PAIRS)[c["prox"]]


def table_grad(table, dtype):
    """the closure with a counter that serves the table (to the device: float32; to the oracle: its float64 casts)"""
    state = {"i": 0}

    def grad(A, S):
        GA, GS = table[min(state["i"], len(table) - 1)]
        state["i"] += 1
        return GA.astype(dtype), GS.astype(dtype)
    grad.state = state
    return grad


# ---------------------------------------------------------------------------------------------------------------------
# the reference: oracle runs, with probes on its stopping decisions and hard thresholds
# ---------------------------------------------------------------------------------------------------------------------
def prox_specs(c):
    """the pair of prox specs of a case; a relative hard threshold gets thresh = hard_T / (nominal step handed to the prox):
    adaprox hands gamma = alpha / max(Psi), max(Psi) ~ 1.5e3 with this table; pgm hands the block's step"""
    pair = _prox_pairs(c)
    if c["prox"] != "hard":
        return pair
    nominal = [a / 1.5e3 for a in c["step"]] if c["backend"] == "ada" else list(c["step"])
    return tuple((q[0], float(np.float32(c["hard_T"] / nominal[j])), q[2]) for j, q in enumerate(pair))


class Probe:
    """records, inside one oracle run: every stopping decision (d, n) = (|x' - x|^2, |x'|^2), the closest any argument of a
    hard threshold comes to the threshold, and per entry the largest update magnitude |alpha Phi / Psi| / |step g|"""

    def __init__(self, orc):
        self.orc, self.decisions, self.hard_margin, self.U, self.alpha = orc, [], np.inf, [0.0, 0.0], None
        self._pend, self._nmom = None, 0

    def __enter__(self):
        o = self.orc
        self._saved = (o._sumsq, o.apply_prox, o.moment_update)
        sumsq, apply_prox, moment_update = self._saved

        def _sumsq(x):
            v = sumsq(x)
            if self._pend is None:
                self._pend = v
            else:
                self.decisions.append((float(self._pend), float(v)))
                self._pend = None
            return v

        def _apply_prox(X, step, spec):
            if spec is not None and spec[0] in ("hard", "hard_plus"):
                t = o._threshold(step, spec[1], spec[2] if len(spec) > 2 else "relative")
                with np.errstate(invalid="ignore", divide="ignore"):
                    m = np.nanmin(np.abs(np.abs(X) - t) / t) if np.isfinite(X).any() else np.inf
                self.hard_margin = min(self.hard_margin, float(m))
            return apply_prox(X, step, spec)

        def _moment_update(scheme, it, G, *a):
            Phi, Psi = moment_update(scheme, it, G, *a)
            j = self._nmom % 2
            self._nmom += 1
            with np.errstate(invalid="ignore", divide="ignore"):
                self.U[j] = np.fmax(self.U[j], np.abs(self.alpha[j] * Phi / Psi))
            return Phi, Psi
        o._sumsq, o.apply_prox, o.moment_update = _sumsq, _apply_prox, _moment_update
        return self

    def __exit__(self, *exc):
        self.orc._sumsq, self.orc.apply_prox, self.orc.moment_update = self._saved
        return False


def run_reference(c, dtype=np.float64):
    from oracle import nmf_oracle as orc
    inp = make_inputs(c)
    A, S = inp["A0"].astype(dtype), inp["S0"].astype(dtype)
    pA, pS = prox_specs(c)
    grad = table_grad(inp["table"], dtype)
    out = dict(dtype=dtype)
    with Probe(orc) as pr:
        if c["backend"] == "ada":
            def step(A_, S_, it):
                pr.alpha = orc.adaprox_steps(A_, S_) if c["step"] == "rule" else tuple(c["step"])
                return pr.alpha
            warm = {k: [x.astype(dtype) for x in inp[k]] for k in ("M", "V", "Vhat")} if c["warm"] else {}
            conv, Mo, Vo, Vh, n_it, sub = orc.adaprox_nmf(None, A, S, pA, pS, step=step, scheme=c["scheme"], b1=inp["b1"], b2=c["b2"],
                                                          eps=c["eps"], check_convergence=c["check"], p=c["p"], max_iter=c["iters"],
                                                          e_rel=c["e_rel"], prox_max_iter=c["pmi"], grad=grad, **warm)
            out.update(M=Mo, V=Vo, Vhat=Vh, sub=[int(x) for x in sub])
        else:
            def step(E0, E1, it, G):
                s = orc.lipschitz_steps(E0, E1) if c["step"] == "rule" else tuple(c["step"])
                for j in range(2):
                    pr.U[j] = np.fmax(pr.U[j], np.abs(s[j] * G[j]))
                return s
            conv, G, St, n_it = orc.pgm_nmf(None, A, S, pA, pS, step=step, accelerated=c["accelerated"], max_iter=c["iters"],
                                            e_rel=c["e_rel"], grad=grad)
            out.update(G=G, steps=[float(s) for s in St])
    out.update(A=A, S=S, conv=tuple(conv), n_iter=int(n_it), U=pr.U, decisions=pr.decisions, hard_margin=pr.hard_margin)
    return out


@functools.lru_cache(maxsize=4)
def reference(case_id):
    """the fp64 oracle run of a case: computed once, shared by the tests that need it, never modified"""
    return run_reference(CASE_BY_ID[case_id])


CASE_BY_ID = {c["id"]: c for c in ALL_CASES}


def decision_e_rel(c, i):
    """e_rel of the i-th probed decision (a pair only in pgm, whose decisions alternate between the blocks)"""
    return c["e_rel"][i % 2] if isinstance(c["e_rel"], tuple) else c["e_rel"]


def radam_switch_iteration(b2, n=10000):
    """first 0-based iteration at which radam's rho exceeds 4 (algorithms.py:231-236)"""
    rho_inf = 2 / (1 - b2) - 1
    for it in range(n):
        t = it + 1
        if rho_inf - 2 * t * b2 ** t / (1 - b2 ** t) > 4:
            return it
    raise AssertionError("rho never exceeds 4")


def units(got, want, scale):
    """largest |got - want| in units of 2^-23 x scale over the finite entries of `want` (a zero scale admits no difference)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), want.shape)
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    err = np.abs(got - want)[fin]
    sc = ULP * scale[fin]
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where(err == 0, 0.0, err / sc)
    return float(np.max(np.where(np.isnan(u), np.inf, u)))


def quantities(c, run, ref):
    """[(name, tolerance key, units of `run` against `ref`)] for everything a solver hands back as numbers"""
    out = []
    for j, name in enumerate("AS"):
        out.append((name, "X", units(run[name], ref[name], np.fmax(np.abs(ref[name]), ref["U"][j]))))
    if c["backend"] == "ada":
        for key in ("M", "V") + (("Vhat",) if c["warm"] else ()):
            for j in range(2):
                out.append(("%s[%d]" % (key, j), key.upper(), units(run[key][j], ref[key][j], np.abs(ref[key][j]))))
    else:
        for j in range(2):
            out.append(("step[%d]" % j, "STEP", units(run["steps"][j], ref["steps"][j], abs(ref["steps"][j]))))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the conditions under which "every entry, equal decisions" is a fair demand
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in ALL_CASES])
def test_reference_preconditions(cid):
    """On the fp64 oracle alone: guard band of the hard thresholds, margins of every stopping decision, and that each case
    exercises what it is there for (radam's switch inside the window, the early stop, the exhausted proximal loop, NaN)."""
    c = CASE_BY_ID[cid]
    ref = reference(cid)
    if c["prox"] == "hard":
        assert ref["hard_margin"] < np.inf, "the hard threshold never ran"
        assert ref["hard_margin"] >= HARD_GUARD, "an argument of the hard threshold lies within %g of it" % ref["hard_margin"]
        for X in (ref["A"], ref["S"]):
            assert 0.05 < np.mean(X == 0) < 0.95, "the threshold must zero some entries and keep others"
    n_nan = 0
    for i, (d, n) in enumerate(ref["decisions"]):
        e2 = decision_e_rel(c, i) ** 2
        if np.isnan(d) or np.isnan(n):
            n_nan += 1            # NaN <= x is False on the device as well
            continue
        if d == 0:
            continue              # met exactly: nothing moved
        q = d / (e2 * n) if n > 0 else np.inf
        assert not (BAND[0] <= q <= BAND[1]), "a stopping decision with d / (e^2 n) = %g" % q
    assert ref["decisions"], "no stopping decision was probed"
    assert (n_nan > 0) == bool(c["nan"])
    if c["stop_at"] is not None:
        assert ref["n_iter"] == c["stop_at"] < c["iters"] and all(ref["conv"])
    else:
        assert ref["n_iter"] == c["iters"]
    if c["backend"] == "ada":
        if c["scheme"] == "radam":
            assert 0 < radam_switch_iteration(c["b2"]) < c["iters"] - 1
        if c["hits_pmi"]:
            assert ref["sub"][1] == c["pmi"] * c["iters"], ref["sub"]
        if c["warm"]:
            inp = make_inputs(c)
            assert all((vh > v).any() and (vh < v).any() for vh, v in zip(inp["Vhat"], inp["V"]))
        if c["nan"]:
            assert np.isnan(ref["A"]).all() and np.isfinite(ref["S"]).all()
        if c["eps"] == 0:
            assert all((ga != 0).all() and (gs != 0).all() for ga, gs in make_inputs(c)["table"])
    if c["table"] == "full" and c["shape"][2] >= 2:
        t = make_inputs(c)["table"]
        K = c["shape"][2]
        assert all((ga[:, K // 2] == 0).all() and (gs[K // 2] == 0).all() for ga, gs in t)
        g = np.abs(np.concatenate([t[0][0].ravel(), t[0][1].ravel()]))
        if g.size >= 2000:
            assert (g == 0).any() and ((g > 0) & (g < 2e-6)).any() and (g > 400).any() and ((g > 1e-3) & (g <= 1)).any()


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pm():
    import __graft_entry__ as g
    g.build()
    import proxmin_amd
    return proxmin_amd


def spec_to_prox(pm, spec):
    if spec is None:
        return None
    ops = pm.operators
    if spec[0] == "seq":
        return ops.AlternatingProjections([spec_to_prox(pm, q) for q in spec[1]], repeat=spec[2])
    fn = getattr(ops, "prox_" + spec[0])
    if spec[0] in ("unity", "unity_plus"):
        return partial(fn, axis=spec[1])
    if len(spec) > 1:
        return partial(fn, thresh=spec[1], type=spec[2])
    return fn


@contextlib.contextmanager
def completed_log():
    """what the solvers log like the reference does (algorithms.py:140, :415-417): iterations and sub-iterations"""
    got = {}

    class H(logging.Handler):
        def emit(self, record):
            m = re.match(r"Completed (\d+) iterations(?: and \[(\d+), (\d+)\] sub-iterations)?", record.getMessage())
            if m:
                got["n_iter"] = int(m.group(1))
                if m.group(2) is not None:
                    got["sub"] = [int(m.group(2)), int(m.group(3))]
    log = logging.getLogger("proxmin")
    h, level = H(), log.level
    log.addHandler(h)
    log.setLevel(logging.INFO)
    try:
        yield got
    finally:
        log.removeHandler(h)
        log.setLevel(level)


def run_device(pm, c):
    inp = make_inputs(c)
    A, S = inp["A0"].copy(), inp["S0"].copy()
    prox = [spec_to_prox(pm, q) for q in prox_specs(c)]
    grad = table_grad(inp["table"], np.float32)
    out = {}
    with completed_log() as log:
        if c["backend"] == "ada":
            step = pm.nmf.step_adaprox if c["step"] == "rule" else pm.nmf.constant_step(*c["step"])
            warm = {k: [x.copy() for x in inp[k]] for k in ("M", "V", "Vhat")} if c["warm"] else {}
            conv, Mo, Vo, Vh = pm.adaprox([A, S], grad, step, prox=prox, scheme=c["scheme"], b1=inp["b1"], b2=c["b2"], eps=c["eps"],
                                          check_convergence=c["check"], p=c["p"], e_rel=c["e_rel"], max_iter=c["iters"],
                                          prox_max_iter=c["pmi"], **warm)
            out.update(M=Mo, V=Vo, Vhat=Vh)
        else:
            step = pm.nmf.step_pgm if c["step"] == "rule" else pm.nmf.constant_step(*c["step"])
            conv, G, St = pm.pgm([A, S], grad, step, prox=prox, accelerated=c["accelerated"], e_rel=c["e_rel"], max_iter=c["iters"])
            out.update(G=G, steps=[float(s) for s in St])
    out.update(A=A, S=S, conv=tuple(conv), served=grad.state["i"], **log)
    return out


def assert_meets_reference(c, run, ref, what):
    tol = {"X": TOL_ADA_X, "M": TOL_ADA_M, "V": TOL_ADA_V, "VHAT": TOL_ADA_VHAT} if c["backend"] == "ada" else {"X": TOL_PGM_X, "STEP": TOL_PGM_STEP}
    assert run["conv"] == ref["conv"], (what, run["conv"], ref["conv"])
    assert run["n_iter"] == ref["n_iter"] == run["served"], (what, run["n_iter"], ref["n_iter"], run["served"])
    if c["backend"] == "ada":
        assert run["sub"] == ref["sub"], (what, run["sub"], ref["sub"])
        if not c["warm"]:
            assert list(run["Vhat"]) == [None, None] == list(ref["Vhat"])        # the reference's cold start keeps no running maximum
        names = [("A", run["A"], ref["A"]), ("S", run["S"], ref["S"])]
        names += [("%s[%d]" % (k, j), run[k][j], ref[k][j]) for k in ("M", "V") + (("Vhat",) if c["warm"] else ()) for j in range(2)]
        for name, got, want in names:                                            # NaNs where the reference has them, nowhere else
            np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg="%s: NaN pattern of %s" % (what, name))
    else:
        for j in range(2):                                                       # the callable's own result at the last evaluation point
            np.testing.assert_array_equal(run["G"][j], ref["G"][j].astype(np.float32), err_msg="%s: G[%d]" % (what, j))
        assert np.isfinite(run["A"]).all() and np.isfinite(run["S"]).all()
    q = quantities(c, run, ref)
    print("%s %s: %s" % (c["id"], what, ", ".join("%s %.3g" % (n, u) for n, _, u in q)))
    for name, key, u in q:
        assert u <= tol[key], "%s: %s differs from the fp64 oracle by %.4g x 2^-23 x scale on some entry (allowed: %.4g)" % (what, name, u, tol[key])


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c["id"] for c in ADA_CASES])
def test_adaprox_update_matches_the_oracle_on_every_entry(pm, monkeypatch, cid):
    """A, S, M, V (, Vhat), `converged`, the iteration count and the accumulated sub-iteration counts of adaprox fed by the
    gradient table: the fused tail (k_ada_tail) and the chain of kernels each against the fp64 oracle on every entry, and
    against each other bit for bit."""
    c = CASE_BY_ID[cid]
    ref = reference(cid)
    runs = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("PMX_TAIL_FUSED", fused)
        runs[fused] = run_device(pm, c)
        assert_meets_reference(c, runs[fused], ref, "PMX_TAIL_FUSED=" + fused)
    f, u = runs["1"], runs["0"]
    assert f["conv"] == u["conv"] and f["n_iter"] == u["n_iter"] and f["sub"] == u["sub"]
    for key in ("A", "S"):
        np.testing.assert_array_equal(f[key], u[key])
    for key in ("M", "V") + (("Vhat",) if c["warm"] else ()):
        for j in range(2):
            np.testing.assert_array_equal(f[key][j], u[key][j])


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c["id"] for c in PGM_CASES])
def test_pgm_update_matches_the_oracle_on_every_entry(pm, cid):
    """A, S, the returned gradient and steps, `converged` and the iteration count of pgm / FISTA fed by the gradient table
    against the fp64 oracle on every entry."""
    c = CASE_BY_ID[cid]
    assert_meets_reference(c, run_device(pm, c), reference(cid), "pgm")


# ---------------------------------------------------------------------------------------------------------------------
# how REF_ERR_* were obtained: python tests/test_gpu_update_step.py  (CPU only)
# ---------------------------------------------------------------------------------------------------------------------
def measure(cases=ALL_CASES, verbose=True):
    worst = {}
    for c in cases:
        ref = run_reference(c, np.float64)
        r32 = run_reference(c, np.float32)
        same = r32["conv"] == ref["conv"] and r32["n_iter"] == ref["n_iter"] and r32.get("sub") == ref.get("sub")
        q = quantities(c, r32, ref)
        if verbose:
            qs = [d / (decision_e_rel(c, i) ** 2 * n) for i, (d, n) in enumerate(ref["decisions"]) if d > 0 and n > 0]
            near = min(qs, key=lambda x: abs(np.log(x))) if qs else None
            print("%-70s %s decisions %s  nearest q %s hard %.3g | %s" % (c["id"], ("" if same else "DECISIONS DIFFER") + ("" if near is None or not 0.5 <= near <= 2 else " IN BAND"), (ref["n_iter"], ref.get("sub")), near, ref["hard_margin"],
                                                                          " ".join("%s %.3g" % (n, u) for n, _, u in q)), flush=True)
        for _, key, u in q:
            k = (c["backend"], key)
            if u > worst.get(k, (0, None))[0]:
                worst[k] = (u, c["id"])
    for k in sorted(worst):
        print("REF_ERR %s %s = %.4g   (%s)" % (k[0], k[1], worst[k][0], worst[k][1]))
    return worst


if __name__ == "__main__":
    pat = sys.argv[1] if len(sys.argv) > 1 else ""
    measure([c for c in ALL_CASES if re.search(pat, c["id"])])
