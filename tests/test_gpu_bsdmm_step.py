"""Single-step parity of the bSDMM block update (csrc/k_update.hip: k_bsdmm_update<NC, ME>, k_bsdmm_decide, and the Boyd test
that rides in k_gram_reduce) with the fp64 oracle: X_j, every Z_i and every U_i on EVERY entry after EVERY iteration, the two
sums of every block (d2 = sum (X_new - X_old)^2, x2 = sum X_new^2), `converged` and the iteration count.

The gradient comes from a table -- a list of (GA, GS) float32 pairs, one per iteration, independent of X -- uploaded into the
gradient buffers of a context with set_host_grad(True): K1 never runs there and the update kernel reads that buffer as its only
slab, so Y, K1 and their summation-order noise are out of the picture.  Two routes:

  split   engine level, DeviceNMF.bsdmm_split: the step of every block update is chosen here (no step rule runs), stage 2 alone
          (device prox_f, every constraint on the device), stage 1 + 2 (`host_f`: prox_f applied by the host) and stage 2 + 3 (a
          `host_g` mask: those members of proxs_g applied by the host).  A hosted operator is the oracle's apply_prox in float32 on
          what the device handed out, uploaded back the way algorithms._bsdmm_nmf.advance does it.
  fused   DeviceNMF.bsdmm_run(1) once per iteration: stage 0 with its partial-Gram and maxima side outputs and the Boyd test in
          the next k_gram_reduce.  The steps are the device's Lipschitz rule (pinned in test_gpu_step_rule.py): they are read from
          the result of each call, rounded to float32 as the kernel rounds them, and handed to the oracle.

Tolerances are measured, not chosen.  For every case the oracle runs in float32 and in float64 on the very inputs and steps
(`python tests/test_gpu_bsdmm_step.py`, CPU only, prints the table); the largest element-wise difference after any iteration is
expressed in units of 2^-23 times the entry's natural scale: the largest magnitude among the terms the entry was formed from in
that update -- |x| before and after, |step_f g|, every |Z_i| and |U_i| before and after -- or in an earlier one (an error made
at a large scale stays in the entry when it shrinks) and, where an operator of the block is `unity`, the largest such value of
the row (the sum runs over it).  x2 is measured against itself and d2 against
sqrt(d2 * sum scale^2): d2 sums differences of neighbours, each off by 2^-23 x scale, so its own error is 2 sqrt(d2) times the
root of the summed squares of those.  REF_ERR_BSDMM_* are the largest values over the case list and the device is allowed
4 x that (fma contraction, another summation order in `unity` and in the sums), the margin of test_gpu_update_step.py.

    float32 oracle against float64 oracle (REF_ERR_BSDMM_*):   X 6.48    Z 6.14    U 17.3    NORM 3.13
    allowed to the device (4 x):                               X 25.9    Z 24.6    U 69.2    NORM 12.5
    worst seen on an MI355X, device against float64 oracle:    X 4.18    Z 5.92    U 7.46    NORM 1.84

What keeps "equal decisions" a fair demand is checked on the oracle alone (test_reference_preconditions, no GPU): no argument
of a hard threshold within HARD_GUARD (relative) of it, and every Boyd decision has lR / e_pri and lS / e_dual outside BAND in
both precisions (a ratio 0 / 0 -- nothing moved, nothing demanded -- is met exactly in any arithmetic).

Which shape reaches what (rows per workgroup: per = 32 ceil(rows / 8192); the partial-Gram side output runs for a block when
K <= 64, the problem is not "eig-small" (K <= 16 with M, N <= 8192) and per <= 64):

  (8192, 33, 3)      NC = 1, ragged K; eig-small: side output OFF.  8192 rows: every workgroup holds 32; 33 rows: one full
                     share, a last share of ONE row, 254 empty ones.  K = 3 meets 8192 rows.
  (8193, 40, 16)     K <= 16 with M > 8192: not eig-small, side output ON (KP = 32); 8193 rows: per = 64, 128 full shares, a
                     one-row share, empty ones; 40 rows: a ragged second share of 8.
  (33, 8193, 17)     K = 17 (KP = 32), ragged, meets 8193 rows; side output ON in both blocks.
  (8192, 31, 33)     NC = 2, ragged (KP = 64), meets 8192 rows; side output ON; 31 rows: a single ragged share.
  (8193, 16384, 64)  K = 64 (KP = 64), NC = 2 full; per = 64 in both blocks, 16384 rows fill every share; side output ON.
  (16385, 33, 63)    16385 rows: per = 96 (170 full shares, one of 65 rows): side output OFF for block A and ON for block S
                     in the same call; NC = 2 ragged, K = 63 meets 16385 rows.  With the default order S's partials are written
                     and never read (one iteration per call in a context fed by the caller's gradient, and a call forgets the
                     partials of the call before); the case with update_order = (1, 0) has them read by A's step rule.
  (8193, 1, 65)      K = 65: NC = 3, ragged, side output OFF; meets 8193 rows; a factor of ONE row.
  (31, 16384, 97)    NC = 4, ragged, meets 16384 rows.
  (257, 8191, 128)   NC = 4 full; 8191 rows: per = 32 and a last share of 31 rows.
  SUBSET             (33, 8193, 17), (8192, 31, 33), (257, 33, 128) and (33, 47, 3) carry the axes that are orthogonal to the row
                     mapping: n_g = 0 .. 4 in both blocks (n_g <= 3: the one-shot wave_sum16 reduction; n_g = 4: the two
                     block_sum_store calls, on NC = 1, 2 and 4), the operator menus, stages 1 - 3, update_order, e_abs, NaN,
                     the early stop.
"""
import functools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ULP = 2.0 ** -23

# Largest float32-oracle vs float64-oracle difference over ALL cases below after any iteration, in units of 2^-23 x natural
# scale (module docstring; reproduce with `python tests/test_gpu_bsdmm_step.py`), and the device's allowance: 4 x.
REF_ERR_BSDMM_X, REF_ERR_BSDMM_Z, REF_ERR_BSDMM_U, REF_ERR_BSDMM_NORM = 6.48, 6.14, 17.3, 3.13
TOL = {"X": 4 * REF_ERR_BSDMM_X, "Z": 4 * REF_ERR_BSDMM_Z, "U": 4 * REF_ERR_BSDMM_U, "NORM": 4 * REF_ERR_BSDMM_NORM}

HARD_GUARD = 1e-4            # no |argument| of a hard threshold within this (relative) of the threshold
BAND = (0.5, 2.0)            # no Boyd decision with lR / e_pri or lS / e_dual in here

SHAPES = [(8192, 33, 3), (8193, 40, 16), (33, 8193, 17), (8192, 31, 33), (8193, 16384, 64), (16385, 33, 63), (8193, 1, 65),
          (31, 16384, 97), (257, 8191, 128)]
SUBSET = [(33, 8193, 17), (8192, 31, 33), (257, 33, 128), (33, 47, 3)]
HARD_SHAPES = [(33, 47, 3), (31, 33, 65)]
# constraint counts (block A, block S) given to the shapes in turn: different counts in one call, 0 = `proxs_g[j] is None`
NG_PAIRS = [(0, 1), (2, 3), (4, 1), (3, 0), (1, 4), (2, 2), (3, 4), (1, 0), (4, 2)]

# Operator menus: prox_f of (A, S), then the members proxs_g[j] takes its first n_g from.  Thresholds are written for entries in
# 0.2 .. 1; prox_specs() scales them to the block's typical entry (1 / K of that where the block is normalised for `unity`) and
# divides a relative one by the nominal step its operator is handed (step_f, or step_g = 2 n_g step_f).
# `unity` runs along K, the short axis: axis 1 of A, axis 0 of S.
_MINMAX = ("seq", (("min", 0.3, "absolute"), ("max", 0.8, "absolute")), 1)
MENUS = {
    "mix": dict(f=(("plus",), ("unity_plus", 0)),
                g=([("soft", 0.03, "relative"), _MINMAX, ("plus",), ("soft_plus", 0.02, "absolute")],
                   [("plus",), ("unity", 0), ("soft", 1e-3, "absolute"), ("max", 0.9, "absolute")])),
    "none": dict(f=(None, ("soft", 0.02, "relative")),
                 g=([("max", 0.7, "absolute"), None, ("min", 0.25, "absolute"), ("soft_plus", 0.05, "relative")],
                    [("soft_plus", 0.02, "relative"), ("plus",), _MINMAX, None])),
    "ap": dict(f=(("seq", (("unity", 1), ("plus",)), 2), ("plus",)),
               g=([("unity_plus", 1), ("plus",), ("soft", 0.01, "absolute"), ("unity", 1)],
                  [("seq", (("unity", 0), ("plus",)), 2), ("soft_plus", 0.01, "relative"), ("plus",), ("unity_plus", 0)])),
    "hard": dict(f=(("hard", 0.12, "relative"), ("plus",)),
                 g=([("plus",), ("hard", 0.12, "absolute")], [("hard", 0.12, "relative"), ("hard", 0.12, "absolute")])),
    # the early stop: bounds that never bind, so that Z = X and U = 0 throughout and the run is at rest the moment the table's
    # entries vanish (after a constraint has bound, the duals relax by a factor ~2 per iteration, straight through BAND)
    "stop": dict(f=(("plus",), ("plus",)),
                 g=([("max", 1.05, "absolute"), ("plus",)], [("plus",), ("max", 1.05, "absolute")])),
}


# ---------------------------------------------------------------------------------------------------------------------
# the case list
# ---------------------------------------------------------------------------------------------------------------------
DEFAULTS = dict(route="fused", iters=5, n_g=(2, 3), menu="mix", host_f=False, mask=(0, 0), order=None, e_rel=1e-5, e_abs=0.0,
                table="full", shrink_from=3, step=(1e-4, 5e-5), push=0.1, nan=False, seed=7, stop_at=None)


def _mk(shape, **kw):
    c = dict(DEFAULTS, shape=tuple(shape), **kw)
    tag = [c["route"], "%dx%dx%d" % c["shape"]]
    for k in sorted(kw):
        if k in ("route", "stop_at", "shrink_from", "push"):
            continue
        v = kw[k]
        tag.append("%s=%s" % (k, "_".join(str(x) for x in v) if isinstance(v, (tuple, list)) else v))
    c["id"] = "-".join(tag)
    return c


def _cases():
    out = []
    for s, ng in zip(SHAPES, NG_PAIRS):                                     # the row mapping: the fused route on every shape
        out.append(_mk(s, n_g=ng, menu="mix"))
    # (a context fed by the caller's gradient runs one iteration per call, and a call forgets the partials of the call before: the
    #  partial Gram matrices that the LAST block of an iteration leaves are never read; S's are with S first)
    out.append(_mk((16385, 33, 63), n_g=(2, 2), order=(1, 0)))
    for s in SUBSET:
        for ng in ((0, 1), (4, 3), (3, 4), (1, 0)):                          # every count in both blocks, on both routes
            out.append(_mk(s, n_g=ng))
            out.append(_mk(s, route="split", n_g=ng))
        for menu in ("none", "ap"):
            out.append(_mk(s, menu=menu, n_g=(3, 2)))
            out.append(_mk(s, route="split", menu=menu, n_g=(2, 3)))
        for hf in (False, True):                                             # stages 1, 2, 3: hosted prox_f, hosted members
            for mask in ((0, 0), (0b01, 0b10), (0b10, 0b01), (0b101, 0b1111)):
                if not hf and mask == (0, 0):
                    continue                                                 # (that is route="split", n_g=(3, 4) above)
                out.append(_mk(s, route="split", n_g=(3, 4), host_f=hf, mask=mask))
        out.append(_mk(s, route="split", n_g=(4, 3), menu="none", host_f=True, mask=(0b1111, 0b101)))
        out.append(_mk(s, route="split", menu="none", n_g=(3, 1), mask=(0b100, 0b1)))   # the last member alone (its neighbour bit i ^ 1 names no member), an operator that binds
        for order in ((1, 0), (0,)):
            out.append(_mk(s, route="split", n_g=(2, 1), order=order))
            out.append(_mk(s, n_g=(1, 2), order=order))
        out.append(_mk(s, route="split", e_abs=3e-3))
        out.append(_mk(s, n_g=(0, 4), **(dict(e_abs=3e-4, e_rel=3e-5) if s == (33, 8193, 17) else dict(e_abs=3e-3))))
    for s in SUBSET[:2]:                                                     # both blocks converge at a known iteration
        for route in ("fused", "split"):
            out.append(_mk(s, route=route, menu="stop", n_g=(2, 2), table="shrink", e_rel=1e-3, e_abs=1e-3, iters=6, stop_at=4, push=0.02))
            out.append(_mk(s, route=route, menu="stop", n_g=(0, 1), table="shrink", e_rel=1e-3, e_abs=1e-3, iters=6, stop_at=4, push=0.02))
    out.append(_mk(SUBSET[0], route="split", nan=True))
    out.append(_mk(SUBSET[1], route="split", nan=True, n_g=(4, 1), mask=(0b1000, 0)))
    for s in HARD_SHAPES:
        out.append(_mk(s, route="split", menu="hard", n_g=(2, 2), push=0.002, seed=11))
        out.append(_mk(s, menu="hard", n_g=(2, 2), push=0.002, seed=11))
    return out


# e_rel of the cases in which the default would put a Boyd decision of the ORACLE inside BAND (test_reference_preconditions)
TUNED_E_REL = {
    "fused-8193x40x16-menu=mix-n_g=2_3": 1e-4, "fused-8192x31x33-menu=mix-n_g=3_0": 3e-5, "fused-16385x33x63-menu=mix-n_g=2_2": 3e-5,
    "fused-8193x1x65-menu=mix-n_g=3_4": 3e-5, "fused-8192x31x33-n_g=4_3": 3e-5, "fused-8192x31x33-n_g=1_0": 1e-4,
    "fused-8192x31x33-n_g=1_2-order=1_0": 3e-5, "fused-257x33x128-n_g=1_2-order=1_0": 3e-5, "fused-33x47x3-n_g=4_3": 3e-5,
    "fused-33x47x3-n_g=3_4": 1e-4, "fused-33x47x3-n_g=1_0": 3e-5, "fused-33x47x3-n_g=1_2-order=1_0": 1e-4,
    "fused-16385x33x63-n_g=2_2-order=1_0": 3e-5,
}
CASES = [dict(c, e_rel=TUNED_E_REL.get(c["id"], c["e_rel"])) for c in _cases()]
assert set(TUNED_E_REL) <= {c["id"] for c in CASES}
CASE_BY_ID = {c["id"]: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)
FUSED = [c for c in CASES if c["route"] == "fused"]
SPLIT = [c for c in CASES if c["route"] == "split"]


def blocks_of(c):
    return [0, 1] if c["order"] is None else list(c["order"])


def gram_per(rows):
    return 32 * ((rows + 8191) // 8192)


def side_output_blocks(c):
    """the blocks whose fused update leaves the partial Gram matrices of its rows behind (pmx_api.hip: bsdmm_enqueue_iteration)
    AND has them read: by the step rule of the other block, later in the same call (pmx_bsdmm_run forgets them at its start)"""
    M, N, K = c["shape"]
    if K > 64 or (K <= 16 and M <= 8192 and N <= 8192):
        return []
    b = blocks_of(c)
    return [j for o, j in enumerate(b) if gram_per((M, N)[j]) <= 64 and (1 - j) in b[o + 1:]]


# ---------------------------------------------------------------------------------------------------------------------
# inputs: seeded and fixed
# ---------------------------------------------------------------------------------------------------------------------
def _grad_block(rng, shape):
    """values in +-300, exact zeros, |g| ~ 1e-6, |g| ~ 1e3"""
    u = rng.random(shape)
    g = rng.uniform(-300.0, 300.0, shape)
    sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    mag = 0.5 + rng.random(shape)
    g = np.where(u < 0.25, sign * 1e3 * mag, g)
    g = np.where(u < 0.20, sign * 1e-6 * mag, g)
    g = np.where(u < 0.10, 0.0, g)
    return g


def _has_unity(spec):
    return spec is not None and ("unity" in spec[0] or spec[0] == "seq" and any("unity" in q[0] for q in spec[1]))


def menu_of(c):
    """(prox_f of the two blocks, proxs_g[j]: None or the first n_g[j] members of the menu), thresholds still in units of X"""
    m = MENUS[c["menu"]]
    return list(m["f"]), [None if c["n_g"][j] == 0 else list(m["g"][j][:c["n_g"][j]]) for j in range(2)]


@functools.lru_cache(maxsize=2)
def _inputs(cid):
    from oracle import nmf_oracle as orc
    c = CASE_BY_ID[cid]
    M, N, K = c["shape"]
    rng = np.random.default_rng(c["seed"])
    if c["menu"] == "hard":      # nothing between 0.02 and 0.8: the threshold 0.12 sits in the gap
        def draw(shape):
            return np.where(rng.random(shape) < 0.5, 0.01 + 0.01 * rng.random(shape), 0.8 + 0.2 * rng.random(shape)).astype(np.float32)
    else:
        def draw(shape):
            return (0.2 + 0.8 * rng.random(shape)).astype(np.float32)
    A0, S0 = draw((M, K)), draw((K, N))
    f, g = menu_of(c)
    if any(_has_unity(q) for q in [f[0]] + (g[0] or [])):
        A0 = (A0 / A0.sum(1, keepdims=True)).astype(np.float32)
    if any(_has_unity(q) for q in [f[1]] + (g[1] or [])):
        S0 = (S0 / S0.sum(0, keepdims=True)).astype(np.float32)
    # the nominal steps: the split route's own, the Lipschitz rule at the start for the fused route; the table is scaled so
    # that its large entries push an entry by ~ push x its typical size per iteration
    nominal = tuple(c["step"]) if c["route"] == "split" else tuple(float(s) for s in orc.lipschitz_steps(A0.astype(np.float64), S0.astype(np.float64)))
    typ = (float(np.mean(A0)), float(np.mean(S0)))
    trng = np.random.default_rng(1000 + c["seed"])
    base = [(_grad_block(trng, (M, K)), _grad_block(trng, (K, N))) for _ in range(2)]
    sgn = [np.where(trng.random(s) < 0.5, -1.0, 1.0) for s in ((M, K), (K, N))]
    table = []
    for it in range(c["iters"]):
        G = []
        for j in range(2):
            B = np.abs(np.roll(base[it % 2][j], 13 * it, axis=j)) * sgn[j] * (c["push"] * typ[j] / (1e3 * nominal[j]))
            if c["table"] == "shrink" and it >= c["shrink_from"]:          # later entries vanish: the Boyd test fires at a known iteration
                B = B * 1e-6 ** (it - c["shrink_from"] + 1)
            if K >= 2:                                                     # one component that is zero in every iteration
                if j == 0:
                    B[:, K // 2] = 0
                else:
                    B[K // 2, :] = 0
            G.append(np.ascontiguousarray(B, dtype=np.float32))
        table.append(tuple(G))
    if c["nan"]:
        table[1][0][M // 2, K - 1] = np.nan
    # (the menus' thresholds are written for entries in 0.2 .. 1, mean 0.6: a block normalised for `unity` is 1 / K of that)
    return dict(A0=A0, S0=S0, table=table, nominal=nominal, size=(typ[0] / 0.6, typ[1] / 0.6))


def make_inputs(c):
    return _inputs(c["id"])


def prox_specs(c):
    """the oracle's specs of a case: relative thresholds divided by the nominal step their operator is handed"""
    inp = make_inputs(c)
    nominal, size = inp["nominal"], inp["size"]
    f, g = menu_of(c)

    def conv(q, step, j):
        if q is None:
            return None
        if q[0] == "seq":
            return ("seq", tuple(conv(r, step, j) for r in q[1]), q[2])
        if len(q) > 2:
            t = q[1] * size[j]
            return (q[0], float(np.float32(t / step if q[2] == "relative" else t)), q[2])
        return q
    return ([conv(f[j], nominal[j], j) for j in range(2)],
            [None if g[j] is None else [conv(q, nominal[j] * 2 * len(g[j]), j) for q in g[j]] for j in range(2)])


def split_step(c, it, j):
    """the split route's step of block j in iteration `it`: another value in every iteration, a float32 number"""
    return float(np.float32(c["step"][j] * (1 + 0.25 * it)))


# ---------------------------------------------------------------------------------------------------------------------
# the reference: one oracle run that visits the state after every iteration
# ---------------------------------------------------------------------------------------------------------------------
def _members(ZU, j):
    """Z or U of block j as a list (the oracle keeps a bare array for a block without constraints)"""
    return ZU[j] if isinstance(ZU[j], list) else []


def run_reference(c, dtype=np.float64, steps=None, visit=None, keep=False):
    """bsdmm_nmf on the case's inputs.  steps: [(sA, sS)] per iteration (fused route: the device's, or another run's); None:
    the split route's own, or the Lipschitz rule at the run's own factors, evaluated in float64 and rounded to float32.
    visit(it, st) sees the state after iteration `it`: the live A, S, Z, U, the per-block natural scale of that update, the
    block records of the oracle's log.  keep: also return float copies of every such state."""
    from oracle import nmf_oracle as orc
    inp = make_inputs(c)
    M, N, K = c["shape"]
    A, S = inp["A0"].astype(dtype), inp["S0"].astype(dtype)
    X = [A, S]
    spec_f, spec_g = prox_specs(c)
    unity = [any(_has_unity(q) for q in [spec_f[j]] + (spec_g[j] or [])) for j in range(2)]
    cur = {"it": 0}
    used, log, state, snaps = [], [], {}, []
    hard = {"margin": np.inf}
    apply_prox = orc.apply_prox

    def probed(Xa, step, spec):
        if spec is not None and spec[0] in ("hard", "hard_plus"):
            t = orc._threshold(step, spec[1], spec[2] if len(spec) > 2 else "relative")
            with np.errstate(invalid="ignore", divide="ignore"):
                m = np.nanmin(np.abs(np.abs(Xa) - t) / t) if np.isfinite(Xa).any() else np.inf
            hard["margin"] = min(hard["margin"], float(m))
        return apply_prox(Xa, step, spec)

    def grad(A_, S_):
        GA, GS = inp["table"][cur["it"]]
        return GA.astype(dtype), GS.astype(dtype)

    def step(it, j):
        while len(used) <= it:
            used.append([None, None])
        if steps is not None:
            s = float(steps[it][j])
        elif c["route"] == "split":
            s = split_step(c, it, j)
        else:
            with np.errstate(invalid="ignore", divide="ignore"):
                s = float(np.float32(orc.lipschitz_steps(A.astype(np.float64), S.astype(np.float64))[j]))
        used[it][j] = s
        return s

    prev, acc = {}, [None, None]

    def remember():
        prev["X"] = [x.copy() for x in X]
        prev["Z"] = [[z.copy() for z in _members(state["Z"], j)] for j in range(2)]
        prev["U"] = [[u.copy() for u in _members(state["U"], j)] for j in range(2)]

    def finish(it):
        """the state after iteration `it` (prev: before it)"""
        scale = []
        for j in range(2):
            sc = np.fmax(np.abs(prev["X"][j]), np.abs(X[j])).astype(np.float64)
            if used[it][j] is not None:
                with np.errstate(invalid="ignore"):
                    sc = np.fmax(sc, np.abs(used[it][j] * inp["table"][it][j].astype(np.float64)))
            for old, new in ((prev["Z"][j], _members(state["Z"], j)), (prev["U"][j], _members(state["U"], j))):
                for a, b in zip(old, new):
                    sc = np.fmax(sc, np.fmax(np.abs(a), np.abs(b)))
            sc = acc[j] = sc if acc[j] is None else np.fmax(acc[j], sc)      # (an error made at a large scale stays in the entry)
            if unity[j]:
                sc = np.broadcast_to(np.nanmax(sc, axis=1 - j, keepdims=True), sc.shape)
            scale.append(sc)
        st = dict(A=A, S=S, Z=[_members(state["Z"], j) for j in range(2)], U=[_members(state["U"], j) for j in range(2)], scale=scale,
                  blocks={r[2]: r for r in log if r[0] == "b" and r[1] == it})
        if keep:
            snaps.append(dict(A=A.copy(), S=S.copy(), Z=[[z.copy() for z in zs] for zs in st["Z"]], U=[[u.copy() for u in us] for us in st["U"]],
                              blocks=st["blocks"]))
        if not c["nan"]:
            assert np.isfinite(A).all() and np.isfinite(S).all(), "iteration %d of a case without NaN leaves non-finite entries" % it
        if visit is not None:
            visit(it, st)

    def callback(A_, S_, it):
        if it > 0:
            finish(it - 1)
        cur["it"] = it
        remember()

    orc.apply_prox = probed
    try:
        conv, n_it = orc.bsdmm_nmf(None, A, S, spec_f[0], spec_f[1], proxs_g=spec_g, max_iter=c["iters"], e_rel=c["e_rel"], e_abs=c["e_abs"],
                                   callback=callback, state=state, grad=grad, step=step, update_order=c["order"], log=log)
    finally:
        orc.apply_prox = apply_prox
    finish(n_it - 1)
    return dict(conv=list(conv), n_iter=int(n_it), steps=used, log=log, hard_margin=hard["margin"], snaps=snaps, dtype=dtype)


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


def compare_state(c, got, st, worst, what="", check_nan=False):
    """one iteration's state `got` (dict A, S, Z, U, norms = {j: (d2, x2)}) against the reference's `st`: the worst units per
    quantity into `worst`; check_nan: NaNs where the reference has them and nowhere else"""
    def one(key, name, g, w, sc):
        if check_nan:
            np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg="%s: NaN pattern of %s" % (what, name))
        u = units(g, w, sc)
        if u > worst.get(key, (-1.0, None))[0]:
            worst[key] = (u, "%s %s" % (what, name))
    for j, name in enumerate("AS"):
        one("X", name, got[name], st[name], st["scale"][j])
        assert len(got["Z"][j]) == len(st["Z"][j]) == len(got["U"][j]) == len(st["U"][j])
        for i in range(len(st["Z"][j])):
            one("Z", "Z[%s][%d]" % (name, i), got["Z"][j][i], st["Z"][j][i], st["scale"][j])
            one("U", "U[%s][%d]" % (name, i), got["U"][j][i], st["U"][j][i], st["scale"][j])
        if j in st["blocks"] and j in got["norms"]:
            _, _, _, d2, x2, _ = st["blocks"][j]
            d2, x2 = float(d2), float(x2)
            with np.errstate(invalid="ignore"):
                s2 = float(np.sum(st["scale"][j][np.isfinite(st["scale"][j])] ** 2))
            one("NORM", "d2[%s]" % name, got["norms"][j][0], d2, np.sqrt(d2 * s2) if np.isfinite(d2) else 1.0)
            one("NORM", "x2[%s]" % name, got["norms"][j][1], x2, x2 if np.isfinite(x2) else 1.0)
            if check_nan:
                assert np.isnan(got["norms"][j][0]) == np.isnan(d2) and np.isnan(got["norms"][j][1]) == np.isnan(x2), (what, got["norms"][j], d2, x2)


def decision_ratios(log):
    """(it, j, i, which, ratio) of every Boyd decision; a 0 / 0 (nothing moved, nothing demanded) is left out: it is met exactly"""
    out = []
    for r in log:
        if r[0] != "g":
            continue
        _, it, j, i, lR, lS, e_pri, e_dual = r
        for which, l, e in (("pri", lR, e_pri), ("dual", lS, e_dual)):
            if l == 0 and e == 0:
                continue
            out.append((it, j, i, which, np.inf if e == 0 else l / e))
    return out


def assert_decisions_outside_band(log, what):
    n_nan = 0
    for it, j, i, which, q in decision_ratios(log):
        if np.isnan(q):
            n_nan += 1            # NaN <= x is False on the device as well
            continue
        assert not (BAND[0] <= q <= BAND[1]), "%s: Boyd decision (it %d, block %d, constraint %d, %s) with ratio %g" % (what, it, j, i, which, q)
    return n_nan


def measure_case(c):
    """float32 oracle against float64 oracle on the very inputs and steps of the case -> (worst units per quantity, r32, r64)"""
    r32 = run_reference(c, np.float32, keep=True)
    worst = {}

    def visit(it, st):
        if it < len(r32["snaps"]):
            s = r32["snaps"][it]
            compare_state(c, dict(s, norms={j: (float(b[3]), float(b[4])) for j, b in s["blocks"].items()}), st, worst, "it %d" % it)
    r64 = run_reference(c, np.float64, steps=r32["steps"], visit=visit)
    return worst, r32, r64


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the conditions under which "every entry, equal decisions" is a fair demand, and the table behind REF_ERR_BSDMM_*
# ---------------------------------------------------------------------------------------------------------------------
REF_ERR = {"X": REF_ERR_BSDMM_X, "Z": REF_ERR_BSDMM_Z, "U": REF_ERR_BSDMM_U, "NORM": REF_ERR_BSDMM_NORM}


@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_reference_preconditions(cid):
    """On the oracle alone, in both precisions: the guard band of the hard thresholds, the margin of every Boyd decision, the
    float32 / float64 table within the recorded REF_ERR_BSDMM_*, and that each case exercises what it is there for."""
    c = CASE_BY_ID[cid]
    worst, r32, r64 = measure_case(c)
    for key, (u, where) in worst.items():
        assert u <= REF_ERR[key], "%s: the float32 oracle is %.4g units off at %s, recorded REF_ERR_BSDMM_%s = %.4g" % (cid, u, where, key, REF_ERR[key])
    assert r32["conv"] == r64["conv"] and r32["n_iter"] == r64["n_iter"], (r32["conv"], r64["conv"], r32["n_iter"], r64["n_iter"])
    n_nan = 0
    for r in (r32, r64):
        n_nan += assert_decisions_outside_band(r["log"], str(r["dtype"]))
        if c["menu"] == "hard":
            assert r["hard_margin"] < np.inf, "the hard threshold never ran"
            assert r["hard_margin"] >= HARD_GUARD, "an argument of the hard threshold lies within %g of it" % r["hard_margin"]
    assert (n_nan > 0) == bool(c["nan"])
    assert decision_ratios(r64["log"]), "no Boyd decision was probed"
    if c["stop_at"] is not None:
        assert r64["n_iter"] == c["stop_at"] < c["iters"] and all(r64["conv"]), (r64["n_iter"], r64["conv"])
    else:
        assert r64["n_iter"] == c["iters"]
    if c["nan"]:
        assert r64["conv"][0] is False
    M, N, K = c["shape"]
    assert all((ga[:, K // 2] == 0).all() and (gs[K // 2] == 0).all() for ga, gs in make_inputs(c)["table"]) or K < 2


def test_case_list_reaches_every_branch():
    """the properties the module docstring lists, on the case list itself"""
    fused = {c["shape"] for c in FUSED}
    assert set(SHAPES) <= fused
    rows = {r for s in SHAPES for r in s[:2]}
    assert {1, 31, 33, 8191, 8192, 8193, 16384, 16385} <= rows
    assert {3, 17, 33, 63, 64, 65, 97, 128} <= {s[2] for s in SHAPES}
    for K in {s[2] for s in SHAPES if s[2] % 32}:
        assert any(max(s[:2]) >= 8192 for s in SHAPES if s[2] == K), K
    on = {(c["shape"], j) for c in FUSED for j in side_output_blocks(c)}
    assert ((8193, 40, 16), 0) in on and ((33, 8193, 17), 0) in on and ((33, 8193, 17), 1) in on and ((8193, 16384, 64), 0) in on
    assert ((8192, 31, 33), 0) in on and ((8192, 31, 33), 1) in on and ((16385, 33, 63), 1) in on
    assert not any(s in ((8192, 33, 3), (8193, 1, 65)) for s, _ in on) and ((16385, 33, 63), 0) not in on
    for route in (FUSED, SPLIT):
        assert {n for c in route for n in c["n_g"]} == {0, 1, 2, 3, 4}
        assert any(c["stop_at"] is not None for c in route)
        assert any(c["n_g"][j] == 4 and c["shape"][2] == 128 for c in route for j in range(2))
        assert {None, (1, 0), (0,)} <= {c["order"] for c in route}
    assert {(c["host_f"], c["mask"]) for c in SPLIT} >= {(hf, m) for hf in (False, True) for m in ((0, 0), (0b01, 0b10), (0b101, 0b1111))}
    assert any(c["nan"] for c in SPLIT) and any(c["e_abs"] > 0 for c in SPLIT) and any(c["e_abs"] > 0 for c in FUSED)


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
    from functools import partial
    ops = pm.operators
    if spec is None:
        return ops.prox_id
    if spec[0] == "seq":
        return ops.AlternatingProjections([spec_to_prox(pm, q) for q in spec[1]], repeat=spec[2])
    fn = getattr(ops, "prox_" + spec[0])
    if spec[0] in ("unity", "unity_plus"):
        return partial(fn, axis=spec[1])
    if len(spec) > 1:
        return partial(fn, thresh=spec[1], type=spec[2])
    return fn


def run_device(pm, c):
    """the case on the device -> the state after every iteration, the steps of every iteration, `converged`, the iteration count"""
    from oracle import nmf_oracle as orc
    from proxmin_amd import _lib
    from proxmin_amd.engine import DeviceNMF
    ops = pm.operators
    inp = make_inputs(c)
    M, N, K = c["shape"]
    spec_f, spec_g = prox_specs(c)
    split = c["route"] == "split"
    n_g = c["n_g"]
    mask = [c["mask"][j] if split else 0 for j in range(2)]
    assert all(mask[j] >> n_g[j] == 0 for j in range(2))
    blocks = blocks_of(c)
    seq_f = [ops.device_proxseq(ops.prox_id if (split and c["host_f"]) else spec_to_prox(pm, spec_f[j]), j, for_solver=True) for j in range(2)]
    seq_g = [None if spec_g[j] is None else
             [ops.device_proxseq(ops.prox_id if (mask[j] >> i) & 1 else spec_to_prox(pm, q), j, for_solver=True) for i, q in enumerate(spec_g[j])]
             for j in range(2)]
    snaps, steps = [], []
    f32 = np.float32

    def member(base, j, i):
        out = dev._download(base + j * _lib.MAX_G + i, (M, N)[j])
        return out if j == 0 else out.T

    with DeviceNMF(M, N, K, mode="f32") as dev:
        dev.set_host_grad(True)
        dev.set_factors(inp["A0"], inp["S0"])
        dev.bsdmm_begin(seq_f, seq_g, e_rel=(c["e_rel"],) * 2, e_abs=(c["e_abs"],) * 2, update_order=None if split else c["order"])
        res = None
        for it in range(c["iters"]):
            for j in range(2):
                dev.put(_lib.BUF_GA, j, inp["table"][it][j])
            norms = {}
            if not split:
                res = dev.bsdmm_run(1)
                steps.append([float(f32(res.steps[j])) if j in blocks else None for j in range(2)])
                nr = dev.iter_norms()
                norms = {j: nr[j] for j in blocks}
            else:
                steps.append([None, None])
                for o, j in enumerate(blocks):
                    sf = split_step(c, it, j)
                    steps[-1][j] = sf
                    r0 = dev.bsdmm_split(j, 0, c["host_f"], mask[j], step_f=sf)
                    assert float(r0.steps[j]) == sf
                    if c["host_f"]:           # the argument of prox_f as the device formed it; its result goes back
                        T = np.ascontiguousarray(dev.get(_lib.BUF_TMP_A, j), dtype=f32)
                        dev.put(_lib.BUF_TMP_A, j, orc.apply_prox(T, f32(sf), spec_f[j]))
                    dev.bsdmm_split(j, 1, c["host_f"], mask[j])
                    if mask[j]:
                        sg = f32(f32(sf) * f32(2.0) * f32(n_g[j]))              # get_step_g as the kernel forms it
                        for i in range(n_g[j]):
                            if (mask[j] >> i) & 1:
                                buf = _lib.BUF_TG0 + j * _lib.MAX_G + i
                                T = dev._download(buf, (M, N)[j])
                                T = np.ascontiguousarray(T if j == 0 else T.T, dtype=f32)
                                out = orc.apply_prox(T, sg, spec_g[j][i])
                                dev._upload(buf, out if j == 0 else out.T)
                    res = dev.bsdmm_split(j, 2, c["host_f"], mask[j], last_block=(o == len(blocks) - 1))
                    norms[j] = dev.iter_norms()[j]
            A, S = dev.get_factors()
            snaps.append(dict(A=A, S=S, Z=[[member(_lib.BUF_Z0, j, i) for i in range(n_g[j])] for j in range(2)],
                              U=[[member(_lib.BUF_U0, j, i) for i in range(n_g[j])] for j in range(2)], norms=norms))
            assert res.total_iterations == it + 1
            if res.stopped:
                break
        conv = [bool(res.converged[j]) if j in blocks else None for j in range(2)]
    return dict(snaps=snaps, steps=steps, conv=conv, n_iter=int(res.total_iterations), stopped=bool(res.stopped))


def assert_meets_reference(c, run):
    """the device's state after every iteration against the fp64 oracle run with the device's own steps"""
    worst = {}

    def visit(it, st):
        assert it < len(run["snaps"]), "the oracle goes on after iteration %d, the device stopped" % it
        compare_state(c, run["snaps"][it], st, worst, "it %d" % it, check_nan=True)
    ref = run_reference(c, np.float64, steps=run["steps"], visit=visit)
    n_nan = assert_decisions_outside_band(ref["log"], "with the device's steps")
    assert (n_nan > 0) == bool(c["nan"])
    print("%s: %s" % (c["id"], ", ".join("%s %.3g (%s)" % (k, worst[k][0], worst[k][1]) for k in sorted(worst))))
    assert run["conv"] == ref["conv"], (run["conv"], ref["conv"])
    assert run["n_iter"] == ref["n_iter"] == len(run["snaps"]), (run["n_iter"], ref["n_iter"], len(run["snaps"]))
    assert run["stopped"] == all(ref["conv"])
    if c["stop_at"] is not None:
        assert run["n_iter"] == c["stop_at"]
    if not c["nan"]:
        assert all(np.isfinite(s[k]).all() for s in run["snaps"] for k in "AS")
    for key, (u, where) in sorted(worst.items()):
        assert u <= TOL[key], "%s differs from the fp64 oracle by %.4g x 2^-23 x scale at %s (allowed: %.4g)" % (key, u, where, TOL[key])
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c["id"] for c in SPLIT])
def test_bsdmm_split_update_matches_the_oracle_on_every_entry(pm, cid):
    """stages 1, 2 and 3 of k_bsdmm_update and k_bsdmm_decide with steps chosen here: X, Z_i, U_i on every entry after every
    iteration, the two sums of every block, `converged`, the iteration count."""
    c = CASE_BY_ID[cid]
    run = run_device(pm, c)
    ref = assert_meets_reference(c, run)
    for it, st in enumerate(run["steps"]):
        assert st == ref["steps"][it]


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c["id"] for c in FUSED])
def test_bsdmm_fused_update_matches_the_oracle_on_every_entry(pm, monkeypatch, cid):
    """stage 0 (bsdmm_run, one iteration per call) with the device's own steps handed to the oracle; where a block leaves its
    partial Gram matrices behind, a second context with PMX_GRAM_IN_UPDATE=0 (k_gram_partial forms them) must produce the same
    steps and the same X, Z, U bit for bit."""
    c = CASE_BY_ID[cid]
    monkeypatch.delenv("PMX_GRAM_IN_UPDATE", raising=False)
    run = run_device(pm, c)
    assert_meets_reference(c, run)
    if not side_output_blocks(c):
        return
    monkeypatch.setenv("PMX_GRAM_IN_UPDATE", "0")
    off = run_device(pm, c)
    assert off["steps"] == run["steps"], "the steps differ between the update kernel's partial Gram matrices and k_gram_partial's"
    assert off["conv"] == run["conv"] and off["n_iter"] == run["n_iter"]
    for it, (a, b) in enumerate(zip(run["snaps"], off["snaps"])):
        for k in "AS":
            np.testing.assert_array_equal(a[k], b[k], err_msg="it %d: %s" % (it, k))
        for k in "ZU":
            for j in range(2):
                for x, y in zip(a[k][j], b[k][j]):
                    np.testing.assert_array_equal(x, y, err_msg="it %d: %s of block %d" % (it, k, j))
        assert a["norms"] == b["norms"]


# ---------------------------------------------------------------------------------------------------------------------
# how REF_ERR_BSDMM_* were obtained: python tests/test_gpu_bsdmm_step.py [pattern]  (CPU only)
# ---------------------------------------------------------------------------------------------------------------------
def measure(cases=CASES, verbose=True):
    total = {}
    for c in cases:
        worst, r32, r64 = measure_case(c)
        if verbose:
            qs = [q for r in (r32, r64) for *_, q in decision_ratios(r["log"]) if np.isfinite(q) and q > 0]
            near = min(qs, key=lambda x: abs(np.log(x))) if qs else None
            same = r32["conv"] == r64["conv"] and r32["n_iter"] == r64["n_iter"]
            print("%-64s %s%s n_iter %d conv %s nearest ratio %s hard %.3g | %s" % (
                c["id"], "" if same else "DECISIONS DIFFER ", "" if near is None or not BAND[0] <= near <= BAND[1] else "IN BAND ", r64["n_iter"], r64["conv"],
                "%.3g" % near if near is not None else None, r64["hard_margin"], " ".join("%s %.3g" % (k, worst[k][0]) for k in sorted(worst))), flush=True)
        for k, (u, where) in worst.items():
            if u > total.get(k, (0, None))[0]:
                total[k] = (u, c["id"] + " " + where)
    for k in sorted(total):
        print("REF_ERR_BSDMM_%s = %.4g   (%s)" % (k, total[k][0], total[k][1]))
    return total


if __name__ == "__main__":
    pat = sys.argv[1] if len(sys.argv) > 1 else ""
    measure([c for c in CASES if re.search(pat, c["id"])])
