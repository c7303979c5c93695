"""GPU: per-component operator parameters (PMX_PROX_COMPONENTS, op 12): an array `thresh` / `gamma` on the threshold operators and
prox_components, fused in every update kernel in fp32 and fp64.

1. A table whose rows are equal is the scalar operator, bit for bit: stand-alone, through pgm / adaprox / bsdmm (3 iterations),
   fp32 and fp64, host factors and torch tensors in HBM.
2. Column k of a result with K distinct rows is, bit for bit, column k of the scalar call with row k's operator and threshold:
   stand-alone (also with a per-component step) and through one pgm iteration fed by a gradient table with constant steps.
3. fp32 kernels against the fp64 oracle on every entry, with the single-step construction and the tolerances of
   tests/test_gpu_update_step.py (whose REF_ERR_* the float32 oracle is first shown to respect on these new cases).
4. fp64 kernels against the fp64 oracle with the shapes and `_close` of tests/test_gpu_f64_operators.py.
5. What the real reference can compute -- array thresholds on soft, soft_plus, hard, hard_plus, stand-alone and as nmf() finals after 8
   iterations -- from the fixtures of tests/golden/make_components_golden.py (README_components.md).

K = 2, 33, 65, 127 select the NC = 1, 2, 4, 4 values per lane with a ragged last group of 32; 31 / 33 rows and 8191 / 8193 rows sit
around one sweep of the element-wise grid (tests/test_gpu_update_step.py: SUBSET)."""
import contextlib
import functools
from functools import partial

import numpy as np
import pytest

import test_gpu_update_step as tus
import test_gpu_f64_operators as tgo

SHAPES = [(31, 33, 2), (8193, 33, 33), (33, 8191, 65), (8191, 31, 127)]
THRESH_OPS = ("min", "max", "hard", "hard_plus", "soft", "soft_plus", "max_entropy")
KINDS = ("relative", "absolute")


@pytest.fixture(scope="module")
def pm():
    import __graft_entry__ as g
    g.build()
    import proxmin_amd
    return proxmin_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import nmf_oracle
    return nmf_oracle


def _op(pm, name, value, kind):
    fn = getattr(pm.operators, "prox_" + name)
    return partial(fn, type=kind, **{"gamma" if name == "max_entropy" else "thresh": value})


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b, what):
    assert a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b)), what


def _per_k(values, block):
    """K values in the shape that broadcasts along block's components: (K,) for A (M x K), (K, 1) for S (K x N)"""
    v = np.asarray(values, dtype=np.float64)
    return v if block == 0 else v.reshape(-1, 1)


def _data(shape, seed):
    """entries of both signs around the thresholds used below (0.3 in data units), some exactly zero"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.5, shape).astype(np.float32)
    X[rng.random(shape) < 0.02] = 0.0
    return X


# a mixed list: every element-wise operator, both types
def _mixed(pm, K, scale=1.0):
    """-> (members, distinct): K callables drawn cyclically from ten distinct ones; scale: what a relative threshold is divided by
    (the step the solver hands over) so that threshold x step stays in data units"""
    ops = pm.operators
    distinct = [_op(pm, "soft", 0.3 / scale, "relative"), ops.prox_plus, _op(pm, "hard", 0.4, "absolute"), ops.prox_id,
                _op(pm, "max_entropy", 0.2 / scale, "relative"), _op(pm, "min", 0.1, "absolute"), _op(pm, "max", 0.5 / scale, "relative"),
                ops.prox_zero, _op(pm, "soft_plus", 0.2, "absolute"), _op(pm, "hard_plus", 0.3 / scale, "relative")]
    return [distinct[k % len(distinct)] for k in range(K)], distinct


# ---------------------------------------------------------------------------------------------------------------------
# 1. equal rows are the scalar operator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_standalone_equal_rows_equal_the_scalar_operator(pm, M, N, K):
    ops = pm.operators
    for block, shape in ((0, (M, K)), (1, (K, N))):
        X0 = _data(shape, 3 + block)
        step_k = _per_k(np.linspace(0.5, 2.0, K), block)
        for name in THRESH_OPS:
            for kind in KINDS:
                for step in (0.7, step_k):
                    want = _op(pm, name, 0.3, kind)(X0.copy(), step)
                    X = X0.copy()
                    got = _op(pm, name, _per_k(np.full(K, 0.3), block), kind)(X, step)
                    assert got is X
                    _same(got, want, "%s %s block %d array" % (name, kind, block))
                    got = ops.prox_components(X0.copy(), step, prox=[_op(pm, name, 0.3, kind)] * K, axis=1 - block)
                    _same(got, want, "%s %s block %d components" % (name, kind, block))
        for p in (ops.prox_plus, ops.prox_zero, ops.prox_id):
            _same(ops.prox_components(X0.copy(), 0.7, prox=[p] * K, axis=1 - block), p(X0.copy(), 0.7), "components of %r" % (p,))
        if block == 0:                              # (1, K) on A is (K,)
            _same(ops.prox_soft(X0.copy(), 0.7, thresh=np.full((1, K), 0.3)), ops.prox_soft(X0.copy(), 0.7, thresh=0.3), "(1, K)")


def test_shapes_that_are_not_per_component_raise_on_a_direct_call():
    """(no device is reached: the shape is refused first)"""
    from proxmin_amd import operators as ops
    X = np.ones((5, 3), np.float32)
    for shape in ((5, 3), (2,), (1, 5), (3, 1), (1, 5, 3)):
        with pytest.raises(NotImplementedError) as info:
            ops.prox_soft(X.copy(), 1.0, thresh=np.ones(shape))
        assert str(shape) in str(info.value)


def _solver_kw(pm, orc, algorithm, Y, A0, S0, name, kind):
    """-> (kwargs without the operator, block the operator sits on, the scalar threshold): 0.3 in data units"""
    steps0 = orc.lipschitz_steps(A0.astype(np.float64), S0.astype(np.float64))
    if algorithm == "adaprox":
        g0 = float(np.mean(orc.adaprox_steps(A0, S0)[1])) / (np.sqrt(1e-3) * np.abs(orc.residual_gradients(A0.astype(np.float64), S0.astype(np.float64), Y.astype(np.float64))[1]).max())
        return dict(algorithm=pm.adaprox, scheme="amsgrad", max_iter=3, e_rel=1e-9, prox_max_iter=4), 1, 0.3 / g0 if kind == "relative" else 0.3
    if algorithm == "pgm":
        return dict(max_iter=3, e_rel=1e-9), 1, 0.3 / steps0[1] if kind == "relative" else 0.3
    if algorithm == "fista_A":
        return dict(max_iter=3, e_rel=1e-9, accelerated=True), 0, 0.3 / steps0[0] if kind == "relative" else 0.3
    if algorithm == "bsdmm_prox":
        return dict(algorithm=pm.bsdmm, max_iter=3, e_rel=1e-9), 1, 0.3 / steps0[1] if kind == "relative" else 0.3
    return dict(algorithm=pm.bsdmm, max_iter=3, e_rel=1e-9), "g0", 0.3 / (2 * steps0[0]) if kind == "relative" else 0.3


def _run_nmf(pm, Y, A0, S0, kw, where, prox, resident=False):
    kw = dict(kw)
    if where == "g0":
        kw["proxs_g"] = [[prox], None]
    elif where == 0:
        kw["prox_A"] = prox
    else:
        kw["prox_S"] = prox
    if resident:
        import torch
        A, S = torch.from_numpy(A0.copy()).cuda(), torch.from_numpy(S0.copy()).cuda()
        pm.nmf.nmf(Y, A, S, **kw)
        return A.cpu().numpy(), S.cpu().numpy()
    A, S = A0.copy(), S0.copy()
    pm.nmf.nmf(Y, A, S, **kw)
    return A, S


SOLVER_SHAPES = [(np.float32, s) for s in SHAPES] + [(np.float64, s) for s in ((33, 47, 3), (40, 56, 12), (48, 72, 40), (128, 160, 100))]


@pytest.mark.gpu
@pytest.mark.parametrize("name", THRESH_OPS)
@pytest.mark.parametrize("algorithm", ["pgm", "fista_A", "adaprox", "bsdmm_prox", "bsdmm_g"])
@pytest.mark.parametrize("dtype,shape", SOLVER_SHAPES, ids=lambda v: v.__name__ if isinstance(v, type) else "x".join(map(str, v)))
def test_solvers_equal_rows_equal_the_scalar_operator(pm, orc, caplog, algorithm, dtype, shape, name):
    """3 iterations with thresh = full(K, t), with prox_components([p] * K) and with the scalar p: the same bits in A and S, with host
    factors and with torch tensors of the problem's dtype in HBM, both forms; nothing of it on the host route"""
    import logging
    M, N, K = shape
    Y, A0, S0 = orc.synthetic_problem(M, N, K, dtype, seed=M + N + K)
    for kind in KINDS:
        kw, where, t = _solver_kw(pm, orc, algorithm, Y, A0, S0, name, kind)
        block = 0 if where == "g0" else where
        want = _run_nmf(pm, Y, A0, S0, kw, where, _op(pm, name, t, kind))
        array = _op(pm, name, _per_k(np.full(K, t), block), kind)
        components = partial(pm.operators.prox_components, prox=[_op(pm, name, t, kind)] * K, axis=1 - block)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="proxmin"):
            runs = {"array": _run_nmf(pm, Y, A0, S0, kw, where, array),
                    "components": _run_nmf(pm, Y, A0, S0, kw, where, components),
                    "array, device-resident": _run_nmf(pm, Y, A0, S0, kw, where, array, resident=True),
                    "components, device-resident": _run_nmf(pm, Y, A0, S0, kw, where, components, resident=True)}
        text = " | ".join(r.getMessage() for r in caplog.records)
        assert "one iteration per call" not in text and "user-defined Python callable" not in text, text
        assert not (dtype == np.float64 and "computed in float32" in text), text            # the fp64 kernels ran
        for form, got in runs.items():
            for j in range(2):
                assert got[j].dtype == dtype
                _same(got[j], want[j], "%s %s %s %s, block %d" % (algorithm, name, kind, form, j))


# ---------------------------------------------------------------------------------------------------------------------
# 2. column by column
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_standalone_column_by_column(pm, M, N, K):
    """K distinct thresholds, then a mixed prox_components: component k of the result is the scalar operator of row k on component k
    alone (a rows x 1 array: the operators are element-wise), with a scalar and with a per-component step"""
    ops = pm.operators
    for block, shape in ((0, (M, K)), (1, (K, N))):
        X0 = _data(shape, 11 + block)
        col = (lambda X, k: X[:, k:k + 1]) if block == 0 else (lambda X, k: X[k:k + 1, :])
        ts = np.linspace(0.05, 0.9, K)
        step_k = np.linspace(0.5, 2.0, K)
        members, _ = _mixed(pm, K)
        for step in (0.7, _per_k(step_k, block)):
            sk = (lambda k: 0.7) if np.ndim(step) == 0 else (lambda k: float(step_k[k]))
            for name in THRESH_OPS:
                kind = "relative" if name in ("soft", "min", "hard_plus", "max_entropy") else "absolute"
                got = _op(pm, name, _per_k(ts, block), kind)(X0.copy(), step)
                for k in range(K):
                    want = _op(pm, name, float(ts[k]), kind)(col(X0, k).copy(), sk(k))
                    _same(col(got, k), want, "%s block %d component %d" % (name, block, k))
            got = ops.prox_components(X0.copy(), step, prox=members, axis=1 - block)
            for k in range(K):
                _same(col(got, k), members[k](col(X0, k).copy(), sk(k)), "mixed, block %d component %d" % (block, k))
            assert not np.array_equal(got, X0)


def _pgm_once(pm, c, inp, prox):
    A, S = inp["A0"].copy(), inp["S0"].copy()
    grad = tus.table_grad(inp["table"], np.float32)
    pm.pgm([A, S], grad, pm.nmf.constant_step(*c["step"]), prox=prox, e_rel=c["e_rel"], max_iter=1)
    assert grad.state["i"] == 1
    return A, S


@pytest.mark.gpu
@pytest.mark.parametrize("accelerated", [False, True], ids=["pgm", "fista"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_one_pgm_iteration_column_by_column(pm, M, N, K, accelerated):
    """one pgm iteration fed by a gradient table with constant steps (the components are independent): with five distinct thresholds
    dealt cyclically, then with a mixed prox_components on both blocks, component k of A and of S is component k of the run that
    applies row k's operator to the whole block"""
    c = tus._mk(dict(tus.PGM_DEFAULTS, step=(0.5, 0.25)), (M, N, K), prox="plus_plus", iters=1)
    inp = tus.make_inputs(c)
    inp["A0"], inp["S0"] = inp["A0"] - 0.3, inp["S0"] - 0.3           # (both signs; step x g reaches the thresholds' scale)
    ts = [0.05, 0.2, 0.4, 0.7, 1.1]
    tk = np.array([ts[k % 5] for k in range(K)])
    for name, kind in (("soft", "relative"), ("hard", "absolute"), ("max_entropy", "relative")):
        A, S = _pgm_once(pm, c, inp, [_op(pm, name, _per_k(tk, 0), kind), _op(pm, name, _per_k(tk, 1), kind)])
        for i, t in enumerate(ts[:min(5, K)]):
            Ai, Si = _pgm_once(pm, c, inp, [_op(pm, name, t, kind)] * 2)
            _same(A[:, i::5], Ai[:, i::5], "%s threshold %g on A" % (name, t))
            _same(S[i::5], Si[i::5], "%s threshold %g on S" % (name, t))
    members, distinct = _mixed(pm, K)
    A, S = _pgm_once(pm, c, inp, [partial(pm.operators.prox_components, prox=members, axis=1), partial(pm.operators.prox_components, prox=members, axis=0)])
    for i, p in enumerate(distinct[:min(len(distinct), K)]):
        Ai, Si = _pgm_once(pm, c, inp, [p, p])
        _same(A[:, i::len(distinct)], Ai[:, i::len(distinct)], "member %d on A" % i)
        _same(S[i::len(distinct)], Si[i::len(distinct)], "member %d on S" % i)


# ---------------------------------------------------------------------------------------------------------------------
# 3. fp32 kernels against the fp64 oracle, every entry
# ---------------------------------------------------------------------------------------------------------------------
def components_apply_prox(original):
    """oracle.apply_prox that also understands ("components", [specs], axis): component k along `axis` gets specs[k], with
    component k's own step where the step is per component; everything else goes to the original"""
    def apply_prox(X, step, spec):
        if spec is None or spec[0] != "components":
            return original(X, step, spec)
        axis = spec[2]
        out = np.array(X, copy=True)
        st = np.asarray(step)
        for k, sp in enumerate(spec[1]):
            sk = st.reshape(-1)[k] if st.size > 1 else step
            if axis == 0:
                out[k] = apply_prox(X[k], sk, sp)
            else:
                out[:, k] = apply_prox(X[:, k], sk, sp)
        return out
    return apply_prox


def _spec_to_prox(original):
    def spec_to_prox(pm, spec):
        if spec is not None and spec[0] == "components":
            return partial(pm.operators.prox_components, prox=[original(pm, s) for s in spec[1]], axis=spec[2])
        return original(pm, spec)
    return spec_to_prox


def _gapped_inputs(original):
    """cases with gapped=True draw the factors like that file's "hard" cases, with a wider gap: nothing between 0.002 and 0.8, where the
    thresholds sit (adaprox hands its operators alpha / max(Psi), which moves by a factor of two over the iterations)"""
    def make_inputs(c):
        inp = original(c)
        if c.get("gapped"):
            rng = np.random.default_rng(c["seed"] + 500)
            for key in ("A0", "S0"):
                s = inp[key].shape
                inp[key] = np.where(rng.random(s) < 0.5, 0.001 + 0.001 * rng.random(s), 0.8 + 0.2 * rng.random(s)).astype(np.float32)
        return inp
    return make_inputs


def _oracle_pairs(K, nominal, ada=False):
    """prox-spec pairs (A, S) per name; nominal[j]: the step the solver hands block j's operator, so that a relative threshold T / nominal
    lands at T in data units.  The factors are gapped (half the entries in 0.001 .. 0.002, half in 0.8 .. 1) and every component's
    threshold lies between the two halves, so both outcomes of every row's branch occur -- and what a soft threshold leaves of an entry
    of the upper half keeps that entry's magnitude: |x| - t for x near t has no relative accuracy in ANY arithmetic, and the
    imported tolerances measure relative to the entry."""
    # soft: applied once per iteration by pgm (3 T < 0.8) and up to 3 times per iteration by adaprox's passes (9 T < 0.4: the step
    # adaprox hands over, alpha / max(Psi), moves by up to a factor of two around the nominal one)
    T = np.linspace(0.01, 0.04, K) if ada else np.linspace(0.03, 0.1, K)
    TH = np.linspace(0.12, 0.35, K)                                    # min / max / hard: a fixed level inside the gap

    def rel(j, v):
        return _per_k(np.asarray(v) / nominal[j], j)
    mixed = [[("soft", float(T[k] / nominal[j]), "relative"), ("plus",), ("min", float(TH[k]), "absolute"), ("soft_plus", float(T[k]), "absolute"),
              ("max", float(TH[k] / nominal[j]), "relative"), ("id",)][k % 6] for j in range(2) for k in range(K)]
    return {
        "k_soft": (("soft", _per_k(T, 0), "absolute"), ("soft", rel(1, T), "relative")),
        "k_softplus_min": (("soft_plus", rel(0, T), "relative"), ("min", _per_k(TH, 1), "absolute")),
        "k_max_seq": (("max", rel(0, TH), "relative"), ("seq", (("soft", _per_k(T, 1), "absolute"), ("plus",)), 1)),
        "k_hard": (("hard", rel(0, TH), "relative"), ("hard_plus", _per_k(TH, 1), "absolute")),
        "k_components": (("components", mixed[:K], 1), ("components", mixed[K:], 0)),
    }


ORACLE_SHAPES = SHAPES
ORACLE_PROX = ("k_soft", "k_softplus_min", "k_max_seq", "k_hard", "k_components")


def _oracle_cases():
    out = []
    for s in ORACLE_SHAPES:
        for name in ORACLE_PROX:
            extra = dict(gapped=True, seed=11)
            out.append(tus._mk(tus.PGM_DEFAULTS, s, prox=name, iters=3, **extra))
            if name == "k_soft":       # (FISTA's extrapolation X + omega (X - X_prev) cancels where an operator has just moved an entry: k_soft alone)
                out.append(tus._mk(tus.PGM_DEFAULTS, s, prox=name, iters=3, accelerated=True, **extra))
            for scheme in ("adam", "amsgrad"):
                out.append(tus._mk(tus.ADA_DEFAULTS, s, prox=name, iters=3, scheme=scheme, **dict(extra, step=(0.002, 0.002))))
    return out


ORACLE_CASES = _oracle_cases()
ORACLE_BY_ID = {c["id"]: c for c in ORACLE_CASES}
assert len(ORACLE_BY_ID) == len(ORACLE_CASES)


def _nominal(c):
    """the step the solver hands the operators: pgm its constant steps; adaprox gamma = alpha / max(Psi), max(Psi) ~ 1.5e3 = max |g| of the
    table with adam (bias-corrected; tests/test_gpu_update_step.py: prox_specs), sqrt(1 - b2) of that with amsgrad (algorithms.py:170-180)"""
    if c["backend"] != "ada":
        return list(c["step"])
    psi = 1.5e3 * (np.sqrt(1 - c["b2"]) if c["scheme"] == "amsgrad" else 1.0)
    return [a / psi for a in c["step"]]


@contextlib.contextmanager
def _patched(c):
    """tests/test_gpu_update_step.py's machinery with this file's cases, through pytest's monkeypatch: its prox tables gain the
    case's pair, its oracle and its spec translation learn ("components", ..), its inputs the gapped factors; undone on exit"""
    from oracle import nmf_oracle as orc
    pair = _oracle_pairs(c["shape"][2], _nominal(c), c["backend"] == "ada")[c["prox"]]
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(orc, "apply_prox", components_apply_prox(orc.apply_prox))
        mp.setattr(tus, "spec_to_prox", _spec_to_prox(tus.spec_to_prox))
        mp.setattr(tus, "make_inputs", _gapped_inputs(tus.make_inputs))
        mp.setitem(tus.PROX_PAIRS, c["prox"], pair)
        mp.setitem(tus.PGM_PROX_PAIRS, c["prox"], pair)
        yield pair


@functools.lru_cache(maxsize=2)
def _reference(cid, dtype=np.float64):
    with _patched(ORACLE_BY_ID[cid]):
        return tus.run_reference(ORACLE_BY_ID[cid], dtype)


def _fixed_value_hits(X, spec, j):
    """per component of block j: how many entries sit at the operator's fixed value (0, or the threshold of min / max); None: no branch"""
    if spec[0] in ("id", "plus", "seq", "components"):
        return None
    Xk = X if j == 0 else X.T                                       # rows x K
    if spec[0] in ("min", "max") and spec[2] == "absolute":
        return (Xk == np.asarray(spec[1]).reshape(1, -1)).sum(0)
    if spec[0] in ("min", "max"):
        return None                                                 # (the relative threshold moves with the step: checked through its absolute twin)
    return (Xk == 0).sum(0)


@pytest.mark.parametrize("cid", sorted(ORACLE_BY_ID))
def test_reference_preconditions(cid):
    """on the oracle alone: the float32 oracle stays within that file's REF_ERR_* of the float64 oracle on these cases (the imported
    tolerances were derived from its own), HARD_GUARD, BAND, and both outcomes of every row's branch"""
    c = ORACLE_BY_ID[cid]
    ref = _reference(cid)
    with _patched(c) as pair:
        r32 = tus.run_reference(c, np.float32)
    assert r32["conv"] == ref["conv"] and r32["n_iter"] == ref["n_iter"] == c["iters"] and r32.get("sub") == ref.get("sub")
    lim = {"X": tus.REF_ERR_ADA_X, "M": tus.REF_ERR_ADA_M, "V": tus.REF_ERR_ADA_V} if c["backend"] == "ada" else {"X": tus.REF_ERR_PGM_X, "STEP": tus.REF_ERR_PGM_STEP}
    for name, key, u in tus.quantities(c, r32, ref):
        assert u <= lim[key], "%s: the float32 oracle is %.4g units from the float64 oracle (REF_ERR %.4g)" % (name, u, lim[key])
    if c["prox"] == "k_hard":
        assert tus.HARD_GUARD <= ref["hard_margin"] < np.inf, ref["hard_margin"]
    for i, (d, n) in enumerate(ref["decisions"]):
        if d == 0 or np.isnan(d) or np.isnan(n):
            continue
        q = d / (tus.decision_e_rel(c, i) ** 2 * n) if n > 0 else np.inf
        assert not (tus.BAND[0] <= q <= tus.BAND[1]), q
    assert ref["decisions"]
    for j, X in enumerate((ref["A"], ref["S"])):
        specs = pair[j][1] if pair[j][0] == "components" else [pair[j]]
        hits = _fixed_value_hits(X, pair[j], j)
        if hits is not None:
            rows = X.shape[0] if j == 0 else X.shape[1]
            assert ((hits > 0) & (hits < rows)).all(), (j, pair[j][0], hits.min(), hits.max(), rows)
        if pair[j][0] == "components":                              # member k on component k
            Xk = X if j == 0 else X.T
            for k, sp in enumerate(specs):
                if sp[0] in ("soft", "soft_plus"):
                    assert 0 < (Xk[:, k] == 0).sum() < Xk.shape[0], (j, k, sp)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", sorted(ORACLE_BY_ID))
def test_update_with_per_component_operators_matches_the_oracle_on_every_entry(pm, monkeypatch, cid):
    c = ORACLE_BY_ID[cid]
    ref = _reference(cid)
    if c["backend"] == "ada":
        monkeypatch.setenv("PMX_TAIL_FUSED", "1")                   # (left unfused for op 12 by the library itself)
    with _patched(c):
        run = tus.run_device(pm, c)
    tus.assert_meets_reference(c, run, ref, "per-component")


# ---------------------------------------------------------------------------------------------------------------------
# 4. fp64 kernels against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------
def _f64_spec(case, j, step0, K):
    """per-component twin of tests/test_gpu_f64_operators.py's make_spec: thresholds from half to one and a half times the case's"""
    f = np.linspace(0.5, 1.5, K)
    if case[0] == "components":
        mix = [("soft", 0.2 / step0, "relative"), ("plus",), ("hard_plus", 0.3, "absolute"), ("min", 0.3 / step0, "relative"), ("max", 0.6, "absolute"), ("id",)]
        return ("components", [mix[k % len(mix)] for k in range(K)], 1 - j)
    name, kind, t = case
    return (name, _per_k(f * (t / step0 if kind == "relative" else t), j), kind)


def _f64_prox(pm, spec):
    if spec[0] == "components":
        return partial(pm.operators.prox_components, prox=[tgo.to_prox(pm, s) for s in spec[1]], axis=spec[2])
    return tgo.to_prox(pm, spec)


def _f64_fired(X, spec, j, step=None):
    if spec[0] == "components":
        return bool(0 < (X == 0).sum() < X.size)
    if spec[0] not in ("min", "max"):
        hit = X == 0
    else:
        hit = X == np.broadcast_to(spec[1] * step if spec[2] == "relative" else spec[1], X.shape)
    return bool(0 < hit.sum() < hit.size)


F64_PGM = [("soft", "relative", 0.2), ("hard", "absolute", 0.3), ("min", "relative", 0.3), ("components",)]
F64_ADA = [("soft", "relative", 0.05), ("max", "absolute", 0.6), ("components",)]
F64_BSDMM = [("soft", "relative", 0.2), ("components",)]


@contextlib.contextmanager
def _components_oracle():
    """oracle.nmf_oracle with an apply_prox that understands ("components", ..) (pytest's monkeypatch; undone on exit)"""
    from oracle import nmf_oracle as orc
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(orc, "apply_prox", components_apply_prox(orc.apply_prox))
        yield orc


def _f64_problem(orc, shape):
    M, N, K = shape
    return orc.synthetic_problem(M, N, K, np.float64, seed=M + N + K)


@functools.lru_cache(maxsize=None)
def _f64_pgm_reference(shape, case, j):
    """-> (specs, A, S, the oracle's return value after 3 iterations, whether the thresholds fired in one of iterations 1 .. 3)"""
    with _components_oracle() as orc:
        Y, A0, S0 = _f64_problem(orc, shape)
        steps0 = orc.lipschitz_steps(A0, S0)
        specs = [("plus",), ("plus",)]
        specs[j] = _f64_spec(case, j, steps0[j], shape[2])
        fired = False
        for n in range(1, 4):
            Ao, So = A0.copy(), S0.copy()
            oret = orc.pgm_nmf(Y, Ao, So, prox_A=specs[0], prox_S=specs[1], max_iter=n, e_rel=1e-9)
            fired |= _f64_fired((Ao, So)[j], specs[j], j, oret[2][j])
    return specs, Ao, So, oret, fired


F64_ADA_ITS, F64_ADA_E_REL, F64_BSDMM_ITS = 4, 1e-4, 4


@functools.lru_cache(maxsize=None)
def _f64_ada_reference(shape, case):
    """-> (spec of S, A, S, the oracle's return value after the last iteration, fired)"""
    with _components_oracle() as orc:
        Y, A0, S0 = _f64_problem(orc, shape)
        gamma0 = float(np.mean(orc.adaprox_steps(A0, S0)[1])) / (np.sqrt(1e-3) * np.abs(orc.residual_gradients(A0, S0, Y)[1]).max())
        spec = _f64_spec(case, 1, gamma0, shape[2])
        fired = False
        for n in range(1, F64_ADA_ITS + 1):
            Ao, So = A0.copy(), S0.copy()
            out = orc.adaprox_nmf(Y, Ao, So, ("plus",), spec, scheme="amsgrad", max_iter=n, e_rel=F64_ADA_E_REL, check_convergence=False)
            fired |= _f64_fired(So, spec, 1)
    return spec, Ao, So, out, fired


@functools.lru_cache(maxsize=None)
def _f64_bsdmm_reference(shape, case):
    """-> (specs, A, S, the oracle's state after the last iteration, [fired on Z_A, fired on Z_S])"""
    with _components_oracle() as orc:
        Y, A0, S0 = _f64_problem(orc, shape)
        steps0 = orc.lipschitz_steps(A0, S0)
        specs = [_f64_spec(case, j, 2.0 * steps0[j], shape[2]) for j in range(2)]
        fired = [False, False]
        for n in range(1, F64_BSDMM_ITS + 1):
            Ao, So = A0.copy(), S0.copy()
            state = {}
            orc.bsdmm_nmf(Y, Ao, So, proxs_g=[[specs[0]], [specs[1]]], max_iter=n, e_rel=1e-9, state=state)
            for j in range(2):
                fired[j] |= _f64_fired(state["Z"][j][0], specs[j], j, 2.0 * steps0[j])
    return specs, Ao, So, state, fired


@pytest.mark.parametrize("M,N,K", tgo.SHAPES)
def test_fp64_preconditions(M, N, K):
    """on the oracle alone: in every fp64 case below the thresholds fire on some entries and leave others (both outcomes of the
    operators' branches occur)"""
    shape = (M, N, K)
    for case in F64_PGM:
        for j in range(2):
            assert _f64_pgm_reference(shape, case, j)[4], "pgm: the thresholds of %r miss the data on block %d" % (case, j)
    for case in F64_ADA:
        assert _f64_ada_reference(shape, case)[4], "adaprox: the thresholds of %r miss the data" % (case,)
    for case in F64_BSDMM:
        assert all(_f64_bsdmm_reference(shape, case)[4]), "bsdmm: the thresholds of %r miss the data" % (case,)


@pytest.mark.gpu
@pytest.mark.parametrize("case", F64_PGM, ids=tgo._id)
@pytest.mark.parametrize("M,N,K", tgo.SHAPES)
def test_fp64_pgm_on_either_block(pm, orc, monkeypatch, M, N, K, case):
    from test_gpu_f64_big import _spy
    seen = _spy(monkeypatch)
    shape = (M, N, K)
    Y, A0, S0 = _f64_problem(orc, shape)
    for j in range(2):
        specs, Ao, So, oret, _ = _f64_pgm_reference(shape, case, j)
        del seen[:]
        A, S = A0.copy(), S0.copy()
        conv, G, steps = pm.nmf.nmf(Y, A, S, prox_A=_f64_prox(pm, specs[0]), prox_S=_f64_prox(pm, specs[1]), max_iter=3, e_rel=1e-9)
        assert seen == [("f64", tgo._kernel(shape))], seen
        assert A.dtype == np.float64
        tgo._close(shape, A, Ao, "%r on block %d: A" % (case, j))
        tgo._close(shape, S, So, "%r on block %d: S" % (case, j))
        assert tuple(conv) == tuple(oret[0])


@pytest.mark.gpu
@pytest.mark.parametrize("case", F64_ADA, ids=tgo._id)
@pytest.mark.parametrize("M,N,K", tgo.SHAPES)
def test_fp64_adaprox_in_the_proximal_loop(pm, orc, M, N, K, case):
    from proxmin_amd.engine import DeviceNMF
    ops = pm.operators
    shape = (M, N, K)
    its, e_rel = F64_ADA_ITS, F64_ADA_E_REL
    Y, A0, S0 = _f64_problem(orc, shape)
    spec, Ao, So, out, _ = _f64_ada_reference(shape, case)
    with DeviceNMF(M, N, K, mode="f64") as dev:
        assert dev.k1_info()["kernel"] == tgo._kernel(shape)
        dev.set_Y(Y)
        dev.set_factors(A0, S0)
        dev.adaprox_begin([ops.device_proxseq(ops.prox_plus, 0), ops.device_proxseq(_f64_prox(pm, spec), 1)],
                          scheme="amsgrad", check_convergence=False, e_rel=(e_rel, e_rel))
        res = dev.adaprox_run(np.full(its, 0.9), 0.9)
        A, S = dev.get_factors()
    got = [int(res.sub_iterations[0]), int(res.sub_iterations[1])]
    assert res.iterations == its and got == [int(out[5][0]), int(out[5][1])], (got, out[5])
    tgo._close(shape, A, Ao, "%r: A" % (case,))
    tgo._close(shape, S, So, "%r: S" % (case,))


@pytest.mark.gpu
@pytest.mark.parametrize("case", F64_BSDMM, ids=tgo._id)
@pytest.mark.parametrize("M,N,K", tgo.SHAPES)
def test_fp64_bsdmm_as_constraints(pm, orc, M, N, K, case):
    from proxmin_amd import _lib
    from proxmin_amd.engine import DeviceNMF
    ops = pm.operators
    shape = (M, N, K)
    its = F64_BSDMM_ITS
    Y, A0, S0 = _f64_problem(orc, shape)
    specs, Ao, So, state, _ = _f64_bsdmm_reference(shape, case)
    with DeviceNMF(M, N, K, mode="f64") as dev:
        assert dev.k1_info()["kernel"] == tgo._kernel(shape)
        dev.set_Y(Y)
        dev.set_factors(A0, S0)
        dev.bsdmm_begin([ops.device_proxseq(ops.prox_plus, j) for j in range(2)],
                        [[ops.device_proxseq(_f64_prox(pm, specs[j]), j)] for j in range(2)], e_rel=(1e-9, 1e-9), e_abs=(0.0, 0.0))
        dev.bsdmm_run(its)
        A, S = dev.get_factors()
        Z = [dev._download(_lib.BUF_Z0 + j * _lib.MAX_G, (M, N)[j]) for j in range(2)]
        U = [dev._download(_lib.BUF_U0 + j * _lib.MAX_G, (M, N)[j]) for j in range(2)]
    tgo._close(shape, A, Ao, "%r: A" % (case,))
    tgo._close(shape, S, So, "%r: S" % (case,))
    tgo._close(shape, Z[0], state["Z"][0][0], "Z_A")
    tgo._close(shape, U[0], state["U"][0][0], "U_A", loose=True)
    tgo._close(shape, Z[1].T, state["Z"][1][0], "Z_S")
    tgo._close(shape, U[1].T, state["U"][1][0], "U_S", loose=True)


# ---------------------------------------------------------------------------------------------------------------------
# 5. fixtures from the real reference: array thresholds on soft, soft_plus, hard, hard_plus (tests/golden/README_components.md)
# ---------------------------------------------------------------------------------------------------------------------
def _golden():
    import importlib.util
    import json
    import os
    from conftest import GOLDEN
    if "gen" not in _G:
        spec = importlib.util.spec_from_file_location("make_components_golden", os.path.join(GOLDEN, "make_components_golden.py"))
        gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gen)                    # (imports the reference only inside its main())
        z = np.load(os.path.join(GOLDEN, "components.npz"), allow_pickle=False)
        _G.update(gen=gen, z=z, meta=json.loads(str(z["meta"])), vol={}, dir=GOLDEN)
    return _G


_G = {}


def _final(name, which):
    import os
    g = _golden()
    v = g["meta"]["volumes"][name]
    if v not in g["vol"]:
        g["vol"][v] = np.load(os.path.join(g["dir"], "components_%d.npz" % v), allow_pickle=False)
    return g["vol"][v][name + "/" + which]


def _golden_names(kind):
    import json
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "components.npz")
    return sorted(json.loads(str(np.load(here, allow_pickle=False)["meta"]))[kind])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", _golden_names("op"))
def test_standalone_array_threshold_against_the_reference(pm, name, dtype):
    """The reference's own output.  The kernel works in float32 with (float)thresh: against the reference's float64 evaluation of
    the same input that is the rounding of the threshold, of thresh x step and of |x| - t (and, for float64 arrays, of the input):
    5 x 2^-24 max(|x|, t) per entry; no argument lies within 1e-3 max|X| of its threshold, so the branches agree."""
    g = _golden()
    gen, c = g["gen"], g["meta"]["op"][name]
    K = c["shape"][1] if c["block"] == 0 else c["shape"][0]
    t = gen.thresholds(K, c["level"])
    t_eff = gen.per_component(t * (c["step"] if c["type"] == "relative" else 1.0), c["block"])
    X64 = gen.operator_inputs(tuple(c["shape"]), t_eff, c["seed"])
    assert float(X64.sum()) == c["sum64"]
    X = X64.astype(dtype)
    want = g["z"][name + ("/ref32" if dtype == np.float32 else "/ref64")]
    out = getattr(pm.operators, "prox_" + c["op"])(X, c["step"], thresh=gen.per_component(t, c["block"]), type=c["type"])
    assert out is X and X.dtype == dtype
    np.testing.assert_array_equal(X == 0, want == 0)
    tol = 5 * 2.0 ** -24 * np.maximum(np.abs(X64), np.broadcast_to(t_eff, X64.shape))
    assert (np.abs(X.astype(np.float64) - want) <= tol).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", _golden_names("solver"))
def test_solver_finals_with_array_thresholds_against_the_reference(pm, caplog, name):
    """8 iterations of the reference's nmf() with an array `thresh`: its final factors at the tolerances tests/test_gpu_max_entropy.py
    uses for the same routes and dtypes (imported), in the library's default arithmetic and in exact fp32"""
    import logging
    import test_gpu_max_entropy as tgm
    g = _golden()
    gen, c = g["gen"], g["meta"]["solver"][name]
    shape = name.split("/")[0]
    Y, A0, S0 = gen.solver_problem(c["M"], c["N"], c["K"], c["dtype"], c["seed"])
    assert [float(v.astype(np.float64).sum()) for v in (Y, A0, S0)] == c["sums"], "the regenerated inputs are not the generator's"
    ops = pm.operators
    op = partial(getattr(ops, "prox_" + c["op"]), thresh=gen.per_component(gen.thresholds(c["K"], c["level"]) * c["scale"], c["block"]), type=c["type"])
    kw = dict(max_iter=g["meta"]["iterations"], e_rel=c["e_rel"])
    prox = [ops.prox_plus, ops.prox_plus]
    if c["route"] != "bsdmm_g":
        prox[c["block"]] = op
    else:
        kw["proxs_g"] = [[op], None] if c["block"] == 0 else [None, [op]]
    if c["route"] == "fista":
        kw.update(accelerated=True, step=pm.nmf.scaled_step_pgm(0.5))
    if c["route"] in ("bsdmm_prox", "bsdmm_g"):
        kw["algorithm"] = pm.bsdmm
    if c["route"] == "adam_abs":
        kw.update(algorithm=pm.adaprox, scheme="adam")
    for mode in ((None, "f32") if shape.startswith("f32") else (None,)):
        pm.set_default_mode(mode)
        try:
            A, S = A0.copy(), S0.copy()
            caplog.clear()
            with caplog.at_level(logging.INFO, logger="proxmin"):
                pm.nmf.nmf(Y, A, S, prox_A=prox[0], prox_S=prox[1], **kw)
            text = " | ".join(r.getMessage() for r in caplog.records)
            assert "one iteration per call" not in text and "user-defined Python callable" not in text, text
            assert not (shape.startswith("f64") and "computed in float32" in text), text
            what = "%s (%s)" % (name, pm.get_default_mode())
            tgm._compare(shape, pm.get_default_mode(), A, _final(name, "A"), what + " A")
            tgm._compare(shape, pm.get_default_mode(), S, _final(name, "S"), what + " S")
        finally:
            pm.set_default_mode(None)
