"""GPU: the remaining sites of the per-component operators (PMX_PROX_COMPONENTS, op 12) -- tests/test_gpu_components.py has the
update kernels proper.

* `DeviceNMF.prox_apply` (pmx_prox_apply with the context's tables: k_prox_view on the context's buffer): equal rows are the
  scalar operator, distinct rows and a mixed prox_components are the stand-alone call on an ndarray (which that file checks column
  by column), bit for bit; its tables go into the slots BEHIND those of the running solver, whose next iterations are unchanged.
* pgm / FISTA with op 12 beside prox_unity* along a factor's long axis in ONE sequence (k_pgm_unity's chain): equal rows are the
  scalar sequence, distinct rows are the same call on the host route (the stand-alone kernels between launches), bit for bit.
* the line search (k_bt_update; at 256 x 512 x 64 the K = 64 whole-block kernels, k64b_bt_update) and pgm with step arrays
  (per-element steps, the relative thresholds formed element by element): equal rows are the scalar operator; with step arrays and
  a gradient table, component k is the scalar operator of row k, bit for bit.
* the status codes that include/pmx.h documents for pmx_prox_table and for sequences that name a table.
"""
import ctypes as C
import logging
from functools import partial

import numpy as np
import pytest

import test_gpu_update_step as tus
import test_gpu_unity_long_axis as tgu
from test_gpu_components import KINDS, SHAPES, THRESH_OPS, _data, _mixed, _op, _per_k, _same, pm, orc        # noqa: F401 (fixtures)

INVALID, UNSUPPORTED = -1, -4            # include/pmx.h: PMX_E_INVALID, PMX_E_UNSUPPORTED


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------------------------------------
# DeviceNMF.prox_apply
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_prox_apply_on_the_buffers_of_a_context(pm, M, N, K):
    from proxmin_amd import _lib
    from proxmin_amd.engine import DeviceNMF
    ops = pm.operators
    X0 = [_data((M, K), 21), _data((K, N), 22)]
    ts, step_k = np.linspace(0.05, 0.9, K), np.linspace(0.5, 2.0, K)
    members, _ = _mixed(pm, K)
    # (what prox_apply gets per block, what the stand-alone call on the ndarray gets): equal rows against the scalar operator
    pairs = [([_op(pm, name, _per_k(np.full(K, 0.3), j), kind) for j in range(2)], [_op(pm, name, 0.3, kind)] * 2)
             for name in THRESH_OPS for kind in KINDS]
    pairs += [([partial(ops.prox_components, prox=[_op(pm, name, 0.3, "relative")] * K, axis=1 - j) for j in range(2)], [_op(pm, name, 0.3, "relative")] * 2)
              for name in THRESH_OPS]
    # distinct rows and a mixed list against the same operator on the ndarray
    for name in THRESH_OPS:
        p = [_op(pm, name, _per_k(ts, j), "relative") for j in range(2)]
        pairs.append((p, p))
    p = [partial(ops.prox_components, prox=members, axis=1 - j) for j in range(2)]
    pairs.append((p, p))
    with DeviceNMF(M, N, K, mode="f32") as dev:
        for step in (0.7, step_k):
            for on_device, on_array in pairs:
                dev.set_factors(X0[0], X0[1])
                dev.prox_apply(_lib.BUF_A, ops.device_proxseq(on_device[0], 0), step)
                dev.prox_apply(_lib.BUF_ST, ops.device_proxseq(on_device[1], 1), step)
                got = dev.get_factors()
                for j in range(2):
                    want = on_array[j](X0[j].copy(), step if np.ndim(step) == 0 else _per_k(step, j))
                    _same(np.ascontiguousarray(got[j]), want, "%r on block %d" % (on_device[j], j))
                assert not np.array_equal(got[0], X0[0])


@pytest.mark.gpu
def test_prox_apply_leaves_the_tables_of_the_running_solver_alone(pm, orc):
    """pgm with a per-component operator on either block holds slots 0 and 1; a prox_apply between two of its iterations
    uploads its own table (all rows prox_id: the factor stays what it is) into slot 2, and the iterations that follow give the
    bits of the uninterrupted run.  (Exact fp32 and constant steps: nothing of the iteration depends on what else
    pmx_prox_apply invalidates.)"""
    from proxmin_amd import _lib
    from proxmin_amd.engine import DeviceNMF
    ops = pm.operators
    M, N, K = 33, 47, 5
    Y, A0, S0 = orc.synthetic_problem(M, N, K, np.float32, seed=5)
    steps = orc.lipschitz_steps(A0.astype(np.float64), S0.astype(np.float64))
    prox = [_op(pm, "soft", _per_k(np.linspace(0.05, 0.3, K) / steps[j], j), "relative") for j in range(2)]
    ident = partial(ops.prox_components, prox=[ops.prox_id] * K, axis=1)
    out = []
    for interrupt in (False, True):
        with DeviceNMF(M, N, K, mode="f32") as dev:
            dev.set_Y(Y)
            dev.set_factors(A0, S0)
            dev.pgm_begin([ops.device_proxseq(prox[j], j) for j in range(2)], fixed_steps=steps, e_rel=(1e-9, 1e-9))
            assert dev._ntab_solver == 2
            dev.pgm_run(1)
            if interrupt:
                dev.prox_apply(_lib.BUF_A, ops.device_proxseq(ident, 0), 1.0)
                assert dev._ntab == 3 and dev._ntab_solver == 2
            dev.pgm_run(2)
            out.append(dev.get_factors())
    for j in range(2):
        _same(np.ascontiguousarray(out[1][j]), np.ascontiguousarray(out[0][j]), "block %d" % j)
        assert 0 < (out[0][j] == 0).sum() < out[0][j].size


# ---------------------------------------------------------------------------------------------------------------------
# k_pgm_unity's chain: op 12 beside a long-axis prox_unity* in one sequence
# ---------------------------------------------------------------------------------------------------------------------
def _chain_problem(M, N, K, block):
    """factors that start feasible (tests/test_gpu_unity_long_axis.py: make_problem): the block sums to one along its long
    axis, the other block takes the scale"""
    c = dict(shape=(M, N, K), pA=tgu.UA if block == 0 else tgu.PLUS, pS=tgu.UPS if block == 1 else tgu.PLUS, seed=M + N + K, weighted=False)
    return tgu.make_problem(c)[:3]


def _chain_prox(pm, block, t):
    """block 0: [unity along axis 0, soft], block 1: [unity_plus along axis 1, hard] with absolute thresholds -- the threshold
    first (AlternatingProjections applies last to first), then the sums; prox_plus on the other block"""
    ops = pm.operators
    prox = [ops.prox_plus, ops.prox_plus]
    if block == 0:
        prox[0] = ops.AlternatingProjections([partial(ops.prox_unity, axis=0), _op(pm, "soft", t, "absolute")])
    else:
        prox[1] = ops.AlternatingProjections([partial(ops.prox_unity_plus, axis=1), _op(pm, "hard", t, "absolute")])
    return prox


@pytest.mark.gpu
@pytest.mark.parametrize("accelerated", [False, True], ids=["pgm", "fista"])
@pytest.mark.parametrize("block", [0, 1], ids=["A", "S"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_pgm_unity_chain_with_per_component_thresholds(pm, monkeypatch, M, N, K, block, accelerated):
    from proxmin_amd import _lib
    from proxmin_amd.engine import DeviceNMF
    Y, A0, S0 = _chain_problem(M, N, K, block)
    level = 1.0 / (M, N)[block]                    # the mean entry of a block that sums to one along its long axis
    begun = []
    real = DeviceNMF.pgm_begin

    def spy(self, prox, *a, **kw):
        begun.append(([[(int(q.seq[i].op), int(q.seq[i].unit)) for i in range(q.n)] for q in prox], tuple(kw.get("host_prox", (False, False)))))
        return real(self, prox, *a, **kw)
    monkeypatch.setattr(DeviceNMF, "pgm_begin", spy)

    def run(prox):
        A, S = A0.copy(), S0.copy()
        pm.nmf.nmf(Y, A, S, prox_A=prox[0], prox_S=prox[1], accelerated=accelerated, max_iter=3, e_rel=1e-9)
        return A, S
    want = run(_chain_prox(pm, block, 0.8 * level))
    del begun[:]
    got = run(_chain_prox(pm, block, _per_k(np.full(K, 0.8 * level), block)))
    # one begin, nothing for the host, and the block's sequence holds the long-axis operator next to op 12
    assert len(begun) == 1 and not any(begun[0][1]), begun
    entries = begun[0][0][block]
    assert sorted(op for op, _ in entries) == sorted([_lib.PROX["components"], _lib.PROX["unity" if block == 0 else "unity_plus"]]), entries
    assert any(unit != 0 for _, unit in entries), entries
    for j in range(2):
        _same(got[j], want[j], "equal rows, block %d" % j)
    assert np.isfinite(got[block]).all() and 0 < (got[block] == 0).sum() < got[block].size
    # distinct rows: the same call with the sequence as a Python function is the host route -- the stand-alone kernels on the
    # downloaded argument -- and gives the same bits
    t = _per_k(np.linspace(0.45, 0.9, K) * level, block)      # (inside the block's entries, 0.33 .. 1.63 x level: no component is emptied)
    fused = run(_chain_prox(pm, block, t))
    assert not np.array_equal(fused[block], got[block])
    if (M, N)[block] > _lib.MAXK:       # (a short "long" axis: the direct call sums it inside one row of the transposed array, in another order)
        del begun[:]
        q = _chain_prox(pm, block, t)
        q[block] = lambda X, s, ap=q[block]: ap(X, s)
        host = run(q)
        assert begun and all(hp[block] for _, hp in begun), begun
        for j in range(2):
            _same(fused[j], host[j], "distinct rows against the host route, block %d" % j)
    zeros = (fused[block] == 0).sum(0 if block == 0 else 1)          # per component
    assert np.isfinite(fused[block]).all() and 0 < zeros.sum() < fused[block].size and len(set(zeros.tolist())) > 1, zeros


# ---------------------------------------------------------------------------------------------------------------------
# the line search and step arrays
# ---------------------------------------------------------------------------------------------------------------------
BT_SHAPES = [(np.float32, s) for s in SHAPES + [(256, 512, 64)]] + [(np.float64, s) for s in ((48, 72, 40), (128, 160, 100))]


@pytest.mark.gpu
@pytest.mark.parametrize("accelerated", [False, True], ids=["pgm", "fista"])
@pytest.mark.parametrize("dtype,shape", BT_SHAPES, ids=lambda v: v.__name__ if isinstance(v, type) else "x".join(map(str, v)))
def test_line_search_equal_rows_equal_the_scalar_operator(pm, orc, caplog, dtype, shape, accelerated):
    """pgm / FISTA with backtracking=True, 3 iterations from 1.5 x the Lipschitz steps (the search has something to halve): a
    table of equal rows and prox_components([p] * K) give the bits of the scalar operator, on either block, for a relative and an
    absolute operator and for prox_max_entropy"""
    M, N, K = shape
    Y, A0, S0 = orc.synthetic_problem(M, N, K, dtype, seed=M + N + K)
    steps0 = orc.lipschitz_steps(A0.astype(np.float64), S0.astype(np.float64))
    kw = dict(backtracking=True, f=partial(pm.nmf.log_likelihood, Y=Y), step=pm.nmf.scaled_step_pgm(1.5), accelerated=accelerated, max_iter=3, e_rel=1e-9)

    def run(block, p):
        prox = [pm.operators.prox_plus] * 2
        prox[block] = p
        A, S = A0.copy(), S0.copy()
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="proxmin"):
            pm.nmf.nmf(Y, A, S, prox_A=prox[0], prox_S=prox[1], **kw)
        text = " | ".join(r.getMessage() for r in caplog.records)
        assert "one iteration per call" not in text and "user-defined Python callable" not in text, text
        assert not (dtype == np.float64 and "computed in float32" in text), text
        return A, S
    for block in range(2):
        plain = run(block, pm.operators.prox_plus)
        for name, kind, t in (("soft", "relative", 0.3 / steps0[block]), ("hard_plus", "absolute", 0.3), ("max_entropy", "relative", 0.3 / steps0[block])):
            want = run(block, _op(pm, name, t, kind))
            got = run(block, _op(pm, name, _per_k(np.full(K, t), block), kind))
            comp = run(block, partial(pm.operators.prox_components, prox=[_op(pm, name, t, kind)] * K, axis=1 - block))
            for j in range(2):
                _same(got[j], want[j], "%s on block %d, array: block %d" % (name, block, j))
                _same(comp[j], want[j], "%s on block %d, components: block %d" % (name, block, j))
            # (from these starts the search may accept no step on A in three iterations, whatever the operator: A then stays what it was in
            # all of the runs; S moves in every case, and a soft threshold or an entropy term moves every positive entry of it)
            assert block == 0 or name == "hard_plus" or not np.array_equal(want[block], plain[block])


def _pgm_once_with_step_arrays(pm, c, inp, prox, step_arrays, accelerated):
    A, S = inp["A0"].copy(), inp["S0"].copy()
    grad = tus.table_grad(inp["table"], np.float32)
    pm.pgm([A, S], grad, lambda *X, it=None: step_arrays, prox=prox, accelerated=accelerated, e_rel=c["e_rel"], max_iter=1)
    assert grad.state["i"] == 1
    return A, S


@pytest.mark.gpu
@pytest.mark.parametrize("accelerated", [False, True], ids=["pgm", "fista"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_step_arrays_column_by_column(pm, M, N, K, accelerated):
    """one pgm iteration whose user `step` returns a full-shape array for A and a per-component (K, 1) array for S, fed by a
    gradient table: relative thresholds are formed element by element.  Equal rows give the scalar operator's bits; with five
    distinct thresholds dealt cyclically, then a mixed prox_components, component k is the run with row k's operator on the
    whole block"""
    c = tus._mk(dict(tus.PGM_DEFAULTS, step=(0.5, 0.25)), (M, N, K), prox="plus_plus", iters=1)
    inp = tus.make_inputs(c)
    inp["A0"], inp["S0"] = inp["A0"] - 0.3, inp["S0"] - 0.3
    rng = np.random.default_rng(M + K)
    arrays = ((0.5 * (0.5 + rng.random((M, K)))).astype(np.float32), (0.25 * (0.5 + rng.random((K, 1)))).astype(np.float32))
    once = partial(_pgm_once_with_step_arrays, pm, c, inp, step_arrays=arrays, accelerated=accelerated)
    ts = [0.05, 0.2, 0.4, 0.7, 1.1]
    tk = np.array([ts[k % 5] for k in range(K)])
    for name in ("soft", "max_entropy"):
        scalar = [once([_op(pm, name, t, "relative")] * 2) for t in ts[:min(5, K)]]
        A, S = once([_op(pm, name, _per_k(np.full(K, ts[0]), j), "relative") for j in range(2)])
        _same(A, scalar[0][0], "%s equal rows, A" % name)
        _same(S, scalar[0][1], "%s equal rows, S" % name)
        A, S = once([_op(pm, name, _per_k(tk, j), "relative") for j in range(2)])
        for i, (Ai, Si) in enumerate(scalar):
            _same(A[:, i::5], Ai[:, i::5], "%s threshold %g on A" % (name, ts[i]))
            _same(S[i::5], Si[i::5], "%s threshold %g on S" % (name, ts[i]))
        if K >= 2:
            assert not np.array_equal(scalar[0][0], scalar[1][0])
    members, distinct = _mixed(pm, K)
    A, S = once([partial(pm.operators.prox_components, prox=members, axis=1), partial(pm.operators.prox_components, prox=members, axis=0)])
    for i, p in enumerate(distinct[:min(len(distinct), K)]):
        Ai, Si = once([p, p])
        _same(A[:, i::len(distinct)], Ai[:, i::len(distinct)], "member %d on A" % i)
        _same(S[i::len(distinct)], Si[i::len(distinct)], "member %d on S" % i)


# ---------------------------------------------------------------------------------------------------------------------
# status codes (include/pmx.h: pmx_prox_table, PMX_PROX_COMPONENTS)
# ---------------------------------------------------------------------------------------------------------------------
def _table(_lib, K, op="soft"):
    rows = (_lib.Prox * K)()
    for k in range(K):
        rows[k].op, rows[k].thresh, rows[k].relative = _lib.PROX[op], 0.1 * (k + 1), 0
    return rows


def _names_table(_lib, reserved, unit=0):
    q = _lib.ProxSeq()
    q.n, q.repeat = 1, 1
    q.seq[0].op, q.seq[0].unit, q.seq[0].reserved = _lib.PROX["components"], unit, reserved
    return q


@pytest.mark.gpu
def test_status_codes_of_tables_and_of_sequences_that_name_them(pm, orc):
    from proxmin_amd import _lib
    from proxmin_amd.engine import DeviceNMF
    M, N, K = 31, 33, 5
    Y, A0, S0 = orc.synthetic_problem(M, N, K, np.float32, seed=1)
    sk = np.ones(K, np.float32)
    with DeviceNMF(M, N, K, mode="f32") as dev:
        lib, h = dev.lib, dev.h
        dev.set_Y(Y)
        dev.set_factors(A0, S0)
        apply = lambda q: lib.pmx_prox_apply(h, _lib.BUF_A, C.byref(q), _vp(sk))
        # a sequence that names a table before any table exists
        assert apply(_names_table(_lib, 1)) == INVALID
        assert b"not been set" in lib.pmx_last_error()
        # pmx_prox_table: K other than the context's, an index outside 0 .. PMX_MAX_TABLES - 1, rows that are not element-wise
        assert lib.pmx_prox_table(h, 0, _table(_lib, K - 1), K - 1) == INVALID
        assert lib.pmx_prox_table(h, 0, _table(_lib, K + 1), K + 1) == INVALID
        assert lib.pmx_prox_table(h, -1, _table(_lib, K), K) == INVALID
        assert lib.pmx_prox_table(h, _lib.MAX_TABLES, _table(_lib, K), K) == INVALID
        for bad in ("unity", "unity_plus", "components"):
            rows = _table(_lib, K)
            rows[K - 1].op = _lib.PROX[bad]
            assert lib.pmx_prox_table(h, 0, rows, K) == INVALID, bad
            assert b"element-wise" in lib.pmx_last_error()
        rows = _table(_lib, K)
        rows[0].op = 13
        assert lib.pmx_prox_table(h, 0, rows, K) == INVALID
        assert apply(_names_table(_lib, 1)) == INVALID                      # none of those calls made a table
        # a table that exists; its neighbours still do not
        assert lib.pmx_prox_table(h, 1, _table(_lib, K), K) == 0
        assert apply(_names_table(_lib, 2)) == 0
        assert apply(_names_table(_lib, 1)) == INVALID and apply(_names_table(_lib, 3)) == INVALID
        assert apply(_names_table(_lib, _lib.MAX_TABLES)) == INVALID         # the last slot: valid index, never set
        assert apply(_names_table(_lib, 0)) == INVALID                      # no table at all
        assert apply(_names_table(_lib, 2, unit=1)) == INVALID              # along the rows
        assert apply(_names_table(_lib, _lib.MAX_TABLES + 1)) == UNSUPPORTED  # more tables than a context has
        # the solvers' begin calls answer the same way
        p = _lib.PgmParams()
        p.prox[0], p.prox[1] = _names_table(_lib, 2), _names_table(_lib, 3)
        p.e_rel[0] = p.e_rel[1] = 1e-6
        p.step_scale = 1.0
        assert lib.pmx_pgm_begin(h, C.byref(p)) == INVALID
        b = _lib.BsdmmParams()
        b.prox_f[0], b.prox_f[1] = _names_table(_lib, 2), _names_table(_lib, _lib.MAX_TABLES + 1)
        assert lib.pmx_bsdmm_begin(h, C.byref(b)) == UNSUPPORTED
        with pytest.raises(NotImplementedError):
            _lib.check(UNSUPPORTED)
        a = _lib.AdaproxParams()
        a.prox[0], a.prox[1] = _names_table(_lib, 2), _names_table(_lib, 1)
        a.b2, a.eps, a.p, a.prox_max_iter = 0.999, 1e-8, 0.25, 10
        assert lib.pmx_adaprox_begin(h, C.byref(a), 0) == INVALID
        # the factors are what they were after the one call that ran: soft thresholds 0.1 (k + 1), absolute
        got = dev.get_factors()[0]
        want = pm.operators.prox_soft(A0.copy(), 1.0, thresh=0.1 * (np.arange(K) + 1), type="absolute")
        _same(got, want, "the one application that was accepted")
    # the context-free entry point: tables counted against `ntables`
    X = np.ones((4, K), np.float32)
    call = lambda q, tab, n: lib.pmx_prox_array_tables(0, _vp(X), 4, K, C.byref(q), _vp(sk), tab, n)
    assert call(_names_table(_lib, 1), None, 0) == INVALID
    assert call(_names_table(_lib, 2), _table(_lib, K), 1) == INVALID
    assert call(_names_table(_lib, 1), _table(_lib, K), _lib.MAX_TABLES + 1) == INVALID
    assert call(_names_table(_lib, 1, unit=1), _table(_lib, K), 1) == INVALID
    rows = _table(_lib, K)
    rows[2].op = _lib.PROX["unity"]
    assert call(_names_table(_lib, 1), rows, 1) == INVALID
    assert np.array_equal(X, np.ones((4, K), np.float32))
    assert call(_names_table(_lib, 1), _table(_lib, K), 1) == 0
    assert np.array_equal(X, np.broadcast_to(np.float32(1.0) - (0.1 * (np.arange(K) + 1)).astype(np.float32), (4, K)))
