"""nmf.nmf_batch on the device: every problem of a batch gets the bits of its single nmf() call, stops where that call and the fp64
oracle stop, whatever the number of workgroups and the order of the batch, and whatever a neighbour does.

Inputs are oracle.nmf_oracle.synthetic_problem(M, N, K, dtype=np.float32, seed=1234).  The shapes are the smallest that reach each thing that
can go wrong (tiles of grad_small_tile are 16 rows x 256 columns):
    33 x 47 x 3     three row tiles, the last with one row; the fixtures' ragged shape
    17 x 300 x 5    two column tiles, so two gA slabs
    5 x 600 x 2     fewer rows than a tile; three column tiles
    40 x 257 x 9    the KM = 16 bucket, one column into a second tile
    16 x 256 x 16   exact tile, K at its limit
    8 x 40 x 8      KM = 8 full
    100 x 50 x 3    the reference's example size
"""
import hashlib
import os
import subprocess
import sys
from functools import lru_cache, partial

import numpy as np
import pytest

from oracle import nmf_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(33, 47, 3), (17, 300, 5), (5, 600, 2), (40, 257, 9), (16, 256, 16), (8, 40, 8), (100, 50, 3)]
RTOL, ATOL = 2e-4, 2e-5                       # tests/test_gpu_nmf.py: atol is ATOL * max|ref|

# the stopping batches: (shape, iterations the fp64 oracle runs) with e_rel = 1e-2, max_iter = 120
E_REL, MAX_ITER = 1e-2, 120
PGM_STOPS = [((16, 256, 16), 13), ((40, 257, 9), 73), ((33, 47, 3), 120), ((5, 600, 2), 120), ((100, 50, 3), 120)]
FISTA_STOPS = [((33, 47, 3), 30), ((16, 256, 16), 44), ((40, 257, 9), 55)]
# how near to 1 the test ratio d / (e^2 n) of either block comes over the whole run (fp64 oracle, measured on the CPU)
PGM_NEAREST = {(16, 256, 16): 2.3e-2, (40, 257, 9): 9.8e-3, (33, 47, 3): 229.0, (5, 600, 2): 12.7, (100, 50, 3): 13.4}
FISTA_NEAREST = {(33, 47, 3): 4.8e-2, (16, 256, 16): 2.9e-3, (40, 257, 9): 3.9e-3}
MARGIN = 2e-3


@pytest.fixture(scope="module")
def pm():
    import __graft_entry__ as g
    g.build()
    import proxmin_amd
    return proxmin_amd


@lru_cache(maxsize=None)
def problem(shape, seed=1234):
    out = orc.synthetic_problem(*shape, dtype=np.float32, seed=seed)
    for x in out:
        x.setflags(write=False)
    return out


def half_lipschitz(E0, E1, it, G):
    return tuple(.5 * s for s in orc.lipschitz_steps(E0, E1))


@lru_cache(maxsize=None)
def oracle_run(shape, accelerated, dtype, max_iter=MAX_ITER):
    """-> (converged, iterations, A, S, ratios[it][block]) of the oracle's pgm / FISTA (the latter with half the Lipschitz step) in `dtype`;
    the ratio of the stopping test d / (e^2 n) is formed in fp64 from the iterates"""
    Y, A, S = (x.astype(dtype) for x in problem(shape))
    trace = []
    conv, _, _, n = orc.pgm_nmf(Y, A, S, step=half_lipschitz if accelerated else None, accelerated=accelerated, max_iter=max_iter, e_rel=E_REL, trace=trace)
    pts = trace + [(A.copy(), S.copy())]
    ratios = np.array([[((pts[i + 1][j].astype(np.float64) - pts[i][j]) ** 2).sum() / (E_REL ** 2 * (pts[i + 1][j].astype(np.float64) ** 2).sum()) for j in range(2)]
                       for i in range(n)])
    return tuple(conv), n, A, S, ratios


def single(pm, shape, seed=1234, count=False, **kw):
    """nmf() on one problem alone, library default mode -> (A, S, steps, converged, callbacks)"""
    Y, A0, S0 = problem(shape, seed)
    A, S = A0.copy(), S0.copy()
    calls = []
    if count:
        kw["callback"] = lambda *X, it=None: calls.append(it)
    conv, _, steps = pm.nmf.nmf(Y, A, S, **kw)
    return A, S, steps, conv, len(calls)


def batch_of(shapes, seeds=None):
    ps = [problem(s, 1234 if seeds is None else seeds[i]) for i, s in enumerate(shapes)]
    return [p[0] for p in ps], [p[1].copy() for p in ps], [p[2].copy() for p in ps]


# ---------------------------------------------------------------------------------------------------------------------
# 1. preconditions (CPU): the stopping tests below are decided far from the edge
# ---------------------------------------------------------------------------------------------------------------------
def test_preconditions_of_the_stopping_batches():
    """Facts about the oracle that the stopping tests rest on, measured on the CPU (fp64 / fp32 oracle, e_rel = 1e-2, max_iter = 120):
        pgm     16 x 256 x 16 stops after 13 iterations, ratio never nearer to 1 than 2.3 %;  40 x 257 x 9 after 73, 0.98 %;
                33 x 47 x 3, 5 x 600 x 2, 100 x 50 x 3 run all 120 with ratios >= 230, 13.7, 14.4
        FISTA   (half the Lipschitz step) 33 x 47 x 3 stops after 30, 4.8 %;  16 x 256 x 16 after 44, 0.29 %;  40 x 257 x 9 after 55, 0.39 %
    The fp32 and fp64 oracle ratios differ by 1.6e-6 .. 1.03e-5 relative (the largest at 5 x 600 x 2).  Asserted: |ratio - 1| >= 2e-3 at
    every iteration of every problem, in both precisions, and the two precisions within 1e-4 of each other -- a twentieth of that
    margin, which is what a float32 trajectory needs to decide like the fp64 one."""
    for accelerated, table, nearest in ((False, PGM_STOPS, PGM_NEAREST), (True, FISTA_STOPS, FISTA_NEAREST)):
        for shape, n_want in table:
            c64, n64, _, _, r64 = oracle_run(shape, accelerated, np.float64)
            c32, n32, _, _, r32 = oracle_run(shape, accelerated, np.float32)
            print(shape, "FISTA" if accelerated else "pgm", "iterations", n64, n32, "nearest to 1: %.4g / %.4g" % (np.abs(r64 - 1).min(), np.abs(r32 - 1).min()),
                  "fp32 vs fp64: %.3g" % np.abs(r32 / r64 - 1).max())
            assert n64 == n_want and n32 == n_want
            assert c64 == c32 == ((True, True) if n_want < MAX_ITER else (False, False))
            assert np.abs(r64 - 1).min() >= MARGIN and np.abs(r32 - 1).min() >= MARGIN
            assert np.abs(r64 - 1).min() >= 0.95 * nearest[shape]
            assert np.abs(r32 / r64 - 1).max() <= 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# 2. bit for bit with the single call
# ---------------------------------------------------------------------------------------------------------------------
def _operator_pairs(ops):
    return {"plus": (ops.prox_plus, ops.prox_plus),
            "unity_plus_S": (ops.prox_plus, partial(ops.prox_unity_plus, axis=0)),
            "soft_A_projections_S": (partial(ops.prox_soft, thresh=0.01), ops.AlternatingProjections([partial(ops.prox_unity, axis=0), ops.prox_plus]))}


def _rules(nmf):
    return {"pgm_lipschitz": dict(step=None, accelerated=False),
            "pgm_constant": dict(step=nmf.constant_step(1e-3, 5e-4), accelerated=False),
            "fista_half_lipschitz": dict(step=nmf.scaled_step_pgm(0.5), accelerated=True)}


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["pgm_lipschitz", "pgm_constant", "fista_half_lipschitz"])
@pytest.mark.parametrize("pair", ["plus", "unity_plus_S", "soft_A_projections_S"])
def test_ragged_batch_is_the_single_call_bit_for_bit(pm, pair, rule):
    prox_A, prox_S = _operator_pairs(pm.operators)[pair]
    kw = dict(prox_A=prox_A, prox_S=prox_S, max_iter=6, e_rel=1e-9, **_rules(pm.nmf)[rule])
    Ys, As, Ss = batch_of(SHAPES)
    res = pm.nmf.nmf_batch(Ys, As, Ss, **kw)
    assert res.iterations.tolist() == [6] * len(SHAPES) and not res.converged.any()
    for b, shape in enumerate(SHAPES):
        A, S, steps, conv, _ = single(pm, shape, **kw)
        assert not np.array_equal(A, problem(shape)[1])
        np.testing.assert_array_equal(As[b], A, err_msg="A of %r" % (shape,))
        np.testing.assert_array_equal(Ss[b], S, err_msg="S of %r" % (shape,))
        np.testing.assert_array_equal(res.steps[b], steps, err_msg="steps of %r" % (shape,))


# ---------------------------------------------------------------------------------------------------------------------
# 3. stops where the single call and the oracle stop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("accelerated", [False, True], ids=["pgm", "fista"])
def test_every_problem_stops_where_its_single_call_and_the_oracle_stop(pm, accelerated):
    table = FISTA_STOPS if accelerated else PGM_STOPS
    shapes = [s for s, _ in table]
    kw = dict(max_iter=MAX_ITER, e_rel=E_REL, accelerated=accelerated, step=pm.nmf.scaled_step_pgm(0.5) if accelerated else None)
    Ys, As, Ss = batch_of(shapes)
    res = pm.nmf.nmf_batch(Ys, As, Ss, **kw)
    assert res.iterations.tolist() == [n for _, n in table]
    for b, (shape, n) in enumerate(table):
        conv64, n64, Ao, So, _ = oracle_run(shape, accelerated, np.float64)
        A, S, steps, conv, calls = single(pm, shape, count=True, **kw)
        assert calls == n == n64 == res.iterations[b]
        assert tuple(res.converged[b]) == tuple(conv64) == tuple(conv)
        np.testing.assert_array_equal(As[b], A)
        np.testing.assert_array_equal(Ss[b], S)
        np.testing.assert_array_equal(res.steps[b], steps)
        for got, what in ((A, "single"), (As[b], "batch")):
            np.testing.assert_allclose(got, Ao, rtol=RTOL, atol=ATOL * np.abs(Ao).max(), err_msg="%s A of %r" % (what, shape))
        for got, what in ((S, "single"), (Ss[b], "batch")):
            np.testing.assert_allclose(got, So, rtol=RTOL, atol=ATOL * np.abs(So).max(), err_msg="%s S of %r" % (what, shape))


# ---------------------------------------------------------------------------------------------------------------------
# 4. more problems than workgroups
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_more_problems_than_workgroups_any_grid_any_order(pm):
    B, shape = 600, (8, 40, 2)
    seeds = list(range(B))
    kw = dict(max_iter=3, e_rel=1e-9)
    Ys, As, Ss = batch_of([shape] * B, seeds)
    res = pm.nmf.nmf_batch(Ys, As, Ss, **kw)
    assert res.iterations.tolist() == [3] * B
    _, A3, S3 = batch_of([shape] * B, seeds)
    res3 = pm.nmf.nmf_batch(Ys, A3, S3, max_workgroups=3, **kw)
    _, Ar, Sr = batch_of([shape] * B, seeds)
    resr = pm.nmf.nmf_batch(Ys[::-1], Ar[::-1], Sr[::-1], **kw)
    for b in range(B):
        assert not np.array_equal(As[b], problem(shape, b)[1])
        np.testing.assert_array_equal(A3[b], As[b])
        np.testing.assert_array_equal(S3[b], Ss[b])
        np.testing.assert_array_equal(Ar[b], As[b])
        np.testing.assert_array_equal(Sr[b], Ss[b])
    np.testing.assert_array_equal(res3.steps, res.steps)
    np.testing.assert_array_equal(resr.steps[::-1], res.steps)
    for b in range(7, B, 30):                       # 20 of them
        A, S, steps, _, _ = single(pm, shape, seed=b, **kw)
        np.testing.assert_array_equal(As[b], A)
        np.testing.assert_array_equal(Ss[b], S)
        np.testing.assert_array_equal(res.steps[b], steps)


# ---------------------------------------------------------------------------------------------------------------------
# 5. a problem that turns NaN stays alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_problem_that_turns_nan_stays_alone(pm):
    """a zero row of A under prox_unity_plus along the row (axis=1 on A), Y scaled by -0.1 so that A S - Y > 0 in that row too: its gradient
    is positive, the step makes the row negative, `plus` leaves zeros and the division 0 / 0 (the reference has no guard)"""
    ops = pm.operators
    kw = dict(prox_A=partial(ops.prox_unity_plus, axis=1), max_iter=4, e_rel=1e-3)
    shapes = [(33, 47, 3), (17, 300, 5), (40, 257, 9)]
    Y1, A1, S1 = problem(shapes[1])
    Ysick = (-0.1 * Y1).astype(np.float32)
    Asick = A1.copy()
    Asick[4, :] = 0.0
    Ys, As, Ss = batch_of(shapes)
    Ys[1], As[1] = Ysick, Asick.copy()
    res = pm.nmf.nmf_batch(Ys, As, Ss, **kw)                      # (the launch ends)
    # the sick problem alone
    A, S = Asick.copy(), S1.copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        pm.nmf.nmf(Ysick, A, S, **kw)
    assert np.isnan(A[4]).all()
    np.testing.assert_array_equal(np.isnan(As[1]), np.isnan(A))
    np.testing.assert_array_equal(np.isnan(Ss[1]), np.isnan(S))
    np.testing.assert_array_equal(As[1], A)
    np.testing.assert_array_equal(Ss[1], S)
    assert res.iterations[1] == 4 and not res.converged[1].all()
    for b in (0, 2):
        A, S, steps, conv, _ = single(pm, shapes[b], **kw)
        assert np.isfinite(As[b]).all() and np.isfinite(Ss[b]).all()
        np.testing.assert_array_equal(As[b], A)
        np.testing.assert_array_equal(Ss[b], S)
        np.testing.assert_array_equal(res.steps[b], steps)
        assert tuple(res.converged[b]) == tuple(conv)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the first device call of a process; PMX_DEVICE selects the GPU
# ---------------------------------------------------------------------------------------------------------------------
def _child(device):
    env = dict(os.environ, PMX_DEVICE=str(device), PMX_TORCH_PRELOAD="0")
    return subprocess.run([sys.executable, os.path.join(ROOT, "tests", "nmf_batch_process.py")], env=env, capture_output=True, text=True, timeout=120)


@pytest.mark.gpu
def test_first_call_in_a_fresh_process_and_pmx_device(pm):
    from proxmin_amd import _lib
    shapes = [(33, 47, 3), (40, 257, 9), (8, 40, 8)]
    Ys, As, Ss = batch_of(shapes)
    res = pm.nmf_batch(Ys, As, Ss, max_iter=5, e_rel=1e-9)
    h = hashlib.sha256()
    for x in As + Ss + [res.steps, res.iterations, res.converged]:
        h.update(np.ascontiguousarray(x).tobytes())
    ndev = _lib.load().pmx_device_count()
    last = _child(ndev - 1)                                        # the last GPU there is (the only one: 0)
    assert last.returncode == 0, last.stdout + last.stderr
    assert "digest " + h.hexdigest() in last.stdout
    none = _child(ndev)                                            # one past the last: the variable is what the call goes by
    assert none.returncode == 3 and "PmxError" in none.stdout, none.stdout + none.stderr
