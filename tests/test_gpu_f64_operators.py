"""GPU: every operator of proxmin.operators (operators.py:20-160) in fp64, through every instantiation of the fp64 update kernels.

The eleven op-codes run inside pgm on either block, with a relative and an absolute threshold where the operator has one; the
thresholded ones and a two-entry AlternatingProjections run inside adaprox's proximal sub-iterations (per-component steps) and
as bsdmm constraints.  Shapes are the smallest that select each instantiation: 33 x 47 x 3 and 40 x 56 x 12 take the
small-problem kernels (k_small_f64.hip: 8 / 16 lanes per row in the single-workgroup adaprox / bsdmm kernels), K = 20, 40, 100
the kernels of k_big_f64.hip with 1, 2, 4 values per lane.  prox_unity* runs along the short axis only (the long axis is
k_pgm_unity's: tests/test_gpu_unity_long_axis.py).

Everything is compared with the fp64 oracle at the tolerances the fp64 suites use for these routes (test_gpu_f64.py: RTOL;
test_gpu_f64_big.py: _close).  Thresholds sit inside the bulk of the data, and every case first checks ON THE ORACLE'S RESULT
that both outcomes of the operator's branch occur (some entries at the operator's fixed value, some not)."""
from functools import partial

import numpy as np
import pytest

from test_gpu_f64 import RTOL as RTOL_SMALL
from test_gpu_f64_big import _close as _close_big

pytestmark = pytest.mark.gpu

SMALL = [(33, 47, 3), (40, 56, 12)]
BIG = [(40, 56, 20), (48, 72, 40), (128, 160, 100)]
SHAPES = SMALL + BIG

# (operator, threshold type, the threshold's value in data units); a relative threshold is this value divided by the step the
# solver starts with, so that threshold x step lands in the bulk of the factors (entries of order 0.1 .. 1) at every shape
PGM_OPS = [("id",), ("zero",), ("plus",), ("unity",), ("unity_plus",)] + [
    (name, kind, t) for name, t in (("min", 0.3), ("max", 0.6), ("hard", 0.3), ("hard_plus", 0.3), ("soft", 0.2), ("soft_plus", 0.2))
    for kind in ("relative", "absolute")]
ADA_OPS = [("soft", "relative", 0.05), ("hard_plus", "relative", 0.2), ("min", "absolute", 0.3), ("max", "absolute", 0.6), ("seq",)]
BSDMM_OPS = [("soft", "relative", 0.2), ("max", "absolute", 0.6)]


def _id(case):
    return "-".join(str(x) for x in case[:2])


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


def _close(shape, got, want, name="", loose=False):
    """factors and Z at the route's tolerance; `loose`: the scaled dual variables U, as the two suites compare them"""
    if shape in SMALL:
        if loose:
            np.testing.assert_allclose(got, want, rtol=1e-8, atol=1e-13, err_msg=name)
        else:
            np.testing.assert_allclose(got, want, rtol=RTOL_SMALL, atol=1e-14, err_msg=name)
    elif loose:
        _close_big(got, want, rtol=1e-7, name=name)
    else:
        _close_big(got, want, name=name)


def _kernel(shape):
    return "k64_front" if shape in SMALL else "k64_grad_pass"


def make_spec(case, j, step0):
    """oracle prox spec of `case` on block j (0 = A, 1 = S); step0: the step the solver starts with on that block"""
    if case[0] in ("id", "zero", "plus"):
        return (case[0],)
    if case[0] in ("unity", "unity_plus"):
        return (case[0], 1 - j)                              # the short axis: A's rows, S's columns
    if case[0] == "seq":
        return ("seq", [("plus",), ("unity", 1 - j)], 2)
    name, kind, t = case
    return (name, t / step0 if kind == "relative" else t, kind)


def to_prox(pm, spec):
    ops = pm.operators
    if spec[0] == "seq":
        return ops.AlternatingProjections([to_prox(pm, s) for s in spec[1]], repeat=spec[2])
    fn = getattr(ops, "prox_" + spec[0])
    if spec[0] in ("unity", "unity_plus"):
        return partial(fn, axis=spec[1])
    if len(spec) > 1:
        return partial(fn, thresh=spec[1], type=spec[2])
    return fn


def both_outcomes(X, spec, step=None):
    """Did the operator's branch go both ways on this (oracle) result, the output of the operator's last application?  Entries
    the operator moved sit at its fixed value (0, or the threshold of prox_min / prox_max); operators without a branch per
    entry have nothing to check.  The callers ask after 1, 2, .. iterations: a threshold may stop biting as the run settles."""
    name = spec[0]
    if name in ("id", "zero", "unity", "seq"):
        return True
    if name in ("min", "max"):
        t = spec[1] * step if spec[2] == "relative" else spec[1]
        hit = X == t
    else:
        hit = X == 0
    return bool(0 < hit.sum() < hit.size)


@pytest.mark.parametrize("case", PGM_OPS, ids=_id)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_fp64_pgm_every_operator_on_either_block(pm, orc, monkeypatch, M, N, K, case):
    from test_gpu_f64_big import _spy
    seen = _spy(monkeypatch)
    shape = (M, N, K)
    Y, A0, S0 = orc.synthetic_problem(M, N, K, np.float64, seed=M + N + K)
    steps0 = orc.lipschitz_steps(A0, S0)
    its = 1 if case[0] == "zero" else 3                     # (after prox_zero the other block's Lipschitz step is 1 / 0)
    for j in range(2):
        specs = [("plus",), ("plus",)]
        specs[j] = make_spec(case, j, steps0[j])
        fired = False
        for n in range(1, its + 1):                         # (the last run is the one the device is compared with)
            Ao, So = A0.copy(), S0.copy()
            oret = orc.pgm_nmf(Y, Ao, So, prox_A=specs[0], prox_S=specs[1], max_iter=n, e_rel=1e-9)
            fired |= both_outcomes((Ao, So)[j], specs[j], oret[2][j])
        assert fired, "the threshold of %r misses the data on block %d" % (specs[j], j)
        del seen[:]
        A, S = A0.copy(), S0.copy()
        conv, G, steps = pm.nmf.nmf(Y, A, S, prox_A=to_prox(pm, specs[0]), prox_S=to_prox(pm, specs[1]), max_iter=its, e_rel=1e-9)
        assert seen == [("f64", _kernel(shape))], seen
        assert A.dtype == np.float64
        _close(shape, A, Ao, "%r on block %d: A" % (case, j))
        _close(shape, S, So, "%r on block %d: S" % (case, j))
        assert tuple(conv) == tuple(oret[0])


@pytest.mark.parametrize("case", ADA_OPS, ids=_id)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_fp64_adaprox_operators_in_the_proximal_loop(pm, orc, M, N, K, case):
    """the operator on S next to prox_plus on A: per-component steps gamma (algorithms.py:384) reach a relative threshold, the
    row sums of the sequence run in every pass; pass counts equal to the oracle's"""
    from proxmin_amd.engine import DeviceNMF
    ops = pm.operators
    shape = (M, N, K)
    its, e_rel = 4, 1e-4
    Y, A0, S0 = orc.synthetic_problem(M, N, K, np.float64, seed=M + N + K)
    # gamma of the first iteration: alpha / max Psi, Psi = sqrt((1 - b2) G^2) (amsgrad, algorithms.py:170-180)
    gamma0 = float(np.mean(orc.adaprox_steps(A0, S0)[1])) / (np.sqrt(1e-3) * np.abs(orc.residual_gradients(A0, S0, Y)[1]).max())
    spec = make_spec(case, 1, gamma0)
    fired = False
    for n in range(1, its + 1):                             # (the last run is the one the device is compared with)
        Ao, So = A0.copy(), S0.copy()
        out = orc.adaprox_nmf(Y, Ao, So, ("plus",), spec, scheme="amsgrad", max_iter=n, e_rel=e_rel, check_convergence=False)
        fired |= both_outcomes(So, spec)
    assert fired, "the threshold of %r misses the data" % (spec,)
    with DeviceNMF(M, N, K, mode="f64") as dev:
        assert dev.k1_info()["kernel"] == _kernel(shape)
        dev.set_Y(Y)
        dev.set_factors(A0, S0)
        dev.adaprox_begin([ops.device_proxseq(ops.prox_plus, 0), ops.device_proxseq(to_prox(pm, spec), 1)],
                          scheme="amsgrad", check_convergence=False, e_rel=(e_rel, e_rel))
        res = dev.adaprox_run(np.full(its, 0.9), 0.9)
        A, S = dev.get_factors()
    got = [int(res.sub_iterations[0]), int(res.sub_iterations[1])]
    assert res.iterations == its and got == [int(out[5][0]), int(out[5][1])], (got, out[5])
    _close(shape, A, Ao, "%r: A" % (case,))
    _close(shape, S, So, "%r: S" % (case,))


@pytest.mark.parametrize("case", BSDMM_OPS, ids=_id)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_fp64_bsdmm_operators_as_constraints(pm, orc, M, N, K, case):
    """one constraint per block with prox_f = prox_plus; X, Z and U against the oracle's"""
    from proxmin_amd import _lib
    from proxmin_amd.engine import DeviceNMF
    ops = pm.operators
    shape = (M, N, K)
    its = 4
    Y, A0, S0 = orc.synthetic_problem(M, N, K, np.float64, seed=M + N + K)
    steps0 = orc.lipschitz_steps(A0, S0)
    specs = [make_spec(case, j, 2.0 * steps0[j]) for j in range(2)]      # step_g = 2 n_g step_f (utils.py:269-279)
    fired = [False, False]
    for n in range(1, its + 1):                                            # (the last run is the one the device is compared with)
        Ao, So = A0.copy(), S0.copy()
        state = {}
        orc.bsdmm_nmf(Y, Ao, So, proxs_g=[[specs[0]], [specs[1]]], max_iter=n, e_rel=1e-9, state=state)
        for j in range(2):
            fired[j] |= both_outcomes(state["Z"][j][0], specs[j])
    assert all(fired), "the threshold of %r misses the data (%r)" % (case, fired)
    with DeviceNMF(M, N, K, mode="f64") as dev:
        assert dev.k1_info()["kernel"] == _kernel(shape)
        dev.set_Y(Y)
        dev.set_factors(A0, S0)
        dev.bsdmm_begin([ops.device_proxseq(ops.prox_plus, j) for j in range(2)],
                        [[ops.device_proxseq(to_prox(pm, specs[j]), j)] for j in range(2)], e_rel=(1e-9, 1e-9), e_abs=(0.0, 0.0))
        dev.bsdmm_run(its)
        A, S = dev.get_factors()
        Z = [dev._download(_lib.BUF_Z0 + j * _lib.MAX_G, (M, N)[j]) for j in range(2)]
        U = [dev._download(_lib.BUF_U0 + j * _lib.MAX_G, (M, N)[j]) for j in range(2)]
    _close(shape, A, Ao, "%r: A" % (case,))
    _close(shape, S, So, "%r: S" % (case,))
    _close(shape, Z[0], state["Z"][0][0], "Z_A")
    _close(shape, U[0], state["U"][0][0], "U_A", loose=True)
    _close(shape, Z[1].T, state["Z"][1][0], "Z_S")
    _close(shape, U[1].T, state["U"][1][0], "U_S", loose=True)
