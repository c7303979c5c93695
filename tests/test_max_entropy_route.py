"""CPU: prox_max_entropy (operators.py:163-184) is an operator of this library, so every solver keeps the whole iteration on
the device with it -- no host route, no refusal with device-resident factors.  How it is translated into a device operator
sequence, how it is classified, and -- against the recording stand-in engine of tests/test_host_routes.py -- which device calls
pgm, adaprox and bsdmm make with it."""
from functools import partial

import numpy as np
import pytest

import test_host_routes as thr
from test_device_factors_host import Fake

from proxmin_amd import _lib, algorithms, distributed, nmf as dnmf, operators

ME = 11


def test_the_op_code_and_the_abi_version():
    assert _lib.PROX["max_entropy"] == ME and _lib.ABI_VERSION == 7
    assert "prox_max_entropy" in operators.__all__ and operators._BY_FUNC[operators.prox_max_entropy] == "max_entropy"


@pytest.mark.parametrize("for_solver", [False, True, "pgm"])
@pytest.mark.parametrize("block", [0, 1])
def test_device_proxseq_maps_the_operator(block, for_solver):
    me = operators.prox_max_entropy

    def entry(seq, i=0):
        q = seq.seq[i]
        return (q.op, q.unit, q.thresh, q.relative)

    seq = operators.device_proxseq(me, block, for_solver=for_solver)
    assert (seq.n, seq.repeat) == (1, 1) and entry(seq) == (ME, 0, 1.0, 1)                 # defaults: gamma = 1, relative
    seq = operators.device_proxseq(partial(me, gamma=0.1), block, for_solver=for_solver)
    assert entry(seq) == (ME, 0, 0.1, 1)
    seq = operators.device_proxseq(partial(me, gamma=2.5, type="absolute"), block, for_solver=for_solver)
    assert entry(seq) == (ME, 0, 2.5, 0)
    seq = operators.device_proxseq(partial(me, type="relative"), block, for_solver=for_solver)
    assert entry(seq) == (ME, 0, 1.0, 1)
    ap = operators.AlternatingProjections([operators.prox_plus, partial(me, gamma=0.3, type="absolute")], repeat=2)
    seq = operators.device_proxseq(ap, block, for_solver=for_solver)                        # applied last to first
    assert (seq.n, seq.repeat) == (2, 2) and entry(seq, 0) == (ME, 0, 0.3, 0) and entry(seq, 1)[0] == _lib.PROX["plus"]
    assert not operators.has_long_axis(seq)
    assert not distributed.projection_type(seq)
    assert not distributed.projection_type(operators.device_proxseq(partial(me, type="absolute"), block))


@pytest.mark.parametrize("bad", [dict(thresh=0.1), dict(gamma=1, axis=0), dict(gama=2)])
def test_an_unknown_keyword_is_not_the_librarys_operator(bad):
    with pytest.raises(NotImplementedError):
        operators.device_proxseq(partial(operators.prox_max_entropy, **bad), 0)
    with pytest.raises(NotImplementedError):
        operators.device_proxseq(partial(operators.prox_max_entropy, 0.5), 1)              # positional arguments of a partial


ME_S = partial(operators.prox_max_entropy, gamma=0.1)
ME_ABS = partial(operators.prox_max_entropy, gamma=0.05, type="absolute")
ROUTES = {
    "pgm": lambda c: thr.pgm(c, prox=[thr.PLUS, ME_S]),
    "fista": lambda c: thr.pgm(c, prox=[ME_S, thr.PLUS], accelerated=True),
    "pgm_bt": lambda c: thr.pgm(c, prox=[thr.PLUS, ME_S], backtracking=True, f=c.f()),
    "pgm_ap": lambda c: thr.pgm(c, prox=[thr.PLUS, operators.AlternatingProjections([thr.PLUS, ME_S])]),
    "ada": lambda c: thr.ada(c, prox=[thr.PLUS, ME_ABS]),
    "ada_relative": lambda c: thr.ada(c, prox=[ME_S, thr.PLUS]),
    "bsdmm_prox": lambda c: thr.bsd(c, prox=(thr.PLUS, ME_S)),
    "bsdmm_g": lambda c: thr.bsd(c, proxs_g=[[ME_S], None]),
}
BEGIN = {"pgm": "pgm_begin", "fista": "pgm_begin", "pgm_bt": "pgm_begin", "pgm_ap": "pgm_begin", "ada": "adaprox_begin",
         "ada_relative": "adaprox_begin", "bsdmm_prox": "bsdmm_begin", "bsdmm_g": "bsdmm_begin"}
RUN = {"pgm_begin": "pgm_run", "adaprox_begin": "adaprox_run", "bsdmm_begin": "bsdmm_run"}


@pytest.mark.parametrize("name", sorted(ROUTES))
def test_the_solvers_take_the_fused_route(name, monkeypatch):
    """one *_begin whose sequences name op 11, then runs: no call of a Python callable, nothing put on the device and nothing
    fetched from it between the runs, no host-path warning"""
    monkeypatch.setitem(thr.ROUTES, "max_entropy_" + name, (ROUTES[name], {}))
    T = thr.run_route("max_entropy_" + name, monkeypatch.setattr)
    begins = [t for t in T if t.split(" ")[0].endswith("_begin")]
    assert len(begins) == 1 and begins[0].startswith(BEGIN[name] + " "), T
    assert "%d/0/" % ME in begins[0], begins[0]
    assert "True" not in begins[0].split("host_prox=")[-1].split("]")[0].split(")")[0] or "host_prox" not in begins[0], begins[0]
    head = [t.split(" ")[0] for t in T]
    if name == "pgm_bt":                                   # (the line search is driven trial by trial: its fused form)
        assert "pgm_bt_split" in head or RUN[BEGIN[name]] in head, T
    else:
        assert RUN[BEGIN[name]] in head, T
    last_run = max(i for i, h in enumerate(head) if h in (RUN[BEGIN[name]], "pgm_bt_split"))
    for i, (t, h) in enumerate(zip(T, head)):
        assert h not in ("call", "put", "_upload", "operators._run_rows", "pgm_split", "adaprox_split", "bsdmm_split"), t
        assert h not in ("get", "_download", "get_factors") or i > last_run, t      # (what the solver returns is fetched once, at the end)
        assert not (h == "log" and ("one iteration per call" in t or "user-defined Python callable" in t)), t
        assert not t.startswith("raise "), t
    assert T[-1] == "warned []", T[-1]


def test_the_same_calls_with_the_operator_as_a_user_callable_take_the_host_route(monkeypatch):
    """what the fused route is measured against: a Python function of the same shape is called once per iteration"""
    def user(X, step):
        return X
    monkeypatch.setitem(thr.ROUTES, "max_entropy_user", (lambda c: thr.pgm(c, prox=[thr.PLUS, c.rec("prox", user)]), {}))
    T = thr.run_route("max_entropy_user", monkeypatch.setattr)
    assert any(t.startswith("call prox") for t in T) and any(t.startswith("put ") for t in T)


class _Reached(Exception):
    pass


@pytest.mark.parametrize("algorithm", ["pgm", "adaprox", "bsdmm", "bsdmm_g"])
def test_device_resident_factors_are_not_refused_for_the_operator(algorithm, monkeypatch):
    """with A and S in HBM a user prox is refused before a device is opened (tests/test_device_factors_host.py); the library's
    operator gets as far as opening it (the stand-in raises there: the fake arrays' addresses are never dereferenced)"""
    def opened(*a, **k):
        raise _Reached()
    monkeypatch.setattr(algorithms, "_open_device", opened)
    M, N, K = 6, 9, 2
    A, S = Fake("<f4", (M, K), ptr=1 << 20), Fake("<f4", (K, N), ptr=1 << 21)
    Y = np.ones((M, N), np.float32)
    kw = dict(algorithm={"pgm": algorithms.pgm, "adaprox": algorithms.adaprox}.get(algorithm, algorithms.bsdmm), max_iter=1)
    if algorithm == "bsdmm_g":
        kw["proxs_g"] = [[ME_S], None]
    else:
        kw["prox_S"] = ME_ABS if algorithm == "adaprox" else ME_S
    with pytest.raises(_Reached):
        dnmf.nmf(Y, A, S, **kw)

    def user(X, step):
        return X
    if algorithm == "bsdmm_g":
        kw["proxs_g"] = [[user], None]
    else:
        kw["prox_S"] = user
    with pytest.raises(NotImplementedError, match="prox"):
        dnmf.nmf(Y, A, S, **kw)
