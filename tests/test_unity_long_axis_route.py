"""CPU: which calls keep prox_unity* along a factor's long axis (axis=0 on A, axis=1 on S) on the device.

pgm / FISTA take such a sequence into their update chain (csrc/k_update.hip: k_pgm_unity) when nothing else of the call needs
the host; every other route -- adaprox, bsdmm, pgm with a line search, a user grad / step, or a user prox on the other block --
is the one it was: the operator is a host prox of its block (one iteration per call, one-time warning)."""
import logging
import os
import sys
from functools import partial

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as g
    g.build()
    from proxmin_amd import algorithms, operators
    return algorithms, operators


def _long_ops(ops):
    """(prox, block, long-axis entries per period, repeat)"""
    return [
        (ops.prox_unity, 0, 1, 1),                                           # axis=0 is the operator's default
        (partial(ops.prox_unity_plus, axis=0), 0, 1, 1),
        (partial(ops.prox_unity_plus, axis=1), 1, 1, 1),
        (ops.AlternatingProjections([partial(ops.prox_unity_plus, axis=1), partial(ops.prox_hard, thresh=0.1, type="absolute")]), 1, 1, 1),
        (ops.AlternatingProjections([partial(ops.prox_unity, axis=0), partial(ops.prox_unity, axis=1), ops.prox_plus], repeat=2), 0, 1, 2),
    ]


def test_device_proxseq_per_solver(mods):
    alg, ops = mods
    for prox, block, nlong, repeat in _long_ops(ops):
        plain = ops.device_proxseq(prox, block)
        assert ops.has_long_axis(plain)
        assert sum(plain.seq[i].unit != 0 for i in range(plain.n)) == nlong and plain.repeat == repeat
        with pytest.raises(ops.NotFusable):
            ops.device_proxseq(prox, block, for_solver=True)
        s = ops.device_proxseq(prox, block, for_solver="pgm")
        assert bytes(s) == bytes(plain)
    # the short axis is fused everywhere, and is no long-axis sequence
    for prox, block in ((partial(ops.prox_unity_plus, axis=1), 0), (ops.prox_unity, 1), (ops.prox_plus, 0), (None, 1)):
        for mode in (True, "pgm"):
            assert not ops.has_long_axis(ops.device_proxseq(prox, block, for_solver=mode))
    # a user callable is no device sequence for any solver
    for mode in (False, True, "pgm"):
        with pytest.raises(NotImplementedError) as e:
            ops.device_proxseq(lambda X, s: X, 0, for_solver=mode)
        assert not isinstance(e.value, ops.NotFusable)


def _route(alg, prox, host_route):
    long_axis = []
    seqs, host = alg._split_prox(prox, none_is_id=True, long_axis=long_axis)
    fused = alg._fuse_long_axis(seqs, host, long_axis, host_route=host_route)
    return fused, seqs, host


def test_pgm_route_against_every_other(mods, caplog):
    alg, ops = mods
    uA, uS = partial(ops.prox_unity_plus, axis=0), partial(ops.prox_unity, axis=1)

    def user(X, s):
        return X

    saved = set(alg._warned)
    try:
        _check_routes(alg, ops, uA, uS, user, caplog)
    finally:
        alg._warned.clear()
        alg._warned.update(saved)


def _check_routes(alg, ops, uA, uS, user, caplog):
    with caplog.at_level(logging.WARNING, logger="proxmin"):
        # pgm, nothing else on the host: the sequences go to the device whole, no warning
        alg._warned.clear()
        for prox in ((uA, ops.prox_plus), (None, uS), (uA, uS)):
            fused, seqs, host = _route(alg, prox, host_route=False)
            assert fused and host == [None, None]
            assert [ops.has_long_axis(s) for s in seqs] == [p in (uA, uS) for p in prox]
        assert not caplog.records
        # no long-axis operator: nothing changes, nothing is fused "long"
        fused, seqs, host = _route(alg, (ops.prox_plus, partial(ops.prox_unity_plus, axis=0)), host_route=False)
        assert not fused and host == [None, None] and not any(ops.has_long_axis(s) for s in seqs)
        assert not caplog.records
        # a user grad / step or the line search (host_route), or a user prox on the other block: the host route, with its warning
        for prox, host_route in (((uA, ops.prox_plus), True), ((uA, user), False), ((user, uS), False), ((uA, uS), True)):
            alg._warned.clear()
            caplog.clear()
            fused, seqs, host = _route(alg, prox, host_route=host_route)
            assert not fused
            assert [h is not None for h in host] == [p in (uA, uS, user) for p in prox]
            assert not any(ops.has_long_axis(s) for s in seqs)              # the device slot of a host block is prox_id
            msgs = [r.getMessage() for r in caplog.records if "one iteration per call" in r.getMessage()]
            assert len(msgs) == sum(p in (uA, uS) for p in prox), msgs
        # adaprox and bsdmm call _split_prox as before: a host prox and the warning, whatever else the call holds
        alg._warned.clear()
        caplog.clear()
        seqs, host = alg._split_prox((uA, ops.prox_plus), none_is_id=False)
        assert host[0] is uA and host[1] is None and seqs[0].n == 0
        assert sum("one iteration per call" in r.getMessage() for r in caplog.records) == 1
