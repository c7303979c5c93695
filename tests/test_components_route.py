"""CPU: per-component operator parameters -- an array `thresh` / `gamma` on the threshold operators, and prox_components
(operators.py:87-103) -- are ONE device mechanism: a sequence entry PMX_PROX_COMPONENTS (op 12) whose table holds one
(op, thresh, relative) row per component.  How the callables are translated, which shapes and members are refused (and
how), and -- against the recording stand-in engine of tests/test_host_routes.py -- which device calls the solvers make."""
from functools import partial

import numpy as np
import pytest

import test_host_routes as thr
from test_device_factors_host import Fake

from proxmin_amd import _lib, algorithms, distributed, nmf as dnmf, operators

OP = 12
P = _lib.PROX
THRESH_OPS = {"min": operators.prox_min, "max": operators.prox_max, "hard": operators.prox_hard, "hard_plus": operators.prox_hard_plus,
              "soft": operators.prox_soft, "soft_plus": operators.prox_soft_plus, "max_entropy": operators.prox_max_entropy}


def _kw(name, value):
    return {"gamma" if name == "max_entropy" else "thresh": value}


def test_the_op_code_the_symbols_and_the_unchanged_abi():
    assert P["components"] == OP and _lib.ABI_VERSION == 7 and _lib.MAX_TABLES >= 8
    assert {"pmx_prox_table", "pmx_prox_array_tables"} <= set(_lib.EXPORTED_SYMBOLS)
    assert "prox_components" in operators.__all__ and operators._BY_FUNC[operators.prox_components] == "components"
    import ctypes
    assert ctypes.sizeof(_lib.Prox) == 24


@pytest.mark.parametrize("kind", ["relative", "absolute"])
@pytest.mark.parametrize("name", sorted(THRESH_OPS))
def test_an_array_threshold_becomes_a_table_whose_rows_share_the_op(name, kind):
    t = np.array([0.5, 0.25, 2.0])
    for block, shapes in ((0, [(3,), (1, 3)]), (1, [(3, 1)])):
        for shape in shapes:
            for for_solver in (False, True, "pgm"):
                seq = operators.device_proxseq(partial(THRESH_OPS[name], type=kind, **_kw(name, t.reshape(shape))), block, for_solver=for_solver)
                q = seq.seq[0]
                assert (seq.n, seq.repeat, q.op, q.unit, q.reserved) == (1, 1, OP, 0, 1)
                assert len(seq.tables) == 1
                assert operators.table_rows(seq.tables[0]) == [(P[name], float(v), int(kind == "relative")) for v in t]
                assert all(r.unit == 0 and r.reserved == 0 for r in seq.tables[0])
                assert operators.has_tables(seq) and not operators.has_long_axis(seq)
                assert not distributed.projection_type(seq)


@pytest.mark.parametrize("name", sorted(THRESH_OPS))
def test_a_size_one_array_is_the_scalar_byte_for_byte(name):
    for block in (0, 1):
        want = operators.device_proxseq(partial(THRESH_OPS[name], **_kw(name, 0.3)), block)
        for arr in (np.array(0.3), np.array([0.3]), np.array([[0.3]])):
            got = operators.device_proxseq(partial(THRESH_OPS[name], **_kw(name, arr)), block)
            assert bytes(got) == bytes(want) and not operators.seq_tables(got)


@pytest.mark.parametrize("block,shape", [(0, (3, 1)), (0, (5, 3)), (0, (2, 1, 3)), (1, (3,)), (1, (1, 3)), (1, (3, 7))])
def test_per_row_and_per_element_thresholds_raise_and_name_the_shape(block, shape):
    for name in sorted(THRESH_OPS):
        with pytest.raises(NotImplementedError) as info:
            operators.device_proxseq(partial(THRESH_OPS[name], **_kw(name, np.ones(shape))), block)
        assert type(info.value) is NotImplementedError                       # (not NotFusable: the host route of a user prox)
        assert str(shape) in str(info.value)


MEMBERS = [partial(operators.prox_soft, thresh=0.5), operators.prox_plus, partial(operators.prox_max_entropy, gamma=0.1, type="absolute"),
           operators.prox_id, partial(operators.prox_hard_plus, thresh=2.0, type="absolute"), operators.prox_zero,
           partial(operators.prox_min, thresh=-1.0), partial(operators.prox_max, thresh=3.0, type="absolute")]
MEMBER_ROWS = [(P["soft"], 0.5, 1), (P["plus"], 0.0, 0), (P["max_entropy"], 0.1, 0), (P["id"], 0.0, 0), (P["hard_plus"], 2.0, 0),
               (P["zero"], 0.0, 0), (P["min"], -1.0, 1), (P["max"], 3.0, 0)]


@pytest.mark.parametrize("block", [0, 1])
def test_prox_components_with_mixed_members(block):
    axis = 1 if block == 0 else 0
    for for_solver in (False, True, "pgm"):
        seq = operators.device_proxseq(partial(operators.prox_components, prox=MEMBERS, axis=axis), block, for_solver=for_solver)
        assert (seq.n, seq.seq[0].op, seq.seq[0].unit, seq.seq[0].reserved) == (1, OP, 0, 1)
        assert operators.table_rows(seq.tables[0]) == MEMBER_ROWS
        assert not distributed.projection_type(seq)
    # one callable for every component is that operator
    seq = operators.device_proxseq(partial(operators.prox_components, prox=MEMBERS[0], axis=axis), block)
    assert bytes(seq) == bytes(operators.device_proxseq(MEMBERS[0], block))


def test_prox_components_inside_alternating_projections_is_reversed_like_the_others():
    pc = partial(operators.prox_components, prox=MEMBERS[:2], axis=0)
    soft = partial(operators.prox_soft, thresh=np.array([[0.1], [0.2]]))
    ap = operators.AlternatingProjections([operators.prox_plus, pc, partial(operators.prox_unity, axis=0), soft], repeat=3)
    seq = operators.device_proxseq(ap, 1)
    assert (seq.n, seq.repeat) == (4, 3)
    assert [seq.seq[i].op for i in range(4)] == [OP, P["unity"], OP, P["plus"]]          # applied last to first
    assert [seq.seq[i].reserved for i in range(4)] == [1, 0, 2, 0]
    assert operators.table_rows(seq.tables[0]) == [(P["soft"], 0.1, 1), (P["soft"], 0.2, 1)]
    assert operators.table_rows(seq.tables[1]) == MEMBER_ROWS[:2]


def _user(X, step):
    return X


@pytest.mark.parametrize("block,bad", [
    (0, dict(prox=MEMBERS[:2], axis=0)), (1, dict(prox=MEMBERS[:2], axis=1)), (0, dict(prox=MEMBERS[:2])),      # the other axis (default 0 on A)
    (1, dict(prox=[operators.prox_plus, _user], axis=0)),                                                         # a user member
    (1, dict(prox=[operators.prox_plus, partial(operators.prox_unity, axis=0)], axis=0)),                         # a unity member
    (1, dict(prox=[operators.prox_plus, operators.AlternatingProjections([operators.prox_plus])], axis=0)),       # nested compositions
    (1, dict(prox=[operators.prox_plus, partial(operators.prox_components, prox=[operators.prox_plus], axis=0)], axis=0)),
    (1, dict(prox=[operators.prox_plus, partial(operators.prox_soft, thresh=np.array([[1.0], [2.0]]))], axis=0)),   # a member with a table of its own
    (1, dict(prox=[operators.prox_plus, partial(operators.prox_soft, 0.5)], axis=0)),                             # positional arguments
])
def test_what_is_not_fused_is_a_plain_not_implemented_error(block, bad):
    for wrap in (lambda q: q, lambda q: operators.AlternatingProjections([operators.prox_plus, q])):
        for for_solver in (False, True, "pgm"):
            with pytest.raises(NotImplementedError) as info:
                operators.device_proxseq(wrap(partial(operators.prox_components, **bad)), block, for_solver=for_solver)
            assert type(info.value) is NotImplementedError
    with pytest.raises(NotImplementedError):
        operators.device_proxseq(operators.prox_components, block)                                                # bare: no members


# -- the Python body: the contract on host arrays, arbitrary callables --------------------------------------------------------
def test_the_python_body_gives_component_k_its_own_callable_and_its_own_step():
    seen = []

    def member(tag):
        def f(X, step):
            seen.append((tag, np.array(X), np.array(step)))
            return X * tag
        return f
    X = np.arange(6, dtype=np.float64).reshape(2, 3)
    out = operators.prox_components(X.copy(), 0.5, prox=[member(2), member(3)], axis=0)
    assert np.array_equal(out, X * np.array([[2.0], [3.0]])) and [s[0] for s in seen] == [2, 3]
    assert all(s[2].ndim == 0 and s[2] == 0.5 for s in seen) and np.array_equal(seen[1][1], X[1])
    del seen[:]
    out = operators.prox_components(X.copy(), np.array([0.1, 0.2, 0.3]), prox=[member(1), member(2), member(4)], axis=1)
    assert np.array_equal(out, X * np.array([1.0, 2.0, 4.0])) and [float(s[2]) for s in seen] == [0.1, 0.2, 0.3]
    del seen[:]
    out = operators.prox_components(X.copy(), np.array([[0.1], [0.2]]), prox=member(5), axis=0)            # one callable: every component
    assert np.array_equal(out, X * 5) and [float(s[2]) for s in seen] == [0.1, 0.2]
    with pytest.raises(ValueError):
        operators.prox_components(X.copy(), 0.5, prox=[member(2)] * 3, axis=0)


# -- routes -----------------------------------------------------------------------------------------------------------------
K = thr.K
SOFT_S = partial(operators.prox_soft, thresh=np.linspace(0.01, 0.02, K).reshape(K, 1))
SOFT_A = partial(operators.prox_soft, thresh=np.linspace(0.01, 0.02, K), type="absolute")
HARD_ABS_S = partial(operators.prox_hard, thresh=np.linspace(0.01, 0.02, K).reshape(K, 1), type="absolute")
MIX = [partial(operators.prox_soft_plus, thresh=0.01), operators.prox_plus, partial(operators.prox_max_entropy, gamma=0.1)]
COMP_S = partial(operators.prox_components, prox=[MIX[k % 3] for k in range(K)], axis=0)
COMP_A = partial(operators.prox_components, prox=[MIX[(k + 1) % 3] for k in range(K)], axis=1)
ROUTES = {
    "pgm": lambda c: thr.pgm(c, prox=[thr.PLUS, SOFT_S]),
    "pgm_components": lambda c: thr.pgm(c, prox=[COMP_A, COMP_S]),
    "fista": lambda c: thr.pgm(c, prox=[SOFT_A, thr.PLUS], accelerated=True),
    "pgm_bt": lambda c: thr.pgm(c, prox=[thr.PLUS, COMP_S], backtracking=True, f=c.f()),
    "pgm_ap": lambda c: thr.pgm(c, prox=[thr.PLUS, operators.AlternatingProjections([thr.PLUS, COMP_S])]),
    "ada": lambda c: thr.ada(c, prox=[thr.PLUS, HARD_ABS_S]),
    "ada_relative": lambda c: thr.ada(c, prox=[COMP_A, SOFT_S]),
    "bsdmm_prox": lambda c: thr.bsd(c, prox=(thr.PLUS, SOFT_S)),
    "bsdmm_g": lambda c: thr.bsd(c, proxs_g=[[COMP_A], None]),
}
BEGIN = {"ada": "adaprox_begin", "ada_relative": "adaprox_begin", "bsdmm_prox": "bsdmm_begin", "bsdmm_g": "bsdmm_begin"}
RUN = {"pgm_begin": "pgm_run", "adaprox_begin": "adaprox_run", "bsdmm_begin": "bsdmm_run"}


@pytest.mark.parametrize("name", sorted(ROUTES))
def test_the_solvers_take_the_fused_route(name, monkeypatch):
    """one *_begin whose sequences name op 12, then runs: no call of a Python callable, nothing put on the device and nothing
    fetched from it between the runs, no host-path warning -- with the stand-in engine unchanged (it knows no table call)"""
    monkeypatch.setitem(thr.ROUTES, "components_" + name, (ROUTES[name], {}))
    T = thr.run_route("components_" + name, monkeypatch.setattr)
    begin = BEGIN.get(name, "pgm_begin")
    begins = [t for t in T if t.split(" ")[0].endswith("_begin")]
    assert len(begins) == 1 and begins[0].startswith(begin + " "), T
    assert "%d/0/" % OP in begins[0], begins[0]
    head = [t.split(" ")[0] for t in T]
    if name == "pgm_bt":
        assert "pgm_bt_split" in head or RUN[begin] in head, T
    else:
        assert RUN[begin] in head, T
    last_run = max(i for i, h in enumerate(head) if h in (RUN[begin], "pgm_bt_split"))
    for i, (t, h) in enumerate(zip(T, head)):
        assert h not in ("call", "put", "_upload", "operators._run_rows", "pgm_split", "adaprox_split", "bsdmm_split"), t
        assert h not in ("get", "_download", "get_factors") or i > last_run, t
        assert not (h == "log" and ("one iteration per call" in t or "user-defined Python callable" in t)), t
        assert not t.startswith("raise "), t
    assert T[-1] == "warned []", T[-1]


def test_prox_components_with_a_user_member_takes_the_host_route(monkeypatch):
    def route(c):
        members = [thr.PLUS] * (K - 1) + [c.rec("member", lambda X, step: np.maximum(X, 0))]
        return thr.pgm(c, prox=[thr.PLUS, partial(operators.prox_components, prox=members, axis=0)])
    monkeypatch.setitem(thr.ROUTES, "components_user", (route, {}))
    T = thr.run_route("components_user", monkeypatch.setattr)
    assert any(t.startswith("call member") for t in T) and any(t.startswith("put ") for t in T), T
    assert any(t.startswith("log WARNING") and "user-defined Python callable" in t for t in T), T
    assert not any(t.startswith("raise ") for t in T), T


class _Reached(Exception):
    pass


def _opened(*a, **k):
    raise _Reached()


@pytest.mark.parametrize("what", ["thresh", "components"])
@pytest.mark.parametrize("algorithm", ["pgm", "adaprox", "bsdmm", "bsdmm_g"])
def test_device_resident_factors_are_not_refused_for_these_operators(algorithm, what, monkeypatch):
    monkeypatch.setattr(algorithms, "_open_device", _opened)
    M, N, Kf = 6, 9, 2
    A, S = Fake("<f4", (M, Kf), ptr=1 << 20), Fake("<f4", (Kf, N), ptr=1 << 21)
    Y = np.ones((M, N), np.float32)
    kw = dict(algorithm={"pgm": algorithms.pgm, "adaprox": algorithms.adaprox}.get(algorithm, algorithms.bsdmm), max_iter=1)
    on_S = (partial(operators.prox_soft, thresh=np.array([[0.1], [0.2]]), type="absolute" if algorithm == "adaprox" else "relative")
            if what == "thresh" else partial(operators.prox_components, prox=[operators.prox_plus, partial(operators.prox_soft, thresh=0.1)], axis=0))
    on_A = (partial(operators.prox_hard, thresh=np.array([0.1, 0.2])) if what == "thresh"
            else partial(operators.prox_components, prox=[operators.prox_plus, partial(operators.prox_soft, thresh=0.1)], axis=1))
    if algorithm == "bsdmm_g":
        kw["proxs_g"] = [[on_A], None]
    else:
        kw["prox_S"] = on_S
    with pytest.raises(_Reached):
        dnmf.nmf(Y, A, S, **kw)
    user = partial(operators.prox_components, prox=[operators.prox_plus, _user], axis=1 if algorithm == "bsdmm_g" else 0)
    if algorithm == "bsdmm_g":
        kw["proxs_g"] = [[user], None]
    else:
        kw["prox_S"] = user
    with pytest.raises(NotImplementedError, match="prox"):
        dnmf.nmf(Y, A, S, **kw)


@pytest.mark.parametrize("algorithm", ["pgm", "adaprox", "bsdmm", "bsdmm_g"])
def test_a_table_of_the_wrong_length_is_a_value_error_before_a_device_is_opened(algorithm, monkeypatch):
    monkeypatch.setattr(algorithms, "_open_device", _opened)
    M, N, Kf = 6, 9, 2
    rng = np.random.default_rng(0)
    Y, A, S = (rng.random(s).astype(np.float32) for s in ((M, N), (M, Kf), (Kf, N)))
    A0, S0 = A.copy(), S.copy()
    kw = dict(algorithm={"pgm": algorithms.pgm, "adaprox": algorithms.adaprox}.get(algorithm, algorithms.bsdmm), max_iter=1)
    if algorithm == "bsdmm_g":
        kw["proxs_g"] = [None, [partial(operators.prox_components, prox=[operators.prox_plus] * 3, axis=0)]]
    else:
        kw["prox_S"] = partial(operators.prox_soft, thresh=np.ones((3, 1)))
    with pytest.raises(ValueError, match="3 values"):
        dnmf.nmf(Y, A, S, **kw)
    assert np.array_equal(A, A0) and np.array_equal(S, S0)


def test_the_sharded_drivers_refuse_op_12_before_a_process_group_is_touched(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("a context or a process group was touched")
    monkeypatch.setattr(distributed, "_session", touched)
    monkeypatch.setattr(_lib, "require_torch", touched)
    Y, A, S = np.ones((4, 5), np.float32), np.ones((4, 2), np.float32), np.ones((2, 5), np.float32)
    arr = partial(operators.prox_hard, thresh=np.array([[0.1], [0.2]]), type="absolute")
    comp = partial(operators.prox_components, prox=[operators.prox_plus, operators.prox_id], axis=1)
    for drv in (distributed.nmf_pgm_sharded, distributed.nmf_adaprox_sharded, distributed.nmf_bsdmm_sharded):
        with pytest.raises(NotImplementedError, match="per-component"):
            drv(Y, A, S, 8, prox_S=arr)
        with pytest.raises(NotImplementedError, match="per-component"):
            drv(Y, A, S, 8, prox_A=comp)
    with pytest.raises(NotImplementedError, match="per-component"):
        distributed.nmf_bsdmm_sharded(Y, A, S, 8, proxs_g=[[comp], None])
    for algorithm in (algorithms.pgm, algorithms.adaprox, algorithms.bsdmm):
        with pytest.raises(NotImplementedError, match="per-component"):
            dnmf.nmf(Y, A, S, algorithm=algorithm, prox_S=arr, M_global=8)


def test_the_engine_stamps_copies_and_checks_before_it_writes():
    """DeviceNMF._stamp_tables on a stand-in context: the context's slot indices go into COPIES (the caller's sequence keeps its
    own numbering), every table is checked before the first upload"""
    from proxmin_amd.engine import DeviceNMF

    class Lib:
        def __init__(self):
            self.calls = []

        def pmx_prox_table(self, h, index, rows, K):
            self.calls.append((index, operators.table_rows(rows), K))
            return 0
    eng = DeviceNMF.__new__(DeviceNMF)
    eng.lib, eng.h, eng.K = Lib(), None, 2
    ap = operators.AlternatingProjections([partial(operators.prox_soft, thresh=np.array([0.1, 0.2])), thr.PLUS,
                                           partial(operators.prox_components, prox=MEMBERS[:2], axis=1)])
    a, b = operators.device_proxseq(ap, 0), operators.device_proxseq(SOFT_S if K == 2 else partial(operators.prox_soft, thresh=np.ones((2, 1))), 1)
    before = bytes(a), bytes(b)
    out = eng._stamp_tables([a, operators.device_proxseq(thr.PLUS, 0), b], first=3)
    assert [c[0] for c in eng.lib.calls] == [3, 4, 5] and eng.lib.calls[0][1] == MEMBER_ROWS[:2]
    assert [out[0].seq[i].reserved for i in range(3)] == [4, 0, 5] and out[2].seq[0].reserved == 6
    assert (bytes(a), bytes(b)) == before and out[0] is not a and eng._ntab == 6
    eng.lib.calls.clear()
    with pytest.raises(ValueError):
        eng._stamp_tables([a, operators.device_proxseq(partial(operators.prox_soft, thresh=np.ones(3)), 0)])
    assert eng.lib.calls == []
    with pytest.raises(NotImplementedError):
        eng._stamp_tables([a] * 9)
    assert eng.lib.calls == []
