"""The Lipschitz step rule (csrc/k_gram.hip: step_A = 1 / lmax(S S^T), step_S = 1 / lmax(A^T A)) against fp64 eigenvalues on
spectra and shapes where an iterative solver goes wrong: clustered and multiple top eigenvalues, rank deficiency, exactly
(block-)diagonal Gram matrices, mixed-sign factors whose dominant eigenvector is orthogonal to the all-ones cold start, start
vectors in the null space of a non-zero Gram matrix, 2^+-40 scales, and every row count at which the Gram sum changes its
layout.  The reference gets these numbers from LAPACK (utils.get_spectral_norm, utils.py:14-35); the yardstick here is
oracle.nmf_oracle.lipschitz_steps in float64 on the very arrays the device got.

Four parts:
  1. constructed factors X = U diag(sqrt(lambda)) V^T with a prescribed spectrum and eigenvector frame, and small-integer
     families whose fp32 Gram matrix is exact; each hard factor once as A and once as S^T (the two run in different workgroups);
  2. the cold start (nmf.step_pgm), float32 and float64 arrays (k64_front with force_exact = 1, k64_gram + k_eig with 2);
  3. the warm start inside a solver: pgm() fed by a gradient table that moves one factor across an eigenvalue crossing;
  4. the Gram routes of fused runs: the steps nmf() returns after n iterations against the eigenvalues of the device's own
     iterate n - 1.

Tolerances (relative error of a step), neither tuned to the device's output.
  separated (oracle top gap >= 10 %): the Rayleigh quotient's error is quadratic in the eigenvector error, what is left is the
     rounding of the Gram sum.  REF_ERR_SEP[KP] is what the reference's own arithmetic does with float32 arrays -- L.T.dot(L)
     and np.linalg.eigvals(...).max() in float32 -- against the fp64 oracle, the largest value over all separated cases of a K
     class (`python tests/test_gpu_step_rule.py` prints the table, CPU only); the device is allowed 4 x that: another, equally
     valid summation order (fp32 over a share of rows, fp64 from there on).
  clustered (delta <= 1e-2, exact multiplicities, the crossings): the kernel's acceptance rule, read from its code: an
     accepted l has an eigenvalue within 1e-6 l, the dominance probe (on a cold start also the Rayleigh quotient of power steps
     kept orthogonal to the accepted vector) lets lmax exceed l by at most 1e-5 l -- 1.1e-5 plus the separated allowance.  test_case_is_what_it_claims says for every clustered case whether the second eigenvalue lies outside
     that bound, i.e. whether a wrong pick would fail (at delta = 1e-6 it does not: that case guards against garbage only).
  a step that a solver returns is cast to the factors' dtype (float32): 2^-24 more.
  float64 arrays: 1e-10 on the small path (tests/test_gpu_f64.py), 1e-9 on the large one (tests/test_gpu_f64_big.py).
  the all-zero factor: exactly inf, the reference's 1 / 0.
"""
import functools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_gpu_update_step import table_grad  # noqa: E402  (the closure with a counter that serves a gradient table)

# Largest relative error of the reference's float32 arithmetic against the fp64 oracle over the separated cases below, per
# K class (KP = 32: K <= 32, 64: K <= 64, 128); reproduce with `python tests/test_gpu_step_rule.py`.
REF_ERR_SEP = {32: 2.375e-07, 64: 1.189e-07, 128: 3.63e-07}
TOL_SEP = {kp: 4 * e for kp, e in REF_ERR_SEP.items()}
ACCEPT = 1e-6 + 1e-5                   # k_gram.hip: residual test at 1e-6 l, dominance probe with margin 1e-5
CAST32 = 2.0 ** -24                    # a returned step rounded to float32
TOL_F64 = {"k64_front": 1e-10, "k64_grad_pass": 1e-9}
GAP_SEP = 0.10
OTHER = 48                             # rows of the benign factor


def kp_of(K):
    return 32 if K <= 32 else 64 if K <= 64 else 128


def tol_of(klass, K):
    return TOL_SEP[kp_of(K)] + (ACCEPT if klass == "clu" else 0.0)


def eig_small_applies(M, N, K):
    """pmx_api.hip: the factors-only route of a float32 context (k_eig_small forms the Gram matrix itself)"""
    return K <= 16 and M <= 8192 and N <= 8192


def f64_path(M, N, K):
    """the K1 kernel of a float64 context (engine.f64_applies' small limit): k64_front (force_exact = 1) or the large path"""
    return "k64_front" if (K <= 16 and M <= 4096 and N <= 8192 and M * N <= (1 << 20)) else "k64_grad_pass"


# ---------------------------------------------------------------------------------------------------------------------
# constructed factors
# ---------------------------------------------------------------------------------------------------------------------
def householder_frame(u):
    """orthogonal matrix whose first column is the unit vector u"""
    K = u.size
    w = -u.astype(np.float64)
    w[0] += 1.0
    n2 = w @ w
    return np.eye(K) if n2 == 0 else np.eye(K) - 2.0 * np.outer(w, w) / n2


def frame(kind, K, seed):
    if kind == "identity":
        return np.eye(K)
    if kind == "random":
        Q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((K, K)))
        return Q
    if kind == "perron":               # the case the cold start assumes
        return householder_frame(np.full(K, 1.0 / np.sqrt(K)))
    if kind == "pair":                 # (1, -1, 0, ...) / sqrt(2): orthogonal to all-ones
        u = np.zeros(K)
        u[0], u[1] = np.sqrt(0.5), -np.sqrt(0.5)
        return householder_frame(u)
    if kind == "alt":                  # +-1 / sqrt(K): orthogonal to all-ones for even K
        return householder_frame(np.where(np.arange(K) % 2 == 0, 1.0, -1.0) / np.sqrt(K))
    raise ValueError(kind)


def spectrum(kind, K, delta=None):
    geo = 0.7 ** np.minimum(np.arange(K), 12)            # top gap 30 %, a flat tail
    if kind == "geo":
        return geo
    if kind == "gap":                                    # relative top gap delta, the rest well below
        lam = 0.5 * geo
        lam[0] = 1.0
        if K > 1:
            lam[1] = 1.0 - delta
        return lam
    if kind == "mult2":
        lam = 0.5 * geo
        lam[:2] = 1.0
        return lam
    if kind == "multK":                                  # G = c I
        return np.full(K, 0.75)
    if kind == "rank1":
        lam = np.zeros(K)
        lam[0] = 1.0
        return lam
    raise ValueError(kind)


def constructed(rows, K, lam, V, seed, dtype):
    """X = U diag(sqrt(lam)) V^T (rows x K), U orthonormal from the QR of a seeded Gaussian; rows < K: min(rows, K) eigenvalues"""
    r = min(rows, K)
    U, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((rows, r)))
    return ((U * np.sqrt(lam[:r])) @ V[:, :r].T).astype(dtype)


def integer_factor(kind, K, seed):
    """small-integer entries: every product and every partial sum of the fp32 Gram matrix is exact"""
    rng = np.random.default_rng(seed)
    if kind == "example":              # G 1 = 0 at K = 4
        return np.array([[1, -1, 0, 0], [0, 0, 2, -2], [1, -1, 1, -1]], dtype=np.float64)
    if kind == "diag":                 # disjoint supports, unequal norms: G exactly diagonal, the largest entry not in front
        rows = 4 * K
        X = np.zeros((rows, K))
        v = 1.0 + (np.arange(K) % 7)
        v[K // 2] = 9.0
        X[np.arange(rows), np.arange(rows) % K] = v[np.arange(rows) % K]
        return X
    if kind == "block":                # two disjoint groups of overlapping non-negative columns: G exactly block-diagonal
        h = max(K // 2, 1)
        X = np.zeros((6 * K, K))
        X[:3 * K, :h] = rng.integers(0, 4, (3 * K, h))
        X[3 * K:, h:] = 2 * rng.integers(0, 4, (3 * K, K - h))
        return X
    if kind == "zerosum":              # every row sums to zero: G 1 = 0, the cold start is a null vector of a non-zero G
        rows = 3 * K
        X = np.zeros((rows, K))
        for r in range(rows):
            for _ in range(2):
                i, j = rng.choice(K, 2, replace=False)
                a = float(rng.integers(1, 4))
                X[r, i] += a
                X[r, j] -= a
        X[:8, 0] += 4.0                # (a clear largest eigenvalue)
        X[:8, 1] -= 4.0
        return X
    if kind == "halfnull":             # block-diagonal G whose DOMINANT block has zero row sums: from all-ones the iteration never enters it
        h = K // 2
        X = np.zeros((6 * K, K))
        X[:6, :h] = rng.integers(0, 3, (6, h))             # (overlapping non-negative columns on a few rows: the smaller block)
        Z = np.zeros((3 * K, K - h))
        for r in range(3 * K):
            i, j = (0, 1) if K - h == 2 else rng.choice(K - h, 2, replace=False)
            a = float(rng.integers(1, 4))
            Z[r, i] += a
            Z[r, j] -= a
        Z[:8, 0] += 4.0
        Z[:8, 1] -= 4.0
        X[3 * K:, h:] = 2 * Z
        return X
    raise ValueError(kind)


def _case(family, K, rows, side, klass, **kw):
    c = dict(family=family, K=K, rows=rows, side=side, klass=klass, spec=None, delta=None, frame=None, scale=0)
    c.update(kw)
    tag = [family] + [str(kw[k]) for k in ("delta", "frame", "scale") if k in kw] + ["K%d" % K, "rows%d" % rows, side]
    c["id"] = "-".join(tag)
    return c


FRAMES = ("perron", "identity", "random", "pair", "alt")


def _hard_factors():
    """(family, K, rows, klass, extras): pairings of spectrum family, frame, K and the row count of the hard factor; not the product"""
    out = []
    # well separated: geometric decay in a random frame over every (K, rows) the kernels distinguish.  K <= 16 with rows <= 8192:
    # k_eig_small<8|16>; with 8193 / 16385: k_gram_partial<32> + k_eig wave<32>; 17..32 wave<32>; 33..64 wave<64>; 65..128 the
    # workgroup solver.  rows 1024 / 1025: gram_nparts = 32 / 33, the octet boundary of gram_fold_octet; 8192: the last share at
    # per = 32; 8193 / 16385: per = 64 / 96.  Every K that is no multiple of 16 meets a row count > 8192.
    for K, rows in ((1, 1), (1, 8193), (2, 31), (2, 16385), (3, 33), (3, 8193), (8, 1024), (8, 8193), (9, 1025), (9, 16385), (16, 8192),
                    (16, 8193), (17, 32), (17, 8193), (31, 1025), (31, 16385), (32, 1024), (32, 1), (33, 33), (33, 8193), (63, 1025),
                    (63, 16385), (64, 8192), (64, 31), (65, 1024), (65, 8193), (127, 1025), (127, 16385), (128, 8192), (128, 16385),
                    (128, 33)):
        out.append(("geo", K, rows, "sep", dict(spec="geo", frame="random" if K > 1 else "identity")))
    for K, rows in ((8, 1025), (16, 1025), (64, 1025), (128, 1025), (31, 8193)):          # the baseline: one random non-negative factor
        out.append(("nonneg", K, rows, "sep", {}))
    # the five eigenvector frames under the separated spectrum (pair / alt: the dominant eigenvector is orthogonal to the cold start)
    for K, rows in ((2, 33), (16, 1024), (31, 8193), (64, 1025), (127, 8193)):
        for fr in FRAMES:
            if fr != "random":
                out.append(("frame", K, rows, "sep", dict(spec="geo", frame=fr)))
    # clustered: relative top gap delta, every delta on every solver, the frames taking turns
    n = 0
    for K, rows in ((2, 1025), (16, 1025), (32, 1025), (64, 1025), (128, 1025)):
        for delta in (1e-2, 1e-3, 1e-4, 1e-6):
            out.append(("gap", K, rows, "clu", dict(spec="gap", delta=delta, frame=FRAMES[n % 5])))
            n += 1
    for K, rows, fr in ((9, 8193, "pair"), (31, 8193, "alt"), (63, 16385, "pair"), (127, 8193, "random"), (3, 32, "perron")):
        out.append(("gap", K, rows, "clu", dict(spec="gap", delta=1e-3, frame=fr)))
    for K, rows in ((2, 33), (16, 1024), (32, 1025), (64, 1025), (128, 1025), (3, 8193)):
        out.append(("mult2", K, rows, "clu", dict(spec="mult2", frame=FRAMES[n % 5])))
        out.append(("multK", K, rows, "clu", dict(spec="multK", frame=FRAMES[(n + 2) % 5])))
        n += 1
    # rank deficiency
    for K, rows in ((3, 33), (16, 1025), (32, 1024), (64, 1025), (128, 1025), (9, 8193)):
        out.append(("rank1", K, rows, "sep", dict(spec="rank1", frame=FRAMES[n % 5])))
        n += 1
    for K, rows in ((2, 33), (8, 1025), (16, 8193), (32, 1025), (64, 1024), (128, 1025)):
        out.append(("halfzero", K, rows, "sep", {}))      # rank K / 2 from exact zero columns
        out.append(("halfdup", K, rows, "sep", {}))       # rank K / 2 from duplicated columns
    for K, rows in ((1, 33), (16, 1025), (32, 8193), (64, 33), (128, 1025)):
        out.append(("zero", K, rows, "zero", {}))
    for K, rows in ((3, 33), (16, 1025), (32, 1025), (64, 8193), (128, 1025)):
        for e in (-40, 40):
            out.append(("scale", K, rows, "sep", dict(spec="geo", frame="random", scale=e)))
    # exact arithmetic (the class is set from the oracle's gap by _classify below)
    for K in (1, 2, 4, 16, 64, 128):
        out.append(("diag", K, 4 * K, None, {}))
    for K in (2, 4, 16, 64, 128):
        out.append(("block", K, 6 * K, None, {}))
        out.append(("zerosum", K, 3 * K, None, {}))
    out.append(("example", 4, 3, None, {}))
    for K in (4, 16, 64, 128):
        out.append(("halfnull", K, 6 * K, None, {}))
    return out


def hard_factor(c, dtype):
    """the hard factor of a case as a tall rows x K array of `dtype`"""
    fam, K, rows = c["family"], c["K"], c["rows"]
    seed = 1000 * K + rows % 997 + sum(map(ord, fam))
    if fam in ("diag", "block", "zerosum", "example", "halfnull"):
        return integer_factor(fam, K, seed).astype(dtype)
    if fam == "nonneg":
        return np.random.default_rng(seed).random((rows, K)).astype(dtype)
    if fam == "zero":
        return np.zeros((rows, K), dtype)
    if fam in ("halfzero", "halfdup"):
        h = K // 2
        Xh = constructed(rows, h, spectrum("geo", h), frame("random", h, seed + 1), seed, np.float64)
        X = np.zeros((rows, K))
        X[:, 0::2] = Xh
        if fam == "halfdup":
            X[:, 1::2] = Xh
        return X.astype(dtype)
    X = constructed(rows, K, spectrum(c["spec"], K, c["delta"]), frame(c["frame"], K, seed + 1), seed, np.float64)
    return (X * 2.0 ** c["scale"]).astype(dtype)


def _classify(fam, K, rows):
    """separated / clustered for the exact-arithmetic families, from the fp64 oracle's top gap"""
    c = dict(family=fam, K=K, rows=rows)
    ev = np.linalg.eigvalsh(hard_factor(c, np.float64).T @ hard_factor(c, np.float64))
    return "sep" if K == 1 or (ev[-1] - ev[-2]) >= GAP_SEP * ev[-1] else "clu"


def _cases():
    out = []
    for fam, K, rows, klass, kw in _hard_factors():
        if klass is None:
            klass = _classify(fam, K, rows)
        for side in "AS":              # once as A with a benign non-negative S, once as S^T with a benign A
            out.append(_case(fam, K, rows, side, klass, **kw))
    return out


CASES = _cases()
CASE_BY_ID = {c["id"]: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)


def make_factors(c, dtype):
    """(A, S) of a case: the hard factor on its side, a benign non-negative random factor on the other"""
    X = hard_factor(c, dtype)
    rows, K = X.shape
    benign = np.random.default_rng(77 + K).random((OTHER, K)).astype(dtype) + dtype(0.1)
    if c["side"] == "A":
        return np.ascontiguousarray(X), np.ascontiguousarray(benign.T)
    return benign, np.ascontiguousarray(X.T)


def shape_of(c):
    return (c["rows"], OTHER, c["K"]) if c["side"] == "A" else (OTHER, c["rows"], c["K"])


def oracle_steps(A, S):
    from oracle import nmf_oracle as orc
    with np.errstate(divide="ignore"):
        return tuple(float(s) for s in orc.lipschitz_steps(A.astype(np.float64), S.astype(np.float64)))


def float32_reference_steps(A, S):
    """what the reference itself does with float32 arrays (utils.py:20, :34), no float64 anywhere"""
    out = []
    for L in (S.T, A):
        L = np.ascontiguousarray(L, dtype=np.float32)
        with np.errstate(divide="ignore"):
            out.append(1 / np.real(np.linalg.eigvals(L.T.dot(L)).max()))
    return tuple(float(s) for s in out)


def rel_err(got, want):
    if not np.isfinite(want):
        return 0.0 if got == want else np.inf
    return abs(got / want - 1.0) if np.isfinite(got) else np.inf


def top_eigs(X):
    ev = np.linalg.eigvalsh(X.astype(np.float64).T @ X.astype(np.float64))
    return ev[-1], (ev[-2] if ev.size > 1 else 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: every case is what it claims to be
# ---------------------------------------------------------------------------------------------------------------------
def cluster_is_resolved(c, dtype=np.float32):
    """a clustered case whose second eigenvalue lies OUTSIDE the bound: a solver that picks it fails the test"""
    l1, l2 = top_eigs(hard_factor(c, dtype))
    return (l1 - l2) / l2 > tol_of("clu", c["K"]) if l2 > 0 else True


# gap family: delta = 1e-6 lies inside the bound (garbage guard only), every other delta outside; exact multiplicities can never
# be told apart (and need not be)
RESOLVED = {cid: (c["delta"] is not None and c["delta"] >= 1e-4) for cid, c in CASE_BY_ID.items() if c["klass"] == "clu" and c["family"] in ("gap", "mult2", "multK")}


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["side"] == "A"])
def test_case_is_what_it_claims(cid):
    """On the fp64 oracle alone, on the float32 arrays the device gets: the class (top gap), the prescribed spectrum, the
    eigenvector frame (orthogonality to the cold start), exactness of the integer families, rank, and for every clustered
    case whether its second eigenvalue lies outside the bound."""
    c = CASE_BY_ID[cid]
    X = hard_factor(c, np.float32)
    K, fam = c["K"], c["family"]
    assert X.shape == (c["rows"], K)
    G = X.astype(np.float64).T @ X.astype(np.float64)
    ev, vec = np.linalg.eigh(G)
    l1, l2 = ev[-1], (ev[-2] if K > 1 else 0.0)
    ones = np.full(K, 1.0 / np.sqrt(K))
    if c["klass"] == "zero":
        assert not X.any() and oracle_steps(*make_factors(c, np.float32))[1] == np.inf
        return
    assert l1 > 0
    gap = (l1 - l2) / l1
    if c["klass"] == "sep":
        assert gap >= GAP_SEP, gap
    else:
        assert gap < GAP_SEP if fam in ("zerosum", "block", "diag", "halfnull", "example") else gap <= 1.01e-2, gap
        if cid in RESOLVED:
            assert cluster_is_resolved(c) == RESOLVED[cid], ((l1 - l2) / l2, tol_of("clu", K))
    r = min(c["rows"], K)
    if c["spec"] is not None:          # the prescribed spectrum, to float32 rounding of the entries
        want = np.sort(np.concatenate([spectrum(c["spec"], K, c["delta"])[:r], np.zeros(K - r)]))[::-1] * 4.0 ** c["scale"]
        np.testing.assert_allclose(ev[::-1], want, rtol=0, atol=2e-6 * want[0])
        if c["delta"] is not None:
            assert gap == pytest.approx(c["delta"], rel=0.2, abs=2e-7)
    if c["frame"] in ("pair", "alt") and (c["frame"] == "pair" or K % 2 == 0) and gap > 1e-5 and r == K:
        assert abs(vec[:, -1] @ ones) < 1e-6 / gap    # the dominant eigenvector is orthogonal to the cold start (float32 entries: 1e-7 / gap)
        assert (vec[:, -1] > 0).any() and (vec[:, -1] < 0).any()
    if c["frame"] == "perron" and gap > 1e-5:
        assert abs(abs(vec[:, -1] @ ones) - 1) < 1e-6 / gap
    if fam == "rank1":
        assert l2 <= 1e-6 * l1
    if fam in ("halfzero", "halfdup"):
        assert np.linalg.matrix_rank(G, tol=1e-6 * l1) == K // 2
        assert (X[:, 1::2] == (0 if fam == "halfzero" else X[:, 0::2])).all()
    if fam in ("diag", "block", "zerosum", "example", "halfnull"):
        assert (X == np.round(X)).all() and np.abs(X).max() <= 32
        G32 = X.T.dot(X)                                  # float32 throughout
        assert G32.dtype == np.float32 and (G32 == G).all() and np.abs(G).max() < 2 ** 24, "the fp32 Gram matrix is not exact"
        h = max(K // 2, 1)
        if fam == "diag":
            assert (G == np.diag(np.diag(G))).all() and (K == 1 or (np.argmax(np.diag(G)) != 0 and len(set(np.diag(G))) > 1))
        if fam in ("block", "halfnull"):
            assert not G[:h, h:].any() and (K <= 2 or (G[:h, :h] != np.diag(np.diag(G[:h, :h]))).any())
        if fam in ("zerosum", "example"):
            assert not X.sum(1).any() and not (G @ np.ones(K)).any() and l1 > 0
        if fam == "halfnull":          # the largest eigenvalue lives in the block that all-ones never enters
            assert not (G[h:, h:] @ np.ones(K - h)).any()
            assert np.linalg.eigvalsh(G[h:, h:])[-1] == pytest.approx(l1) and np.linalg.eigvalsh(G[:h, :h])[-1] < 0.5 * l1
    for s in oracle_steps(*make_factors(c, np.float32)):
        assert np.isfinite(s) and s > 0


def test_case_list_reaches_every_route():
    """every solver instantiation, both Gram routes of a factors-only context, every fold boundary, both fp64 paths per family"""
    shapes = {shape_of(c) for c in CASES}
    small = {K for M, N, K in shapes if eig_small_applies(M, N, K)}
    assert {1, 2, 3, 8, 9, 16} <= small
    big_rows = {K for M, N, K in shapes if max(M, N) > 8192}
    assert {1, 2, 3, 8, 9, 17, 31, 33, 63, 65, 127} <= big_rows       # every K that is no multiple of 16
    assert {17, 31, 32, 33, 63, 64, 65, 127, 128} <= {c["K"] for c in CASES}
    assert {1, 31, 32, 33, 1024, 1025, 8192, 8193, 16385} <= {c["rows"] for c in CASES}
    assert max(max(M, N) * K for M, N, K in shapes) == 16385 * 128
    for fam in {c["family"] for c in CASES}:
        paths = {f64_path(*shape_of(c)) for c in CASES if c["family"] == fam}
        assert "k64_grad_pass" in paths or fam == "example", fam          # (the 3 x 4 example is one shape)
        assert "k64_front" in paths or not any(c["K"] <= 16 for c in CASES if c["family"] == fam), fam
    for fam in {c["family"] for c in CASES}:
        assert {c["side"] for c in CASES if c["family"] == fam} == {"A", "S"}


# ---------------------------------------------------------------------------------------------------------------------
# part 3 on the CPU: the crossing is a trap for a warm-started solver without the probe
# ---------------------------------------------------------------------------------------------------------------------
def _xing(K, rows, side, kind="qr"):
    return dict(K=K, rows=rows, side=side, kind=kind, id="xing-%s-K%d-%s" % (kind, K, side))


# K = 2: k_eig_small (a gradient from a table: no K1 in the iteration, hence no k_small_front); 24: wave<32>; 48: wave<64>; 96: workgroup
XING = [_xing(2, 64, "A"), _xing(24, 200, "S"), _xing(48, 200, "A"), _xing(96, 200, "S"), _xing(4, 16, "S", "int"), _xing(64, 256, "A", "int")]
XING_BY_ID = {c["id"]: c for c in XING}
XING_ITERS = 3


@functools.lru_cache(maxsize=None)
def xing_problem(cid):
    """-> (A0, S0, table): orthogonal columns with scales (2, 1, 1/2, ...); G_0 = (X_0 - X_1*) / step_0 takes the crossing factor to
    X_1* with the first two scales swapped, the second table entry moves only the OTHER factor (a run that moves nothing stops),
    the third nothing."""
    c = XING_BY_ID[cid]
    K, rows = c["K"], c["rows"]
    rng = np.random.default_rng(31 * K + rows)
    s0 = np.full(K, 0.5)
    s0[:2] = (2.0, 1.0)
    s1 = s0.copy()
    s1[:2] = (1.0, 2.0)
    if c["kind"] == "int":             # disjoint supports, integer entries: the Gram matrix is exactly diagonal at X_0 and at X_1
        P = np.zeros((rows, K))
        P[np.arange(rows), np.arange(rows) % K] = 1.0
        s0, s1 = 2 * s0, 2 * s1
    else:
        P, _ = np.linalg.qr(rng.standard_normal((rows, K)))
    X0, X1 = (P * s0).astype(np.float32), (P * s1).astype(np.float32)
    other = (rng.random((OTHER, K)) + 0.1).astype(np.float32)
    A0, S0 = (X0, np.ascontiguousarray(other.T)) if c["side"] == "A" else (other, np.ascontiguousarray(X0.T))
    j = "AS".index(c["side"])
    step0 = oracle_steps(A0, S0)[j]
    D = ((X0.astype(np.float64) - X1.astype(np.float64)) / step0).astype(np.float32)
    zA, zS = np.zeros_like(A0), np.zeros_like(S0)
    nudge = (1e-3 * rng.standard_normal(other.shape)).astype(np.float32)
    if c["side"] == "A":
        table = [(D, zS), (zA, np.ascontiguousarray(nudge.T)), (zA, zS)]
    else:
        table = [(zA, np.ascontiguousarray(D.T)), (nudge, zS), (zA, zS)]
    for t in table:
        for g in t:
            g.setflags(write=False)
    A0.setflags(write=False)
    S0.setflags(write=False)
    return A0, S0, table


@functools.lru_cache(maxsize=None)
def xing_reference(cid, n):
    """oracle.pgm_nmf on the table in fp64: (steps returned after n iterations, (A, S) after n iterations)"""
    from oracle import nmf_oracle as orc
    A0, S0, table = xing_problem(cid)
    A, S = A0.astype(np.float64), S0.astype(np.float64)
    if n == 0:
        return None, (A, S), 0
    _, _, St, n_it = orc.pgm_nmf(None, A, S, None, None, grad=table_grad(table, np.float64), max_iter=n, e_rel=0)
    return tuple(float(s) for s in St), (A, S), n_it


@pytest.mark.parametrize("cid", [c["id"] for c in XING])
def test_crossing_is_a_trap_for_a_warm_start(cid):
    """On the fp64 oracle: the top eigenvector v of G(X_0) is, at X_1, an eigenvector to a residual a warm-started iteration
    accepts (|G_1 v - (v^T G_1 v) v| <= 1e-7 v^T G_1 v), and v^T G_1 v <= lmax(G_1) / 2: a step from it is >= 2 x too long.
    The run takes all three iterations, and the third evaluates its rule where the second did."""
    c = XING_BY_ID[cid]
    j = "AS".index(c["side"])
    tall = (lambda X: X) if j == 0 else (lambda X: X.T)
    X0 = tall(xing_reference(cid, 0)[1][j])
    X1 = tall(xing_reference(cid, 1)[1][j])
    X2 = tall(xing_reference(cid, 2)[1][j])
    assert xing_reference(cid, XING_ITERS)[2] == XING_ITERS
    assert (X1 == X2).all()
    G0, G1 = X0.T @ X0, X1.T @ X1
    v = np.linalg.eigh(G0)[1][:, -1]
    rq = v @ G1 @ v
    assert np.linalg.norm(G1 @ v - rq * v) <= 1e-7 * rq
    l1, l2 = top_eigs(X1)
    assert rq <= l1 / 2
    assert (l1 - l2) / l1 >= GAP_SEP and top_eigs(X0)[0] == pytest.approx(l1, rel=1e-5)
    if c["kind"] == "int":
        for X in (X0, X1):
            assert ((X.T @ X) == np.diag(np.diag(X.T @ X))).all()
    s = [xing_reference(cid, n)[0][1 - j] for n in (1, 2, 3)]          # the step of the OTHER block comes from this factor
    assert s[0] == pytest.approx(s[1], rel=1e-5) and s[1] == s[2]


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pm():
    import __graft_entry__ as g
    g.build()
    import proxmin_amd
    return proxmin_amd


def device_steps(pm, A, S):
    """nmf.step_pgm on copies of the arrays -> (steps, K1 kernel name of the context that computed them)"""
    with np.errstate(divide="ignore"):
        s = pm.nmf.step_pgm(A.copy(), S.copy())
    ctx = list(pm.nmf._FACTOR_CTX.values())
    assert len(ctx) == 1
    return (float(s[0]), float(s[1])), ctx[0].k1_info()["kernel"], ctx[0].mode


def check_case(c, got, want, tol, what):
    j = 1 if c["side"] == "A" else 0                      # lmax of A^T A sets step_S, lmax of S S^T sets step_A
    errs = [rel_err(got[i], want[i]) for i in range(2)]
    print("%-58s %-8s hard %.3g (allowed %.3g)  benign %.3g" % (c["id"], what, errs[j], tol, errs[1 - j]))
    if c["klass"] == "zero":
        assert got[j] == np.inf, "%s: the step from an all-zero factor is %r, the reference's 1 / 0 is inf" % (what, got[j])
    else:
        assert np.isfinite(got[j]) and got[j] > 0, "%s: step %r where the fp64 eigenvalue gives %r" % (what, got[j], want[j])
        assert errs[j] <= tol, "%s: the step of the hard factor is off by %.3g relative (allowed %.3g): %r vs %r" % (what, errs[j], tol, got[j], want[j])
    return errs


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_cold_start_matches_fp64_eigenvalues(pm, cid):
    """Both steps of nmf.step_pgm -- a function of its arguments: every call starts from all-ones -- against fp64 eigenvalues,
    with float32 arrays and again with float64 arrays, which must take the fp64 path the case's shape is listed under.

    The mixed-sign frames are the point of the cold start: with a dominant eigenvector +-1 / sqrt(K) (or (1, -1, 0, ...) / sqrt(2))
    all-ones is orthogonal to it to the last bit, the power iteration settles on the SECOND eigenvalue with a small residual, and
    only the cold start's deflated check (k_gram.hip: power steps kept orthogonal to the accepted vector) notices."""
    from proxmin_amd import engine
    c = CASE_BY_ID[cid]
    M, N, K = shape_of(c)
    j = 1 if c["side"] == "A" else 0
    A, S = make_factors(c, np.float32)
    assert (A.shape, S.shape) == ((M, K), (K, N))
    got, _, mode = device_steps(pm, A, S)
    assert mode == "f32"
    want = oracle_steps(A, S)
    errs = check_case(c, got, want, tol_of(c["klass"], K), "float32")
    assert errs[1 - j] <= tol_of("sep", K), "the benign factor's step is off by %.3g" % errs[1 - j]
    if eig_small_applies(M, N, K):     # the same through a context of the caller's own (a fresh one: also a cold start)
        with engine.DeviceNMF(M, N, K, mode="f32") as dev:
            dev.set_factors(A, S)
            again = dev.step_pgm()
        assert tuple(again) == got
    A64, S64 = make_factors(c, np.float64)
    got64, kernel, mode = device_steps(pm, A64, S64)
    assert mode == "f64" and kernel == f64_path(M, N, K), (mode, kernel, f64_path(M, N, K))
    want64 = oracle_steps(A64, S64)
    errs = check_case(c, got64, want64, TOL_F64[kernel], "float64")
    assert errs[1 - j] <= TOL_F64[kernel]


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(1024, OTHER, 32), (1025, OTHER, 32), (8192, OTHER, 64), (8193, OTHER, 64), (16385, OTHER, 128), (OTHER, 1025, 9),
                                   (OTHER, 8193, 9), (8192, 8192, 16), (8193, 31, 16)])
def test_boundary_shapes_through_a_context_of_their_own(pm, M, N, K):
    """engine.DeviceNMF(M, N, K).step_pgm() after set_factors at the fold boundaries, mixed-sign Gaussian factors (no Perron
    argument), twice on the same context with the factors exchanged for others in between: the second call is a cold start too."""
    from proxmin_amd import engine
    rng = np.random.default_rng(M + N + K)
    with engine.DeviceNMF(M, N, K, mode="f32") as dev:
        for _ in range(2):
            A, S = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((K, N)).astype(np.float32)
            dev.set_factors(A, S)
            got, want = dev.step_pgm(), oracle_steps(A, S)
            for i in range(2):
                X = S.T if i == 0 else A
                l1, l2 = top_eigs(X)
                klass = "sep" if (l1 - l2) >= GAP_SEP * l1 else "clu"
                e = rel_err(got[i], want[i])
                print("%dx%dx%d step[%d] %s %.3g" % (M, N, K, i, klass, e))
                assert e <= tol_of(klass, K), (i, klass, e)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c["id"] for c in XING])
def test_warm_start_survives_a_crossing(pm, cid):
    """pgm() fed by the gradient table keeps its eigenvectors from one iteration to the next.  Iteration 2 evaluates the rule where
    the previous eigenvector has just become an exact eigenvector of the SECOND eigenvalue (test_crossing_is_a_trap_for_a_warm_start):
    only the dominance probe sends it to the exact solver.  Iteration 3 evaluates it again at the same point, warm-started from
    the right vector.  Steps against fp64 eigenvalues of the device's own iterate, and against oracle.pgm_nmf's steps."""
    c = XING_BY_ID[cid]
    K = c["K"]
    A0, S0, table = xing_problem(cid)
    M, N = A0.shape[0], S0.shape[1]
    assert eig_small_applies(M, N, K) == (K <= 16)         # K = 2, 4: k_eig_small; the others k_gram_partial + k_eig
    j = "AS".index(c["side"])
    tol = tol_of("clu", K) + CAST32
    prev = (A0, S0)
    for n in range(1, XING_ITERS + 1):
        A, S = A0.copy(), S0.copy()
        grad = table_grad(table, np.float32)
        conv, G, steps = pm.pgm([A, S], grad, pm.nmf.step_pgm, prox=None, e_rel=0, max_iter=n)
        assert grad.state["i"] == n
        own = oracle_steps(*prev)                          # the rule at the point where iteration n evaluated it
        ref, (Ar, Sr), _ = xing_reference(cid, n)
        errs = [rel_err(float(steps[i]), own[i]) for i in range(2)]
        errs_ref = [rel_err(float(steps[i]), ref[i]) for i in range(2)]
        print("%s n=%d: own iterate %.3g %.3g (allowed %.3g), oracle run %.3g %.3g" % (cid, n, errs[0], errs[1], tol, errs_ref[0], errs_ref[1]))
        for i in range(2):
            assert errs[i] <= tol, "iteration %d, step[%d]: %r vs %r" % (n, i, steps[i], own[i])
            # the oracle's iterate differs from the device's by the device's error in step_0 (<= the separated allowance) times the move
            assert errs_ref[i] <= tol + 2 * tol_of("sep", K), "iteration %d, step[%d]: %r vs the oracle run's %r" % (n, i, steps[i], ref[i])
        np.testing.assert_allclose((A, S)[j], (Ar, Sr)[j], rtol=0, atol=1e-5 * np.abs((Ar, Sr)[j]).max())
        prev = (A, S)


FUSED = [(300, 420, 8, None), (1024, 768, 32, None), (1024, 768, 32, "0"), (1024, 768, 64, None), (4097, 768, 64, None), (640, 512, 128, None)]
FUSED_ITERS = 3


def _separated_steps_check(K, steps, A, S, extra, what):
    want = oracle_steps(A, S)
    for i, X in enumerate((S.T, A)):
        l1, l2 = top_eigs(X)
        assert (l1 - l2) >= GAP_SEP * l1, "the iterate's spectrum is not separated"
        e = rel_err(float(steps[i]), want[i])
        print("%s step[%d] %.3g (allowed %.3g)" % (what, i, e, tol_of("sep", K) + extra))
        assert e <= tol_of("sep", K) + extra, "%s: step[%d] = %r, fp64 eigenvalue of the device's own iterate gives %r" % (what, i, steps[i], want[i])


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,fold", FUSED)
def test_fused_run_steps_match_the_eigenvalues_of_its_own_iterate(pm, monkeypatch, M, N, K, fold):
    """nmf() in exact fp32, plain pgm: the steps returned after n iterations were evaluated at X_{n-1} -- the factors a run of
    n - 1 iterations from the same start returns.  Against fp64 lipschitz_steps of that iterate the trajectory's noise cancels;
    what is left is the route's Gram sum (k_small_front's own fold; partials left by k_pgm_update, folded in K1 or by
    k_gram_reduce; k_gram_partial beyond 4096 rows) and the warm-started solve."""
    from oracle import nmf_oracle as orc
    from proxmin_amd import engine
    if fold is not None:
        monkeypatch.setenv("PMX_FOLD_IN_K1", fold)
    Y, A0, S0 = orc.synthetic_problem(M, N, K, np.float32, seed=M + N + K)
    saved = engine.get_default_mode()
    engine.set_default_mode("f32")
    try:
        A, S = A0.copy(), S0.copy()
        pm.nmf.nmf(Y, A, S, max_iter=FUSED_ITERS - 1, e_rel=0)
        A2, S2 = A0.copy(), S0.copy()
        _, _, steps = pm.nmf.nmf(Y, A2, S2, max_iter=FUSED_ITERS, e_rel=0)
    finally:
        engine.set_default_mode(saved)
    assert not np.array_equal(A, A0) and not np.array_equal(A2, A)
    _separated_steps_check(K, steps, A, S, CAST32, "%dx%dx%d fold=%s" % (M, N, K, fold))


@pytest.mark.gpu
def test_bsdmm_steps_match_the_eigenvalues_of_its_own_iterate(pm):
    """bSDMM's Gram partials come from k_bsdmm_update.  Gauss-Seidel: in iteration n step_A is evaluated at S_{n-1}, step_S at the
    A that iteration n has just updated (A_n); both from runs of n - 1 and n iterations from the same start."""
    from oracle import nmf_oracle as orc
    from proxmin_amd import engine, operators as ops
    M, N, K = 1024, 768, 32
    Y, A0, S0 = orc.synthetic_problem(M, N, K, np.float32, seed=5)
    out = {}
    for n in (FUSED_ITERS - 1, FUSED_ITERS):
        with engine.DeviceNMF(M, N, K, mode="f32") as dev:
            dev.set_Y(Y)
            dev.set_factors(A0, S0)
            plus = [ops.device_proxseq(ops.prox_plus, 0), ops.device_proxseq(ops.prox_plus, 1)]
            dev.bsdmm_begin(plus, [[plus[0]], [plus[1]]], e_rel=(0.0, 0.0))
            r = dev.bsdmm_run(n)
            assert r.iterations == n
            out[n] = (dev.get_factors(), (r.steps[0], r.steps[1]))
    (A_prev, S_prev), _ = out[FUSED_ITERS - 1]
    (A_n, _), steps = out[FUSED_ITERS]
    _separated_steps_check(K, steps, A_n, S_prev, 0.0, "bsdmm %dx%dx%d" % (M, N, K))


# ---------------------------------------------------------------------------------------------------------------------
# how REF_ERR_SEP were obtained: python tests/test_gpu_step_rule.py  (CPU only)
# ---------------------------------------------------------------------------------------------------------------------
def measure(cases=CASES, verbose=True):
    worst = {32: 0.0, 64: 0.0, 128: 0.0}
    for c in cases:
        A, S = make_factors(c, np.float32)
        want, ref32 = oracle_steps(A, S), float32_reference_steps(A, S)
        j = 1 if c["side"] == "A" else 0
        l1, l2 = top_eigs(hard_factor(c, np.float32))
        e = [rel_err(ref32[i], want[i]) for i in range(2)]
        if verbose:
            print("%-58s %-4s %-13s gap %-9.3g oracle step %-12.6g float32 reference: hard %-9.3g benign %-9.3g%s" % (
                c["id"], c["klass"], "%dx%dx%d" % shape_of(c), (l1 - l2) / l1 if l1 > 0 else 0, want[j], e[j], e[1 - j],
                "" if c["klass"] != "clu" else "  second eigenvalue %s the bound" % ("outside" if cluster_is_resolved(c) else "inside")), flush=True)
        kp = kp_of(c["K"])
        worst[kp] = max(worst[kp], e[1 - j], e[j] if c["klass"] == "sep" else 0.0)        # (the benign factor is separated in every case)
    if verbose:
        for kp in sorted(worst):
            print("REF_ERR_SEP[%d] = %.4g" % (kp, worst[kp]))
    return worst


if __name__ == "__main__":
    pat = sys.argv[1] if len(sys.argv) > 1 else ""
    measure([c for c in CASES if re.search(pat, c["id"])])
