"""GPU: kernel-level parity of the HIP path (through the C ABI) against the CPU oracle and the
reference-generated golden fixtures."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc():
    from oracle import nmf_oracle
    return nmf_oracle


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as g
    g.build()
    from proxmin_amd import engine
    return engine


SHAPES = [(33, 47, 3), (64, 96, 8), (100, 300, 12), (513, 700, 16), (128, 128, 32), (200, 1000, 5), (257, 513, 33), (300, 260, 64),
          (1024, 640, 64), (384, 1100, 100), (512, 512, 128), (4096, 4096, 32)]


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "f16x2", "f16x2r"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_fused_gradient_matches_oracle(eng, orc, M, N, K, mode):
    """K1 (nmf.grad_likelihood + log_likelihood) vs NumPy, fp32 tolerance: the contraction runs on
    exact-fp32 MFMA, so the difference is summation order only."""
    Y, A, S = orc.synthetic_problem(M, N, K, np.float32, seed=M + N + K)
    with eng.DeviceNMF(M, N, K, mode=mode) as dev:
        dev.set_Y(Y)
        dev.set_factors(A, S)
        gA, gS = dev.grad()
        loss = dev.loglike()
    A64, S64, Y64 = A.astype(np.float64), S.astype(np.float64), Y.astype(np.float64)
    rA, rS = orc.residual_gradients(A64, S64, Y64)
    # tolerance relative to the gradient scale (entries can cancel to ~0)
    np.testing.assert_allclose(gA, rA, rtol=2e-5, atol=2e-5 * np.abs(rA).max())
    np.testing.assert_allclose(gS, rS, rtol=2e-5, atol=2e-5 * np.abs(rS).max())
    assert loss == pytest.approx(orc.half_sq_residual(A64, S64, Y64), rel=2e-5)


@pytest.mark.parametrize("variant", [0, 1, 7])
@pytest.mark.parametrize("M,N,K", [(128, 64, 64), (1024, 640, 64), (640, 1536, 64), (2304, 832, 64), (5120, 4096, 64), (256, 320, 40), (384, 256, 32)])
def test_split_bf16_kernel_variants_agree_with_oracle(eng, orc, monkeypatch, M, N, K, variant):
    """Every implementation of the split-bf16 K1 (guarded, LDS-DMA pipeline, the producer / consumer kernel v7; selected per
    context by PMX_K1_VARIANT, shapes that a variant does not take fall through to the next; the intermediate variants 4
    and 5 of rounds 1-2 were removed in round 4) gives the oracle's
    gradients and loss; asymmetric data, so a swapped tile or operand orientation cannot pass."""
    monkeypatch.setenv("PMX_K1_VARIANT", str(variant))
    Y, A, S = orc.synthetic_problem(M, N, K, np.float32, seed=11 * M + N + K)
    A[:, 0] += np.linspace(0.0, 1.0, M, dtype=np.float32)
    S[K - 1, :] += np.linspace(1.0, 0.0, N, dtype=np.float32)
    with eng.DeviceNMF(M, N, K, mode="bf16x3") as dev:
        dev.set_Y(Y)
        dev.set_factors(A, S)
        gA, gS = dev.grad()
        loss = dev.loglike()
    A64, S64, Y64 = A.astype(np.float64), S.astype(np.float64), Y.astype(np.float64)
    rA, rS = orc.residual_gradients(A64, S64, Y64)
    np.testing.assert_allclose(gA, rA, rtol=2e-5, atol=2e-5 * np.abs(rA).max())
    np.testing.assert_allclose(gS, rS, rtol=2e-5, atol=2e-5 * np.abs(rS).max())
    assert loss == pytest.approx(orc.half_sq_residual(A64, S64, Y64), rel=2e-5)


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "f16x2"])
def test_gradient_is_transpose_sensitive(eng, orc, mode):
    """asymmetric inputs: a swapped tile mapping cannot pass (guide rule: A=I with asymmetric B)."""
    M, N, K = 96, 160, 32
    A = np.zeros((M, K), np.float32)
    A[np.arange(K), np.arange(K)] = 1.0
    S = (np.arange(K * N, dtype=np.float32).reshape(K, N) % 97) / 97.0
    Y = np.zeros((M, N), np.float32)
    Y[5, 7] = 3.0
    with eng.DeviceNMF(M, N, K, mode=mode) as dev:
        dev.set_Y(Y)
        dev.set_factors(A, S)
        gA, gS = dev.grad()
    rA, rS = orc.residual_gradients(A.astype(np.float64), S.astype(np.float64), Y.astype(np.float64))
    np.testing.assert_allclose(gA, rA, rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(gS, rS, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("M,N,K", [(64, 96, 8), (120, 500, 12), (4000, 200, 16), (8192, 40, 9), (300, 260, 64), (2048, 1024, 128), (1000, 3000, 5)])
def test_step_rules_match_oracle(eng, orc, M, N, K):
    Y, A, S = orc.synthetic_problem(M, N, K, np.float32, seed=3)
    with eng.DeviceNMF(M, N, K) as dev:
        dev.set_Y(Y)
        dev.set_factors(A, S)
        sA, sS = dev.step_pgm()
        aA, aS = dev.step_adaprox()
    oA, oS = orc.lipschitz_steps(A.astype(np.float64), S.astype(np.float64))
    assert sA == pytest.approx(oA, rel=2e-6)
    assert sS == pytest.approx(oS, rel=2e-6)
    qA, qS = orc.adaprox_steps(A.astype(np.float64), S.astype(np.float64))
    np.testing.assert_allclose(aA, qA, rtol=2e-6)
    np.testing.assert_allclose(aS, qS[:, 0], rtol=2e-6)


def test_lambda_max_degenerate_spectrum(eng, orc):
    """nearly equal top eigenvalues: the power iteration must still deliver lmax to ~1e-5."""
    rng = np.random.default_rng(5)
    K, M, N = 16, 400, 300
    Q, _ = np.linalg.qr(rng.standard_normal((M, K)))
    sv = np.linspace(1.0, 0.999, K)
    A = (Q * sv).astype(np.float32)
    S = rng.random((K, N)).astype(np.float32)
    with eng.DeviceNMF(M, N, K) as dev:
        dev.set_Y(np.zeros((M, N), np.float32))
        dev.set_factors(A, S)
        sA, sS = dev.step_pgm()
    oA, oS = orc.lipschitz_steps(A.astype(np.float64), S.astype(np.float64))
    assert sS == pytest.approx(oS, rel=2e-5)
    assert sA == pytest.approx(oA, rel=2e-6)


def test_operators_match_reference_fixture():
    """every prox op-code on the device vs the outputs recorded from the reference"""
    from proxmin_amd import operators as ops
    from functools import partial
    z, meta = load_golden("operators.npz")
    for e in meta["entries"]:
        k, spec = e["key"], e["spec"]
        X, step = z[k + "/X"].copy(), z[k + "/step"]
        fn = getattr(ops, "prox_" + spec[0])
        if spec[0] in ("unity", "unity_plus"):
            fn = partial(fn, axis=spec[1])
        elif len(spec) > 1:
            fn = partial(fn, thresh=spec[1], type=spec[2])
        step = float(step) if step.ndim == 0 else step
        out = fn(X, step)
        assert out is X                                      # in-place contract
        # unity divides by a sum of mixed-sign entries that can cancel: summation order shows up at ~1e-5
        tol = dict(rtol=3e-5, atol=1e-6) if spec[0].startswith("unity") else dict(rtol=2e-6, atol=2e-7)
        np.testing.assert_allclose(out, z[k + "/out"], err_msg=str(e), **tol)
    ap = meta["ap"]
    X = z["ap/X"].copy()
    comp = ops.AlternatingProjections([partial(ops.prox_unity, axis=1), ops.prox_plus], repeat=ap["repeat"])
    np.testing.assert_allclose(comp(X, ap["step"]), z["ap/out"], rtol=5e-6, atol=1e-7)


def test_operator_edge_cases():
    from proxmin_amd import operators as ops
    X = np.array([[-0.0, 0.0, -1.5, 2.0, np.nan, np.inf]], dtype=np.float32)
    out = ops.prox_plus(X.copy(), 1.0)
    assert np.isnan(out[0, 4]) and out[0, 5] == np.inf and out[0, 2] == 0 and out[0, 3] == 2
    out = ops.prox_soft(X.copy(), 1.0, thresh=0.5)
    np.testing.assert_array_equal(out[0, :4], np.array([0.0, 0.0, -1.0, 1.5], np.float32))
    assert np.isnan(out[0, 4])
    # zero-sum slice -> NaN, like the reference (no guard in prox_unity)
    Z = np.zeros((3, 4), np.float32)
    with np.errstate(all="ignore"):
        assert np.isnan(ops.prox_unity(Z, 1.0, axis=1)).all()


def test_split_bf16_gradient_near_solution_is_fp32_class(eng, orc):
    """Where cancellation bites (|R| << |A S|): the split-bf16 kernel and the two-term fp16 kernel must be as close to
    the fp64 gradient as the exact-fp32 kernel is (within 3x), and all ~1e-5 of the gradient norm."""
    M, N, K = 1536, 2048, 64
    Y, A, S = orc.synthetic_problem(M, N, K, np.float32, seed=31)
    orc.adaprox_nmf(Y, A, S, scheme="amsgrad", max_iter=60, e_rel=1e-3, check_convergence=False)
    g64 = orc.residual_gradients(A.astype(np.float64), S.astype(np.float64), Y.astype(np.float64))
    err = {}
    for mode in ("f32", "bf16x3", "f16x2"):
        with eng.DeviceNMF(M, N, K, mode=mode) as dev:
            dev.set_Y(Y)
            dev.set_factors(A, S)
            g = dev.grad()
        err[mode] = [np.linalg.norm(g[j] - g64[j]) / np.linalg.norm(g64[j]) for j in range(2)]
    for j in range(2):
        assert err["f32"][j] < 5e-5
        assert err["bf16x3"][j] < max(3 * err["f32"][j], 2e-5), err
        assert err["f16x2"][j] < max(3 * err["f32"][j], 2e-5), err


def test_full_size_gradient_properties(eng):
    """BASELINE's headline shape (Y 16384 x 16384, K = 64), where the oracle would take minutes: size-independent
    properties instead.  (1) the two independent K1 implementations (exact-fp32 MFMA and split-bf16 producer/consumer)
    agree to fp32 rounding; (2) the gradient is affine in Y, gA(Y + E) - gA(Y) = -E S^T and gS(Y + E) - gS(Y) = -A^T E,
    checked exactly for a sparse E; (3) at an exact factorisation Y = A S the loss and the gradients vanish to
    rounding (the residual is pure cancellation: the third bf16 term earns its keep here)."""
    import torch
    M = N = 16384
    K = 64
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    Y = torch.rand((M, N), generator=gen, device="cuda", dtype=torch.float32)
    rng = np.random.default_rng(7)
    A = rng.random((M, K), dtype=np.float32)
    S = rng.random((K, N), dtype=np.float32)
    # sparse perturbation: 64 entries, values exactly representable
    ii = rng.integers(0, M, 64)
    jj = rng.integers(0, N, 64)
    vv = (rng.integers(1, 9, 64) * 0.25).astype(np.float32)
    Y2 = Y.clone()
    Y2[torch.from_numpy(ii).cuda(), torch.from_numpy(jj).cuda()] += torch.from_numpy(vv).cuda()
    Yx = torch.from_numpy(A).cuda() @ torch.from_numpy(S).cuda()   # fp32 product: Y - A S is at rounding level
    out = {}
    for mode in ("f32", "bf16x3", "f16x2"):
        with eng.DeviceNMF(M, N, K, mode=mode) as dev:
            dev.set_factors(A, S)
            dev.set_Y_device(Y.data_ptr(), ld=N, copy=False, keepalive=Y)
            gA, gS = dev.grad()
            loss = dev.loglike()
            dev.set_Y_device(Y2.data_ptr(), ld=N, copy=False, keepalive=Y2)
            gA2, gS2 = dev.grad()
            dev.set_Y_device(Yx.data_ptr(), ld=N, copy=False, keepalive=Yx)
            gAx, gSx = dev.grad()
            lossx = dev.loglike()
        out[mode] = (gA, gS, loss)
        # (2) affine in Y: only the touched rows / columns change, by -E S^T and -A^T E
        dA = np.zeros((M, K), np.float64)
        dS = np.zeros((K, N), np.float64)
        for i, j, v in zip(ii, jj, vv):
            dA[i] -= float(v) * S[:, j].astype(np.float64)
            dS[:, j] -= float(v) * A[i].astype(np.float64)
        scaleA, scaleS = np.abs(gA).max(), np.abs(gS).max()
        np.testing.assert_allclose(gA2.astype(np.float64) - gA, dA, atol=4e-6 * scaleA)
        np.testing.assert_allclose(gS2.astype(np.float64) - gS, dS, atol=4e-6 * scaleS)
        # (3) exact factorisation: residual entries are fp32 rounding of a K-term dot product (<= ~K eps |A||S|)
        assert lossx < 1e-9 * loss
        assert np.abs(gAx).max() < 2e-5 * scaleA and np.abs(gSx).max() < 2e-5 * scaleS
    # (1) three implementations, one answer
    for fast in ("bf16x3", "f16x2"):
        for a, b in zip(out["f32"][:2], out[fast][:2]):
            assert np.linalg.norm(a - b) <= 2e-6 * np.linalg.norm(a), fast
            np.testing.assert_allclose(b, a, rtol=0, atol=1e-5 * np.abs(a).max(), err_msg=fast)
        assert out[fast][2] == pytest.approx(out["f32"][2], rel=1e-6)


@pytest.mark.parametrize("pitch_extra,offset", [(0, 0), (64, 0), (3, 0), (64, 1)])
def test_zero_copy_Y_with_row_pitch_and_alignment(eng, orc, pitch_extra, offset):
    """Y adopted zero-copy from a device pointer (pmx_set_Y_device, copy=0) with a row pitch larger than N and with /
    without 16-byte alignment (the default split-bf16 kernel loads Y with dword loads and takes any pitch; the LDS-DMA
    variants need 16-byte aligned rows and fall back otherwise) -- same gradients either way."""
    import torch
    M, N, K = 512, 768, 64
    Y, A, S = orc.synthetic_problem(M, N, K, np.float32, seed=77)
    ld = N + pitch_extra
    buf = torch.zeros(M * ld + 8, dtype=torch.float32, device="cuda")
    view = buf[offset:offset + M * ld].view(M, ld)
    view[:, :N] = torch.from_numpy(Y).cuda()
    if pitch_extra:
        view[:, N:] = 1e30            # must never be read as data
    A64, S64, Y64 = A.astype(np.float64), S.astype(np.float64), Y.astype(np.float64)
    rA, rS = orc.residual_gradients(A64, S64, Y64)
    for mode in ("f32", "bf16x3", "f16x2"):
        with eng.DeviceNMF(M, N, K, mode=mode) as dev:
            dev.set_Y_device(view.data_ptr(), ld=ld, copy=False, keepalive=buf)
            dev.set_factors(A, S)
            gA, gS = dev.grad()
            loss = dev.loglike()
        np.testing.assert_allclose(gA, rA, rtol=2e-5, atol=2e-5 * np.abs(rA).max())
        np.testing.assert_allclose(gS, rS, rtol=2e-5, atol=2e-5 * np.abs(rS).max())
        assert loss == pytest.approx(orc.half_sq_residual(A64, S64, Y64), rel=2e-5)


def test_split_bf16_default_kernel_on_many_region_shapes(eng):
    """Whole-block shapes with every kind of region raggedness (row panels that do not divide evenly over the row
    regions, a last column region of 1..7 blocks, tiny and tall-thin problems): the default split-bf16 K1 against the
    exact-fp32 K1 (independent implementations), gradients and loss."""
    rng = np.random.default_rng(2024)
    shapes = [(128, 64), (128, 2048), (3712, 64), (1152, 1984), (2944, 4160), (640, 16448), (8320, 320), (4224, 2368)]
    for M, N in shapes:
        K = 64
        Y = rng.random((M, N), dtype=np.float32)
        A = rng.random((M, K), dtype=np.float32)
        S = rng.random((K, N), dtype=np.float32)
        out = {}
        for mode in ("f32", "bf16x3", "f16x2"):
            with eng.DeviceNMF(M, N, K, mode=mode) as dev:
                dev.set_Y(Y)
                dev.set_factors(A, S)
                gA, gS = dev.grad()
                out[mode] = (gA, gS, dev.loglike())
        for fast in ("bf16x3", "f16x2"):
            for a, b in zip(out["f32"][:2], out[fast][:2]):
                np.testing.assert_allclose(b, a, rtol=0, atol=1e-5 * np.abs(a).max(), err_msg="%s shape %dx%d" % (fast, M, N))
            assert out[fast][2] == pytest.approx(out["f32"][2], rel=1e-6)


@pytest.mark.parametrize("K", [64, 128])
@pytest.mark.parametrize("case", ["tiny_factors", "huge_factors", "mixed_magnitudes", "zero_A", "big_Y", "big_weights"])
def test_fp16_two_term_kernel_operand_scaling(eng, orc, case, K):
    """k_grad_f16_v8 / k_grad_f16_k128 scale A, S and the residual by powers of two taken from their maxima so that the
    fp16 terms stay in the normal range: factors of very different magnitudes (1e-4 .. 1e3, entries spanning eight decades,
    an all-zero factor, |Y| ~ 1e4, weights up to 50) must still give fp32-class gradients -- no overflow to inf, no flush
    to zero."""
    M, N = 384, 768
    rng = np.random.default_rng(hash(case) % 1000)
    Y, A, S = orc.synthetic_problem(M, N, K, np.float32, seed=5)
    W = None
    if case == "tiny_factors":
        A *= 1e-4
        S *= 3e-3
    elif case == "huge_factors":
        A *= 1e3
        S *= 40.0
    elif case == "mixed_magnitudes":
        A *= (10.0 ** rng.uniform(-6, 2, size=A.shape)).astype(np.float32)
        S *= (10.0 ** rng.uniform(-6, 2, size=S.shape)).astype(np.float32)
    elif case == "zero_A":
        A[:] = 0
    elif case == "big_Y":
        Y = (Y * 1e4).astype(np.float32)
    elif case == "big_weights":
        W = (50.0 * rng.random((M, N))).astype(np.float32)
    with eng.DeviceNMF(M, N, K, mode="f16x2") as dev:
        assert dev.k1_info()["kernel"] == ("k_grad_f16_v8" if K == 64 else "k_grad_f16_k128")
        dev.set_Y(Y)
        if W is not None:
            dev.set_W(W)
        dev.set_factors(A, S)
        gA, gS = dev.grad()
        loss = dev.loglike()
    x64 = [x.astype(np.float64) for x in (A, S, Y)] + ([W.astype(np.float64)] if W is not None else [])
    rA, rS = orc.residual_gradients(*x64)
    assert np.isfinite(gA).all() and np.isfinite(gS).all()
    np.testing.assert_allclose(gA, rA, rtol=2e-5, atol=2e-5 * max(np.abs(rA).max(), 1e-30))
    np.testing.assert_allclose(gS, rS, rtol=2e-5, atol=2e-5 * max(np.abs(rS).max(), 1e-30))
    assert loss == pytest.approx(orc.half_sq_residual(*x64), rel=2e-5)


@pytest.mark.parametrize("M,N,K", [(33, 47, 3), (150, 333, 11), (257, 513, 33), (1024, 640, 64), (1024, 768, 64), (2304, 4096, 64), (384, 1100, 100), (512, 512, 128)])
def test_weighted_gradient_matches_oracle(eng, orc, M, N, K):
    """D = W (A S - Y), loss = 1/2 sum W (Y - A S)^2 (nmf.py:13-41) with an M x N weight array incl. zero (masked)
    entries, ragged and whole-block shapes, in both arithmetic modes (split-bf16: the shapes of its default kernel)."""
    Y, A, S = orc.synthetic_problem(M, N, K, np.float32, seed=M + N + K)
    rng = np.random.default_rng(5)
    W = (0.1 + 2.0 * rng.random((M, N))).astype(np.float32)
    W[rng.random((M, N)) < 0.15] = 0
    with eng.DeviceNMF(M, N, K, mode="f32") as dev:
        dev.set_Y(Y)
        dev.set_W(W)
        dev.set_factors(A, S)
        gA, gS = dev.grad()
        loss = dev.loglike()
        dev.set_W(None)
        gA1, gS1 = dev.grad()
    A64, S64, Y64, W64 = (x.astype(np.float64) for x in (A, S, Y, W))
    rA, rS = orc.residual_gradients(A64, S64, Y64, W64)
    np.testing.assert_allclose(gA, rA, rtol=2e-5, atol=2e-5 * np.abs(rA).max())
    np.testing.assert_allclose(gS, rS, rtol=2e-5, atol=2e-5 * np.abs(rS).max())
    assert loss == pytest.approx(orc.half_sq_residual(A64, S64, Y64, W64), rel=2e-5)
    uA, uS = orc.residual_gradients(A64, S64, Y64)
    np.testing.assert_allclose(gA1, uA, rtol=2e-5, atol=2e-5 * np.abs(uA).max())
    if K <= 64:
        # the 16-bit split modes take weights where their fast kernels apply, and say so loudly elsewhere
        for fast in ("bf16x3", "f16x2"):
            with eng.DeviceNMF(M, N, K, mode=fast) as dev:
                dev.set_Y(Y)
                fr = dev.k1_info()["frame"]        # (M, N), or the zero-padded frame a ragged shape runs on (test_gpu_frame.py)
                if (K == 64 and fr[0] % 128 == 0 and fr[1] % 256 == 0) or dev.k1_info()["kernel"] == "k_grad_small":
                    dev.set_W(W)
                    dev.set_factors(A, S)
                    bA, bS = dev.grad()
                    bloss = dev.loglike()
                    np.testing.assert_allclose(bA, rA, rtol=2e-5, atol=2e-5 * np.abs(rA).max(), err_msg=fast)
                    np.testing.assert_allclose(bS, rS, rtol=2e-5, atol=2e-5 * np.abs(rS).max(), err_msg=fast)
                    assert bloss == pytest.approx(orc.half_sq_residual(A64, S64, Y64, W64), rel=2e-5)
                else:
                    with pytest.raises(NotImplementedError):
                        dev.set_W(W)


# ------------------------------------------------------------------------------------------------------------------
# chained in-place accumulation of gA (k_grad_f16_v8<CHAIN>): the workgroups of a chain add their contributions to one
# slab through the XCD's L2 instead of writing one slab per column region
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,mode,cap,want", [(4096, 4096, 64, "f16x2", 32, 2), (4096, 16384, 64, "f16x2", 32, 8), (4096, 16384, 64, "f16x2", 4, 4),
                                                 (8192, 8192, 64, "f16x2", 32, 8), (16384, 4096, 64, "f16x2", 32, 8), (2048, 16384, 64, "f16x2", 32, 4),
                                                 (4096, 4096, 64, "f32", 32, 2), (4096, 16384, 64, "f32", 32, 8), (8192, 8192, 32, "f32", 32, 8),
                                                 (2048, 16384, 32, "f32", 4, 4),
                                                 (4096, 4096, 64, "bf16x3", 32, 2), (4096, 16384, 64, "bf16x3", 32, 8), (8192, 8192, 64, "bf16x3", 4, 4),
                                                 # [r4] K = 128 (k_grad_f16_k128<.., CHAIN>): chains of 4 / 8 / 16, panel rotation stride 1 and 2
                                                 (4096, 4096, 128, "f16x2", 32, 4), (4096, 8192, 128, "f16x2", 32, 8), (8192, 4096, 128, "f16x2", 32, 8),
                                                 (16384, 2048, 128, "f16x2", 32, 8), (8192, 16384, 128, "f16x2", 32, 32), (8192, 16384, 128, "f16x2", 16, 16), (8192, 16384, 128, "f16x2", 4, 4)])
def test_chained_gradient_matches_oracle(eng, orc, monkeypatch, M, N, K, mode, cap, want):
    """Shapes whose region plan gives chains of 2 .. 16 workgroups, in the kernels that carry the protocol
    (k_grad_f16_v8 in mode f16x2 -- k_grad_f16_k128 at K = 128 --, k_grad_f32_pc in mode f32, k_grad_bf16_v7 in mode bf16x3): gradients and loss against the fp64 oracle, the same
    tolerance as every other K1; the chained launch must be the one that ran (no fault, no silent fall-back), twice in a
    row bit-identically (fixed order of the in-place sums), and equal to the slab path up to summation order."""
    monkeypatch.setenv("PMX_K1_CHAIN", str(cap))
    Y, A, S = orc.synthetic_problem(M, N, K, np.float32, seed=M + N)
    A[:, 0] += np.linspace(0.0, 1.0, M, dtype=np.float32)
    S[K - 1, :] += np.linspace(1.0, 0.0, N, dtype=np.float32)
    with eng.DeviceNMF(M, N, K, mode=mode) as dev:
        info = dev.k1_info()
        kernel = "k_grad_f16_k128" if K == 128 else {"f16x2": "k_grad_f16_v8", "f32": "k_grad_f32_pc", "bf16x3": "k_grad_bf16"}[mode]
        assert info["kernel"] == kernel and info["chain"] == want, info
        assert info["slabs_A"] == info["col_regions"] // want
        dev.set_Y(Y)
        dev.set_factors(A, S)
        gA, gS = dev.grad()
        gA2, gS2 = dev.grad()
        loss = dev.loglike()
        assert dev.k1_info()["chain_faults"] == 0 and dev.k1_info()["chain"] == want
        if K == 128:                     # the weighted chained instance (<HASW, CHAIN>)
            rng = np.random.default_rng(3)
            W = (0.1 + 2.0 * rng.random((M, N), dtype=np.float32)).astype(np.float32)
            W[rng.random((M, N), dtype=np.float32) < 0.15] = 0
            dev.set_W(W)
            wA, wS = dev.grad()
            assert dev.k1_info()["chain_faults"] == 0 and dev.k1_info()["chain"] == want
            idx = np.sort(np.random.default_rng(4).choice(M, 256, replace=False))
            D = W[idx].astype(np.float64) * (A[idx].astype(np.float64) @ S.astype(np.float64) - Y[idx].astype(np.float64))
            rAw = D @ S.astype(np.float64).T
            np.testing.assert_allclose(wA[idx], rAw, rtol=2e-5, atol=2e-5 * np.abs(rAw).max())
    assert np.array_equal(gA, gA2) and np.array_equal(gS, gS2)
    A64, S64, Y64 = A.astype(np.float64), S.astype(np.float64), Y.astype(np.float64)
    rA, rS = orc.residual_gradients(A64, S64, Y64)
    np.testing.assert_allclose(gA, rA, rtol=2e-5, atol=2e-5 * np.abs(rA).max())
    np.testing.assert_allclose(gS, rS, rtol=2e-5, atol=2e-5 * np.abs(rS).max())
    assert loss == pytest.approx(orc.half_sq_residual(A64, S64, Y64), rel=2e-5)
    monkeypatch.setenv("PMX_K1_CHAIN", "0")
    with eng.DeviceNMF(M, N, K, mode=mode) as dev:
        assert dev.k1_info()["chain"] == 0
        dev.set_Y(Y)
        dev.set_factors(A, S)
        sA, sS = dev.grad()
    np.testing.assert_allclose(gA, sA, rtol=0, atol=2e-6 * np.abs(rA).max())
    np.testing.assert_allclose(gS, sS, rtol=0, atol=2e-6 * np.abs(rS).max())   # (a chain member visits its row panels rotated)


def _subsampled_oracle_gradients(A, S, Yd, rows, cols):
    """fp64 gradients of 1/2 |A S - Y|^2 on a subset: gA[rows] needs only Y[rows, :], gS[:, cols] only Y[:, cols]."""
    import torch
    A64, S64 = A.astype(np.float64), S.astype(np.float64)
    Yr = Yd[torch.as_tensor(rows, device=Yd.device)].cpu().numpy().astype(np.float64)
    Yc = Yd[:, torch.as_tensor(cols, device=Yd.device)].cpu().numpy().astype(np.float64)
    gA_rows = (A64[rows] @ S64 - Yr) @ S64.T
    gS_cols = A64.T @ (A64 @ S64[:, cols] - Yc)
    return gA_rows, gS_cols


@pytest.mark.parametrize("M,N,K", [(128, 256, 64), (1024, 768, 64), (2304, 4096, 64), (8320, 512, 64), (128, 256, 32), (5120, 1024, 32),
                                   (4096, 4096, 32), (384, 16384, 32)])
@pytest.mark.parametrize("weighted", [False, True])
def test_exact_fp32_producer_consumer_kernel(eng, orc, M, N, K, weighted):
    """Mode f32 at K = 32 / 64, M % 128 = 0, N % 256 = 0 runs k_grad_f32_pc (the producer / consumer frame with fp32 MFMA
    operands; cfg2 and cfg3 / cfg5 in the library's default arithmetic): one region, many regions, short last row regions,
    more workgroups than CUs, with and without weights (zeros included); fp64 oracle, the tolerance of every fp32 K1;
    bitwise repeatable.  Neighbouring shapes keep k_grad_f32."""
    Y, A, S = orc.synthetic_problem(M, N, K, np.float32, seed=M + N + K)
    W = None
    if weighted:
        rng = np.random.default_rng(8)
        W = (0.1 + 2.0 * rng.random((M, N))).astype(np.float32)
        W[rng.random((M, N)) < 0.15] = 0
    with eng.DeviceNMF(M, N, K, mode="f32") as dev:
        assert dev.k1_info()["kernel"] == "k_grad_f32_pc", dev.k1_info()
        dev.set_Y(Y)
        if weighted:
            dev.set_W(W)
        dev.set_factors(A, S)
        gA, gS = dev.grad()
        loss = dev.loglike()
        gA2, gS2 = dev.grad()
    assert np.array_equal(gA, gA2) and np.array_equal(gS, gS2)
    x64 = [x.astype(np.float64) for x in (A, S, Y)] + ([W.astype(np.float64)] if weighted else [])
    rA, rS = orc.residual_gradients(*x64)
    np.testing.assert_allclose(gA, rA, rtol=2e-5, atol=2e-5 * np.abs(rA).max())
    np.testing.assert_allclose(gS, rS, rtol=2e-5, atol=2e-5 * np.abs(rS).max())
    assert loss == pytest.approx(orc.half_sq_residual(*x64), rel=2e-5)
    if M == 128 and not weighted:
        for Mr, Nr, Kr in ((128, 128, K), (136, 256, K)):
            with eng.DeviceNMF(Mr, Nr, Kr, mode="f32") as dev:
                assert dev.k1_info()["kernel"] in ("k_grad_f32", "k_grad_small")
        with eng.DeviceNMF(128, 256, 48, mode="f32") as dev:       # an in-between K runs the next tuned one (tests/test_gpu_frame.py)
            assert dev.k1_info()["kernel"] == "k_grad_f32_pc" and dev.k1_info()["frame_K"] == 64


@pytest.mark.parametrize("M,N", [(128, 128), (2048, 1024), (1024, 4096), (3200, 2176), (8192, 384), (8320, 16384)])
def test_k128_two_term_fp16_kernel(eng, orc, M, N):
    """K = 128 in mode f16x2 (k_grad_f16_k128: BASELINE's 8-GPU case, 8192-row shards of 65536 x 16384): one region, many
    regions, row regions whose last one is short (3200 rows = 25 panels over 13 regions of 2; 8320 = 65 panels), more
    workgroups than CUs; gradients and loss against the fp64 oracle at the tolerance of the fp32 kernel.  Shapes it does
    not take (ragged M or N) run the exact-fp32 kernel; a weighted likelihood runs the kernel's <HASW> instance."""
    Y, A, S = orc.synthetic_problem(M, N, 128, np.float32, seed=M + N)
    with eng.DeviceNMF(M, N, 128, mode="f16x2") as dev:
        info = dev.k1_info()
        assert info["kernel"] == "k_grad_f16_k128" and info["col_regions"] == N // 128, info
        dev.set_Y(Y)
        dev.set_factors(A, S)
        gA, gS = dev.grad()
        loss = dev.loglike()
        gA2, gS2 = dev.grad()
        # weighted likelihood (round 3: k_grad_f16_k128<HASW>; zeros included), then back to W == 1
        rng = np.random.default_rng(8)
        W = (0.1 + 2.0 * rng.random((M, N))).astype(np.float32)
        W[rng.random((M, N)) < 0.15] = 0
        dev.set_W(W)
        gAw, gSw = dev.grad()
        lossw = dev.loglike()
        dev.set_W(None)
        gA3, gS3 = dev.grad()
    assert np.array_equal(gA, gA2) and np.array_equal(gS, gS2)          # fixed summation order: bitwise repeatable
    assert np.array_equal(gA, gA3) and np.array_equal(gS, gS3)
    A64, S64, Y64 = (x.astype(np.float64) for x in (A, S, Y))
    rAw, rSw = orc.residual_gradients(A64, S64, Y64, W.astype(np.float64))
    np.testing.assert_allclose(gAw, rAw, rtol=2e-5, atol=2e-5 * np.abs(rAw).max())
    np.testing.assert_allclose(gSw, rSw, rtol=2e-5, atol=2e-5 * np.abs(rSw).max())
    assert lossw == pytest.approx(orc.half_sq_residual(A64, S64, Y64, W.astype(np.float64)), rel=2e-5)
    A64, S64, Y64 = (x.astype(np.float64) for x in (A, S, Y))
    rA, rS = orc.residual_gradients(A64, S64, Y64)
    np.testing.assert_allclose(gA, rA, rtol=2e-5, atol=2e-5 * np.abs(rA).max())
    np.testing.assert_allclose(gS, rS, rtol=2e-5, atol=2e-5 * np.abs(rS).max())
    assert loss == pytest.approx(orc.half_sq_residual(A64, S64, Y64), rel=2e-5)
    if M == 128:
        for Mr, Nr in ((136, 128), (128, 192)):
            with eng.DeviceNMF(Mr, Nr, 128, mode="f16x2") as dev:
                assert dev.k1_info()["kernel"] == "k_grad_f32"


@pytest.mark.parametrize("M,N", [(128, 256), (1024, 768), (4096, 4096), (5120, 1024), (384, 16384), (8320, 512)])
def test_k32_two_term_fp16_kernel(eng, orc, M, N):
    """[r4] K = 32 in mode f16x2 (k_grad_f16_k32: BASELINE cfg2's shape): one region, many regions, short last row regions,
    more workgroups than CUs; gradients and loss against the fp64 oracle at the tolerance of every fp32-class K1, bitwise
    repeatable, operands of very different magnitudes (the power-of-two scales).  Neighbouring shapes keep the split-bf16
    kernels; a weighted context says it has no kernel for that (the host wrapper reopens in fp32)."""
    Y, A, S = orc.synthetic_problem(M, N, 32, np.float32, seed=M + N)
    with eng.DeviceNMF(M, N, 32, mode="f16x2") as dev:
        info = dev.k1_info()
        assert info["kernel"] == "k_grad_f16_k32" and info["col_regions"] == N // 256 and info["slabs_S"] == info["row_regions"], info
        dev.set_Y(Y)
        dev.set_factors(A, S)
        gA, gS = dev.grad()
        loss = dev.loglike()
        gA2, gS2 = dev.grad()
        A2, S2 = (A * 1e-3).astype(np.float32), (S * 40.0).astype(np.float32)
        dev.set_factors(A2, S2)
        hA, hS = dev.grad()
        if M == 128:
            with pytest.raises(NotImplementedError):
                dev.set_W(np.ones((M, N), np.float32))
    assert np.array_equal(gA, gA2) and np.array_equal(gS, gS2)
    x64 = [x.astype(np.float64) for x in (A, S, Y)]
    rA, rS = orc.residual_gradients(*x64)
    np.testing.assert_allclose(gA, rA, rtol=2e-5, atol=2e-5 * np.abs(rA).max())
    np.testing.assert_allclose(gS, rS, rtol=2e-5, atol=2e-5 * np.abs(rS).max())
    assert loss == pytest.approx(orc.half_sq_residual(*x64), rel=2e-5)
    qA, qS = orc.residual_gradients(A2.astype(np.float64), S2.astype(np.float64), x64[2])
    np.testing.assert_allclose(hA, qA, rtol=2e-5, atol=2e-5 * np.abs(qA).max())
    np.testing.assert_allclose(hS, qS, rtol=2e-5, atol=2e-5 * np.abs(qS).max())
    if M == 128:
        for Mr, Nr, Kr in ((128, 128, 32), (136, 256, 32)):
            with eng.DeviceNMF(Mr, Nr, Kr, mode="f16x2") as dev:
                assert dev.k1_info()["kernel"] in ("k_grad_bf16", "k_grad_small")
        with eng.DeviceNMF(128, 256, 24, mode="f16x2") as dev:     # an in-between K runs the next tuned one (tests/test_gpu_frame.py)
            assert dev.k1_info()["kernel"] == "k_grad_f16_k32" and dev.k1_info()["frame_K"] == 32


@pytest.mark.parametrize("K,variant", [(64, "hh"), (64, "r3"), (32, "r3"), (128, "hh")])
def test_mode_f16x2r_removes_the_coherent_error(eng, orc, K, variant, monkeypatch):
    """What mode f16x2r is for.  With two fp16 terms per operand, P = A S carries the operands' representation errors -- 2^-23 each, far
    below P's accumulation noise entry by entry, but the SAME dS[k][n] in every row of P: gS = A^T R picks up A^T A dS, a sum that grows
    with M and not with sqrt(M).  On a problem with non-negative factors (every entry of A^T A positive) the error of gS against fp64 is
    about twice exact fp32's in mode f16x2 and back at exact fp32's in mode f16x2r, gA alike through S S^T -- whichever way the mode gets
    there: [r5] "hh", the residual from the high x high product + the exact K x K correction slab (k_grad_f16_v8<HH> / k_grad_f16_k128<HH>
    + k_gfix.hip; scratch/r5_gradient_error_table.py is its NumPy model), or [r4] "r3", third terms in a second accumulator (K = 32, and
    K = 64 under PMX_F16_R3=1; scratch/r4_emulate_modes.py)."""
    M, N = 2048, 2048
    Y, A, S = orc.synthetic_problem(M, N, K, np.float32, unity_S=True, seed=4321)
    r64 = orc.residual_gradients(A.astype(np.float64), S.astype(np.float64), Y.astype(np.float64))
    if variant == "r3" and K == 64:
        monkeypatch.setenv("PMX_F16_R3", "1")
    names = {64: ("k_grad_f32_pc", "k_grad_f16_v8", "k_grad_f16_v8_hh" if variant == "hh" else "k_grad_f16_v8_r3"),
             32: ("k_grad_f32_pc", "k_grad_f16_k32", "k_grad_f16_k32_r3"), 128: ("k_grad_f32", "k_grad_f16_k128", "k_grad_f16_k128_hh")}[K]
    err = {}
    for mode, name in zip(("f32", "f16x2", "f16x2r"), names):
        if mode == "f16x2":
            monkeypatch.delenv("PMX_F16_R3", raising=False)       # (the switch applies to any f16x2 context)
        elif variant == "r3" and K == 64:
            monkeypatch.setenv("PMX_F16_R3", "1")
        with eng.DeviceNMF(M, N, K, mode=mode) as dev:
            assert dev.k1_info()["kernel"] == name
            dev.set_Y(Y)
            dev.set_factors(A, S)
            g = dev.grad()
            g2 = dev.grad()
            assert np.array_equal(g[0], g2[0]) and np.array_equal(g[1], g2[1])
        err[mode] = [float(np.sqrt(((g[j] - r64[j]) ** 2).mean()) / np.abs(r64[j]).max()) for j in range(2)]
    assert err["f16x2r"][1] <= 0.7 * err["f16x2"][1], err          # gS: the coherent part is gone ...
    assert err["f16x2r"][1] <= 1.3 * err["f32"][1] and err["f16x2r"][0] <= 1.3 * err["f32"][0], err      # ... and both are exact fp32's class


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "f16x2", "f16x2r"])
def test_full_size_gradient_against_subsampled_oracle(eng, mode):
    """BASELINE's headline shape (16384 x 16384, K = 64): the gradients of 256 random rows of A and 256 random columns of
    S against the fp64 oracle (which needs only those rows / columns of Y), every arithmetic mode; mode f16x2 runs the
    chained kernel with 16 workgroups per chain."""
    import torch
    import bench
    M = N = 16384
    K = 64
    Yd, A, S = bench.make_problem_device(M, N, K, True, 1234, torch.device("cuda", 0))
    rng = np.random.default_rng(99)
    rows = np.sort(rng.choice(M, 256, replace=False))
    cols = np.sort(rng.choice(N, 256, replace=False))
    rA, rS = _subsampled_oracle_gradients(A, S, Yd, rows, cols)
    with eng.DeviceNMF(M, N, K, mode=mode) as dev:
        if mode == "f16x2":
            assert dev.k1_info()["chain"] == 16, dev.k1_info()
        dev.set_Y_device(Yd.data_ptr(), ld=N, copy=False, keepalive=Yd)
        dev.set_factors(A, S)
        gA, gS = dev.grad()
        assert dev.k1_info()["chain_faults"] == 0
    np.testing.assert_allclose(gA[rows], rA, rtol=2e-5, atol=2e-5 * np.abs(rA).max())
    np.testing.assert_allclose(gS[:, cols], rS, rtol=2e-5, atol=2e-5 * np.abs(rS).max())


def test_lambda_max_after_an_eigenvalue_crossing(eng, orc):
    """Three COLD starts on one context.  Orthogonal columns make A^T A diagonal; the column scales are swapped between the
    calls, so the largest eigenvalue moves from e_1 to e_2.  This was written as a warm-start test (after the first call the
    iterate is e_1, which the swap turns into an exact eigenvector of the SMALLER eigenvalue), but pmx_step_pgm resets a
    context without a solver before every call (reset_status: nmf.step_pgm is a function of its arguments), so each of the
    three calls starts from all-ones and none of them meets the crossing.  The warm start and the dominance probe that
    guards it are pinned by tests/test_gpu_step_rule.py::test_warm_start_survives_a_crossing, inside pgm()."""
    M, N, K = 64, 48, 2
    rng = np.random.default_rng(0)
    Q, _ = np.linalg.qr(rng.standard_normal((M, K)))
    S = rng.standard_normal((K, N)).astype(np.float32)          # mixed signs: no Perron argument
    with eng.DeviceNMF(M, N, K) as dev:
        dev.set_Y(np.zeros((M, N), np.float32))
        for scales in ((2.0, 1.0), (1.0, 2.0), (1.0, 2.0)):
            A = (Q * np.array(scales)).astype(np.float32)
            dev.set_factors(A, S)
            sA, sS = dev.step_pgm()
            oA, oS = orc.lipschitz_steps(A.astype(np.float64), S.astype(np.float64))
            assert sS == pytest.approx(oS, rel=1e-5), scales        # 1 / lmax(A^T A) = 1 / 4
            assert sA == pytest.approx(oA, rel=1e-5)
