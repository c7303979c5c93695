"""Mode f16x2r's correction slab (csrc/k_gfix.hip: k_gfix_gram, k_gfix_reduce, k_gfix_apply) against fp64 BY ITSELF, on every entry.

K1 <HH> forms its residual from the high x high fp16 product alone, R0 = a0 s0 - Y; the three launches of k_gfix.hip restore
A S - a0 s0 = A s_r + a_r s0 through K x K matrices as one more gradient slab (SlabRef::extra).  That slab is ~2^-12 of the gradient's
terms, so a test of the WHOLE gradient at fp32's noise level sees 2^-12 of what goes wrong inside it.

The inputs here make K1's own contribution exactly zero.  A and S are x0 + f with x0 in {0} u {n / 8: 2 <= n <= 15} (4 bits) and a
low part f that round-to-nearest at K1's power-of-two scale removes again, so the kernels' a0 and s0 are the x0's; P0 = a0 s0 has
8-bit products on a 2^-6 grid and every partial sum of at most 128 of them fits 24 bits: exact in fp32 in any order; and Y = P0.
Then R0 is exactly 0, every K1 slab is exactly 0 and what pmx_grad or an update kernel sees as "the gradient" is the correction
slab alone -- while the TRUE gradient of these inputs, oracle.residual_gradients in fp64, is that same correction.  No formula of
the kernel is restated for the reference.  Two families of low parts: "one" (f a multiple of ulp16(x0) / 1024, |multiple| <= 255:
x_r = f is ONE fp16 term) and "full" (f = m ulp32(x0), |m| < 2^12: x_r needs the second and third terms).  Variants: random signs,
all-zero rows, a maximum that IS a power of two, a maximum just below one (it rounds up into the next binade of fp16).

THE BOUND (derived from the kernel's term list, never from what the device returns).  For a block X (rows x K) with the other factor
Z the kernel evaluates C_X = X Qr + x_r Q0, Qr = z_r^T Z, Q0 = z0^T Z.  Per entry let
    s = |X| (|z_r|^T |Z|) + |x_r| (|z0|^T |Z|)                          (fp64 on the host).
Family "one":  |C_dev - C_ref| <= 2^-20 s.
  * k_gfix_gram holds Z as zh + zl (= z0 + z1) and z_r as z1.  In this family z_r = z1 and Z = z0 + z1 exactly: no term is omitted,
    its fp16 products are exact in fp32, and what is left is the fp32 accumulation of a share (<= 144 rows: 9 steps x 2 MFMAs per
    accumulator), the fp64 reduce of 128 partials and ONE rounding of Q to fp32.
  * k_gfix_apply splits the rows into xh + xl + xm (here xh = x0, xl = f, xm = 0) and each matrix into qh + ql with a remainder
    q' <= 2^-22 |q|:  X Qr ~ xh qh + xh ql + xl qh omits xl ql (<= 2^-11 2^-11) and xh q' (<= 2^-22);  x_r Q0 ~ xl qh + xl ql
    (+ xm qh) omits xl q' (<= 2^-22).  Each omitted product is <= 2^-22 of its half of s: 3 x 2^-22 s at the very worst.
  * What remains of 2^-20 s = 4 x 2^-22 s is 2^-22 s = 4 u (u = 2^-24) for the roundings: ~45 of them along one entry's path (18 in
    a Gram share, 1 for Q, <= 24 MFMAs of the apply, the two rescalings and the final sum), each relative to a partial sum that is
    below the absolute sums in s, independent, and averaged again over the K terms of the contraction: sqrt(45) x 0.4 u < 3 u.
    (The float32 NumPy evaluation of the same formula stays within ~2 x 2^-23 s: profiles/gfix_isolated_error.txt.)
Family "full":  add 1.25 |X| (|z_r - z1|^T |Z|), z1 the one-term fp16 image of z_r at the kernel's scale -- k_gfix_gram's documented
z_r ~ z1, evaluated exactly on the host; the quarter on top (2^-13 of the first half of s) covers the further omissions that appear
only here: xm qh in X Qr, xm ql and x_r - xl - xm in x_r Q0, Z - zh - zl in both matrices (2^-22 each).

K1's low-order path (<R3>: k_grad_f16_k32<R3>, k_grad_f16_v8<R3>, the loss-only pass of mode f16x2r) keeps a0 s0 - Y in one
accumulator -- exactly 0 here -- and ah (sl + s3) + (al + a3) sh in a second one: everything of A S - a0 s0 = a0 s_r + a_r s0 + a_r s_r
but the last product.  Its bound is twice that product's contribution, (|a_r| |s_r|) contracted with |S| / |A| on the host, plus 2^-20
of the absolute-sum scale of what the second accumulator carries, (|A| |s_r| + |a_r| |s0|) contracted likewise (the residual's own
fp32 accumulation, its two-term fp16 split and the three-product contraction are each relative to THAT, not to |A| |S|).  The loss:
with d = 2 |a_r| |s_r| + 2^-20 (|A| |s_r| + |a_r| |s0|) entry by entry,  |L_dev - L| <= sum(|R| d + d^2 / 2) + 2^-20 L.
The omitted product dominates these bounds: they resolve the low-order path to about 2^-10 of the correction, not to 2^-20 (the
device sits at 0.0003 .. 0.06 of them, profiles/gfix_isolated_error.txt) -- a missing a0 s_r or a_r s0 term, a wrong scale or a dropped
third term is seen, a last-bits error of the second accumulator is not.

Every update route must fold the slab: one iteration from these inputs, and the gradient the update kernel used must be grad()'s.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B20 = 2.0 ** -20
FULL_EXTRA = 1.25

# (M, N, K): small shapes that between them reach each code path of k_gfix.hip.  A Gram share is 16 ceil(rows / 2048) rows; a load batch of
# k_gfix_gram is 128 rows (K = 64: NB = 8 steps of 16; K = 128: the LDS exchange's eight steps), so a SECOND batch needs more than 16384 rows.
SLAB_SHAPES = [
    (128, 256, 64), (256, 256, 64),              # most of the 128 Gram shares are empty
    (2176, 512, 64),                             # 32-row shares, the last ones empty
    (16640, 256, 64), (256, 16640, 64),          # 144-row shares: a second, partial load batch; k_gfix_apply's second round past 256 workgroups
    (128, 128, 128), (1152, 1024, 128),          # KT = 4
    (8320, 128, 128), (128, 8320, 128),          # KT = 4: 80-row shares (one partial batch), the apply's second round past 128 workgroups
    (16640, 128, 128), (128, 16640, 128),        # KT = 4: 144-row shares -- the second batch rewrites the LDS fragments behind the trailing barrier
    (1000, 1500, 50), (1000, 1500, 100),         # padded frames, Kk > K
]
VARIANT_SHAPES = [(128, 256, 64), (128, 128, 128), (1000, 1500, 50)]
VARIANTS = ("signs", "zero_rows", "pow2", "below")
FAMILIES = ("one", "full")
R3_CONFIGS = [((128, 256, 32), None), ((5120, 1024, 32), None), ((128, 256, 64), "1"), ((2176, 512, 64), "1")]      # (shape, PMX_F16_R3)
LOSS_SHAPES = [(128, 256, 64), (2176, 512, 64), (128, 128, 128), (1152, 1024, 128)]
ROUTE_SHAPES = [(2176, 512, 64), (8320, 128, 128)]


def _cid(shape, family, variant):
    return "%dx%dx%d-%s-%s" % (shape + (family, variant))


SLAB_CASES = [(s, f, "plain") for s in SLAB_SHAPES for f in FAMILIES] + [(s, f, v) for s in VARIANT_SHAPES for v in VARIANTS for f in FAMILIES]
R3_RUNS = [(s, f, "plain", r3) for s, r3 in R3_CONFIGS for f in FAMILIES] + [((128, 256, 32), "full", "signs", None), ((128, 256, 64), "full", "signs", "1")]
R3_CASES = [r[:3] for r in R3_RUNS]
ALL_CASES = {_cid(*c): c for c in SLAB_CASES + R3_CASES}


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def kernel_scale(mx):
    """2^e with mx 2^e in [2^13, 2^14): gfix_scale / K1's eA, eS"""
    return 2.0 ** (14 - np.frexp(np.float32(mx))[1]) if mx > 0 else 1.0


def fp16_image(X, sc):
    """round-to-nearest fp16 of X sc, unscaled (X sc is exact: a power of two)"""
    with np.errstate(over="raise"):
        return (np.asarray(X, dtype=np.float64) * sc).astype(np.float16).astype(np.float64) / sc


PIN = {"plain": (1.875, 1.875), "signs": (1.875, 1.875), "zero_rows": (1.875, 1.875), "pow2": (2.0, 2.0),
       "below": (2.0 - 2.0 ** -13, 2.0)}                       # variant -> (pinned maximum, its high term)
PIN_FULL_BELOW = 2.0 - 2.0 ** -13 - 5 * 2.0 ** -23


def tall_factor(rng, rows, K, family, variant):
    """(X, x0) as float64, rows x K: X = x0 + f, built so that fp16 rounding at the kernel's scale returns x0"""
    pin, pin0 = PIN[variant]
    if variant == "below" and family == "full":
        pin = PIN_FULL_BELOW
    sc = kernel_scale(pin)
    n = rng.integers(1, 16, (rows, K))
    x0 = np.where(n == 1, 0.0, n / 8.0)
    e = np.floor(np.log2(np.where(x0 > 0, x0, 1.0)))

    def draw(shape_like):
        if family == "one":
            return rng.integers(-255, 256, shape_like.shape) * 2.0 ** (shape_like - 10 - 10)          # ulp16(x0) / 1024
        m = rng.integers(1, 2 ** 12, shape_like.shape) * np.where(rng.random(shape_like.shape) < 0.5, -1, 1)
        return m * 2.0 ** (shape_like - 23)                                                           # ulp32(x0)
    f = np.where(x0 > 0, draw(e), 0.0)
    for _ in range(64):
        bad = fp16_image(x0 + f, sc) != x0           # negative f next to a power of two
        if not bad.any():
            break
        f[bad] = draw(e[bad])
    else:
        raise AssertionError("redrawing did not converge")
    X = x0 + f
    if variant == "signs":
        sg = np.where(rng.random((rows, K)) < 0.5, -1.0, 1.0)
        X, x0 = X * sg, x0 * sg
    if variant == "zero_rows":
        idx = 2 + rng.choice(rows - 2, size=max(2, rows // 8), replace=False)       # (row 1 carries the pinned maximum)
        X[idx], x0[idx] = 0.0, 0.0
    X[1, 1] = pin
    x0[1, 1] = pin0
    return X, x0


@functools.lru_cache(maxsize=3)
def make_case(cid):
    """the inputs of a case: built once, shared, never modified"""
    (M, N, K), family, variant = ALL_CASES[cid]
    rng = np.random.default_rng([M, N, K, FAMILIES.index(family), (("plain",) + VARIANTS).index(variant)])
    A, a0 = tall_factor(rng, M, K, family, variant)
    St, st0 = tall_factor(rng, N, K, family, variant)
    Y = a0 @ st0.T
    out = dict(shape=(M, N, K), family=family, A64=A, St64=St, a0=a0, st0=st0, Y64=Y,
               A=A.astype(np.float32), S=np.ascontiguousarray(St.T.astype(np.float32)), Y=Y.astype(np.float32))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def block_terms(X, x0, Z, z0):
    """per entry of block X: s of the module docstring, the full family's extra term, and the float32 NumPy yardstick of C_X"""
    x_r, z_r = X - x0, Z - z0
    s = np.abs(X) @ (np.abs(z_r).T @ np.abs(Z)) + np.abs(x_r) @ (np.abs(z0).T @ np.abs(Z))
    z1 = fp16_image(z_r, kernel_scale(np.abs(Z).max()))
    t = np.abs(X) @ (np.abs(z_r - z1).T @ np.abs(Z))
    f = np.float32
    c32 = X.astype(f) @ (z_r.astype(f).T @ Z.astype(f)) + x_r.astype(f) @ (z0.astype(f).T @ Z.astype(f))
    c64 = X @ (z_r.T @ Z) + x_r @ (z0.T @ Z)
    return s, t, c32, c64


@functools.lru_cache(maxsize=3)
def reference(cid):
    """fp64: the true gradient of a case (= its correction), the bound's terms per entry, the float32 yardstick"""
    from oracle import nmf_oracle as orc
    c = make_case(cid)
    gA, gS = orc.residual_gradients(c["A64"], np.ascontiguousarray(c["St64"].T), c["Y64"])
    out = dict(C=(gA, gS.T))
    tA = block_terms(c["A64"], c["a0"], c["St64"], c["st0"])
    tS = block_terms(c["St64"], c["st0"], c["A64"], c["a0"])
    out["s"], out["t"], out["c32"], out["c64"] = zip(tA, tS)
    out["bound"] = tuple(B20 * s + (FULL_EXTRA * t if c["family"] == "full" else 0.0) for s, t in zip(out["s"], out["t"]))
    return out


def worst_ratio(got, want, scale):
    """largest |got - want| / scale; a zero scale admits no difference"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / scale)
    return float(np.max(np.where(np.isnan(r), np.inf, r)))


# ---------------------------------------------------------------------------------------------------------------------
# 1. CPU: the inputs do what the module docstring says
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(ALL_CASES))
def test_isolating_inputs_preconditions(cid):
    c = make_case(cid)
    M, N, K = c["shape"]
    for name in ("A", "Y"):
        assert np.array_equal(c[name].astype(np.float64), c[name + "64"]), name + " is not exactly float32"
    assert np.array_equal(c["S"].astype(np.float64), c["St64"].T)
    fits = []
    for X, x0 in ((c["A64"], c["a0"]), (c["St64"], c["st0"])):
        sc = kernel_scale(np.abs(X).max())
        assert 2.0 ** 13 <= np.abs(X).max() * sc < 2.0 ** 14
        assert np.array_equal(fp16_image(X, sc), x0), "the fp16 round trip at the kernel's scale does not return the high terms"
        assert np.array_equal(x0 * 8, np.round(x0 * 8)) and np.abs(x0).max() <= 2.0          # a 2^-3 grid: products on a 2^-6 grid
        x_r = X - x0
        assert np.array_equal((X.astype(np.float32) - x0.astype(np.float32)).astype(np.float64), x_r)     # x_r = X - x0 is an exact fp32 subtraction
        fits.append(fp16_image(x_r, sc) == x_r)
        assert (x_r[x0 == 0] == 0).all()
    # a0 s0: exact in fp32, with every partial sum in any order (all terms on a 2^-6 grid, the absolute sum below 2^24 grid steps)
    assert np.array_equal(c["Y64"].astype(np.float32).astype(np.float64), c["Y64"])
    assert np.array_equal(c["Y64"] * 64, np.round(c["Y64"] * 64))
    assert (np.abs(c["a0"]) @ np.abs(c["st0"]).T).max() * 64 < 2 ** 24
    ymax = np.abs(c["Y64"]).max()
    assert ymax > 0 and K * np.abs(c["A64"]).max() * np.abs(c["St64"]).max() / ymax < 2 ** 10            # the range guard trips at 2^16
    frac = np.mean([f[x != 0].mean() for f, x in zip(fits, (c["A64"], c["St64"]))])
    if c["family"] == "one":
        assert frac == 1.0, "a one-term residue does not fit one fp16 term"
    else:
        assert frac < 0.8, "the full family's residues fit one fp16 term"
    # the identity the whole module rests on: the kernel's formula IS the true gradient of these inputs
    ref = reference(cid)
    for j in range(2):
        assert np.abs(ref["c64"][j] - ref["C"][j]).max() <= 1e-9 * ref["s"][j].max()          # (fp64's own cancellation in A S - Y: ~2^-35 s)
        assert worst_ratio(ref["c32"][j], ref["C"][j], ref["s"][j]) <= B20                   # the yardstick meets the bound itself
        nz = ref["s"][j] > 0
        assert nz.any() and (np.abs(ref["C"][j])[nz] > 0).mean() > 0.9
    if "zero_rows" in cid:
        assert (ref["s"][0] == 0).any() and (ref["s"][1] == 0).any()


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as g
    g.build()
    from proxmin_amd import engine
    return engine


def open_case(eng, c, A=None, S=None, kernel_suffix="_hh"):
    M, N, K = c["shape"]
    dev = eng.DeviceNMF(M, N, K, mode="f16x2r")
    try:
        assert dev.k1_info()["kernel"].endswith(kernel_suffix), dev.k1_info()
        dev.set_Y(c["Y"])
        dev.set_factors(c["A"] if A is None else A, c["S"] if S is None else S)
    except BaseException:
        dev.close()
        raise
    return dev


def check_kernel_after(dev, suffix):
    info = dev.k1_info()
    assert info["kernel"].endswith(suffix) and not info["range_faults"] and not info["chain_faults"], info


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [_cid(*c) for c in SLAB_CASES])
def test_high_terms_alone_give_an_exactly_zero_gradient(eng, cid):
    """A = a0, S = s0, Y = a0 s0: K1 <HH>'s residual and the correction are both exactly zero (-0.0 passes)."""
    c = make_case(cid)
    with open_case(eng, c, c["a0"].astype(np.float32), np.ascontiguousarray(c["st0"].T.astype(np.float32))) as dev:
        gA, gS = dev.grad()
        check_kernel_after(dev, "_hh")
    assert (gA == 0).all() and (gS == 0).all()


def one_block_pass_folded(eng, c, j):
    """What a gradient pass for block j ALONE leaves in the slabs of both blocks, folded by a kernel that runs neither K1 nor k_gfix.
    pmx_time_grad only fills slabs; the one route that folds them without a gradient pass of its own is the line search with user
    operators: pmx_pgm_split(phase 0) evaluates the gradient at the evaluation point and marks it fresh, and pmx_pgm_bt_split(phase 0)
    then forms the operators' arguments from the slabs as they are (k_bt_update, first trial: it writes the folded gradient to G) and
    returns to the caller.  Under FISTA the evaluation point is a buffer of its own, copied from the factors at pgm_begin: it keeps
    a0 / s0 -- every slab of both blocks exactly zero after phase 0 -- while the factors proper become A / S for the one-block pass."""
    from proxmin_amd import _lib, operators as ops
    none = [ops.device_proxseq(None, 0), ops.device_proxseq(None, 1)]
    with open_case(eng, c, c["a0"].astype(np.float32), np.ascontiguousarray(c["st0"].T.astype(np.float32))) as dev:
        dev.pgm_begin(none, accelerated=True, backtracking=True, host_prox=(True, True), fixed_steps=(1.0, 1.0))
        dev.set_factors(c["A"], c["S"])
        dev.pgm_split(0)                                           # at a0 / s0: all slabs zero
        assert (dev.get(_lib.BUF_GA, 0) == 0).all() and (dev.get(_lib.BUF_GA, 1) == 0).all()
        ms = C.c_double()
        _lib.check(dev.lib.pmx_time_grad(dev.h, int(j == 0), int(j == 1), 1, C.byref(ms)))       # at A / S, block j alone
        need, _, _ = dev.pgm_bt_split(0)
        assert need == 3
        G = (dev.get(_lib.BUF_GA, 0), dev.get(_lib.BUF_GA, 1))
        check_kernel_after(dev, "_hh")
    return G


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [_cid(*c) for c in SLAB_CASES])
def test_correction_slab_matches_fp64_on_every_entry(eng, cid):
    c, ref = make_case(cid), reference(cid)
    with open_case(eng, c) as dev:
        g = dev.grad()
        check_kernel_after(dev, "_hh")
        g2 = dev.grad()
    got = (g[0], g[1].T)
    ratios = [worst_ratio(got[j], ref["C"][j], B20 * ref["s"][j]) for j in range(2)]
    yard = [worst_ratio(ref["c32"][j], ref["C"][j], B20 * ref["s"][j]) for j in range(2)]
    print("GFIX_ISOLATED %-32s device %.3f %.3f  float32-numpy %.3f %.3f   (|C - C_ref| / (2^-20 s), blocks A, S)" % (cid, ratios[0], ratios[1], yard[0], yard[1]))
    for j, name in enumerate("AS"):
        err = np.abs(got[j].astype(np.float64) - ref["C"][j])
        bad = err > ref["bound"][j]
        assert not bad.any(), "block %s: %d entries beyond the bound, the worst at %s by %.3g x" % (
            name, bad.sum(), np.unravel_index(np.argmax(err - ref["bound"][j]), err.shape), worst_ratio(got[j], ref["C"][j], ref["bound"][j]))
    assert np.array_equal(g[0], g2[0]) and np.array_equal(g[1], g2[1])           # two passes, the same bits
    # the one-block passes (bsdmm's): the wanted block's slab equals the two-block pass bit for bit, the other block's is not touched
    for j in range(2):
        G = one_block_pass_folded(eng, c, j)
        assert np.array_equal(G[j], g[j]), "a pass for block %s alone does not give the two-block pass's bits" % "AS"[j]
        assert (G[1 - j] == 0).all(), "a pass for block %s alone wrote the other block's slab" % "AS"[j]


# ---------------------------------------------------------------------------------------------------------------------
# 4. K1's low-order path
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def r3_reference(cid):
    from oracle import nmf_oracle as orc
    c = make_case(cid)
    A, St, a0, st0 = c["A64"], c["St64"], c["a0"], c["st0"]
    S = np.ascontiguousarray(St.T)
    R = A @ S - c["Y64"]
    gA, gS = orc.residual_gradients(A, S, c["Y64"])
    left_out = np.abs(A - a0) @ np.abs(St - st0).T                                     # |a_r| |s_r|, M x N
    carried = np.abs(A) @ np.abs(St - st0).T + np.abs(A - a0) @ np.abs(st0).T          # what the second accumulator holds, in absolute sums
    d = 2 * left_out + B20 * carried
    return dict(C=(gA, gS.T), bound=(d @ np.abs(St), d.T @ np.abs(A)), L=0.5 * np.sum(R * R),
                L_bound=np.sum(np.abs(R) * d + 0.5 * d * d) + B20 * 0.5 * np.sum(R * R))


@pytest.mark.gpu
@pytest.mark.parametrize("cid,r3", [(_cid(*r[:3]), r[3]) for r in R3_RUNS])
def test_r3_gradient_on_isolating_inputs(eng, monkeypatch, cid, r3):
    """k_grad_f16_k32<R3> (K = 32) and k_grad_f16_v8<R3> (K = 64 under PMX_F16_R3=1): the second accumulator's low-order products."""
    if r3 is not None:
        monkeypatch.setenv("PMX_F16_R3", r3)
    c, ref = make_case(cid), r3_reference(cid)
    with open_case(eng, c, c["a0"].astype(np.float32), np.ascontiguousarray(c["st0"].T.astype(np.float32)), "_r3") as dev:
        z = dev.grad()
        assert (z[0] == 0).all() and (z[1] == 0).all()
        dev.set_factors(c["A"], c["S"])
        g = dev.grad()
        check_kernel_after(dev, "_r3")
    got = (g[0], g[1].T)
    print("GFIX_ISOLATED_R3 %-28s PMX_F16_R3=%s  %.3f %.3f of the bound" % (cid, r3, worst_ratio(got[0], ref["C"][0], ref["bound"][0]), worst_ratio(got[1], ref["C"][1], ref["bound"][1])))
    for j, name in enumerate("AS"):
        err = np.abs(got[j].astype(np.float64) - ref["C"][j])
        assert (err <= ref["bound"][j]).all(), "block %s: %.3g x the bound" % (name, worst_ratio(got[j], ref["C"][j], ref["bound"][j]))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("family", FAMILIES)
def test_loss_only_pass_on_isolating_inputs(eng, shape, family):
    """loglike() in mode f16x2r: the loss-only <R3> pass of the K = 64 / 128 kernels; with the high terms alone exactly 0."""
    cid = _cid(shape, family, "plain")
    c, ref = make_case(cid), r3_reference(cid)
    with open_case(eng, c, c["a0"].astype(np.float32), np.ascontiguousarray(c["st0"].T.astype(np.float32))) as dev:
        assert dev.loglike() == 0
        dev.set_factors(c["A"], c["S"])
        L = dev.loglike()
        check_kernel_after(dev, "_hh")
    print("GFIX_ISOLATED_LOSS %-28s device %.17g fp64 %.17g  |diff| / bound %.3g" % (cid, L, ref["L"], abs(L - ref["L"]) / ref["L_bound"]))
    assert ref["L"] > 0 and abs(L - ref["L"]) <= ref["L_bound"]


# ---------------------------------------------------------------------------------------------------------------------
# 5. every route folds the slab: ONE iteration from the isolating inputs; the gradient the update kernel used is grad()'s
# ---------------------------------------------------------------------------------------------------------------------
ROUTES = ("pgm", "fista", "pgm_unity", "pgm_split", "adaprox_fused", "adaprox_chain", "bsdmm_A", "bsdmm_S", "sharded_pgm", "sharded_adaprox")
B1 = 0.9


def pow2_step(g):
    """a power of two (exact in every format) with step max|g| in (0.125, 0.25]"""
    return float(2.0 ** np.floor(np.log2(0.25 / np.abs(g).max())))


def assert_step_taken(X, X_new, g, step, what, x_term_only=False):
    """pgm routes (a power-of-two step): X_new = X - step g to one rounding of each term,
    |(X - X_new) / step - g| <= 2^-23 (|X| / step + |g|) per entry.
    bsdmm (x_term_only): 2^-23 |X| / step per entry, nothing more, wherever X != 0 (two roundings of 2^-24 |X| each: of the
    difference, and of step g, which is far below |X| here).  Where X == 0 that tolerance is zero while x - step g IS the rounded product
    of a step that is no power of two, so (X - X_new) / step cannot return g's bits: there the rounded product itself is checked,
    |X_new + step g| <= 2^-23 step |g| (its one rounding, 2^-24, and as much for the step's own rounding to float32)."""
    X, X_new, g = (np.asarray(v, dtype=np.float64) for v in (X, X_new, g))
    if x_term_only:
        z = X == 0
        assert z.any() and (np.abs(X_new + step * g)[z] <= 2.0 ** -23 * step * np.abs(g)[z]).all(), "%s: entries with X = 0 are not -step x grad()" % what
        X, X_new, g = X[~z], X_new[~z], g[~z]
    err = np.abs((X - X_new) / step - g)
    tol = 2.0 ** -23 * (np.abs(X) / step + (0.0 if x_term_only else np.abs(g)))
    assert (err <= tol).all(), "%s: the step taken is not step x grad() (%d entries, worst %.3g x the tolerance)" % (what, (err > tol).sum(), worst_ratio((X - X_new) / step, g, tol))


def assert_first_moment(Mj, g, what):
    want = ((1.0 - B1) * np.asarray(g, dtype=np.float64)).astype(np.float32)
    assert (np.abs(Mj.astype(np.float64) - want) <= np.spacing(np.abs(want))).all(), "%s: M is not float32((1 - b1) grad()) within one ulp" % what


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", ROUTE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_every_route_folds_the_correction_slab(eng, monkeypatch, shape, route):
    from functools import partial
    from proxmin_amd import _lib, operators as ops
    c = make_case(_cid(shape, "full", "plain"))
    none = [ops.device_proxseq(None, 0), ops.device_proxseq(None, 1)]
    if route.startswith("adaprox") or route == "sharded_adaprox":
        monkeypatch.setenv("PMX_TAIL_FUSED", "0" if route == "adaprox_chain" else "1")
    with open_case(eng, c) as dev:
        g = dev.grad()
        assert np.abs(g[0]).max() > 0 and np.abs(g[1]).max() > 0
        X = (c["A"], c["S"])
        steps = (pow2_step(g[0]), pow2_step(g[1]))
        shard = None
        if route.startswith("sharded"):
            from proxmin_amd import distributed
            shard = distributed.ShardEngine(dev, 1, 0, shape[0], algorithm=route.split("_")[1])       # world 1: nothing to reduce
        if route in ("pgm", "fista", "pgm_split", "pgm_unity", "sharded_pgm"):
            prox = list(none)
            if route == "pgm_unity":
                prox[0] = ops.device_proxseq(partial(ops.prox_unity_plus, axis=0), 0)
                assert ops.has_long_axis(prox[0])
            dev.pgm_begin(prox, accelerated=route == "fista", fixed_steps=steps, e_rel=(1e-9, 1e-9))
            if route == "pgm_split":
                dev.pgm_split(0)
                dev.pgm_split(2, steps=steps)
            elif shard is not None:
                shard.phase(0, 0)
                shard.phase(1, 0)
                dev.sync()
            else:
                assert dev.pgm_run(1).iterations == 1
            G = (dev.get(_lib.BUF_GA, 0), dev.get(_lib.BUF_GA, 1))
            Xn = dev.get_factors()
            for j, name in enumerate("AS"):
                assert np.array_equal(G[j], g[j]), "%s: the gradient k_pgm_update folded for block %s is not grad()'s" % (route, name)
                if not (route == "pgm_unity" and j == 0):
                    assert_step_taken(X[j], Xn[j], g[j], steps[j], "%s block %s" % (route, name))
        elif "adaprox" in route:
            dev.adaprox_begin(none, scheme="adam", fixed_alpha=(1e-3, 1e-3), check_convergence=False)
            assert dev.k1_info()["tail_fused"] == (route != "adaprox_chain")
            if shard is not None:
                shard.phase(0, 0, B1, B1)
                shard.phase(1, 0, B1, B1, 0)
                dev.sync()
            else:
                assert dev.adaprox_run([B1], B1).iterations == 1
            for j, name in enumerate("AS"):
                assert_first_moment(dev.get(_lib.BUF_MA, j), g[j], "%s block %s" % (route, name))
        else:
            j = "AS".index(route[-1])
            plus = [[ops.device_proxseq(ops.prox_plus, 0)], [ops.device_proxseq(ops.prox_plus, 1)]]
            dev.bsdmm_begin(none, plus, e_rel=(1e-9, 1e-9), update_order=[j])        # Z = X, U = 0: the first step is X - step_f g
            r = dev.bsdmm_run(1)
            step = float(np.float32(r.steps[j]))
            assert step > 0
            Xn = dev.get_factors()
            assert np.array_equal(Xn[1 - j], X[1 - j])
            # tolerance: 2^-23 |X| / step per entry (assert_step_taken says what that covers, and what is asked where X = 0)
            assert_step_taken(X[j], Xn[j], g[j], step, route, x_term_only=True)
        check_kernel_after(dev, "_hh")
