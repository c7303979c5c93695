// k_gfix_dev.h -- the K x K correction of the <HH> K1s (k_gfix.hip: what it computes and why) as callable pieces, ONE copy for the
// stand-alone kernels (k_gfix_gram / k_gfix_reduce / k_gfix_apply) and for the K1 that carries the three stages on its own idle waves
// (k_grad_f16_v8<.., GF>).  Both run the same arithmetic in the same order: the correction slab is the same bit for bit whoever formed it.
//
// WT (the pieces inside K1): producers and readers of a stage live in ONE launch, on different XCDs, so there is no kernel boundary
// between them -- partials and Q are stored write-through and read with agent-scope loads (served by memory, never by an XCD's own L2,
// which may still hold the previous launch's lines), as k_ada_tail does with its records.  The stand-alone kernels keep plain accesses.
#pragma once
#include "pmx_common.h"

constexpr int GFIX_PARTS = 128;          // partial matrices per factor (one workgroup each)

struct GfixArgs {
    const float* X[2];       // K1's operands: A (M x K), St (N x K), row pitch K (K1's K: 64 or 128)
    int64_t rows[2];
    int K;
    const float* absmax;     // [2][256] partial maxima of |A|, |St|: the operand scales are K1's own (k_absmax / the update kernels' finish)
    float* part;             // [2][GFIX_PARTS][2][K * K]
    float* Q;                // [2][2][K * K]: Q[f][0] = x0^T X, Q[f][1] = x_r^T X of factor f
    float* out[2];           // correction slab of block j (rows x ld)
    int ld;
    int want[2];             // correct gA / gSt
    const DevStatus* status;
    long long* prof;         // tuning (PMX_GFIX_PROF=1): 100 MHz time stamps of workgroup (0, 0): [0..3] gram, [4..5] reduce, [6..10] apply; else nullptr
};

typedef _Float16 gf16x8 __attribute__((ext_vector_type(8)));

template <bool WT>
__device__ __forceinline__ float gfix_ld(const float* p) {
    if constexpr (WT) return __builtin_bit_cast(float, __hip_atomic_load(reinterpret_cast<const unsigned*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    else return *p;
}
template <bool WT>
__device__ __forceinline__ void gfix_st(float* p, float v) {
    if constexpr (WT) __hip_atomic_store(reinterpret_cast<unsigned*>(p), __builtin_bit_cast(unsigned, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}

// 2^e with max|X_f| 2^e in [2^13, 2^14): K1's scale (k_grad_f16_v8: eA / eS).  (A workgroup barrier inside: not for role-split code.)
__device__ __forceinline__ float gfix_scale(const float* absmax, int f, float* red) {
    float m = 0.f;
    for (int i = threadIdx.x; i < 256; i += blockDim.x) m = fmaxf(m, absmax[f * 256 + i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    float mx = red[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) mx = fmaxf(mx, red[i]);
    int q = 0;
    (void)frexpf(mx, &q);
    return ldexpf(1.f, mx > 0.f ? 14 - q : 0);
}

// butterfly exchange with the lane index in hand: __shfl_xor derives its addresses from the hardware lane id, and inside K1 the compiler then
// shares them with the kernel's first reductions and carries them through the whole launch (registers K1's loops do not have)
__device__ __forceinline__ float gfix_xor_f(float v, int o, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((lane ^ o) << 2, __builtin_bit_cast(int, v)));
}
// the same number by ONE wave on its own (no barrier, no LDS: role-split code, and code that would otherwise carry the scale in a register
// across a whole launch).  Maxima are exact whatever their order.
__device__ __forceinline__ float gfix_scale_wave(const float* absmax, int f, int lane) {
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) m = fmaxf(m, absmax[f * 256 + lane + 64 * i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, gfix_xor_f(m, o, lane));
    int q = 0;
    (void)frexpf(m, &q);
    return ldexpf(1.f, m > 0.f ? 14 - q : 0);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Gram stage.  KT = K / 32.  Four waves; wave W owns the output tiles (ti, tj) of linear index W KT^2 / 4 .. (KT = 2: one tile, KT = 4: a
// tile row) of both matrices and walks ALL rows of share `part` (of GFIX_PARTS) of factor X, sixteen at a time (one 32 x 32 x 16 step).
// The stage is a chain of memory round trips, not arithmetic (a share is 128 rows at 16384): the loads of NB steps are in flight together.
//   gfix_gram_share    the share's rows
//   gfix_gram_request  one batch of loads (NB steps of sixteen rows) from row rb on
//   gfix_gram_compute  split and contract every batch of the share (the first one requested by the caller), sc = the operand scale
//   gfix_gram_store    the wave's tiles of both partial matrices, un = 1 / sc^2
// ---------------------------------------------------------------------------------------------------------------------------
template <int KT> struct GfixGram {
    static constexpr int K = 32 * KT, TPW = KT * KT / 4, NB = KT == 2 ? 8 : 4;    // (K = 64: a 128-row share is ONE batch of loads, K = 128: two)
};
__device__ __forceinline__ void gfix_gram_share(int64_t rows, int part, int64_t& r0, int64_t& r1) {
    const int64_t per = 16 * ((rows + 16 * GFIX_PARTS - 1) / (16 * GFIX_PARTS));
    r0 = (int64_t)part * per;
    r1 = r0 + per < rows ? r0 + per : rows;
}
// Xf: the factor's base (uniform).  SB (inside K1, whose waves have 256 registers, not 512): ONE wave-uniform base per batch and a 32-bit
// offset per row instead of a 64-bit address per load -- rows past the share's end read the batch's first row (always inside) and are
// zeroed like the others'.  The same values either way.
template <int KT, int NB, bool SB>
__device__ __forceinline__ void gfix_gram_request(const float* Xf, int64_t rb, int64_t r1, int l31, int hi, float (&v)[NB][KT][8]) {
    constexpr int K = GfixGram<KT>::K;
    if constexpr (SB) {
        const char* base = reinterpret_cast<const char*>(Xf + rb * K);
        const int nrow = (int)(r1 - rb);
#pragma unroll
        for (int s = 0; s < NB; ++s)
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int rr = 16 * s + 8 * hi + q;
                const bool in = rr < nrow;
                const unsigned off = (unsigned)((in ? rr : 0) * K + l31) * 4u;
#pragma unroll
                for (int c = 0; c < KT; ++c) {
                    const float x = *reinterpret_cast<const float*>(base + off + 128u * c);
                    v[s][c][q] = in ? x : 0.f;
                }
            }
    } else {
        const float* X = Xf + l31;
#pragma unroll
        for (int s = 0; s < NB; ++s)
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int64_t r = rb + 16 * s + 8 * hi + q;
#pragma unroll
                for (int c = 0; c < KT; ++c) v[s][c][q] = r < r1 ? X[r * K + 32 * c] : 0.f;
            }
    }
}
template <int KT, int W, int NB, bool SB>
__device__ __forceinline__ void gfix_gram_compute(const float* X, int64_t r0, int64_t r1, int l31, int hi, float sc, float (&v)[NB][KT][8],
                                                  f32x16 (&acc0)[GfixGram<KT>::TPW], f32x16 (&accr)[GfixGram<KT>::TPW]) {
    constexpr int TPW = GfixGram<KT>::TPW;
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc0[t][i] = 0.f; accr[t][i] = 0.f; }
    for (int64_t rb = r0; rb < r1; rb += 16 * NB) {
        gf16x8 h[NB][KT], l[NB][KT];
#pragma unroll
        for (int s = 0; s < NB; ++s)
#pragma unroll
            for (int c = 0; c < KT; ++c)
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float x = v[s][c][q] * sc;
                    const _Float16 t = (_Float16)x;
                    h[s][c][q] = t;
                    l[s][c][q] = (_Float16)(x - (float)t);
                }
        if (rb + 16 * NB < r1) gfix_gram_request<KT, NB, SB>(X, rb + 16 * NB, r1, l31, hi, v);
#pragma unroll
        for (int s = 0; s < NB; ++s)
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                constexpr int idx0 = W * TPW;
                const int ti = (idx0 + t) / KT, tj = (idx0 + t) % KT;          // (compile-time after unrolling)
                acc0[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(h[s][ti], l[s][tj], acc0[t], 0, 0, 0);
                accr[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(l[s][ti], l[s][tj], accr[t], 0, 0, 0);
                acc0[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(h[s][ti], h[s][tj], acc0[t], 0, 0, 0);
                accr[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(l[s][ti], h[s][tj], accr[t], 0, 0, 0);
            }
    }
}
// out: the share's pair of partial matrices
template <int KT, int W, bool WT>
__device__ __forceinline__ void gfix_gram_store(float* out, int l31, int hi, float un, const f32x16 (&acc0)[GfixGram<KT>::TPW], const f32x16 (&accr)[GfixGram<KT>::TPW]) {
    constexpr int K = GfixGram<KT>::K, TPW = GfixGram<KT>::TPW;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int ti = (W * TPW + t) / KT, tj = (W * TPW + t) % KT;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int kp = 32 * ti + (i & 3) + 8 * (i >> 2) + 4 * hi, k = 32 * tj + l31;
            gfix_st<WT>(out + kp * K + k, acc0[t][i] * un);
            gfix_st<WT>(out + K * K + kp * K + k, accr[t][i] * un);
        }
    }
}
// one share, start to end, with the scale in hand (inside K1; the stand-alone kernel interleaves its scale's round trip and its stamps).
// NB: steps of sixteen rows per batch of loads -- the rows enter the MFMAs in the same order whatever the batch, so the sums do not
// depend on it; K1's waves have 256 registers where the stand-alone kernel's have 512, and take a quarter of its batch (NB = 2: with 4 the chained
// instance spilled two registers more than its counterpart without the ride).
template <int KT, int W, bool WT, int NB>
__device__ __forceinline__ void gfix_gram_one(const float* Xf, int64_t rows, int part, float* partBase, int f, float sc, int lane) {
    constexpr int K = GfixGram<KT>::K;
    const int l31 = lane & 31, hi = lane >> 5;
    int64_t r0, r1;
    gfix_gram_share(rows, part, r0, r1);
    float v[NB][KT][8];
    f32x16 acc0[GfixGram<KT>::TPW], accr[GfixGram<KT>::TPW];
    if (r0 < r1) gfix_gram_request<KT, NB, true>(Xf, r0, r1, l31, hi, v);
    gfix_gram_compute<KT, W, NB, true>(Xf, r0, r1, l31, hi, sc, v, acc0, accr);
    gfix_gram_store<KT, W, WT>(partBase + ((int64_t)f * GFIX_PARTS + part) * 2 * K * K, l31, hi, 1.f / (sc * sc), acc0, accr);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Reduce stage: share bx (of 4 n / 256, n = 2 K^2) of factor f, 256 threads (t256 = the thread's index among them; a quad never
// straddles a wave and every lane takes part in the shuffles).  Entry e of Q[f][m]: four threads fold 32 partials each (all loads in
// flight), then the four sums in a fixed order.
// ---------------------------------------------------------------------------------------------------------------------------
template <bool WT>
__device__ __forceinline__ void gfix_reduce_share(const float* part, float* Q, int K, int f, int bx, int t256) {
    const int n = 2 * K * K;
    const int t = bx * 256 + t256, e = t >> 2, q = t & 3;
    static_assert(GFIX_PARTS == 128, "four threads x 32 partials");
    double s = 0.0;
    if (e < n) {
        const float* p = part + (int64_t)f * GFIX_PARTS * n + (int64_t)(q * 32) * n + e;
        float v[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) v[i] = gfix_ld<WT>(p + (int64_t)i * n);
#pragma unroll
        for (int i = 0; i < 32; ++i) s += (double)v[i];
    }
    const int base = t256 & 60;
    double tot = __shfl(s, base);
#pragma unroll
    for (int i = 1; i < 4; ++i) tot += __shfl(s, base + i);
    if (e < n && q == 0) gfix_st<WT>(Q + (int64_t)f * n + e, (float)tot);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Apply stage.  C_X = X Qr(Z) + x_r Q0(Z): one wave per task (32 rows, 32 output columns).  Split-fp16 MFMA like K1's own contractions
// (exact-fp32 MFMA runs at the vector rate: the same product took 13 us at 16384 rows x 64, MFMA-bound): the rows as three fp16 terms of
// X 2^e (xh + xl + xm: xh is K1's a0 / s0, xl + xm = x_r to 2^-22), each matrix as two terms scaled by a power of two from its own
// maximum, transposed in LDS so that a lane's eight contraction indices are one 16-byte read;
// X Qr ~ xh qh + xh ql + xl qh,  x_r Q0 ~ xl qh + xl ql + xm qh,  two accumulators (two scales).
// NT threads (a multiple of K, NT / 64 waves) stage the other factor's matrices ONCE per workgroup; staging is element-wise and a task is
// a wave's own, so the sums do not depend on NT:
//   gfix_apply_fetch    this thread's entries of both matrices and the per-wave maxima into redq[2][NT / 64]
//   [workgroup barrier]
//   gfix_apply_planes   the matrices' scales (sq) and the four transposed fp16 planes into qpl (4 K (K + 8) halves)
//   [workgroup barrier]
//   gfix_apply_load_x / gfix_apply_task   per wave
// ---------------------------------------------------------------------------------------------------------------------------
template <int KT, int NT> struct GfixApply {
    static constexpr int K = 32 * KT, LDQ = K + 8;          // halves per row of a transposed plane (+ 16 bytes: the 16-byte reads of 32 rows spread over the banks)
    static constexpr int NW = NT / 64, TPK = NT / K, NBLK = K / 8 / TPK;        // waves; threads per column, blocks of eight k' per thread
    static_assert(NT % K == 0 && (K / 8) % TPK == 0, "");
};
// The matrices, read so that the TRANSPOSED planes are written with one 16-byte store per eight k': thread t takes column k = t % K and the
// blocks of eight k' = 8 (t / K + (NT / K) i) .. -- 8 scalar loads per block, each coalesced across the lanes (consecutive k), one
// conflict-free ds_write_b128 per term.  (A float4-per-thread read with sixty-four 2-byte scattered stores, 16-way bank conflicts, was the
// kernel: 13 us of its 14.)   src: Q of the OTHER factor, [2][K * K]
template <int KT, int NT, bool WT>
__device__ __forceinline__ void gfix_apply_fetch(const float* src, int tid, float (&tq)[2][GfixApply<KT, NT>::NBLK][8], float* redq) {
    using G = GfixApply<KT, NT>;
    constexpr int K = G::K, TPK = G::TPK, NBLK = G::NBLK, NW = G::NW;
    const int kcol = tid % K, kb0 = tid / K, lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int i = 0; i < NBLK; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) tq[m][i][e] = gfix_ld<WT>(src + (size_t)m * K * K + (size_t)(8 * (kb0 + TPK * i) + e) * K + kcol);
    float mx[2] = {0.f, 0.f};
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int i = 0; i < NBLK; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) mx[m] = fmaxf(mx[m], fabsf(tq[m][i][e]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mx[0] = fmaxf(mx[0], gfix_xor_f(mx[0], o, lane)); mx[1] = fmaxf(mx[1], gfix_xor_f(mx[1], o, lane)); }
    if (lane == 0) { redq[w] = mx[0]; redq[NW + w] = mx[1]; }
}
template <int KT, int NT>
__device__ __forceinline__ void gfix_apply_planes(_Float16* qpl, int tid, const float (&tq)[2][GfixApply<KT, NT>::NBLK][8], const float* redq, float (&sq)[2]) {
    using G = GfixApply<KT, NT>;
    constexpr int K = G::K, LDQ = G::LDQ, TPK = G::TPK, NBLK = G::NBLK, NW = G::NW;
    const int kcol = tid % K, kb0 = tid / K;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        float v = redq[m * NW];
#pragma unroll
        for (int i = 1; i < NW; ++i) v = fmaxf(v, redq[m * NW + i]);
        int q = 0;
        (void)frexpf(v, &q);
        sq[m] = ldexpf(1.f, v > 0.f ? 14 - q : 0);
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {            // matrix m (0 = Q0, 1 = Qr) -> planes 2 (1 - m), + 1: Qr first
        _Float16* ph = qpl + (size_t)((1 - m) * 2) * K * LDQ + (size_t)kcol * LDQ;
        _Float16* pl = ph + (size_t)K * LDQ;
#pragma unroll
        for (int i = 0; i < NBLK; ++i) {
            gf16x8 h8, l8;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = tq[m][i][e] * sq[m];
                const _Float16 h = (_Float16)v;
                h8[e] = h;
                l8[e] = (_Float16)(v - (float)h);
            }
            *reinterpret_cast<gf16x8*>(ph + 8 * (kb0 + TPK * i)) = h8;
            *reinterpret_cast<gf16x8*>(pl + 8 * (kb0 + TPK * i)) = l8;
        }
    }
}
// this lane's row of task t, components 16 ks + 8 hi .. + 7 (the MFMA's A operand: i = lane & 31, k = 8 (lane >> 5) ..)
template <int KT>
__device__ __forceinline__ void gfix_apply_load_x(const float* X, int64_t rows, int64_t t, int l31, int hi, f32x4 (&x)[2 * KT][2]) {
    constexpr int K = 32 * KT;
    const int64_t row_ = (t / KT) * 32 + l31;
    const f32x4* xr = reinterpret_cast<const f32x4*>(X + (row_ < rows ? row_ : 0) * K + 8 * hi);
#pragma unroll
    for (int ks = 0; ks < K / 16; ++ks) { x[ks][0] = xr[4 * ks]; x[ks][1] = xr[4 * ks + 1]; }
}
// sc: the scale of X (K1's own), sq: the matrices' (gfix_apply_planes)
template <int KT>
__device__ __forceinline__ void gfix_apply_task(int64_t rows, float* out, int ld, const _Float16* qpl, int64_t task, int l31, int hi,
                                                float sc, const float (&sq)[2], const f32x4 (&x)[2 * KT][2]) {
    constexpr int K = 32 * KT, LDQ = K + 8;
    const int64_t rt = task / KT;
    const int c = (int)(task % KT);
    const bool live = rt * 32 + l31 < rows;
    f32x16 acc1, acc2;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc1[i] = 0.f; acc2[i] = 0.f; }
    const _Float16* qb = qpl + (size_t)(32 * c + l31) * LDQ + 8 * hi;
#pragma unroll
    for (int ks = 0; ks < K / 16; ++ks) {
        gf16x8 xh, xl, xm;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = (live ? x[ks][e >> 2][e & 3] : 0.f) * sc;
            const _Float16 h = (_Float16)v;
            const float r1 = v - (float)h;
            const _Float16 l = (_Float16)r1;
            xh[e] = h; xl[e] = l; xm[e] = (_Float16)(r1 - (float)l);
        }
        const gf16x8 qrh = *reinterpret_cast<const gf16x8*>(qb + 16 * ks);
        const gf16x8 qrl = *reinterpret_cast<const gf16x8*>(qb + (size_t)K * LDQ + 16 * ks);
        const gf16x8 q0h = *reinterpret_cast<const gf16x8*>(qb + (size_t)2 * K * LDQ + 16 * ks);
        const gf16x8 q0l = *reinterpret_cast<const gf16x8*>(qb + (size_t)3 * K * LDQ + 16 * ks);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl, qrh, acc1, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(xm, q0h, acc2, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, qrl, acc1, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl, q0l, acc2, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, qrh, acc1, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl, q0h, acc2, 0, 0, 0);
    }
    const float u1 = 1.f / (sc * sq[1]), u2 = 1.f / (sc * sq[0]);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t r = rt * 32 + (i & 3) + 8 * (i >> 2) + 4 * hi;
        if (r < rows) out[r * ld + 32 * c + l31] = acc1[i] * u1 + acc2[i] * u2;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The ride inside K1 (k_grad_f16_v8<.., GF>, K = 64): what the launch needs beside its own arguments.  Stage s of workgroup b has
// happened in THIS launch when arrive[s * GFIX_RIDE_WGS + b] == seq (seq: the launch's number, armed by the host; a launch that is
// skipped -- a halted chain of kernels -- leaves the words alone and the next one does not care: nothing is counted).  Only the first
// GFIX_RIDE_WGS workgroups of a launch hold shares of the gram and reduce stages (256 of each at K = 64): they are dispatched first.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int GFIX_RIDE_WGS = 2 * GFIX_PARTS;
struct GfixRide {
    int64_t rows[2];         // the factors' own rows (K1's frame may be larger)
    float* part;             // GfixArgs::part, ::Q, ::out
    float* Q;
    float* out[2];
    unsigned* arrive;        // [2][GFIX_RIDE_WGS]
    unsigned seq;            // 0: no ride in this launch
    int inject;              // tests: report the ride's fault code from this launch (nothing waits longer, nothing traps)
};
// (This, gfix_xor_f and the gram's batch of 2 x 16 rows are there for the register allocator of one toolchain, not for the hardware: none of them
// changes a value.  The contract is tests/test_build_resources_gfix.py -- the instances that carry the stages spill no more than those that do not --
// and a compiler that no longer needs the coaxing, or needs another, shows there.)
// The thread's index for a stage inside K1, opaque to the compiler: what a stage derives from it (lane, row and column offsets) is computed where
// the stage runs instead of being carried from the top of the kernel through K1's loops, whose waves have no register to spare.
__device__ __forceinline__ int gfix_ride_tid() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

// all of the first n (<= GFIX_RIDE_WGS) words equal seq?  One wave; uniform result.
__device__ __forceinline__ bool gfix_ride_arrived(const unsigned* words, int n, unsigned seq, int lane) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < GFIX_RIDE_WGS / 64; ++i) {
        const int b = lane + 64 * i;
        const unsigned v = b < n ? __hip_atomic_load(words + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : seq;
        ok = ok && v == seq;
    }
    return __builtin_amdgcn_ballot_w64(!ok) == 0;
}
// Bounded wait of one wave (ChainLink::wait's manner: 20 ms, and out at once when the chain of kernels is halted).  false: do not go on
// (the fault has been reported, or somebody else's was seen).
__device__ __forceinline__ bool gfix_ride_wait(const unsigned* words, int n, unsigned seq, const DevStatus* st, DevStatus* wst, int lane) {
    bool ok = gfix_ride_arrived(words, n, seq, lane);
    if (!ok) {
        const long long t0 = wall_clock64();          // 100 MHz
        for (int spins = 1;; ++spins) {
            __builtin_amdgcn_s_sleep(8);
            if (gfix_ride_arrived(words, n, seq, lane)) { ok = true; break; }
            if ((spins & 15) == 0) {
                if (chain_halted(st)) break;
                if (wall_clock64() - t0 > 2000000) {
                    if (lane == 0) {
                        wst->k1_fault = K1_FAULT_GFIX;
                        wst->reason = HALT_ERROR;
                        __threadfence();
                        wst->halt = 1;
                    }
                    break;
                }
            }
        }
    }
    asm volatile("" ::: "memory");           // the loads of what has arrived stay behind the check
    return ok;
}
