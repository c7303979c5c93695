// [r5] The correction that lets K1 form its residual from ONE fp16 product (k_grad_f16_v8<.., HH>, k_grad_f16_k128<.., HH>).
//
// Reference: nmf.grad_likelihood (proxmin/nmf.py:28-41)  D = A S - Y,  gA = D S^T,  gS = A^T D  in the caller's fp32.
// K1 <HH> computes P0 = a0 s0 with a0 = fp16(A 2^eA) 2^-eA, s0 = fp16(S 2^eS) 2^-eS (11 significant bits each, products exact,
// fp32 accumulation) and contracts R0 = P0 - Y.  What the high terms leave out is known exactly,
//     A S - a0 s0  =  A s_r + a_r s0  =  a0 s_r + a_r S          (x_r = X - x0: an exact fp32 subtraction),
// and its contribution to both gradients goes through K x K matrices instead of M x N x K products:
//     gA  += A  (s_r S^T) + a_r (s0 S^T)             gSt += St (a_r^T A) + st_r (a0^T A)
// i.e. for either block X with the OTHER factor Z (both tall, rows x K):   C_X = X Qr(Z) + x_r Q0(Z),
//     Qr(Z) = z_r^T Z,   Q0(Z) = z0^T Z              (K x K, Q[k'][k] = sum over rows of U[row][k'] Z[row][k]).
// 4 (M + N) K^2 flops beside K1's 6 M N K: 0.1 % at 16384^2 x 64.  The correction is 2^-12 of the gradient's terms and needs 2^-12 of
// relative accuracy to leave exact fp32's error class untouched; it is computed to ~2^-22.  Three stages that depend on the factors only -- three launches
// behind K1 here, or carried by K1 itself on its idle waves (k_grad_f16_v8<.., GF>, K1's K = 64 with both gradients wanted: the same code, k_gfix_dev.h):
//   k_gfix_gram    per-workgroup partial Q0 / Qr of both factors (fp16 MFMA on the very terms K1 uses: z0 exact, Z = z0 + z1, z_r ~ z1)
//   k_gfix_reduce  fixed-order sum of the partials (deterministic: no float atomics)
//   k_gfix_apply   C_X for every row of both blocks (split-fp16 MFMA: the rows as three fp16 terms, the matrices as two, transposed in LDS) into the
//                  CORRECTION SLAB the update kernels fold behind K1's own slabs (SlabRef::extra)
// Unweighted likelihood only: with weights the missing term is W o (A s_r + a_r s0), which does not factor.
// Row-sharded runs: every term is a sum over the rank's own rows (A's) or over replicated data (S's) -- nothing to exchange.
#include "pmx_common.h"
#include "k_gfix_dev.h"                  // the stages as callable pieces: these kernels and the K1 that carries them (k_grad_f16_v8<.., GF>) run the same code

#define GFIX_STAMP(i) do { if (a.prof != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) a.prof[i] = wall_clock64(); } while (0)

// One share of the gram stage by wave W of the stand-alone kernel (k_gfix_dev.h: the pieces): the first batch of loads goes out before
// the scale's own round trip.
template <int KT, int W>
__device__ __forceinline__ void gfix_gram_wave(const GfixArgs& a, int f, float* red) {
    constexpr int K = GfixGram<KT>::K;
    const int lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
    int64_t r0, r1;
    gfix_gram_share(a.rows[f], blockIdx.x, r0, r1);
    const float* X = a.X[f];
    float v[GfixGram<KT>::NB][KT][8];
    f32x16 acc0[GfixGram<KT>::TPW], accr[GfixGram<KT>::TPW];
    GFIX_STAMP(0);
    if (r0 < r1) gfix_gram_request<KT, GfixGram<KT>::NB, false>(X, r0, r1, l31, hi, v);
    const float sc = gfix_scale(a.absmax, f, red), un = 1.f / (sc * sc);
    GFIX_STAMP(1);
    gfix_gram_compute<KT, W, GfixGram<KT>::NB, false>(X, r0, r1, l31, hi, sc, v, acc0, accr);
    GFIX_STAMP(2);
    gfix_gram_store<KT, W, false>(a.part + ((int64_t)f * GFIX_PARTS + blockIdx.x) * 2 * K * K, l31, hi, un, acc0, accr);
    GFIX_STAMP(3);
}
// K = 128 (KT = 4): wave w owns tile row ti = w (its four tiles of both matrices) and needs ALL four 32-column chunks of every row.  Each wave
// loads and splits ONE chunk (its own) and the four exchange the fp16 fragments through LDS: a quarter of the loads and conversions of the
// scheme above, where every wave fetched and split whole rows (18.6 us at cfg4's share, most of it that).
template <int W>
__device__ __forceinline__ void gfix_gram_wave_k128(const GfixArgs& a, int f, float* red, gf16x8* frag) {
    constexpr int K = 128, KT = 4, NB = 8;   // steps of sixteen rows per batch: frag[step][chunk][term][lane], 64 KB
    const int lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
    const int64_t rows = a.rows[f];
    const int64_t per = 16 * ((rows + 16 * GFIX_PARTS - 1) / (16 * GFIX_PARTS));
    const int64_t r0 = (int64_t)blockIdx.x * per, r1 = r0 + per < rows ? r0 + per : rows;
    const float* X = a.X[f] + 32 * W + l31;
    f32x16 acc0[KT], accr[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc0[t][i] = 0.f; accr[t][i] = 0.f; }
    float v[NB][8];
#define GFIX_REQUEST(rb_)                                                                          \
    _Pragma("unroll") for (int s = 0; s < NB; ++s)                                                 \
    _Pragma("unroll") for (int q = 0; q < 8; ++q) {                                                \
        const int64_t r = (rb_) + 16 * s + 8 * hi + q;                                             \
        v[s][q] = r < r1 ? X[r * K] : 0.f;                                                         \
    }
    if (r0 < r1) { GFIX_REQUEST(r0) }
    const float sc = gfix_scale(a.absmax, f, red), un = 1.f / (sc * sc);
    for (int64_t rb = r0; rb < r1; rb += 16 * NB) {
        gf16x8 h[NB], l[NB];
#pragma unroll
        for (int s = 0; s < NB; ++s) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float x = v[s][q] * sc;
                const _Float16 t = (_Float16)x;
                h[s][q] = t;
                l[s][q] = (_Float16)(x - (float)t);
            }
            frag[((s * KT + W) * 2 + 0) * 64 + lane] = h[s];
            frag[((s * KT + W) * 2 + 1) * 64 + lane] = l[s];
        }
        if (rb + 16 * NB < r1) { GFIX_REQUEST(rb + 16 * NB) }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < NB; ++s)
#pragma unroll
            for (int tj = 0; tj < KT; ++tj) {
                const gf16x8 hj = tj == W ? h[s] : frag[((s * KT + tj) * 2 + 0) * 64 + lane];
                const gf16x8 lj = tj == W ? l[s] : frag[((s * KT + tj) * 2 + 1) * 64 + lane];
                acc0[tj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(h[s], lj, acc0[tj], 0, 0, 0);
                accr[tj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(l[s], lj, accr[tj], 0, 0, 0);
                acc0[tj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(h[s], hj, acc0[tj], 0, 0, 0);
                accr[tj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(l[s], hj, accr[tj], 0, 0, 0);
            }
        __syncthreads();                     // (the fragments are rewritten by the next batch)
    }
#undef GFIX_REQUEST
    float* out = a.part + ((int64_t)f * GFIX_PARTS + blockIdx.x) * 2 * K * K;
#pragma unroll
    for (int tj = 0; tj < KT; ++tj)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int kp = 32 * W + (i & 3) + 8 * (i >> 2) + 4 * hi, k = 32 * tj + l31;
            out[kp * K + k] = acc0[tj][i] * un;
            out[K * K + kp * K + k] = accr[tj][i] * un;
        }
}
template <int KT>
__global__ __launch_bounds__(256) void k_gfix_gram(GfixArgs a) {
    __shared__ float red[4];
    if (chain_halted(a.status)) return;
    const int f = blockIdx.y;
    if (!a.want[1 - f]) return;              // factor f's matrices correct the OTHER block's gradient
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if constexpr (KT == 4) {
        extern __shared__ gf16x8 gfrag[];    // [8 steps][4 chunks][2 terms][64 lanes]: 64 KB
        if (w == 0) gfix_gram_wave_k128<0>(a, f, red, gfrag);
        else if (w == 1) gfix_gram_wave_k128<1>(a, f, red, gfrag);
        else if (w == 2) gfix_gram_wave_k128<2>(a, f, red, gfrag);
        else gfix_gram_wave_k128<3>(a, f, red, gfrag);
    } else {
        if (w == 0) gfix_gram_wave<KT, 0>(a, f, red);
        else if (w == 1) gfix_gram_wave<KT, 1>(a, f, red);
        else if (w == 2) gfix_gram_wave<KT, 2>(a, f, red);
        else gfix_gram_wave<KT, 3>(a, f, red);
    }
}

// k_gfix_dev.h: gfix_reduce_share
__global__ __launch_bounds__(256) void k_gfix_reduce(GfixArgs a) {
    if (chain_halted(a.status)) return;
    const int f = blockIdx.y;
    if (!a.want[1 - f]) return;
    GFIX_STAMP(4);
    gfix_reduce_share<false>(a.part, a.Q, a.K, f, blockIdx.x, threadIdx.x);
    GFIX_STAMP(5);
}

// k_gfix_dev.h: the apply stage's pieces
template <int KT>
__global__ __launch_bounds__(KT == 4 ? 512 : 256) void k_gfix_apply(GfixArgs a) {
    constexpr int K = 32 * KT;
    constexpr int NT = KT == 4 ? 512 : 256, NW = NT / 64;      // K = 128: eight waves share one staging of the (4 x larger) matrices
    extern __shared__ _Float16 qpl[];        // [matrix: Qr, Q0][term][column k][k']
    __shared__ float red[8];
    if (chain_halted(a.status)) return;
    const int f = blockIdx.y;                // the block whose gradient is corrected
    if (!a.want[f]) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int64_t rows = a.rows[f];
    const float* X = a.X[f];
    const int64_t ntask = (rows + 31) / 32 * KT, stride = (int64_t)gridDim.x * NW;     // a wave per task and round (launch_gfix: <= 256 workgroups, the matrices staged once each)
    if ((int64_t)blockIdx.x * NW >= ntask) return;
    GFIX_STAMP(6);
    f32x4 x[K / 16][2];
    const int64_t task0 = (int64_t)blockIdx.x * NW + w;
    if (task0 < ntask) gfix_apply_load_x<KT>(X, rows, task0, l31, hi, x);
    float tq[2][GfixApply<KT, NT>::NBLK][8];
    __shared__ float redq[2 * NW];
    gfix_apply_fetch<KT, NT, false>(a.Q + (int64_t)(1 - f) * 2 * K * K, tid, tq, redq);
    const float sc = gfix_scale(a.absmax, f, red);        // (its barrier publishes redq as well)
    GFIX_STAMP(7);
    float sq[2];
    gfix_apply_planes<KT, NT>(qpl, tid, tq, redq, sq);
    __syncthreads();
    GFIX_STAMP(8);
    for (int64_t task = (int64_t)blockIdx.x * NW + w; task < ntask; task += stride) {
        if (task != task0) gfix_apply_load_x<KT>(X, rows, task, l31, hi, x);   // (the first task's rows were requested before the matrices: one round trip less)
        gfix_apply_task<KT>(rows, a.out[f], a.ld, qpl, task, l31, hi, sc, sq, x);
        GFIX_STAMP(9);
    }
    GFIX_STAMP(10);
}

static hipError_t launch_gfix(const GfixArgs& a, hipStream_t s) {
    const int n = 2 * a.K * a.K;
    const size_t lds = (size_t)4 * a.K * (a.K + 8) * sizeof(_Float16);      // k_gfix_apply: two matrices x two fp16 terms, transposed
    const int64_t rmax = a.rows[0] > a.rows[1] ? a.rows[0] : a.rows[1];
    const int nw = a.K == 128 ? 8 : 4;                                               // waves per workgroup of k_gfix_apply
    unsigned nb = (unsigned)(((rmax + 31) / 32 * (a.K / 32) + nw - 1) / nw);         // k_gfix_apply: a wave per (32 rows, 32 columns) and round
    // one staging of the matrices per workgroup: at most as many workgroups as can be resident (K = 128: 139 KB of LDS = one per CU, two blocks: 128 each)
    if (nb > (a.K == 128 ? 128u : 256u)) nb = a.K == 128 ? 128 : 256;
    if (a.K == 64) {
        hipError_t e = hipFuncSetAttribute((const void*)k_gfix_apply<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_gfix_gram<2>, dim3(GFIX_PARTS, 2), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_gfix_reduce, dim3((n * 4 + 255) / 256, 2), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_gfix_apply<2>, dim3(nb, 2), dim3(256), lds, s, a);
    } else if (a.K == 128) {
        hipError_t e = hipFuncSetAttribute((const void*)k_gfix_apply<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        e = hipFuncSetAttribute((const void*)k_gfix_gram<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_gfix_gram<4>, dim3(GFIX_PARTS, 2), dim3(256), 64 * 1024, s, a);
        hipLaunchKernelGGL(k_gfix_reduce, dim3((n * 4 + 255) / 256, 2), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_gfix_apply<4>, dim3(nb, 2), dim3(512), lds, s, a);
    } else return hipErrorInvalidValue;
    return hipGetLastError();
}
