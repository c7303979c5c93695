// Device-to-device transfer of ONE factor block between a caller's 2-D view and a context buffer
// (pmx_factor_from_device / pmx_factor_to_device, include/pmx.h).
//
// The context's side is what pmx_upload / pmx_download move: dense rows x K (rows = M for block 0, N for block 1: S lives
// as S^T), K <= 128.  The caller's side is the block in the reference's orientation (A: M x K, S: K x N) given as a pointer
// and two element strides of which one is 1.  Seen from the context's (row r, component k) the caller's element sits at
// r * sr + k * sk, and there are two kernels:
//   sk == 1  k_xfer_copy       both sides run along k: a pitched copy (row-major A; column-major S such as St.T)
//   sr == 1  k_xfer_transpose  the caller's side runs along r: a transpose through LDS (row-major S; column-major A)
// Both are written as  src (P x Q, pitch ps, unit stride along Q)  ->  dst, so the two DIRECTIONS (in: caller -> context,
// out: context -> caller) are the same code with the operands exchanged.  Elements move as 32- / 64-bit integers: no
// arithmetic touches them, so NaN payloads, -0.0 and denormals keep their bits.  Only the P x Q logical elements of dst are
// written: pitch padding, whatever lies before or behind a caller's view, and the zero rows behind a frame's real ones stay.
#include "pmx_common.h"

template <typename T> struct xfer_bits;
template <> struct xfer_bits<float> { typedef uint32_t type; };
template <> struct xfer_bits<double> { typedef uint64_t type; };

constexpr int XFER_THREADS = 256;
constexpr int XFER_TILE = 32;
// LDS pitch of the transpose tile, in elements.  A tile row is written along the lanes (32 consecutive elements per
// 32-lane half) and read back down a column (lane l at l * pitch + c).  ds_write_* and ds_read_b32 bank on 32 dwords,
// ds_read_b64 on 64, and only the lanes of one group (32 lanes; 16 for ds_write_b64) can conflict:
//   4-byte elements  pitch 33 dwords: the column read hits banks (33 l + c) mod 32 = (l + c) mod 32, all 32 distinct;
//                    the row write hits 32 consecutive dwords: conflict degree 1 (none) both ways
//   8-byte elements  pitch 66 dwords: the column read (ds_read_b64) starts at banks (66 l + 2 c) mod 64 = (2 l + 2 c) mod 64,
//                    32 distinct even banks, two banks each: all 64 once; the row write (ds_write_b64, groups of 16
//                    contiguous lanes) covers 32 consecutive dwords per group: conflict degree 1 (none) both ways
constexpr int XFER_PITCH = XFER_TILE + 1;

// dst[q * pd + p] = src[p * ps + q] for p < P, q < Q.  One 32 x 32 tile per workgroup, 256 threads as 32 x 8: global reads run
// along q (src's unit stride), global writes along p (dst's), ragged edges by predication.
template <typename T>
__global__ __launch_bounds__(XFER_THREADS) void k_xfer_transpose(const T* __restrict__ src_, int64_t ps, T* __restrict__ dst_, int64_t pd,
                                                                  int64_t P, int64_t Q, int64_t tilesQ) {
    typedef typename xfer_bits<T>::type U;
    const U* src = reinterpret_cast<const U*>(src_);
    U* dst = reinterpret_cast<U*>(dst_);
    __shared__ U tile[XFER_TILE][XFER_PITCH];
    const int tx = threadIdx.x & (XFER_TILE - 1), ty = threadIdx.x >> 5;
    const int64_t p0 = ((int64_t)blockIdx.x / tilesQ) * XFER_TILE, q0 = ((int64_t)blockIdx.x % tilesQ) * XFER_TILE;
#pragma unroll
    for (int i = 0; i < XFER_TILE; i += XFER_THREADS / XFER_TILE) {
        const int64_t p = p0 + ty + i, q = q0 + tx;
        if (p < P && q < Q) tile[ty + i][tx] = src[p * ps + q];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < XFER_TILE; i += XFER_THREADS / XFER_TILE) {
        const int64_t q = q0 + ty + i, p = p0 + tx;
        if (p < P && q < Q) dst[q * pd + p] = tile[tx][ty + i];
    }
}

// dst[p * pd + q] = src[p * ps + q] for p < P, q < Q, V elements per thread.  V > 1 (16-byte accesses) only where the host
// has checked that both bases and both pitches are multiples of 16 bytes and Q of V; V == 1 takes any view.
template <typename T, int V>
__global__ __launch_bounds__(XFER_THREADS) void k_xfer_copy(const T* __restrict__ src_, int64_t ps, T* __restrict__ dst_, int64_t pd,
                                                             int64_t P, int64_t Q) {
    typedef typename xfer_bits<T>::type U;
    typedef U UV __attribute__((ext_vector_type(V)));
    const int64_t QV = Q / V;
    const int64_t e = (int64_t)blockIdx.x * XFER_THREADS + threadIdx.x;
    if (e >= P * QV) return;
    const int64_t p = e / QV, q = (e % QV) * V;
    if constexpr (V == 1) {
        reinterpret_cast<U*>(dst_)[p * pd + q] = reinterpret_cast<const U*>(src_)[p * ps + q];
    } else {
        *reinterpret_cast<UV*>(reinterpret_cast<U*>(dst_) + p * pd + q) = *reinterpret_cast<const UV*>(reinterpret_cast<const U*>(src_) + p * ps + q);
    }
}

// One block between the context's dense rows x K array `ctx` and the caller's view `usr` (strides sr along the context's
// rows, sk along its components; exactly the checked cases of pmx_factor_*_device).  out: context -> caller.
template <typename T>
static void launch_xfer(T* ctx, T* usr, int64_t rows, int64_t K, int64_t sr, int64_t sk, bool out, hipStream_t stream) {
    if (rows <= 0 || K <= 0) return;
    if (sk == 1 && (sr >= K || rows == 1)) {
        const T* src = out ? ctx : usr;
        T* dst = out ? usr : ctx;
        const int64_t ps = out ? K : sr, pd = out ? sr : K;
        constexpr int V = 16 / (int)sizeof(T);
        const bool vec = K % V == 0 && sr % V == 0 && (reinterpret_cast<uintptr_t>(ctx) & 15) == 0 && (reinterpret_cast<uintptr_t>(usr) & 15) == 0;
        const int64_t n = vec ? rows * (K / V) : rows * K;
        const dim3 grid((unsigned)((n + XFER_THREADS - 1) / XFER_THREADS));
        if (vec) hipLaunchKernelGGL((k_xfer_copy<T, V>), grid, dim3(XFER_THREADS), 0, stream, src, ps, dst, pd, rows, K);
        else hipLaunchKernelGGL((k_xfer_copy<T, 1>), grid, dim3(XFER_THREADS), 0, stream, src, ps, dst, pd, rows, K);
        return;
    }
    // sr == 1: the caller's array is K x rows with pitch sk
    const int64_t tr = (rows + XFER_TILE - 1) / XFER_TILE, tk = (K + XFER_TILE - 1) / XFER_TILE;
    const dim3 grid((unsigned)(tr * tk));
    if (out) hipLaunchKernelGGL((k_xfer_transpose<T>), grid, dim3(XFER_THREADS), 0, stream, (const T*)ctx, K, usr, sk, rows, K, tk);
    else hipLaunchKernelGGL((k_xfer_transpose<T>), grid, dim3(XFER_THREADS), 0, stream, (const T*)usr, sk, ctx, K, K, rows, tr);
}
