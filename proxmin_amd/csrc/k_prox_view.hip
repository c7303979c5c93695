// Stand-alone proximal operators on the CALLER'S OWN MEMORY, in the array's element type: what `prox(X, step)` called on a float32 or
// float64 array maps to (pmx_prox_view / pmx_prox_flat, include/pmx.h; proxmin/operators.py:20-184 mutate at the array's dtype), and
// what pmx_prox_apply / pmx_prox_array / pmx_prox_array_tables run on a context's buffer / a float32 host array.
//
//   k_prox_view<T, NC, ME, CM, CS> a rows x K VIEW, element (r, k) at X + r * s0 + k * s1 with one stride equal to 1 (the rule of
//                                pmx_factor_from_device).  The operators are prox_row<T, NC, 32, ME> of k_update.hip -- the one
//                                implementation the fp32 and fp64 solver kernels run -- so the float instance computes what
//                                the fp32 update kernels compute, bit for bit, and the double one what k_big_f64.hip's updates do.
//                                Row r belongs to half-wave r mod 8192 of the grid (ROW_LOOP_BEGIN's mapping), NC values per lane.
//       CM = false  s1 == 1 (row-major, any pitch): read and written in place along the components.
//       CM = true   s0 == 1 (column-major: a K x N `S` seen as N rows of K components, or St.T): global accesses run along
//                   the rows.  A workgroup's 32 rows of one sweep are 32 consecutive rows (its 32 half-waves), so they pass
//                   through one LDS tile of K x 32 elements: half-wave h loads / stores components h, h + 32, ... of the 32 rows
//                   (32 consecutive elements), and reads / writes ITS row down the tile's columns (pitch 33 elements: k_xfer.hip's
//                   bank argument for 4- and 8-byte elements).  Same rows per thread as CM = false: the column sums below agree.
//       div / sum   prox_unity* ALONG THE ROWS (pmx_prox::unit = 1) as two launches, k_pgm_unity's scheme: `sum` leaves the
//                   workgroup's column sums of the result in colpart (per-thread sums in row order in T, the 32 half-waves added
//                   in double: colsum_store, k_colsum's), `div` opens with colsum_totals -- colsum_fold's fixed-order fold, the
//                   totals rounded to T -- and divides every row by them.  For float this is k_pgm_unity's arithmetic, bit for bit.
//   k_prox_flat<T, ME>           an element-wise operator with ONE step on n contiguous elements, the tail guarded: prox_row with one
//                                value per lane (no component structure, so no per-component tables and no prox_unity*).
//
// Only the view's logical elements are written: pitch padding and whatever lies before or behind the view keep their bits, and no
// alignment beyond the element's own is assumed (every access is one element wide).
#include "pmx_common.h"

constexpr int PV_TILE_PITCH = 33;
static_assert(EW_THREADS / 32 == 32, "k_prox_view<.., CM>: a workgroup's rows of one sweep are the 32 rows of one LDS tile");

template <class T>
struct ProxViewArgs {
    T* X;
    int64_t rows;
    int K;
    int64_t s0, s1;          // element strides along the rows / the components
    ProxSeq prox;
    T stepk[MAXK];
    double* colpart;         // [EW_BLOCKS][MAXK]: read by `div`, written by `sum`
    int div;                 // open with the division by the column sums folded from colpart
    int sum;                 // leave the column sums of the result in colpart
};

// CS: the instance holds `div` / `sum` (the two launches of prox_unity* along the rows).  The plain instances -- every other call --
// carry neither colsum_fold's 32 doubles in flight nor the fold's and the column sums' LDS.
template <class T, int NC, bool ME, bool CM, bool CS>
__global__ __launch_bounds__(EW_THREADS) void k_prox_view(ProxViewArgs<T> a) {
    __shared__ double asum[CS ? ALPHA_NG : 1][CS ? MAXK : 1];
    __shared__ T tot[CS ? MAXK : 1];
    __shared__ T sm[CS ? (EW_THREADS / 32) * MAXK : 1];
    __shared__ T tile[CM ? 32 * NC : 1][CM ? PV_TILE_PITCH : 1];
    const int K = a.K;
    const int l32 = threadIdx.x & 31, hwi = threadIdx.x >> 5;
    const bool div = CS && a.div, sum = CS && a.sum;
    if constexpr (CS) {
        if (div) colsum_totals(a.colpart, K, asum, tot);
    }
    T cs[NC];
    bool ok[NC];
    T sk[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int kk = l32 + 32 * c;
        cs[c] = (T)0;
        ok[c] = kk < K;
        sk[c] = ok[c] ? a.stepk[kk] : (T)0;
    }
    const int64_t nhw = ((int64_t)EW_BLOCKS * EW_THREADS) >> 5;
    // (the bound is the workgroup's, not the half-wave's: with CM every half-wave of the workgroup meets the barriers)
    for (int64_t r0 = (int64_t)blockIdx.x * (EW_THREADS / 32); r0 < a.rows; r0 += nhw) {
        const int64_t r = r0 + hwi;
        const bool live = r < a.rows;
        T v[NC];
        if constexpr (CM) {
            const bool in = r0 + l32 < a.rows;
            for (int k = hwi; k < K; k += EW_THREADS / 32)
                if (in) tile[k][l32] = a.X[r0 + l32 + (int64_t)k * a.s1];
            __syncthreads();
#pragma unroll
            for (int c = 0; c < NC; ++c) v[c] = (live && ok[c]) ? tile[l32 + 32 * c][hwi] : (T)0;
        } else {
#pragma unroll
            for (int c = 0; c < NC; ++c) v[c] = (live && ok[c]) ? a.X[r * a.s0 + l32 + 32 * c] : (T)0;
        }
        if (live) {
            if constexpr (CS) {
                if (div)
#pragma unroll
                    for (int c = 0; c < NC; ++c)
                        if (ok[c]) v[c] = v[c] / tot[l32 + 32 * c];
            }
            prox_row<T, NC, 32, ME>(v, ok, a.prox, sk);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                if (!ok[c]) continue;
                if (sum) cs[c] += v[c];
                if constexpr (CM) tile[l32 + 32 * c][hwi] = v[c];
                else a.X[r * a.s0 + l32 + 32 * c] = v[c];
            }
        }
        if constexpr (CM) {
            __syncthreads();
            const bool in = r0 + l32 < a.rows;
            for (int k = hwi; k < K; k += EW_THREADS / 32)
                if (in) a.X[r0 + l32 + (int64_t)k * a.s1] = tile[k][l32];
            __syncthreads();                 // (the next sweep's loads overwrite the tile)
        }
    }
    if constexpr (CS) {
        if (sum) colsum_store<NC>(cs, a.colpart, 0, sm);     // (block 0: the 32 half-waves of the workgroup, added in order in double)
    }
}

template <class T>
struct ProxFlatArgs {
    T* X;
    int64_t n;
    ProxSeq prox;
    T step;
};
template <class T, bool ME>
__global__ __launch_bounds__(EW_THREADS) void k_prox_flat(ProxFlatArgs<T> a) {
    const bool ok[1] = {true};
    const T sk[1] = {a.step};
    for (int64_t e = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; e < a.n; e += (int64_t)EW_BLOCKS * EW_THREADS) {
        T v[1] = {a.X[e]};
        prox_row<T, 1, 32, ME>(v, ok, a.prox, sk);
        a.X[e] = v[0];
    }
}

template <class T, bool ME, bool CM, bool CS>
static void launch_prox_view_nc(const ProxViewArgs<T>& a, hipStream_t s) {
    if (a.K <= 32) hipLaunchKernelGGL((k_prox_view<T, 1, ME, CM, CS>), dim3(EW_BLOCKS), dim3(EW_THREADS), 0, s, a);
    else if (a.K <= 64) hipLaunchKernelGGL((k_prox_view<T, 2, ME, CM, CS>), dim3(EW_BLOCKS), dim3(EW_THREADS), 0, s, a);
    else hipLaunchKernelGGL((k_prox_view<T, 4, ME, CM, CS>), dim3(EW_BLOCKS), dim3(EW_THREADS), 0, s, a);
}
// CM is decided here: s1 == 1 is the row-major view (a single column with s0 == 1 as well is both: the in-place kernel)
template <class T>
void launch_prox_view(const ProxViewArgs<T>& a, hipStream_t s) {
    const bool me = seq_has_me(a.prox), cm = a.s1 != 1;
    if (a.div || a.sum) {                    // (their sequences are empty or a lone prox_plus: apply_prox_view; never ME)
        if (cm) launch_prox_view_nc<T, false, true, true>(a, s); else launch_prox_view_nc<T, false, false, true>(a, s);
    } else if (me) { if (cm) launch_prox_view_nc<T, true, true, false>(a, s); else launch_prox_view_nc<T, true, false, false>(a, s); }
    else { if (cm) launch_prox_view_nc<T, false, true, false>(a, s); else launch_prox_view_nc<T, false, false, false>(a, s); }
}
template <class T>
void launch_prox_flat(const ProxFlatArgs<T>& a, hipStream_t s) {
    if (seq_has_me(a.prox)) hipLaunchKernelGGL((k_prox_flat<T, true>), dim3(EW_BLOCKS), dim3(EW_THREADS), 0, s, a);
    else hipLaunchKernelGGL((k_prox_flat<T, false>), dim3(EW_BLOCKS), dim3(EW_THREADS), 0, s, a);
}
