// ------------------------------------------------------------------------------------------------
// k_batch_pgm<KM>: MANY small factorisations in one launch (pmx_nmf_batch_pgm; proxmin_amd.nmf.nmf_batch).
//
// A small problem (K <= 16, M N <= 2^20) run through a context is three launches per iteration -- k_small_front, k_pgm_update<1>,
// and a read of the status every 32 iterations -- that occupy a few dozen workgroups of a 256-CU part: launch latency and an idle
// device.  Here ONE workgroup of 256 threads runs the WHOLE solve of a problem, every iteration up to its own stop, and then draws the
// next problem: one relaxed agent-scope atomicAdd on a counter per problem, the host has ordered the list by M N K descending.
// Workgroups never wait for each other (no grid barrier, no spin, no ticket), so a launch ends whatever a single problem does.
//
// An iteration of a problem is the single call's, piece by piece, with the SAME device bodies (the results are the single call's bit
// for bit):
//   1  grad_small_tile<KM> over the problem's tiles, in the order of k_grad_small's grid, into the workgroup slot's slabs;
//   2  eig_small_body<KM> for factor 0, then factor 1 (DevStatus::step; the eigenvector warm start lives in the problem's DevStatus);
//   3  k_pgm_update<1>'s row: load_grad (slabs in the fixed order), X = prox_row<float, 1, 32>(Xe - s G, s), the FISTA extrapolation
//      with the omega the host uploaded (utils.NesterovAccelerator's sequence);
//   4  the two sums of the stopping test per block: each entry's square in fp32 as k_pgm_update forms it, the sums in fp64;
//      publish_outer_test decides (algorithms.py:130-135).
// Between phases one __syncthreads(): its workgroup-scope release waits for the phase's stores (vmcnt) and the readers sit on the
// same CU, behind the same vector cache -- no agent-scope release (k_pgm_update records what that costs), and lds_barrier() would
// not do: it waits for lgkmcnt only.
//
// Memory per workgroup slot: slabs for the largest problem of the launch, the step rule's Gram copy and Lanczos basis, loss partials.
// Per problem: its DevStatus (reset here as reset_status does on the host), and an Xe pair when accelerated.
// ------------------------------------------------------------------------------------------------
#pragma once

struct BatchArgs {
    const pmx_batch_item* items;   // [B], offsets in floats; S is held transposed (N x K) at offS
    const int* order;              // [n]: the problems of this launch, largest first
    int n;
    unsigned* counter;             // the next position of `order` to hand out
    const float* Y;
    float* X[2];                   // A, St
    float* Xe[2];                  // extrapolated points (accelerated), else nullptr
    DevStatus* status;             // [B]
    pmx_batch_result* out;         // [B]
    float* slabs;                  // [slots][slabFloats]
    int64_t slabFloats;
    double* eigG;                  // [slots][2][32*32]
    double* eigQ;                  // [slots][2][32*32]
    double* lossPart;              // [slots][lossSlots]
    int lossSlots;
    const float* omega;            // [max_iter]: omega_next of iteration it (accelerated)
    ProxSeq prox[2];
    double e_rel[2];
    double scale;
    double fixed[2];
    int use_fixed, accelerated, max_iter;
};

// workgroups per CU the K <= 8 instance is compiled for.  2 holds it to 256 registers (40 bytes of scratch per lane) and is 1.6 x the rate of 1
// (256 + 15 registers, no scratch) from 1024 problems on, the same below (profiles/nmf_batch_rate.txt); -DBATCH_WG8=1 builds the other for an A/B.
// The K <= 16 instance runs one per CU: grad_small_tile<16> alone takes 256 + 78 registers.
#ifndef BATCH_WG8
#define BATCH_WG8 2
#endif
constexpr int BATCH_KP = 32;       // the step rule's frame of a small context (grad_plan_small)

// What the phases of one problem are called with.  It lives in LDS, written once per problem: held in scalar registers across the
// iteration loop the descriptors (and what the compiler hoists out of them) do not fit beside grad_small_tile's and eig_small_body's
// own registers and spill; read where they are used, their live ranges end with the phase.
struct BatchProblem {
    GradArgs ga;
    EigArgs ea;
    SlabRef sr[2];
    float* X[2];
    float* Xe[2];
    int64_t rows[2];
    int tilesX, ntiles, K;
    DevStatus* st;
};

template <int KM>
__device__ __forceinline__ void batch_solve_one(const BatchArgs& a, const int b, float* g, SmallTileSmem<KM>& tile, EigSmallSmem& eig,
                                                double (&red)[4][4], int& s_stop, BatchProblem& pb) {
    const int t = threadIdx.x;
    DevStatus* st = a.status + b;
    // reset_status: zeros, the eigenvector warm start all ones
    {
        int* w = reinterpret_cast<int*>(st);
        for (int e = t; e < (int)(sizeof(DevStatus) / sizeof(int)); e += 256) w[e] = 0;
        __syncthreads();
        for (int e = t; e < 2 * MAXK; e += 256) st->eigvec[e / MAXK][e % MAXK] = 1.0;
        if (t < 2 && a.use_fixed) st->step[t] = a.fixed[t];
    }
    if (t == 0) {
        const pmx_batch_item it = a.items[b];
        const int M = (int)it.M, N = (int)it.N, K = it.K;
        const int tilesX = (N + SG_COLS - 1) / SG_COLS, tilesY = (M + SG_ROWS - 1) / SG_ROWS;
        float* slab = a.slabs + (int64_t)blockIdx.x * a.slabFloats;
        pb.X[0] = a.X[0] + it.offA; pb.X[1] = a.X[1] + it.offS;
        pb.Xe[0] = a.accelerated ? a.Xe[0] + it.offA : pb.X[0];
        pb.Xe[1] = a.accelerated ? a.Xe[1] + it.offS : pb.X[1];
        pb.rows[0] = M; pb.rows[1] = N;
        pb.tilesX = tilesX; pb.ntiles = tilesX * tilesY; pb.K = K;
        pb.st = st;
        GradArgs ga{};
        ga.Y = a.Y + it.offY; ga.ldY = it.ldY;
        ga.A = pb.Xe[0]; ga.St = pb.Xe[1];
        ga.slabA = slab; ga.slabS = slab + (int64_t)tilesX * M * K;
        ga.lossPart = a.lossPart + (int64_t)blockIdx.x * a.lossSlots;
        ga.status = st;
        ga.M = M; ga.N = N; ga.K = K;
        ga.RP = 1; ga.doA = 1; ga.doS = 1;
        pb.ga = ga;
        EigArgs ea{};
        ea.G = ea.Gw = a.eigG + (int64_t)blockIdx.x * 2 * BATCH_KP * BATCH_KP;
        ea.Q = a.eigQ + (int64_t)blockIdx.x * 2 * BATCH_KP * BATCH_KP;
        ea.KP = BATCH_KP; ea.K = K;
        ea.status = st;
        ea.want[0] = ea.want[1] = 1;
        ea.scale = a.scale;
        ea.max_iter = 200;
        ea.X[0] = pb.Xe[0]; ea.X[1] = pb.Xe[1];
        ea.rows[0] = M; ea.rows[1] = N;
        pb.ea = ea;
        SlabRef sr;
        sr.base = ga.slabA; sr.n = tilesX; sr.stride = (int64_t)M * K; sr.ld = K;
        pb.sr[0] = sr;
        sr.base = ga.slabS; sr.n = tilesY; sr.stride = (int64_t)N * K;
        pb.sr[1] = sr;
    }
    __syncthreads();

    const int l32 = t & 31, hw = t >> 5;
    for (int iter = 0; iter < a.max_iter; ++iter) {
        // 1  the gradient at the evaluation point (algorithms.py:105)
        {
            const int tilesX = pb.tilesX, ntiles = pb.ntiles;
            for (int q = 0; q < ntiles; ++q) grad_small_tile<KM>(pb.ga, tile, q % tilesX, q / tilesX, tilesX);
        }
        // 2  the Lipschitz steps at the same point (algorithms.py:106); the pool changes hands
        if (!a.use_fixed) {
#pragma unroll 1
            for (int f = 0; f < 2; ++f) {
                __syncthreads();
                eig_small_body<KM>(pb.ea, f, g, eig);
            }
        }
        __syncthreads();
        // 3  the update (algorithms.py:107-108, :93-99), k_pgm_update<1>'s expressions
        const float om = a.accelerated ? a.omega[iter] : 0.f;
        const int K = pb.K;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float s = (float)st->step[j];
            float* Xj = pb.X[j];
            float* Xej = pb.Xe[j];
            const int64_t rows = pb.rows[j];
            const SlabRef sr = pb.sr[j];
            for (int64_t r = hw; r < rows; r += 256 / 32) {
                bool ok[1];
                float gr[1], v[1], sk[1];
                ok[0] = l32 < K;
                load_grad<1>(gr, ok, sr, rows, K, r, l32);
                const int64_t e = r * K + l32;
                const float xo = ok[0] ? Xj[e] : 0.f;
                const float xe = a.accelerated ? (ok[0] ? Xej[e] : 0.f) : xo;
                const float se = s;
                v[0] = xe - se * gr[0];
                sk[0] = se;
                prox_row<float, 1, 32, false>(v, ok, a.prox[j], sk);
                if (ok[0]) {
                    Xj[e] = v[0];
                    if (a.accelerated) { const float xnext = v[0] + om * (v[0] - xo); Xej[e] = xnext; }
                    const float d = v[0] - xo;
                    acc[2 * j] += (double)(d * d);               // (k_pgm_update: one entry per thread, squared in fp32, summed in fp64)
                    acc[2 * j + 1] += (double)(v[0] * v[0]);
                }
            }
        }
        // 4  the stopping test (algorithms.py:130-135)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = wave_sum(acc[i]);
        if ((t & 63) == 0)
#pragma unroll
            for (int i = 0; i < 4; ++i) red[i][t >> 6] = acc[i];
        __syncthreads();
        if (t == 0) {
            double r4[4];
            for (int i = 0; i < 4; ++i) r4[i] = (red[i][0] + red[i][1]) + (red[i][2] + red[i][3]);
            const double d[2] = {r4[0], r4[2]}, n[2] = {r4[1], r4[3]};
            publish_outer_test(st, d, n, a.e_rel, 1, 1, 1);
            s_stop = st->stopped;
        }
        __syncthreads();
        if (s_stop) break;
    }
    if (t == 0) {
        pmx_batch_result r;
        r.it_done = st->it_done; r.stopped = st->stopped;
        r.conv[0] = st->conv[0]; r.conv[1] = st->conv[1];
        r.step[0] = st->step[0]; r.step[1] = st->step[1];
        for (int j = 0; j < 2; ++j) { r.norms[j][0] = st->norms[j][0]; r.norms[j][1] = st->norms[j][1]; }
        a.out[b] = r;
    }
}

template <int KM>
__global__ __launch_bounds__(256, KM == 8 ? BATCH_WG8 : 1) void k_batch_pgm(BatchArgs a) {
    __shared__ __attribute__((aligned(16))) float g[BATCH_KP * (BATCH_KP + 1)];
    __shared__ union Pool {
        SmallTileSmem<KM> tile;
        EigSmallSmem eig;
        __device__ Pool() {}
    } sm;
    __shared__ double red[4][4];
    __shared__ int s_next, s_stop;
    __shared__ union Problem {
        BatchProblem v;
        __device__ Problem() {}
    } pb;
    for (;;) {
        if (threadIdx.x == 0) {
            s_next = (int)__hip_atomic_fetch_add(a.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_stop = 0;
        }
        __syncthreads();
        const int q = s_next;
        __syncthreads();
        if (q < 0 || q >= a.n) return;          // (uniform: one LDS word)
        batch_solve_one<KM>(a, a.order[q], g, sm.tile, sm.eig, red, s_stop, pb.v);
        __syncthreads();
    }
}
