// k1_instance.h -- which template instance a K1 launch runs: ONE decision per tuned family, used by the launch (enqueue_grad_once arms what the
// decided instance needs, the family's launcher looks the decided flags up in its table) and pinned by tests/test_k1_instances.py against
// tests/golden/k1_instances.json.  Plain C++17, no HIP: a host compiler builds it alone.
#pragma once
#include <stddef.h>
#include <stdlib.h>

// ------------------------------------------------------------------------------------------
// K1's families: pmx_api.hip's select_k1 picks one per context (pmx_k1_info reports it, include/pmx.h)
// ------------------------------------------------------------------------------------------
enum K1Kind {
    K1_SMALL,        // k_grad_small (K <= 16, few million entries), any mode
    K1_F32,          // k_grad_f32: exact fp32, any shape
    K1_F32PC,        // k_grad_f32_pc: exact fp32, producer / consumer (K = 32 / 64, M % 128 = 0, N % 256 = 0)
    K1_BF16,         // k_grad_bf16 / k_grad_bf16_pipe on presplit terms (modes bf16x3 / f16x2, K <= 64)
    K1_BF16_V7,      // k_grad_bf16_v7: split-bf16 on fp32 operands (K = 64, M % 128 = 0, N % 256 = 0)
    K1_F16_V8,       // k_grad_f16_v8: two-term fp16 (mode f16x2 at the shapes of K1_BF16_V7)
    K1_F16_K128,     // k_grad_f16_k128: two-term fp16 at K = 128
    K1_F16_K32,      // k_grad_f16_k32: two-term fp16 at K = 32 (no weights)
    K1_F64_SMALL,    // fp64 contexts (k_small_f64.hip, k_big_f64.hip)
    K1_F64_BIG,
};
// the instance a launch of a family runs: PLAIN; R3 (three terms per operand in the residual); HH (the high x high residual, the rest as a
// correction slab, k_gfix.hip); V7 (k_grad_bf16_v7 in place of k_grad_f16_v8: Y or W cannot be fetched in 8-byte pairs)
enum K1Inst { K1_PLAIN, K1_R3, K1_HH, K1_V7 };
// r3: pmx_ctx::f16_r3; grad: a gradient is wanted (the loss-only pass has nowhere to put a correction); pairs: Y and W fetchable in 8-byte pairs
static inline K1Inst k1_instance(K1Kind k, int r3, bool hasW, bool grad, bool pairs) {
    switch (k) {
    case K1_F16_V8:
        if (!pairs) return K1_V7;
        if (!r3 || hasW) return K1_PLAIN;                  // (a weighted context keeps two terms)
        return r3 == 2 && grad ? K1_HH : K1_R3;
    case K1_F16_K128: return r3 == 2 && !hasW && grad ? K1_HH : K1_PLAIN;
    case K1_F16_K32: return r3 ? K1_R3 : K1_PLAIN;        // (no weights)
    default: return K1_PLAIN;
    }
}
// DevStatus::k1_fault: a K1 launch stopped the chain of kernels before anything was updated; the host repairs and repeats (chain_fault_fallback)
enum K1Fault {
    K1_FAULT_LATE = 1,       // <CHAIN>: a chain predecessor never arrived (workgroups not co-resident)   } the host falls back to
    K1_FAULT_XCD = 2,        // <CHAIN>: the predecessor runs on another XCD                              } one slab per column region
    K1_FAULT_INJECTED = 3,   // <CHAIN>: asked for by the tests (chainInject)                             }
    K1_FAULT_RANGE = 4,      // a two-term fp16 K1 found the residual's bound too far above max|Y| for ONE fp16 scale (f16_range_fault): exact fp32 from here on
    K1_FAULT_GFIX = 5,       // <GF>: a stage of the ride did not arrive in time (the host falls back to the stand-alone correction launches)
};

// The launch-time switches (A/B runs and the tests; "0" turns one off).  Read at every K1 launch that has a use for them, once, here and nowhere else:
// the tests flip them inside a live context.
struct K1Switches {
    bool role_split;         // PMX_K1_ROLE_SPLIT: the <RS> / <ONLYS> instances
    bool y16;                // PMX_K1_Y16: Y sixteen bytes per lane where its pitch and base allow it
    bool gfix;               // PMX_K1_GFIX: the K x K correction rides in K1
};
static inline bool k1_switch(const char* name) {
    const char* e = getenv(name);
    return !(e && atoi(e) == 0);
}
static inline K1Switches k1_read_switches() { return K1Switches{k1_switch("PMX_K1_ROLE_SPLIT"), k1_switch("PMX_K1_Y16"), k1_switch("PMX_K1_GFIX")}; }

// what a launch is, as far as the choice of instance goes
struct K1Facts {
    K1Inst inst;             // k1_instance
    bool doA, doS;           // gradients wanted (doA & 1: its bit 1 is a tuning switch of the kernels)
    bool chain;              // gA is summed along chains in this launch (chainL > 0)
    bool hasW;               // weights
    bool prof;               // a phase profile is collected
    bool y16;                // Y's pitch and base allow sixteen-byte fetches
    bool ride;               // the context can carry the K x K correction in this launch (enqueue_grad_once)
};

// An instance is the set of its kernel's boolean template parameters that are true; K1_*_INSTANCES lists the sets that are instantiated, one line each
// (the launchers build their tables from the same lists).
template <size_t N>
constexpr int k1_find_instance(const unsigned (&keys)[N], unsigned flags) {
    for (size_t i = 0; i < N; ++i)
        if (keys[i] == flags) return (int)i;
    return -1;
}
#define K1_INSTANCE_KEY(flags) (flags),

// ---- k_grad_f16_v8<PROF, HASW, CHAIN, LOSS, R3, HH, RS, ONLYS, Y16, GF> ----
enum : unsigned { V8_PROF = 1, V8_HASW = 2, V8_CHAIN = 4, V8_LOSS = 8, V8_R3 = 16, V8_HH = 32, V8_RS = 64, V8_ONLYS = 128, V8_Y16 = 256, V8_GF = 512 };
#define K1_F16_V8_INSTANCES(X)                          \
    X(0)                                                \
    X(V8_PROF)                                          \
    X(V8_HASW)                                          \
    X(V8_CHAIN)                                         \
    X(V8_CHAIN | V8_HASW)                               \
    X(V8_LOSS)                                          \
    X(V8_LOSS | V8_HASW)                                \
    X(V8_R3)                                            \
    X(V8_R3 | V8_CHAIN)                                 \
    X(V8_R3 | V8_LOSS)                                  \
    X(V8_HH)                                            \
    X(V8_HH | V8_CHAIN)                                 \
    X(V8_HH | V8_Y16)                                   \
    X(V8_HH | V8_Y16 | V8_CHAIN)                        \
    X(V8_HH | V8_ONLYS)                                 \
    X(V8_HH | V8_ONLYS | V8_Y16)                        \
    X(V8_HH | V8_RS)                                    \
    X(V8_HH | V8_RS | V8_CHAIN)                         \
    X(V8_HH | V8_RS | V8_Y16)                           \
    X(V8_HH | V8_RS | V8_Y16 | V8_CHAIN)                \
    X(V8_HH | V8_RS | V8_GF)                            \
    X(V8_HH | V8_RS | V8_GF | V8_CHAIN)                 \
    X(V8_HH | V8_RS | V8_GF | V8_Y16)                   \
    X(V8_HH | V8_RS | V8_GF | V8_Y16 | V8_CHAIN)
constexpr unsigned K1_F16_V8_KEYS[] = {K1_F16_V8_INSTANCES(K1_INSTANCE_KEY)};
static inline unsigned k1_flags_f16_v8(const K1Facts& f, const K1Switches& sw) {
    const unsigned chain = f.chain ? V8_CHAIN : 0, w = f.hasW ? V8_HASW : 0;
    if (f.inst == K1_HH) {           // the high x high residual whose missing terms arrive as a correction slab (no weights, never <PROF>)
        const unsigned y16 = f.y16 && sw.y16 && !f.prof ? V8_Y16 : 0;
        // <RS>: both gradients wanted.  <GF>: the correction's three stages on that instance's idle waves
        if (sw.role_split && f.doA && f.doS && !f.prof) return V8_HH | V8_RS | chain | y16 | (f.ride && sw.gfix ? V8_GF : 0);
        if (sw.role_split && !f.doA && f.doS) return V8_HH | V8_ONLYS | y16;        // gSt alone: nothing to chain
        return V8_HH | chain | y16;
    }
    const bool lossOnly = !f.doA && !f.doS;          // (no gradient is written: nothing to chain)
    if (f.inst == K1_R3) return lossOnly ? V8_R3 | V8_LOSS : V8_R3 | chain;      // the residual to fp32's class
    if (lossOnly) return V8_LOSS | w;
    if (f.chain) return V8_CHAIN | w;
    if (f.hasW) return V8_HASW;                      // (no phase profiling of the weighted instance)
    return f.prof ? V8_PROF : 0;
}

// ---- k_grad_f16_k128<HASW, CHAIN, HH, RS> ----
enum : unsigned { K128_HASW = 1, K128_CHAIN = 2, K128_HH = 4, K128_RS = 8 };
#define K1_F16_K128_INSTANCES(X)                        \
    X(0)                                                \
    X(K128_HASW)                                        \
    X(K128_CHAIN)                                       \
    X(K128_CHAIN | K128_HASW)                           \
    X(K128_HH)                                          \
    X(K128_HH | K128_CHAIN)                             \
    X(K128_HH | K128_RS)                                \
    X(K128_HH | K128_RS | K128_CHAIN)
constexpr unsigned K1_F16_K128_KEYS[] = {K1_F16_K128_INSTANCES(K1_INSTANCE_KEY)};
static inline unsigned k1_flags_f16_k128(const K1Facts& f, const K1Switches& sw) {
    const unsigned chain = f.chain && f.doA ? K128_CHAIN : 0;        // (only gA is chained)
    if (f.inst == K1_HH) return K128_HH | chain | (sw.role_split && f.doA && f.doS ? K128_RS : 0);      // <RS>: both gradients wanted
    return chain | (f.hasW ? K128_HASW : 0);
}

// ---- k_grad_f16_k32<LOSS, R3> ----
enum : unsigned { K32_LOSS = 1, K32_R3 = 2 };
#define K1_F16_K32_INSTANCES(X)                         \
    X(0)                                                \
    X(K32_LOSS)                                         \
    X(K32_R3)                                           \
    X(K32_R3 | K32_LOSS)
constexpr unsigned K1_F16_K32_KEYS[] = {K1_F16_K32_INSTANCES(K1_INSTANCE_KEY)};
static inline unsigned k1_flags_f16_k32(const K1Facts& f) {
    return (f.inst == K1_R3 ? K32_R3 : 0) | (!f.doA && !f.doS ? K32_LOSS : 0);       // <LOSS>: the loss-only pass (pmx_loglike, the line search)
}

// ---- k_grad_bf16_v7<PROF, HASW, CHAIN> ----
enum : unsigned { V7_PROF = 1, V7_HASW = 2, V7_CHAIN = 4 };
#define K1_BF16_V7_INSTANCES(X)                         \
    X(0)                                                \
    X(V7_PROF)                                          \
    X(V7_HASW)                                          \
    X(V7_CHAIN)                                         \
    X(V7_CHAIN | V7_HASW)
constexpr unsigned K1_BF16_V7_KEYS[] = {K1_BF16_V7_INSTANCES(K1_INSTANCE_KEY)};
static inline unsigned k1_flags_bf16_v7(const K1Facts& f) {
    if (f.chain) return V7_CHAIN | (f.hasW ? V7_HASW : 0);
    if (f.hasW) return V7_HASW;                      // (no phase profiling of the weighted instance)
    return f.prof ? V7_PROF : 0;
}

// ---- k_grad_f32_pc<K, HASW, CHAIN>: K = 64 (PC_K64) or 32 ----
enum : unsigned { PC_K64 = 1, PC_HASW = 2, PC_CHAIN = 4 };
#define K1_F32_PC_INSTANCES(X)                          \
    X(0)                                                \
    X(PC_HASW)                                          \
    X(PC_CHAIN)                                         \
    X(PC_CHAIN | PC_HASW)                               \
    X(PC_K64)                                           \
    X(PC_K64 | PC_HASW)                                 \
    X(PC_K64 | PC_CHAIN)                                \
    X(PC_K64 | PC_CHAIN | PC_HASW)
constexpr unsigned K1_F32_PC_KEYS[] = {K1_F32_PC_INSTANCES(K1_INSTANCE_KEY)};
static inline unsigned k1_flags_f32_pc(int K, const K1Facts& f) {
    return (K == 64 ? PC_K64 : 0) | (f.hasW ? PC_HASW : 0) | (f.chain ? PC_CHAIN : 0);
}
