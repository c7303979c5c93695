// Prints K1's instance decision (proxmin_amd/csrc/k1_instance.h) over its whole input space, one line per input:
//   family <TAB> key <TAB> flags <TAB> has_instance
// in the keys of tests/golden/k1_instances.json.  Built and run by test_k1_instances.py with a host compiler.
#include <stdio.h>
#include <string>
#include "k1_instance.h"

struct Name { unsigned bit; const char* name; };
template <size_t N, size_t M>
static void row(const char* family, const std::string& key, unsigned flags, const Name (&names)[N], const unsigned (&keys)[M]) {
    std::string s;
    for (const Name& n : names)
        if (flags & n.bit) s += (s.empty() ? "" : " ") + std::string(n.name);
    printf("%s\t%s\t%s\t%d\n", family, key.c_str(), s.empty() ? "-" : s.c_str(), k1_find_instance(keys, flags) >= 0);
}
static std::string bits(int v, int n) {
    std::string s;
    for (int i = n - 1; i >= 0; --i) s += (v >> i & 1) ? '1' : '0';
    return s;
}

int main() {
    static const char* INST[] = {"PLAIN", "R3", "HH", "V7"};
    static const Name v8[] = {{V8_PROF, "PROF"}, {V8_HASW, "HASW"}, {V8_CHAIN, "CHAIN"}, {V8_LOSS, "LOSS"}, {V8_R3, "R3"}, {V8_HH, "HH"}, {V8_RS, "RS"}, {V8_ONLYS, "ONLYS"}, {V8_Y16, "Y16"}, {V8_GF, "GF"}};
    static const Name k128[] = {{K128_HASW, "HASW"}, {K128_CHAIN, "CHAIN"}, {K128_HH, "HH"}, {K128_RS, "RS"}};
    static const Name k32[] = {{K32_LOSS, "LOSS"}, {K32_R3, "R3"}};
    static const Name v7[] = {{V7_PROF, "PROF"}, {V7_HASW, "HASW"}, {V7_CHAIN, "CHAIN"}};
    static const Name pc[] = {{PC_K64, "K64"}, {PC_HASW, "HASW"}, {PC_CHAIN, "CHAIN"}};
    for (K1Inst inst : {K1_PLAIN, K1_R3, K1_HH})
        for (int m = 0; m < 128; ++m)
            for (int s = 0; s < 8; ++s) {
                const K1Facts f{inst, (m >> 6 & 1) != 0, (m >> 5 & 1) != 0, (m >> 4 & 1) != 0, (m >> 3 & 1) != 0, (m >> 2 & 1) != 0, (m >> 1 & 1) != 0, (m & 1) != 0};
                const K1Switches sw{(s >> 2 & 1) != 0, (s >> 1 & 1) != 0, (s & 1) != 0};
                row("f16_v8", std::string(INST[inst]) + " " + bits(m, 7) + " " + bits(s, 3), k1_flags_f16_v8(f, sw), v8, K1_F16_V8_KEYS);
            }
    for (K1Inst inst : {K1_PLAIN, K1_HH})
        for (int m = 0; m < 16; ++m)
            for (int s = 0; s < 2; ++s) {
                const K1Facts f{inst, (m >> 3 & 1) != 0, (m >> 2 & 1) != 0, (m >> 1 & 1) != 0, (m & 1) != 0, false, false, false};
                row("f16_k128", std::string(INST[inst]) + " " + bits(m, 4) + " " + bits(s, 1), k1_flags_f16_k128(f, K1Switches{s != 0, true, true}), k128, K1_F16_K128_KEYS);
            }
    for (K1Inst inst : {K1_PLAIN, K1_R3})
        for (int m = 0; m < 4; ++m) {
            const K1Facts f{inst, (m >> 1 & 1) != 0, (m & 1) != 0, false, false, false, false, false};
            row("f16_k32", std::string(INST[inst]) + " " + bits(m, 2), k1_flags_f16_k32(f), k32, K1_F16_K32_KEYS);
        }
    for (int m = 0; m < 8; ++m) {
        const K1Facts f{K1_V7, true, true, (m >> 2 & 1) != 0, (m >> 1 & 1) != 0, (m & 1) != 0, false, false};
        row("bf16_v7", bits(m, 3), k1_flags_bf16_v7(f), v7, K1_BF16_V7_KEYS);
    }
    for (int K = 32; K <= 64; K += 32)
        for (int m = 0; m < 4; ++m) {
            const K1Facts f{K1_PLAIN, true, true, (m >> 1 & 1) != 0, (m & 1) != 0, false, false, false};
            row("f32_pc", std::to_string(K) + " " + bits(m, 2), k1_flags_f32_pc(K, f), pc, K1_F32_PC_KEYS);
        }
    // the switches are read from the environment by one function: "0" is off, anything else (unset included) is on
    setenv("PMX_K1_ROLE_SPLIT", "0", 1);
    setenv("PMX_K1_Y16", "1", 1);
    unsetenv("PMX_K1_GFIX");
    const K1Switches sw = k1_read_switches();
    printf("switches\t011\t%d%d%d\t1\n", sw.role_split, sw.y16, sw.gfix);
    return 0;
}
