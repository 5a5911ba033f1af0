// emu_kbest_common.h -- what the host emulators of the two K-best-trees workgroups share (emu_kbest.cpp: DepTree, emu_dmv_kbest.cpp:
// DMV1o).  TEST INFRASTRUCTURE ONLY.  The one-lane wave policy under which the walks run on the host, the two arenas a layout is
// carved over, the not-a-sentence fill of the kernels (vlg_kbest_kernels.h: kbest_no_sentence), the ranks of a sentence walked on the
// stacks the wavefronts would use, the switch over the code images and the plan's export.  Included behind emu_dp.cpp (HostX, Arena).
#pragma once
#include "../../vlgae_amd/csrc/vlg_dp_kbest.h"

#include <type_traits>

namespace {

// a "wavefront" of one lane
struct KbSeqX : HostX {
    static constexpr int kWave = 1;
    int lane() const { return 0; }
};

// The LDS and the workspace of one sentence, carved as the kernel carves them (at the placement mode the caller asks for: the spilled
// modes run at any N), with the canary of emu_dp.cpp behind each.  The workspace is pre-filled with stale contents -- quiet NaNs as
// floats, 0xffff back-pointers: nothing may depend on what it held.
struct KbArenas {
    Arena A, W;
    KbArenas(size_t lds_bytes, size_t ws_bytes) : A(lds_bytes), W(ws_bytes) {
        for (size_t i = 0; i + 4 <= ws_bytes; i += 4) {
            const uint32_t nanbits = 0x7fffffffu;
            std::memcpy(W.at(i), &nanbits, 4);
        }
    }
    template <typename T>
    T* at(const vlg::Region& r) { return (T*)(r.lds ? A.at(r.off) : W.at(r.off)); }
    void check() { A.check(); W.check(); }
};

// sentence b is none (len outside 1 ... N - 1): the heads of its K ranks 0, their scores NaN, its count 0.  False for a sentence.
inline bool kbest_no_sentence(int len, int b, int B, int N, int K, long long* heads, float* scores, int32_t* count) {
    if (len >= 1 && len <= N - 1) return false;
    for (int k = 0; k < K; ++k) {
        for (int i = 0; i < N; ++i) heads[((size_t)k * B + b) * N + i] = 0;
        scores[(size_t)k * B + b] = std::nanf("");
    }
    if (count) count[b] = 0;
    return true;
}

// walk(k, stack, heads, score, x) for the K ranks of sentence b, in order: wave k % 8 walks rank k, on its stack of `stacks`
template <typename Walk>
void kbest_each_rank(int b, int B, int N, int K, int* stacks, long long* heads, float* scores, const Walk& walk) {
    KbSeqX x{};
    for (int k = 0; k < K; ++k)
        walk(k, stacks + (k % vlg::kKbestWaves) * vlg::kKbestStack, heads + ((size_t)k * B + b) * N, scores + (size_t)k * B + b, x);
}

// go(KC) for the code image KC, as a compile-time constant
template <typename Go>
void kbest_image_switch(int KC, const Go& go) {
    switch (KC) {
        case 1: go(std::integral_constant<int, 1>{}); break;
        case 2: go(std::integral_constant<int, 2>{}); break;
        case 4: go(std::integral_constant<int, 4>{}); break;
        case 8: go(std::integral_constant<int, 8>{}); break;
        default: go(std::integral_constant<int, 16>{}); break;
    }
}

// the layout as the kernel carves it, for the tests' restatement: out = {KC, mode, lds_bytes, ws_stride} of the plan
template <typename Layout>
void kbest_plan_export(int N, int K, long long* out) {
    const vlg::KbestPlan p = vlg::kbest_plan_of<Layout>(N, K, vlg::kLdsBudget);
    out[0] = p.KC; out[1] = p.mode; out[2] = (long long)p.lds_bytes; out[3] = (long long)p.ws_stride;
}

}  // namespace
