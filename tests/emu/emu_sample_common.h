// emu_sample_common.h -- what the host emulators of the two tree-sampling workgroups share (emu_sample.cpp: DepTree,
// emu_dmv_sample.cpp: DMV1o).  TEST INFRASTRUCTURE ONLY.  The one-lane wave policy under which vlg_sample_common.h's draw and walk
// steps run on the host, the not-a-sentence fill of the kernels (vlg_sample_kernels.h: sample_no_sentence) and the loop over a
// sentence's samples with their uniforms from the explicit table (the counter-based source is device code).  Included behind
// emu_dp.cpp, whose HostX the policy extends.
#pragma once
#include "../../vlgae_amd/csrc/vlg_sample_common.h"

namespace {

// a "wavefront" of one lane: the wave operations become the sequential max / running sum / first match they parallelise
struct SeqX : HostX {
    static constexpr int kWave = 1;
    int lane() const { return 0; }
    float wave_max(float v) { return v; }
    float wave_scan(float v) { return v; }
    float wave_last(float v) { return v; }
    int ballot_first(bool p) { return p ? 0 : -1; }
    int ballot_last(bool p) { return p ? 0 : -1; }
};

// sentence b is none (len outside 1 ... N - 1): logZ NaN, the heads of its S samples 0, their logp NaN.  False for a sentence.
inline bool sample_no_sentence(int len, int b, int B, int N, int S, long long* heads, float* logp, float* logZ) {
    if (len >= 1 && len <= N - 1) return false;
    const float nan = std::nanf("");
    if (logZ) logZ[b] = nan;
    for (int s = 0; s < S; ++s) {
        for (int i = 0; i < N; ++i) heads[((size_t)s * B + b) * N + i] = 0;
        if (logp) logp[(size_t)s * B + b] = nan;
    }
    return true;
}

// walk(us, heads, logp, x) for every sample s of sentence b: us = the table u [S,B,3,N,N] at [s][b], heads / logp that sample's
template <typename Walk>
void sample_each(int b, int B, int N, int S, const float* u, long long* heads, float* logp, const Walk& walk) {
    SeqX x{};
    for (int s = 0; s < S; ++s) {
        const vlg::TableU us{u + ((size_t)s * B + b) * 3 * N * N, N};
        walk(us, heads + ((size_t)s * B + b) * N, logp ? logp + (size_t)s * B + b : nullptr, x);
    }
}

}  // namespace
