// emu_label.cpp -- HOST EMULATOR of the label draw (vlgae_amd/csrc/vlg_label.hip: label_draw_kernel).  TEST INFRASTRUCTURE ONLY.
//
// The SAME body the gfx950 kernel runs (vlg_label_draw.h: label_draw_walk, vlg_sample_common.h: sample_draw) labels the arcs of given
// head vectors, under the one-lane host policy of emu_sample_common.h -- a "wavefront" of one lane, whose in-wave ordering points
// are no-ops.  Uniforms come from the explicit table u_label only (the counter-based source is device code).  The stage buffer is an
// arena of exactly kLabelStage floats with the canary of emu_dp.cpp behind it.
//
// Built two ways: as a shared library for ctypes calls (tests/test_labeled_host.py), and, with -DEMU_LABEL_MAIN, as a stand-alone
// program for the sanitizers, which replays a case file written by the test.
#include "emu_dp.cpp"
#include "emu_sample_common.h"

#include "../../vlgae_amd/csrc/vlg_label_draw.h"

#include <cstdio>

namespace {

struct LabelSeqX : SeqX {
    void lockstep() {}   // one lane: nothing to order
};

template <typename In>
int draw_batch(const void* phi_, const float* arc, const long long* heads, const int64_t* lengths, int B, int N, int L, int S,
               const float* u_label, long long* labels, float* logp) {
    auto phi = (const typename In::T*)phi_;
    LabelSeqX x{};
    for (int s = 0; s < S; ++s)
        for (int b = 0; b < B; ++b) {
            const size_t pair = (size_t)s * B + b, sb = pair * N;
            const int len = lengths ? (int)lengths[b] : N - 1;
            if (len < 1 || len > N - 1) {
                for (int i = 0; i < N; ++i) labels[sb + i] = 0;
                continue;
            }
            Arena A(vlg::kLabelStage * sizeof(float));
            const vlg::LabelTableU us{u_label + sb};
            vlg::label_draw_walk<In>(phi + (size_t)b * N * N * L, arc ? arc + (size_t)b * N * N : nullptr, N, L, len, heads + sb, us,
                                     (float*)A.at(0), labels + sb, logp && arc ? logp + pair : nullptr, x);
            A.check();
        }
    return 0;
}

}  // namespace

extern "C" int emu_label_draw(const void* phi, const float* arc, const long long* heads, const int64_t* lengths, int B, int N, int L, int S,
                              int in_dtype, const float* u_label, long long* labels, float* logp) {
    return in_dtype == 0 ? draw_batch<vlg::F32In>(phi, arc, heads, lengths, B, N, L, S, u_label, labels, logp)
                         : draw_batch<vlg::BF16In>(phi, arc, heads, lengths, B, N, L, S, u_label, labels, logp);
}

#ifdef EMU_LABEL_MAIN
// emu_label CASEFILE: int32 B, N, L, S; int64 lengths[B]; float phi[B N N L]; int64 heads[S B N]; float u_label[S B N];
// int64 expect[S B N].  Exit status 0 iff the draw returns `expect` exactly and no canary tripped.
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[4];
    if (std::fread(hdr, sizeof(int), 4, f) != 4) return 2;
    const int B = hdr[0], N = hdr[1], L = hdr[2], S = hdr[3];
    std::vector<int64_t> lengths(B);
    std::vector<float> phi((size_t)B * N * N * L), u((size_t)S * B * N);
    std::vector<long long> heads((size_t)S * B * N), expect((size_t)S * B * N), labels((size_t)S * B * N, -1);
    bool ok = std::fread(lengths.data(), 8, lengths.size(), f) == lengths.size() && std::fread(phi.data(), 4, phi.size(), f) == phi.size() &&
              std::fread(heads.data(), 8, heads.size(), f) == heads.size() && std::fread(u.data(), 4, u.size(), f) == u.size() &&
              std::fread(expect.data(), 8, expect.size(), f) == expect.size();
    std::fclose(f);
    if (!ok) return 2;
    emu_label_draw(phi.data(), nullptr, heads.data(), lengths.data(), B, N, L, S, 0, u.data(), labels.data(), nullptr);
    int bad = 0;
    for (size_t i = 0; i < labels.size(); ++i) bad += labels[i] != expect[i];
    std::printf("emu_label: B=%d N=%d L=%d S=%d mismatches=%d canary_trips=%d\n", B, N, L, S, bad, emu_canary_trips());
    return bad == 0 && emu_canary_trips() == 0 ? 0 : 1;
}
#endif
