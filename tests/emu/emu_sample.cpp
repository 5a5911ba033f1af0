// emu_sample.cpp -- HOST EMULATOR of the tree-sampling workgroup (vlgae_amd/csrc/vlg_sample.hip).  TEST INFRASTRUCTURE ONLY.
//
// The inside pass runs as in emu_dp.cpp (dep_run under the token barrier, `nt` host threads as lanes); behind it the SAME walk the
// gfx950 kernel runs (vlg_dp_sample.h: dep_sample_walk, vlg_sample_common.h: sample_draw) draws every sample from the charts, under
// the one-lane host policy of emu_sample_common.h.
// The charts and the walk's stack are carved as the kernel carves them -- stack behind DepLayout::lds_bytes -- with the canary of
// emu_dp.cpp behind each arena.  Uniforms come from an explicit table only (the counter-based source is device code).
//
// Built two ways: as part of a shared library for tests/emu/emu.py-style ctypes calls (tests/test_sample_host.py), and, with
// -DEMU_SAMPLE_MAIN, as a stand-alone program for the sanitizers, which replays a case file written by the test.
#include "emu_dp.cpp"
#include "emu_sample_common.h"

#include "../../vlgae_amd/csrc/vlg_dp_sample.h"

#include <cstdio>

namespace {

template <typename In>
int sample_batch(const void* arc_, const int64_t* lengths, int B, int N, int S, const float* u, long long* heads, float* logp,
                 float* logZ, int nt, int order) {
    auto arc = (const typename In::T*)arc_;
    for (int b = 0; b < B; ++b) {
        const int len = lengths ? (int)lengths[b] : N - 1;
        if (sample_no_sentence(len, b, B, N, S, heads, logp, logZ)) continue;
        const vlg::DepLayout L(N, false, false, g_dep_mode);
        Arena A(L.lds_bytes + vlg::kSampleStack * sizeof(int)), W(L.ws_bytes);   // one wave's stack behind the charts' LDS
        auto at = [&](const vlg::Region& r) { return r.lds ? A.at(r.off) : W.at(r.off); };
        vlg::DepCtx c;
        c.Ne = len + 1; c.len = len; c.P = vlg::chart_pitch(N);
        c.C = (float*)at(L.C); c.I = (float*)at(L.I); c.S = (float*)at(L.S);
        c.bpS = (unsigned char*)at(L.bpS); c.bpC = (unsigned char*)at(L.bpC);
        c.gCc = (float*)at(L.gCc); c.gCi = (float*)at(L.gCi); c.gI = (float*)at(L.gI);
        const typename In::T* arc_b = arc + (size_t)b * N * N;
        float lz = 0.f;
        run_workgroup(nt, order, [&](int tid, HostX& x) {
            vlg::dep_run<VLG_SR_LOG, false, In>(c, arc_b, N, 1.f, &lz, nullptr, nullptr, tid, nt, x);
        });
        const float lz2 = c.C[len + 1];
        if (logZ) logZ[b] = lz2 * VLG_LN2;
        int* stack = (int*)A.at(L.lds_bytes);
        sample_each(b, B, N, S, u, heads, logp, [&](const vlg::TableU& us, long long* h, float* lp, SeqX& x) {
            vlg::dep_sample_walk<In>(c, arc_b, N, stack, us, h, lp, lz2, x);
        });
        A.check();
        W.check();
    }
    return 0;
}

}  // namespace

extern "C" int emu_deptree_sample(const void* arc, const int64_t* lengths, int B, int N, int in_dtype, int S, const float* u,
                                  long long* heads, float* logp, float* logZ, int nt, int order) {
    return in_dtype == 0 ? sample_batch<vlg::F32In>(arc, lengths, B, N, S, u, heads, logp, logZ, nt, order)
                         : sample_batch<vlg::BF16In>(arc, lengths, B, N, S, u, heads, logp, logZ, nt, order);
}

#ifdef EMU_SAMPLE_MAIN
// emu_sample CASEFILE: int32 B, N, S; int64 lengths[B]; float arc[B N N]; float u[S B 3 N N]; int64 expect[S B N].
// Exit status 0 iff the walk returns `expect` exactly and no canary tripped.
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[3];
    if (std::fread(hdr, sizeof(int), 3, f) != 3) return 2;
    const int B = hdr[0], N = hdr[1], S = hdr[2];
    std::vector<int64_t> lengths(B);
    std::vector<float> arc((size_t)B * N * N), u((size_t)S * B * 3 * N * N), logp((size_t)S * B), logZ(B);
    std::vector<long long> expect((size_t)S * B * N), heads((size_t)S * B * N, -1);
    bool ok = std::fread(lengths.data(), 8, lengths.size(), f) == lengths.size() && std::fread(arc.data(), 4, arc.size(), f) == arc.size() &&
              std::fread(u.data(), 4, u.size(), f) == u.size() && std::fread(expect.data(), 8, expect.size(), f) == expect.size();
    std::fclose(f);
    if (!ok) return 2;
    emu_deptree_sample(arc.data(), lengths.data(), B, N, 0, S, u.data(), heads.data(), logp.data(), logZ.data(), 16, 2);
    int bad = 0;
    for (size_t i = 0; i < heads.size(); ++i) bad += heads[i] != expect[i];
    std::printf("emu_sample: B=%d N=%d S=%d mismatches=%d canary_trips=%d\n", B, N, S, bad, emu_canary_trips());
    return bad == 0 && emu_canary_trips() == 0 ? 0 : 1;
}
#endif
