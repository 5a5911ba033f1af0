// emu_dmv_sample.cpp -- HOST EMULATOR of the DMV1o tree-sampling workgroup (vlgae_amd/csrc/vlg_dmv_sample.hip).  TEST INFRASTRUCTURE ONLY.
//
// The inside pass runs as in emu_dp.cpp (dmv_run<Log, false> through MergedIO under the token barrier, `nt` host threads as lanes);
// behind it the SAME walk the gfx950 kernel runs (vlg_dmv_sample.h: dmv_sample_walk, vlg_sample_common.h: sample_draw) draws every
// sample from the charts, under the one-lane host policy of emu_sample_common.h.  The charts and the walk's stack are carved as the kernel carves them -- the stack behind DmvLayout::lds_bytes, the
// charts in a second arena (the workspace) for the placements that move them there -- with the canary of emu_dp.cpp behind each arena.
// Uniforms come from an explicit table only (the counter-based source is device code).
//
// Built two ways: as a shared library for ctypes calls (tests/test_dmv_sample_host.py), and, with -DEMU_DMV_SAMPLE_MAIN, as a
// stand-alone program for the sanitizers, which replays a case file written by the test.
#include "emu_dp.cpp"
#include "emu_sample_common.h"

#include "../../vlgae_amd/csrc/vlg_dmv_sample.h"

#include <cstdio>

namespace {

static int g_dmv_sample_mode = -1;   // the placement to emulate: -1 = the one dp_plan picks for this N (the launcher's), 0 / 1 forced

template <typename In>
int dmv_sample_batch(const void* dec_, const void* attach_, const int64_t* lengths, int B, int N, int S, const float* u, long long* heads,
                     float* logp, float* logZ, int nt, int order) {
    auto dec = (const typename In::T*)dec_;
    auto attach = (const typename In::T*)attach_;
    for (int b = 0; b < B; ++b) {
        const int len = (int)lengths[b];
        if (sample_no_sentence(len, b, B, N, S, heads, logp, logZ)) continue;
        const int mode = g_dmv_sample_mode >= 0 ? g_dmv_sample_mode : vlg::placement_of(vlg::dp_plan<vlg::DmvLayout>(N, false, false).image);
        const vlg::DmvLayout L(N, false, false, mode, false);
        Arena A(L.lds_bytes + vlg::kDmvSampleStack * sizeof(int)), W(L.ws_bytes);   // one wave's stack behind the charts' LDS
        auto at = [&](const vlg::Region& r) { return r.lds ? A.at(r.off) : W.at(r.off); };
        vlg::DmvCtx c;
        c.walk = false;
        c.Ne = len + 1; c.len = len; c.P = vlg::chart_pitch(N);
        c.C = (float2*)at(L.C_in); c.I = (float2*)at(L.I_in); c.C2 = (float2*)at(L.C); c.I2 = (float2*)at(L.I);
        c.S = (float*)at(L.S);
        c.bpS = (unsigned char*)at(L.bpS); c.bpC = (unsigned char*)at(L.bpC);
        c.gCc = (float*)at(L.gCc); c.gCi = (float2*)at(L.gCi); c.gI = (float2*)at(L.gI);
        c.decs = (float*)at(L.decs); c.gdecs = (float*)at(L.gdecs);
        vlg::MergedIO<In> io;
        io.dec = dec + (size_t)b * N * 8; io.attach = attach + (size_t)b * N * N * 2; io.N = N;
        io.gdec = nullptr; io.gatt = nullptr; io.heads = nullptr;
        float lz = 0.f;
        run_workgroup(nt, order, [&](int tid, HostX& x) {
            if (mode != 0) vlg::dmv_run<VLG_SR_LOG, false, true>(c, io, 1.f, &lz, tid, nt, x);   // the long-sentence placements: chunked long spans
            else vlg::dmv_run<VLG_SR_LOG, false, false>(c, io, 1.f, &lz, tid, nt, x);
        });
        const float lz2 = c.C[len + 1].y;
        if (logZ) logZ[b] = lz2 * VLG_LN2;
        int* stack = (int*)A.at(L.lds_bytes);
        sample_each(b, B, N, S, u, heads, logp, [&](const vlg::TableU& us, long long* h, float* lp, SeqX& x) {
            vlg::dmv_sample_walk<In>(c, io.dec, io.attach, N, stack, us, h, lp, lz2, x);
        });
        A.check();
        W.check();
    }
    return 0;
}

}  // namespace

extern "C" void emu_set_dmv_sample_mode(int mode) { g_dmv_sample_mode = mode; }

// the placement the emulator takes for this N when none is forced: 0 = both charts behind the first arena's start (LDS), 1 = workspace
extern "C" int emu_dmv_sample_placement(int N) { return vlg::placement_of(vlg::dp_plan<vlg::DmvLayout>(N, false, false).image); }

extern "C" int emu_dmv1o_sample(const void* dec, const void* attach, const int64_t* lengths, int B, int N, int in_dtype, int S,
                                const float* u, long long* heads, float* logp, float* logZ, int nt, int order) {
    return in_dtype == 0 ? dmv_sample_batch<vlg::F32In>(dec, attach, lengths, B, N, S, u, heads, logp, logZ, nt, order)
                         : dmv_sample_batch<vlg::BF16In>(dec, attach, lengths, B, N, S, u, heads, logp, logZ, nt, order);
}

#ifdef EMU_DMV_SAMPLE_MAIN
// emu_dmv_sample CASEFILE: int32 B, N, S; int64 lengths[B]; float dec[B N 8]; float attach[B N N 2]; float u[S B 3 N N];
// int64 expect[S B N].  Exit status 0 iff the walk returns `expect` exactly and no canary tripped.
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[3];
    if (std::fread(hdr, sizeof(int), 3, f) != 3) return 2;
    const int B = hdr[0], N = hdr[1], S = hdr[2];
    std::vector<int64_t> lengths(B);
    std::vector<float> dec((size_t)B * N * 8), attach((size_t)B * N * N * 2), u((size_t)S * B * 3 * N * N), logp((size_t)S * B), logZ(B);
    std::vector<long long> expect((size_t)S * B * N), heads((size_t)S * B * N, -1);
    bool ok = std::fread(lengths.data(), 8, lengths.size(), f) == lengths.size() && std::fread(dec.data(), 4, dec.size(), f) == dec.size() &&
              std::fread(attach.data(), 4, attach.size(), f) == attach.size() && std::fread(u.data(), 4, u.size(), f) == u.size() &&
              std::fread(expect.data(), 8, expect.size(), f) == expect.size();
    std::fclose(f);
    if (!ok) return 2;
    emu_dmv1o_sample(dec.data(), attach.data(), lengths.data(), B, N, 0, S, u.data(), heads.data(), logp.data(), logZ.data(), 16, 2);
    int bad = 0;
    for (size_t i = 0; i < heads.size(); ++i) bad += heads[i] != expect[i];
    std::printf("emu_dmv_sample: B=%d N=%d S=%d mismatches=%d canary_trips=%d\n", B, N, S, bad, emu_canary_trips());
    return bad == 0 && emu_canary_trips() == 0 ? 0 : 1;
}
#endif
