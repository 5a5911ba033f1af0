// emu_expect_common.h -- what the host emulators of the two dual-number workgroups share (emu_expect.cpp: DepTree, emu_dmv_expect.cpp:
// DMV1o).  TEST INFRASTRUCTURE ONLY.  The two arenas a layout is carved over, the not-a-sentence fill of the kernels and the case
// file of the stand-alone programs.  Included behind emu_dp.cpp (Arena, g_canary_trips).
#pragma once
#include "../../vlgae_amd/csrc/vlg_dp_expect.h"

#include <cstdio>
#include <initializer_list>
#include <vector>

namespace {

// The LDS and the workspace of one sentence, carved as the kernel carves them (LDS regions in the first arena, the workspace's in the
// second), with the canary of emu_dp.cpp behind each.
struct ExpectArenas {
    Arena A, W;
    template <typename Layout>
    explicit ExpectArenas(const Layout& L) : A(L.lds_bytes), W(L.ws_bytes) {}
    template <typename T>
    T* at(const vlg::Region& r) { return (T*)(r.lds ? A.at(r.off) : W.at(r.off)); }
    void check() { A.check(); W.check(); }
};

// an output of a sentence (NULL: not asked for) and its element count
struct ExpectOut {
    float* p;
    size_t n;
};

// Sentence b is none (len outside 1 ... N - 1): logZ and ev NaN, every output given zero.  False for a sentence.  Restates the
// convention of the __global__ prologues (vlg_expect.hip, vlg_dmv_expect.hip), which only the GPU tests run.
inline bool expect_no_sentence(int len, int b, int N, float* logZ, float* ev, std::initializer_list<ExpectOut> outs) {
    if (len >= 1 && len <= N - 1) return false;
    logZ[b] = std::nanf("");
    if (ev) ev[b] = std::nanf("");
    for (const ExpectOut& o : outs)
        for (size_t i = 0; o.p && i < o.n; ++i) o.p[i] = 0.f;
    return true;
}

// The case file of a stand-alone program: int32 B, N, mode; int64 lengths[B]; then the float arrays of sizes(B, N), in order.  The
// outputs are logZ[B], ev[B] and, REQUIRED of a model that uses this, one array per input array and of its size, pre-filled with -1:
// an expected count and its tangent are shaped like the potential and the direction they belong to (DepTree: arc, v -> mu, hv; DMV1o:
// dec, attach, v_dec, v_attach -> mu_dec, mu_attach, hv_dec, hv_attach).  run(B, N, mode, lengths, in, logZ, ev, out) computes them.
// Writes them in that order, prints the canary line, exit status 0 iff no canary tripped.
template <typename Sizes, typename Run>
int expect_case_main(const char* name, int argc, char** argv, const Sizes& sizes, const Run& run) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[3];
    if (std::fread(hdr, sizeof(int), 3, f) != 3) {
        std::fclose(f);
        return 2;
    }
    const int B = hdr[0], N = hdr[1], mode = hdr[2];
    std::vector<int64_t> lengths(B);
    bool ok = std::fread(lengths.data(), 8, lengths.size(), f) == lengths.size();
    std::vector<std::vector<float>> in, out;
    for (size_t n : sizes(B, N)) {
        in.emplace_back(n);
        out.emplace_back(n, -1.f);
        ok = ok && std::fread(in.back().data(), 4, n, f) == n;
    }
    std::fclose(f);
    if (!ok) return 2;
    std::vector<float> logZ(B), ev(B);
    run(B, N, mode, lengths.data(), in, logZ.data(), ev.data(), out);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(logZ.data(), 4, logZ.size(), o);
    std::fwrite(ev.data(), 4, ev.size(), o);
    for (const std::vector<float>& a : out) std::fwrite(a.data(), 4, a.size(), o);
    std::fclose(o);
    std::printf("%s: B=%d N=%d mode=%d canary_trips=%d\n", name, B, N, mode, g_canary_trips);
    return g_canary_trips == 0 ? 0 : 1;
}

}  // namespace
