// emu_expect.cpp -- HOST EMULATOR of the dual-number DepTree workgroup (vlgae_amd/csrc/vlg_expect.hip).  TEST INFRASTRUCTURE ONLY.
//
// The SAME body the gfx950 kernel runs (vlg_dp_expect.h: expect_run) under the token barrier of emu_dp.cpp, `nt` host threads as
// lanes.  The charts are carved as the kernel carves them (ExpectLayout at a chosen placement mode: LDS regions in the first arena, the
// workspace's in the second) with the canary of emu_dp.cpp behind each arena.
//
// Built two ways: as a shared library for ctypes calls (tests/test_expect_host.py), and, with -DEMU_EXPECT_MAIN, as a stand-alone
// program for the sanitizers, which replays a case file written by the test and writes what it computed.
#include "emu_dp.cpp"

#include "../../vlgae_amd/csrc/vlg_dp_expect.h"

#include <cstdio>

namespace {

template <bool GRAD>
void expect_one(const float* arc, const float* v, const float* v_sub, int len, int N, int mode, float* logZ, float* ev, float* mu, float* hv,
                int nt, int order) {
    const vlg::ExpectLayout L(N, GRAD, false, mode);
    Arena A(L.lds_bytes), W(L.ws_bytes);
    auto at = [&](const vlg::Region& r) { return (float*)(r.lds ? A.at(r.off) : W.at(r.off)); };
    vlg::ExpectCtx c;
    c.Ne = len + 1; c.len = len; c.P = vlg::chart_pitch(N);
    c.C = at(L.C); c.I = at(L.I); c.S = at(L.S); c.Cd = at(L.Cd); c.Id = at(L.Id); c.Sd = at(L.Sd);
    c.gCc = at(L.gCc); c.gCi = at(L.gCi); c.gI = at(L.gI); c.gCcd = at(L.gCcd); c.gCid = at(L.gCid); c.gId = at(L.gId);
    run_workgroup(nt, order, [&](int tid, HostX& x) {
        vlg::expect_run<GRAD, vlg::F32In, vlg::F32In>(c, arc, v, v_sub, N, logZ, ev, mu, hv, tid, nt, x);
    });
    A.check();
    W.check();
}

}  // namespace

// arc, v, v_sub [B,N,N] float32 (v, v_sub may be null); mu, hv [B,N,N] or null (both null: the forward-only body and layout)
extern "C" int emu_deptree_expect(const float* arc, const float* v, const float* v_sub, const int64_t* lengths, int B, int N, int mode,
                                  float* logZ, float* ev, float* mu, float* hv, int nt, int order) {
    const bool grad = mu || hv;
    for (int b = 0; b < B; ++b) {
        const int len = lengths ? (int)lengths[b] : N - 1;
        const size_t off = (size_t)b * N * N;
        if (len < 1 || len > N - 1) {   // restates the convention of the __global__ prologue (vlg_expect.hip), which only the GPU tests run
            logZ[b] = std::nanf("");
            if (ev) ev[b] = std::nanf("");
            for (size_t i = 0; i < (size_t)N * N; ++i) {
                if (mu) mu[off + i] = 0.f;
                if (hv) hv[off + i] = 0.f;
            }
            continue;
        }
        const float *vb = v ? v + off : nullptr, *sb = v_sub ? v_sub + off : nullptr;
        if (grad) expect_one<true>(arc + off, vb, sb, len, N, mode, logZ + b, ev ? ev + b : nullptr, mu ? mu + off : nullptr, hv ? hv + off : nullptr, nt, order);
        else expect_one<false>(arc + off, vb, sb, len, N, mode, logZ + b, ev ? ev + b : nullptr, nullptr, nullptr, nt, order);
    }
    return 0;
}

#ifdef EMU_EXPECT_MAIN
// emu_expect CASEFILE OUTFILE.  CASEFILE: int32 B, N, mode; int64 lengths[B]; float arc[B N N]; float v[B N N].
// OUTFILE: float logZ[B], ev[B], mu[B N N], hv[B N N].  Exit status 0 iff no canary tripped.
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[3];
    if (std::fread(hdr, sizeof(int), 3, f) != 3) return 2;
    const int B = hdr[0], N = hdr[1], mode = hdr[2];
    std::vector<int64_t> lengths(B);
    std::vector<float> arc((size_t)B * N * N), v(arc.size()), mu(arc.size(), -1.f), hv(arc.size(), -1.f), logZ(B), ev(B);
    const bool ok = std::fread(lengths.data(), 8, lengths.size(), f) == lengths.size() && std::fread(arc.data(), 4, arc.size(), f) == arc.size() &&
                    std::fread(v.data(), 4, v.size(), f) == v.size();
    std::fclose(f);
    if (!ok) return 2;
    emu_deptree_expect(arc.data(), v.data(), nullptr, lengths.data(), B, N, mode, logZ.data(), ev.data(), mu.data(), hv.data(), 16, 2);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(logZ.data(), 4, logZ.size(), o);
    std::fwrite(ev.data(), 4, ev.size(), o);
    std::fwrite(mu.data(), 4, mu.size(), o);
    std::fwrite(hv.data(), 4, hv.size(), o);
    std::fclose(o);
    std::printf("emu_expect: B=%d N=%d mode=%d canary_trips=%d\n", B, N, mode, g_canary_trips);
    return g_canary_trips == 0 ? 0 : 1;
}
#endif
