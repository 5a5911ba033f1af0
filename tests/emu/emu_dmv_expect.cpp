// emu_dmv_expect.cpp -- HOST EMULATOR of the dual-number DMV1o workgroup (vlgae_amd/csrc/vlg_dmv_expect.hip).  TEST INFRASTRUCTURE ONLY.
//
// The SAME body the gfx950 kernel runs (vlg_dmv_expect.h: dmv_expect_run) under the token barrier of emu_dp.cpp, `nt` host threads as
// lanes.  The charts are carved as the kernel carves them (DmvExpectLayout at a chosen placement mode: LDS regions in the first arena,
// the workspace's in the second) with the canary of emu_dp.cpp behind each arena.
//
// Built two ways: as a shared library for ctypes calls (tests/test_dmv_expect_host.py), and, with -DEMU_DMV_EXPECT_MAIN, as a
// stand-alone program for the sanitizers, which replays a case file written by the test and writes what it computed.
#include "emu_dp.cpp"

#include "../../vlgae_amd/csrc/vlg_dmv_expect.h"

#include <cstdio>

namespace {

template <bool GRAD>
void dmv_expect_one(const vlg::DmvExpectIO& io, int len, int N, int mode, int nt, int order) {
    const vlg::DmvExpectLayout L(N, GRAD, false, mode);
    Arena A(L.lds_bytes), W(L.ws_bytes);
    auto at = [&](const vlg::Region& r) { return r.lds ? A.at(r.off) : W.at(r.off); };
    vlg::DmvExpectCtx c;
    c.Ne = len + 1; c.len = len; c.P = vlg::chart_pitch(N);
    c.C = (float2*)at(L.C); c.I = (float2*)at(L.I); c.S = (float*)at(L.S);
    c.Cd = (float2*)at(L.Cd); c.Id = (float2*)at(L.Id); c.Sd = (float*)at(L.Sd);
    c.gCc = (float*)at(L.gCc); c.gCi = (float2*)at(L.gCi); c.gI = (float2*)at(L.gI);
    c.gCcd = (float*)at(L.gCcd); c.gCid = (float2*)at(L.gCid); c.gId = (float2*)at(L.gId);
    c.decs = (float*)at(L.decs); c.decsd = (float*)at(L.decsd);
    run_workgroup(nt, order, [&](int tid, HostX& x) { vlg::dmv_expect_run<GRAD, vlg::F32In, vlg::F32In>(c, io, N, tid, nt, x); });
    A.check();
    W.check();
}

}  // namespace

// dec [B,N,2,2,2], attach [B,N,N,2] float32; v_*, v_sub_* like them or null; mu_*, hv_* like them or null (all four null: the
// forward-only body and layout)
extern "C" int emu_dmv1o_expect(const float* dec, const float* attach, const float* v_dec, const float* v_attach, const float* v_sub_dec,
                                const float* v_sub_attach, const int64_t* lengths, int B, int N, int mode, float* logZ, float* ev,
                                float* mu_dec, float* mu_attach, float* hv_dec, float* hv_attach, int nt, int order) {
    const bool grad = mu_dec || mu_attach || hv_dec || hv_attach;
    for (int b = 0; b < B; ++b) {
        const int len = (int)lengths[b];
        const size_t od = (size_t)b * N * 8, oa = (size_t)b * N * N * 2;
        if (len < 1 || len > N - 1) {   // restates the convention of the __global__ prologue (vlg_dmv_expect.hip), which only the GPU tests run
            logZ[b] = std::nanf("");
            if (ev) ev[b] = std::nanf("");
            for (size_t i = 0; i < (size_t)N * 8; ++i) {
                if (mu_dec) mu_dec[od + i] = 0.f;
                if (hv_dec) hv_dec[od + i] = 0.f;
            }
            for (size_t i = 0; i < (size_t)N * N * 2; ++i) {
                if (mu_attach) mu_attach[oa + i] = 0.f;
                if (hv_attach) hv_attach[oa + i] = 0.f;
            }
            continue;
        }
        vlg::DmvExpectIO io;
        io.dec = dec + od; io.attach = attach + oa;
        io.v_dec = v_dec ? v_dec + od : nullptr; io.v_attach = v_attach ? v_attach + oa : nullptr;
        io.v_sub_dec = v_sub_dec ? v_sub_dec + od : nullptr; io.v_sub_attach = v_sub_attach ? v_sub_attach + oa : nullptr;
        io.logZ = logZ + b; io.ev = ev ? ev + b : nullptr;
        io.mu_dec = mu_dec ? mu_dec + od : nullptr; io.mu_attach = mu_attach ? mu_attach + oa : nullptr;
        io.hv_dec = hv_dec ? hv_dec + od : nullptr; io.hv_attach = hv_attach ? hv_attach + oa : nullptr;
        if (grad) dmv_expect_one<true>(io, len, N, mode, nt, order);
        else dmv_expect_one<false>(io, len, N, mode, nt, order);
    }
    return 0;
}

#ifdef EMU_DMV_EXPECT_MAIN
// emu_dmv_expect CASEFILE OUTFILE.  CASEFILE: int32 B, N, mode; int64 lengths[B]; float dec[B N 8], attach[B N N 2], v_dec[B N 8],
// v_attach[B N N 2].  OUTFILE: float logZ[B], ev[B], mu_dec, mu_attach, hv_dec, hv_attach.  Exit status 0 iff no canary tripped.
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[3];
    if (std::fread(hdr, sizeof(int), 3, f) != 3) return 2;
    const int B = hdr[0], N = hdr[1], mode = hdr[2];
    std::vector<int64_t> lengths(B);
    std::vector<float> dec((size_t)B * N * 8), att((size_t)B * N * N * 2), vd(dec.size()), va(att.size()), logZ(B), ev(B);
    std::vector<float> mud(dec.size(), -1.f), mua(att.size(), -1.f), hvd(dec.size(), -1.f), hva(att.size(), -1.f);
    const bool ok = std::fread(lengths.data(), 8, lengths.size(), f) == lengths.size() && std::fread(dec.data(), 4, dec.size(), f) == dec.size() &&
                    std::fread(att.data(), 4, att.size(), f) == att.size() && std::fread(vd.data(), 4, vd.size(), f) == vd.size() &&
                    std::fread(va.data(), 4, va.size(), f) == va.size();
    std::fclose(f);
    if (!ok) return 2;
    emu_dmv1o_expect(dec.data(), att.data(), vd.data(), va.data(), nullptr, nullptr, lengths.data(), B, N, mode, logZ.data(), ev.data(),
                     mud.data(), mua.data(), hvd.data(), hva.data(), 16, 2);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    for (const std::vector<float>* a : {&logZ, &ev, &mud, &mua, &hvd, &hva}) std::fwrite(a->data(), 4, a->size(), o);
    std::fclose(o);
    std::printf("emu_dmv_expect: B=%d N=%d mode=%d canary_trips=%d\n", B, N, mode, g_canary_trips);
    return g_canary_trips == 0 ? 0 : 1;
}
#endif
