// emu_dmv_expect.cpp -- HOST EMULATOR of the dual-number DMV1o workgroup (vlgae_amd/csrc/vlg_dmv_expect.hip).  TEST INFRASTRUCTURE ONLY.
//
// The SAME body the gfx950 kernel runs (vlg_dmv_expect.h: dmv_expect_run) under the token barrier of emu_dp.cpp, `nt` host threads as
// lanes.  The charts are carved as the kernel carves them (dmv_expect_carve over DmvExpectLayout at a chosen placement mode) over the
// two arenas of emu_expect_common.h.
//
// Built two ways: as a shared library for ctypes calls (tests/test_dmv_expect_host.py), and, with -DEMU_DMV_EXPECT_MAIN, as a
// stand-alone program for the sanitizers, which replays a case file written by the test and writes what it computed.
#include "emu_dp.cpp"

#include "emu_expect_common.h"
#include "../../vlgae_amd/csrc/vlg_dmv_expect.h"

namespace {

template <bool GRAD>
void dmv_expect_one(const vlg::DmvExpectIO& io, int len, int N, int mode, int nt, int order) {
    const vlg::DmvExpectLayout L(N, GRAD, false, mode);
    ExpectArenas arenas(L);
    const vlg::DmvExpectCtx c = vlg::dmv_expect_carve(L, N, len, [&](const vlg::Region& r) { return arenas.at<char>(r); });
    run_workgroup(nt, order, [&](int tid, HostX& x) { vlg::dmv_expect_run<GRAD, vlg::F32In, vlg::F32In>(c, io, N, tid, nt, x); });
    arenas.check();
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
        vlg::DmvExpectIO io;
        io.dec = dec + od; io.attach = attach + oa;
        io.v_dec = v_dec ? v_dec + od : nullptr; io.v_attach = v_attach ? v_attach + oa : nullptr;
        io.v_sub_dec = v_sub_dec ? v_sub_dec + od : nullptr; io.v_sub_attach = v_sub_attach ? v_sub_attach + oa : nullptr;
        io.logZ = logZ + b; io.ev = ev ? ev + b : nullptr;
        io.mu_dec = mu_dec ? mu_dec + od : nullptr; io.mu_attach = mu_attach ? mu_attach + oa : nullptr;
        io.hv_dec = hv_dec ? hv_dec + od : nullptr; io.hv_attach = hv_attach ? hv_attach + oa : nullptr;
        const size_t nd = (size_t)N * 8, na = (size_t)N * N * 2;
        if (expect_no_sentence(len, b, N, logZ, ev, {{io.mu_dec, nd}, {io.hv_dec, nd}, {io.mu_attach, na}, {io.hv_attach, na}})) continue;
        if (grad) dmv_expect_one<true>(io, len, N, mode, nt, order);
        else dmv_expect_one<false>(io, len, N, mode, nt, order);
    }
    return 0;
}

#ifdef EMU_DMV_EXPECT_MAIN
// emu_dmv_expect CASEFILE OUTFILE.  CASEFILE: int32 B, N, mode; int64 lengths[B]; float dec[B N 8], attach[B N N 2], v_dec[B N 8],
// v_attach[B N N 2].  OUTFILE: float logZ[B], ev[B], mu_dec, mu_attach, hv_dec, hv_attach.  Exit status 0 iff no canary tripped.
int main(int argc, char** argv) {
    return expect_case_main(
        "emu_dmv_expect", argc, argv,
        [](int B, int N) { const size_t d = (size_t)B * N * 8, a = (size_t)B * N * N * 2; return std::vector<size_t>{d, a, d, a}; },
        [](int B, int N, int mode, const int64_t* lengths, std::vector<std::vector<float>>& in, float* logZ, float* ev, std::vector<std::vector<float>>& out) {
            emu_dmv1o_expect(in[0].data(), in[1].data(), in[2].data(), in[3].data(), nullptr, nullptr, lengths, B, N, mode, logZ, ev, out[0].data(),
                             out[1].data(), out[2].data(), out[3].data(), 16, 2);
        });
}
#endif
