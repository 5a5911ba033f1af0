// emu_expect.cpp -- HOST EMULATOR of the dual-number DepTree workgroup (vlgae_amd/csrc/vlg_expect.hip).  TEST INFRASTRUCTURE ONLY.
//
// The SAME body the gfx950 kernel runs (vlg_dp_expect.h: expect_run) under the token barrier of emu_dp.cpp, `nt` host threads as
// lanes.  The charts are carved as the kernel carves them (expect_carve over ExpectLayout at a chosen placement mode) over the two
// arenas of emu_expect_common.h.
//
// Built two ways: as a shared library for ctypes calls (tests/test_expect_host.py), and, with -DEMU_EXPECT_MAIN, as a stand-alone
// program for the sanitizers, which replays a case file written by the test and writes what it computed.
#include "emu_dp.cpp"

#include "emu_expect_common.h"

namespace {

template <bool GRAD>
void expect_one(const float* arc, const float* v, const float* v_sub, int len, int N, int mode, float* logZ, float* ev, float* mu, float* hv,
                int nt, int order) {
    const vlg::ExpectLayout L(N, GRAD, false, mode);
    ExpectArenas arenas(L);
    const vlg::ExpectCtx c = vlg::expect_carve(L, N, len, [&](const vlg::Region& r) { return arenas.at<char>(r); });
    run_workgroup(nt, order, [&](int tid, HostX& x) {
        vlg::expect_run<GRAD, vlg::F32In, vlg::F32In>(c, arc, v, v_sub, N, logZ, ev, mu, hv, tid, nt, x);
    });
    arenas.check();
}

}  // namespace

// arc, v, v_sub [B,N,N] float32 (v, v_sub may be null); mu, hv [B,N,N] or null (both null: the forward-only body and layout)
extern "C" int emu_deptree_expect(const float* arc, const float* v, const float* v_sub, const int64_t* lengths, int B, int N, int mode,
                                  float* logZ, float* ev, float* mu, float* hv, int nt, int order) {
    const bool grad = mu || hv;
    for (int b = 0; b < B; ++b) {
        const int len = lengths ? (int)lengths[b] : N - 1;
        const size_t off = (size_t)b * N * N;
        float *mb = mu ? mu + off : nullptr, *hb = hv ? hv + off : nullptr;
        if (expect_no_sentence(len, b, N, logZ, ev, {{mb, (size_t)N * N}, {hb, (size_t)N * N}})) continue;
        const float *vb = v ? v + off : nullptr, *sb = v_sub ? v_sub + off : nullptr;
        if (grad) expect_one<true>(arc + off, vb, sb, len, N, mode, logZ + b, ev ? ev + b : nullptr, mb, hb, nt, order);
        else expect_one<false>(arc + off, vb, sb, len, N, mode, logZ + b, ev ? ev + b : nullptr, nullptr, nullptr, nt, order);
    }
    return 0;
}

#ifdef EMU_EXPECT_MAIN
// emu_expect CASEFILE OUTFILE.  CASEFILE: int32 B, N, mode; int64 lengths[B]; float arc[B N N]; float v[B N N].
// OUTFILE: float logZ[B], ev[B], mu[B N N], hv[B N N].  Exit status 0 iff no canary tripped.
int main(int argc, char** argv) {
    return expect_case_main(
        "emu_expect", argc, argv, [](int B, int N) { return std::vector<size_t>(2, (size_t)B * N * N); },
        [](int B, int N, int mode, const int64_t* lengths, std::vector<std::vector<float>>& in, float* logZ, float* ev, std::vector<std::vector<float>>& out) {
            emu_deptree_expect(in[0].data(), in[1].data(), nullptr, lengths, B, N, mode, logZ, ev, out[0].data(), out[1].data(), 16, 2);
        });
}
#endif
