// vlg_dmv_expect.hip -- expectations under DMV1o on the device (vlg_dmv1o_expect, include/vlgae_amd.h): the gfx950 kernel around
// vlg_dmv_expect.h.  Replaces the reference's StructDistribution.entropy / cross_entropy / kl / risk
// (src/model/torch_struct/distributions.py:79-114: the Python width loop of dmv.py under an expectation semiring, differentiated by
// autograd) for DMV1o.
//
// One workgroup per sentence runs the DMV1o inside pass -- and, when any of mu / hv is wanted, the outside pass -- in dual numbers:
// every chart cell carries its derivative along the direction (v_dec - v_sub_dec, v_attach - v_sub_attach).  One launch returns logZ,
// ev = <mu, d>, the expected counts mu and hv = (Hessian of logZ) d; entropy, cross-entropy, KL and expected scores and all their
// gradients are arithmetic on these.  No atomics, one writer per output element, one barrier per span width.  Charts live in LDS
// where they fit and in the caller's workspace otherwise (DmvExpectLayout, vlg_dmv_expect.h).  The launch frame is vlg_expect_kernels.h.
#include "vlg_expect_kernels.h"
#include "vlg_dmv_expect.h"

namespace vlg {

struct DmvExpectArgs {
    const void *dec, *attach, *v_dec, *v_attach, *v_sub_dec, *v_sub_attach;
    const int64_t* lengths;
    int B, N;
    float *logZ, *ev, *mu_dec, *mu_attach, *hv_dec, *hv_attach;
    char* ws;
    size_t ws_stride, lds;
    hipStream_t s;
};

template <bool GRAD, int MODE, typename In, typename VIn>
__global__ __launch_bounds__(kThreads) void dmv1o_expect_kernel(const DmvExpectArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x, tid = threadIdx.x, N = a.N;
    const int len = (int)a.lengths[b];
    const size_t dec_off = (size_t)b * N * 8, att_off = (size_t)b * N * N * 2;
    if (len < 1 || len > N - 1) {   // not a sentence (block-uniform): NaN values, zero counts -- the convention of dmv1o_kernel
        if (tid == 0) {
            a.logZ[b] = __uint_as_float(0x7fc00000u);
            if (a.ev) a.ev[b] = __uint_as_float(0x7fc00000u);
        }
        if (GRAD) {
            if (a.mu_attach) for (int i = tid; i < N * N * 2; i += kThreads) a.mu_attach[att_off + i] = 0.f;
            if (a.hv_attach) for (int i = tid; i < N * N * 2; i += kThreads) a.hv_attach[att_off + i] = 0.f;
            if (a.mu_dec) for (int i = tid; i < N * 8; i += kThreads) a.mu_dec[dec_off + i] = 0.f;
            if (a.hv_dec) for (int i = tid; i < N * 8; i += kThreads) a.hv_dec[dec_off + i] = 0.f;
        }
        return;
    }
    using T = typename In::T;
    using VT = typename VIn::T;
    char* wsb = a.ws + (size_t)b * a.ws_stride;
    const DmvExpectLayout L(N, GRAD, false, MODE);
    const DmvExpectCtx c = dmv_expect_carve(L, N, len, [&](const Region& r) { return region_ptr<char>(r, smem, wsb); });
    DmvExpectIO io;
    io.dec = (const T*)a.dec + dec_off;
    io.attach = (const T*)a.attach + att_off;
    io.v_dec = a.v_dec ? (const VT*)a.v_dec + dec_off : nullptr;
    io.v_attach = a.v_attach ? (const VT*)a.v_attach + att_off : nullptr;
    io.v_sub_dec = a.v_sub_dec ? (const VT*)a.v_sub_dec + dec_off : nullptr;
    io.v_sub_attach = a.v_sub_attach ? (const VT*)a.v_sub_attach + att_off : nullptr;
    io.logZ = a.logZ + b;
    io.ev = a.ev ? a.ev + b : nullptr;
    io.mu_dec = (GRAD && a.mu_dec) ? a.mu_dec + dec_off : nullptr;
    io.mu_attach = (GRAD && a.mu_attach) ? a.mu_attach + att_off : nullptr;
    io.hv_dec = (GRAD && a.hv_dec) ? a.hv_dec + dec_off : nullptr;
    io.hv_attach = (GRAD && a.hv_attach) ? a.hv_attach + att_off : nullptr;
    DevX x;
    dmv_expect_run<GRAD, In, VIn>(c, io, N, tid, kThreads, x);
}

}  // namespace vlg

extern "C" size_t vlg_dmv1o_expect_workspace(int B, int N, int grad) {
    if (B <= 0 || N < 2 || N > 255) return 0;
    return vlg::expect_workspace_bytes<vlg::DmvExpectLayout>(B, N, grad != 0);
}

extern "C" int vlg_dmv1o_expect(const void* dec, const void* attach, const void* v_dec, const void* v_attach, const void* v_sub_dec,
                                const void* v_sub_attach, const int64_t* lengths, int B, int N, int in_dtype, int v_dtype, float* logZ,
                                float* ev, float* mu_dec, float* mu_attach, float* hv_dec, float* hv_attach, void* ws, size_t ws_bytes,
                                void* stream) {
    using namespace vlg;
    return expect_entry<DmvExpectLayout>("dmv1o_expect", B, N, in_dtype, v_dtype, "dec, attach, lengths and logZ", dec && attach && lengths && logZ,
                                         mu_dec || mu_attach || hv_dec || hv_attach, ws, ws_bytes,
                                         [&](const DpPlan& p, auto G, auto M, auto I, auto V) {
        const DmvExpectArgs a{dec, attach, v_dec, v_attach, v_sub_dec, v_sub_attach, lengths, B, N, logZ, ev, mu_dec, mu_attach, hv_dec,
                              hv_attach, (char*)ws, p.ws_stride, p.lds_bytes, (hipStream_t)stream};
        return launch("dmv1o_expect_kernel", dmv1o_expect_kernel<G.value, M.value, decltype(I), decltype(V)>, dim3(B), dim3(kThreads), a.lds, a.s, a);
    });
}
