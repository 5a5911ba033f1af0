// vlg_dmv_expect.hip -- expectations under DMV1o on the device (vlg_dmv1o_expect, include/vlgae_amd.h): the gfx950 kernel around
// vlg_dmv_expect.h.  Replaces the reference's StructDistribution.entropy / cross_entropy / kl / risk
// (src/model/torch_struct/distributions.py:79-114: the Python width loop of dmv.py under an expectation semiring, differentiated by
// autograd) for DMV1o.
//
// One workgroup per sentence runs the DMV1o inside pass -- and, when any of mu / hv is wanted, the outside pass -- in dual numbers:
// every chart cell carries its derivative along the direction (v_dec - v_sub_dec, v_attach - v_sub_attach).  One launch returns logZ,
// ev = <mu, d>, the expected counts mu and hv = (Hessian of logZ) d; entropy, cross-entropy, KL and expected scores and all their
// gradients are arithmetic on these.  No atomics, one writer per output element, one barrier per span width.  Charts live in LDS
// where they fit and in the caller's workspace otherwise (DmvExpectLayout, vlg_dmv_expect.h).
#include "vlg_dp_kernels.h"
#include "vlg_dmv_expect.h"

namespace vlg {

template <bool GRAD, int MODE>
__device__ __forceinline__ DmvExpectCtx carve_dmv_expect(int N, int len, char* smem, char* wsb) {
    const DmvExpectLayout L(N, GRAD, false, MODE);
    DmvExpectCtx c;
    c.Ne = len + 1;
    c.len = len;
    c.P = chart_pitch(N);
    c.C = region_ptr<float2>(L.C, smem, wsb);
    c.I = region_ptr<float2>(L.I, smem, wsb);
    c.S = region_ptr<float>(L.S, smem, wsb);
    c.Cd = region_ptr<float2>(L.Cd, smem, wsb);
    c.Id = region_ptr<float2>(L.Id, smem, wsb);
    c.Sd = region_ptr<float>(L.Sd, smem, wsb);
    c.gCc = region_ptr<float>(L.gCc, smem, wsb);
    c.gCi = region_ptr<float2>(L.gCi, smem, wsb);
    c.gI = region_ptr<float2>(L.gI, smem, wsb);
    c.gCcd = region_ptr<float>(L.gCcd, smem, wsb);
    c.gCid = region_ptr<float2>(L.gCid, smem, wsb);
    c.gId = region_ptr<float2>(L.gId, smem, wsb);
    c.decs = region_ptr<float>(L.decs, smem, wsb);
    c.decsd = region_ptr<float>(L.decsd, smem, wsb);
    return c;
}

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
    const DmvExpectCtx c = carve_dmv_expect<GRAD, MODE>(N, len, smem, a.ws + (size_t)b * a.ws_stride);
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

template <bool GRAD, int MODE, typename In, typename VIn>
static int launch_dmv_expect(const DmvExpectArgs& a) {
    return launch("dmv1o_expect_kernel", dmv1o_expect_kernel<GRAD, MODE, In, VIn>, dim3(a.B), dim3(kThreads), a.lds, a.s, a);
}

template <bool GRAD, typename In, typename VIn>
static int launch_dmv_expect_mode(int mode, const DmvExpectArgs& a) {
    switch (mode) {
        case 0: return launch_dmv_expect<GRAD, 0, In, VIn>(a);
        case 1: return launch_dmv_expect<GRAD, 1, In, VIn>(a);
        case 2: return launch_dmv_expect<GRAD, 2, In, VIn>(a);
        default:   // (forward only: placements 2 and 3 are the same, staging only)
            if constexpr (GRAD) return launch_dmv_expect<GRAD, 3, In, VIn>(a);
            else return launch_dmv_expect<GRAD, 2, In, VIn>(a);
    }
}

template <typename In, typename VIn>
static int launch_dmv_expect_grad(bool grad, int mode, const DmvExpectArgs& a) {
    return grad ? launch_dmv_expect_mode<true, In, VIn>(mode, a) : launch_dmv_expect_mode<false, In, VIn>(mode, a);
}

}  // namespace vlg

extern "C" size_t vlg_dmv1o_expect_workspace(int B, int N, int grad) {
    if (B <= 0 || N < 2 || N > 255) return 0;
    return vlg::dmv_expect_plan(N, grad != 0).ws_stride * (size_t)B;
}

extern "C" int vlg_dmv1o_expect(const void* dec, const void* attach, const void* v_dec, const void* v_attach, const void* v_sub_dec,
                                const void* v_sub_attach, const int64_t* lengths, int B, int N, int in_dtype, int v_dtype, float* logZ,
                                float* ev, float* mu_dec, float* mu_attach, float* hv_dec, float* hv_attach, void* ws, size_t ws_bytes,
                                void* stream) {
    using namespace vlg;
    if (int e = check_dp_args("dmv1o_expect", B, N, in_dtype, VLG_SR_LOG)) return e;
    if (v_dtype != VLG_F32 && v_dtype != VLG_BF16) return set_error(VLG_ERR_DTYPE, "dmv1o_expect: v_dtype %d", v_dtype);
    if (B == 0) return 0;
    if (!dec || !attach || !lengths || !logZ)
        return set_error(VLG_ERR_ARG, "dmv1o_expect: null buffer (dec, attach, lengths and logZ are required)");
    const bool grad = mu_dec || mu_attach || hv_dec || hv_attach;
    const DpPlan p = dmv_expect_plan(N, grad);
    if (int e = check_dp_workspace("dmv1o_expect", N, p, B, ws, ws_bytes)) return e;
    const DmvExpectArgs a{dec, attach, v_dec, v_attach, v_sub_dec, v_sub_attach, lengths, B, N, logZ, ev, mu_dec, mu_attach, hv_dec,
                          hv_attach, (char*)ws, p.ws_stride, p.lds_bytes, (hipStream_t)stream};
    const int mode = placement_of(p.image);
    if (in_dtype == VLG_F32)
        return v_dtype == VLG_F32 ? launch_dmv_expect_grad<F32In, F32In>(grad, mode, a) : launch_dmv_expect_grad<F32In, BF16In>(grad, mode, a);
    return v_dtype == VLG_F32 ? launch_dmv_expect_grad<BF16In, F32In>(grad, mode, a) : launch_dmv_expect_grad<BF16In, BF16In>(grad, mode, a);
}
