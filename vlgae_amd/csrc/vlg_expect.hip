// vlg_expect.hip -- expectations under DependencyCRF on the device (vlg_deptree_expect, include/vlgae_amd.h): the gfx950 kernel
// around vlg_dp_expect.h.  Replaces the reference's StructDistribution.entropy / cross_entropy / kl / risk
// (src/model/torch_struct/distributions.py:79-114: a Python loop over span widths under an expectation semiring, differentiated by
// autograd) for DependencyCRF.
//
// One workgroup per sentence runs the DepTree inside pass -- and, when mu or hv is wanted, the outside pass -- in dual numbers:
// every chart cell carries its derivative along the direction v - v_sub.  One launch returns logZ, ev = <mu, v>, the arc marginals
// mu and hv = (Hessian of logZ) v; entropy, cross-entropy, KL and expected scores and all their gradients are arithmetic on these.
// No atomics, one writer per output element, one barrier per span width.  Charts live in LDS where they fit and in the caller's
// workspace otherwise (ExpectLayout, vlg_dp_core.h).
#include "vlg_dp_kernels.h"
#include "vlg_dp_expect.h"

namespace vlg {

template <bool GRAD, int MODE>
__device__ __forceinline__ ExpectCtx carve_expect(int N, int len, char* smem, char* wsb) {
    const ExpectLayout L(N, GRAD, false, MODE);
    ExpectCtx c;
    c.Ne = len + 1;
    c.len = len;
    c.P = chart_pitch(N);
    c.C = region_ptr<float>(L.C, smem, wsb);
    c.I = region_ptr<float>(L.I, smem, wsb);
    c.S = region_ptr<float>(L.S, smem, wsb);
    c.Cd = region_ptr<float>(L.Cd, smem, wsb);
    c.Id = region_ptr<float>(L.Id, smem, wsb);
    c.Sd = region_ptr<float>(L.Sd, smem, wsb);
    c.gCc = region_ptr<float>(L.gCc, smem, wsb);
    c.gCi = region_ptr<float>(L.gCi, smem, wsb);
    c.gI = region_ptr<float>(L.gI, smem, wsb);
    c.gCcd = region_ptr<float>(L.gCcd, smem, wsb);
    c.gCid = region_ptr<float>(L.gCid, smem, wsb);
    c.gId = region_ptr<float>(L.gId, smem, wsb);
    return c;
}

template <bool GRAD, int MODE, typename In, typename VIn>
__global__ __launch_bounds__(kThreads) void deptree_expect_kernel(const typename In::T* __restrict__ arc, const typename VIn::T* __restrict__ v,
                                                                  const typename VIn::T* __restrict__ v_sub, const int64_t* __restrict__ lengths,
                                                                  int N, float* __restrict__ logZ, float* __restrict__ ev, float* __restrict__ mu,
                                                                  float* __restrict__ hv, char* __restrict__ ws, size_t ws_stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int len = lengths ? (int)lengths[b] : N - 1;
    const size_t off = (size_t)b * N * N;
    if (len < 1 || len > N - 1) {   // not a sentence (block-uniform): the convention of vlg_deptree_decode
        if (tid == 0) {
            logZ[b] = __uint_as_float(0x7fc00000u);
            if (ev) ev[b] = __uint_as_float(0x7fc00000u);
        }
        if (GRAD) {
            if (mu) for (int i = tid; i < N * N; i += kThreads) mu[off + i] = 0.f;
            if (hv) for (int i = tid; i < N * N; i += kThreads) hv[off + i] = 0.f;
        }
        return;
    }
    const ExpectCtx c = carve_expect<GRAD, MODE>(N, len, smem, ws + (size_t)b * ws_stride);
    DevX x;
    expect_run<GRAD, In, VIn>(c, arc + off, v ? v + off : nullptr, v_sub ? v_sub + off : nullptr, N, logZ + b, ev ? ev + b : nullptr,
                              (GRAD && mu) ? mu + off : nullptr, (GRAD && hv) ? hv + off : nullptr, tid, kThreads, x);
}

struct ExpectArgs {
    const void *arc, *v, *v_sub;
    const int64_t* lengths;
    int B, N;
    float *logZ, *ev, *mu, *hv;
    void* ws;
    size_t ws_stride, lds;
    hipStream_t s;
};

template <bool GRAD, int MODE, typename In, typename VIn>
static int launch_expect(const ExpectArgs& a) {
    return launch("deptree_expect_kernel", deptree_expect_kernel<GRAD, MODE, In, VIn>, dim3(a.B), dim3(kThreads), a.lds, a.s,
                  (const typename In::T*)a.arc, (const typename VIn::T*)a.v, (const typename VIn::T*)a.v_sub, a.lengths, a.N, a.logZ, a.ev, a.mu,
                  a.hv, (char*)a.ws, a.ws_stride);
}

template <bool GRAD, typename In, typename VIn>
static int launch_expect_mode(int mode, const ExpectArgs& a) {
    switch (mode) {
        case 0: return launch_expect<GRAD, 0, In, VIn>(a);
        case 1: return launch_expect<GRAD, 1, In, VIn>(a);
        case 2: return launch_expect<GRAD, 2, In, VIn>(a);
        default:   // (forward only: placements 2 and 3 are the same, everything in the workspace)
            if constexpr (GRAD) return launch_expect<GRAD, 3, In, VIn>(a);
            else return launch_expect<GRAD, 2, In, VIn>(a);
    }
}

template <typename In, typename VIn>
static int launch_expect_grad(bool grad, int mode, const ExpectArgs& a) {
    return grad ? launch_expect_mode<true, In, VIn>(mode, a) : launch_expect_mode<false, In, VIn>(mode, a);
}

}  // namespace vlg

extern "C" int vlg_deptree_expect(const void* arc, const void* v, const void* v_sub, const int64_t* lengths, int B, int N, int in_dtype,
                                  int v_dtype, float* logZ, float* ev, float* mu, float* hv, void* ws, size_t ws_bytes, void* stream) {
    using namespace vlg;
    if (int e = check_dp_args("deptree_expect", B, N, in_dtype, VLG_SR_LOG)) return e;
    if (v_dtype != VLG_F32 && v_dtype != VLG_BF16) return set_error(VLG_ERR_DTYPE, "deptree_expect: v_dtype %d", v_dtype);
    if (B == 0) return 0;
    if (!arc || !logZ) return set_error(VLG_ERR_ARG, "deptree_expect: null buffer (arc and logZ are required)");
    const bool grad = mu || hv;
    const DpPlan p = dp_plan<ExpectLayout>(N, grad, false);
    if (int e = check_dp_workspace("deptree_expect", N, p, B, ws, ws_bytes)) return e;
    const ExpectArgs a{arc, v, v_sub, lengths, B, N, logZ, ev, mu, hv, ws, p.ws_stride, p.lds_bytes, (hipStream_t)stream};
    const int mode = placement_of(p.image);
    if (in_dtype == VLG_F32)
        return v_dtype == VLG_F32 ? launch_expect_grad<F32In, F32In>(grad, mode, a) : launch_expect_grad<F32In, BF16In>(grad, mode, a);
    return v_dtype == VLG_F32 ? launch_expect_grad<BF16In, F32In>(grad, mode, a) : launch_expect_grad<BF16In, BF16In>(grad, mode, a);
}
