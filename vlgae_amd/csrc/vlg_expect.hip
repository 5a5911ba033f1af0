// vlg_expect.hip -- expectations under DependencyCRF on the device (vlg_deptree_expect, include/vlgae_amd.h): the gfx950 kernel
// around vlg_dp_expect.h.  Replaces the reference's StructDistribution.entropy / cross_entropy / kl / risk
// (src/model/torch_struct/distributions.py:79-114: a Python loop over span widths under an expectation semiring, differentiated by
// autograd) for DependencyCRF.
//
// One workgroup per sentence runs the DepTree inside pass -- and, when mu or hv is wanted, the outside pass -- in dual numbers:
// every chart cell carries its derivative along the direction v - v_sub.  One launch returns logZ, ev = <mu, v>, the arc marginals
// mu and hv = (Hessian of logZ) v; entropy, cross-entropy, KL and expected scores and all their gradients are arithmetic on these.
// No atomics, one writer per output element, one barrier per span width.  Charts live in LDS where they fit and in the caller's
// workspace otherwise (ExpectLayout, vlg_dp_expect.h).  The launch frame is vlg_expect_kernels.h.
#include "vlg_expect_kernels.h"

namespace vlg {

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
    char* wsb = ws + (size_t)b * ws_stride;
    const ExpectLayout L(N, GRAD, false, MODE);
    const ExpectCtx c = expect_carve(L, N, len, [&](const Region& r) { return region_ptr<char>(r, smem, wsb); });
    DevX x;
    expect_run<GRAD, In, VIn>(c, arc + off, v ? v + off : nullptr, v_sub ? v_sub + off : nullptr, N, logZ + b, ev ? ev + b : nullptr,
                              (GRAD && mu) ? mu + off : nullptr, (GRAD && hv) ? hv + off : nullptr, tid, kThreads, x);
}

}  // namespace vlg

extern "C" int vlg_deptree_expect(const void* arc, const void* v, const void* v_sub, const int64_t* lengths, int B, int N, int in_dtype,
                                  int v_dtype, float* logZ, float* ev, float* mu, float* hv, void* ws, size_t ws_bytes, void* stream) {
    using namespace vlg;
    return expect_entry<ExpectLayout>("deptree_expect", B, N, in_dtype, v_dtype, "arc and logZ", arc && logZ, mu || hv, ws, ws_bytes,
                                      [&](const DpPlan& p, auto G, auto M, auto I, auto V) {
        using In = decltype(I);
        using VIn = decltype(V);
        return launch("deptree_expect_kernel", deptree_expect_kernel<G.value, M.value, In, VIn>, dim3(B), dim3(kThreads), p.lds_bytes,
                      (hipStream_t)stream, (const typename In::T*)arc, (const typename VIn::T*)v, (const typename VIn::T*)v_sub, lengths, N, logZ, ev,
                      mu, hv, (char*)ws, p.ws_stride);
    });
}
