// vlg_kbest.hip -- the K best dependency trees on the device (vlg_deptree_kbest, include/vlgae_amd.h): the gfx950 kernel around
// vlg_dp_kbest.h.  Replaces the reference's `StructDistribution.kmax` / `topk` (src/model/torch_struct/distributions.py:135-156: a
// Python loop over span widths under KMaxSemiring, a torch.topk per step, plus an autograd pass) for DependencyCRF.
//
// One workgroup per sentence.  It fills the K-best charts (kbest_fill: one barrier per span width; the lanes of a span's group merge
// their splits' candidates in registers, then K group arg-max rounds extract the cell).  Behind the last barrier the charts are
// read-only and the eight wavefronts part ways: wave v walks ranks v and v + 8 top-down over the packed back-pointers.  No atomics,
// one writer per output element.  Placement (kbest_plan_of): everything in LDS, else the back-pointer charts in the workspace, else
// the value charts too.  The frame shared with vlg_dmv_kbest.hip is vlg_kbest_kernels.h.
#include "vlg_kbest_kernels.h"

namespace vlg {

template <int KC, int MODE>
__global__ __launch_bounds__(kThreads) void deptree_kbest_kernel(const void* __restrict__ arc, int bf16, const int64_t* __restrict__ lengths, int N,
                                                                 int K, long long* __restrict__ heads, float* __restrict__ scores,
                                                                 int* __restrict__ count, char* ws, size_t ws_stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x, B = gridDim.x, tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int len = lengths ? (int)lengths[b] : N - 1;
    if (len < 1 || len > N - 1) return kbest_no_sentence(N, K, heads, scores, count);   // the convention of vlg_deptree_decode
    char* wsb = ws + (size_t)b * ws_stride;
    const KbestLayout L(N, KC, MODE);
    KbCtx c;
    c.Ne = len + 1;
    c.len = len;
    c.P = chart_pitch(N);
    c.cells = N * c.P;
    c.C = region_ptr<float>(L.C, smem, wsb);
    c.I = region_ptr<float>(L.I, smem, wsb);
    c.bT = region_ptr<unsigned short>(L.bT, smem, wsb);
    c.bC = region_ptr<unsigned short>(L.bC, smem, wsb);
    KbestX x;
    kbest_fill<KC>(c, KbArc{arc, (size_t)b * N * N, bf16}, N, tid, kThreads, x);
    // (the width loop ends with its barrier: the charts are complete and nothing writes them from here on)
    if (tid == 0 && count) count[b] = kbest_count(c, K);
    int* stack = region_ptr<int>(L.stack, smem, wsb) + wave * kKbestStack;
    for (int k = wave; k < K; k += kKbestWaves)
        kbest_walk<KC>(c, k, N, stack, heads + ((size_t)k * B + b) * N, scores + (size_t)k * B + b, x);
}

}  // namespace vlg

extern "C" {

size_t vlg_deptree_kbest_workspace(int B, int N, int K) { return vlg::kbest_workspace<vlg::KbestLayout>(B, N, K); }

int vlg_deptree_kbest(const void* arc, const int64_t* lengths, int B, int N, int in_dtype, int K, int64_t* heads, float* scores,
                      int32_t* count, void* ws, size_t ws_bytes, void* stream) {
    using namespace vlg;
    KbestArgs a{lengths, B, N, 0, K, heads, scores, count, ws, (hipStream_t)stream};
    const int e = kbest_check<KbestLayout>("deptree_kbest", in_dtype, "arc, heads and scores", arc && heads && scores, ws_bytes, a);
    if (e || !a.p.KC) return e;
    return kbest_dispatch(a.p, [&](auto kc, auto mode) {
        return launch_kbest("deptree_kbest_kernel", deptree_kbest_kernel<decltype(kc)::value, decltype(mode)::value>, a, arc);
    });
}

}  // extern "C"
