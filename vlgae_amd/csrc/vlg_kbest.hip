// vlg_kbest.hip -- the K best dependency trees on the device (vlg_deptree_kbest, include/vlgae_amd.h): the gfx950 kernel around
// vlg_dp_kbest.h.  Replaces the reference's `StructDistribution.kmax` / `topk` (src/model/torch_struct/distributions.py:135-156: a
// Python loop over span widths under KMaxSemiring, a torch.topk per step, plus an autograd pass) for DependencyCRF.
//
// One workgroup per sentence.  It fills the K-best charts (kbest_fill: one barrier per span width; the lanes of a span's group merge
// their splits' candidates in registers, then K group arg-max rounds extract the cell).  Behind the last barrier the charts are
// read-only and the eight wavefronts part ways: wave v walks ranks v and v + 8 top-down over the packed back-pointers.  No atomics,
// one writer per output element.  Placement (kbest_plan): everything in LDS, else the back-pointer charts in the workspace, else the
// value charts too.
#include "vlg_dp_kernels.h"
#include "vlg_dp_kbest.h"

namespace vlg {

static_assert(kKbestWaves == kThreads / 64, "the walk's stacks are carved for the workgroup's wavefronts");

// the walk's wave operations (its control flow is wave-uniform)
struct KbestX : DevX {
    static constexpr int kWave = 64;
    __device__ __forceinline__ int lane() const { return (int)(threadIdx.x & 63); }
};

template <int KC, int MODE>
__global__ __launch_bounds__(kThreads) void deptree_kbest_kernel(const void* __restrict__ arc, int bf16, const int64_t* __restrict__ lengths, int N,
                                                                 int K, long long* __restrict__ heads, float* __restrict__ scores,
                                                                 int* __restrict__ count, char* ws, size_t ws_stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x, B = gridDim.x, tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int len = lengths ? (int)lengths[b] : N - 1;
    if (len < 1 || len > N - 1) {   // not a sentence (block-uniform): the convention of vlg_deptree_decode
        for (int k = 0; k < K; ++k) {
            for (int i = tid; i < N; i += kThreads) heads[((size_t)k * B + b) * N + i] = 0;
            if (tid == 0) scores[(size_t)k * B + b] = __uint_as_float(0x7fc00000u);
        }
        if (tid == 0 && count) count[b] = 0;
        return;
    }
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

struct KbestArgs {
    const void* arc;
    const int64_t* lengths;
    int B, N, bf16, K;
    int64_t* heads;
    float* scores;
    int32_t* count;
    void* ws;
    KbestPlan p;
    hipStream_t s;
};

template <int KC, int MODE>
static int launch_kbest(const KbestArgs& a) {
    return launch("deptree_kbest_kernel", deptree_kbest_kernel<KC, MODE>, dim3(a.B), dim3(kThreads), a.p.lds_bytes, a.s, a.arc, a.bf16, a.lengths, a.N,
                  a.K, (long long*)a.heads, a.scores, (int*)a.count, (char*)a.ws, a.p.ws_stride);
}

template <int KC>
static int launch_kbest_mode(const KbestArgs& a) {
    if (a.p.mode == 0) return launch_kbest<KC, 0>(a);
    return a.p.mode == 1 ? launch_kbest<KC, 1>(a) : launch_kbest<KC, 2>(a);
}

static bool kbest_in_range(int N, int K) { return N >= 2 && N <= 255 && K >= 1 && K <= kKbestMaxK; }

}  // namespace vlg

extern "C" {

size_t vlg_deptree_kbest_workspace(int B, int N, int K) {
    if (B < 1 || !vlg::kbest_in_range(N, K)) return 0;
    return vlg::kbest_plan(N, K, vlg::kLdsBudget).ws_stride * (size_t)B;
}

int vlg_deptree_kbest(const void* arc, const int64_t* lengths, int B, int N, int in_dtype, int K, int64_t* heads, float* scores,
                      int32_t* count, void* ws, size_t ws_bytes, void* stream) {
    using namespace vlg;
    if (int e = check_dp_args("deptree_kbest", B, N, VLG_F32, VLG_SR_MAX)) return e;   // the shape; the dtype's turn is behind K
    if (K < 1 || K > kKbestMaxK) return set_error(VLG_ERR_SHAPE, "deptree_kbest: need 1 <= K <= %d (got %d)", kKbestMaxK, K);
    if (in_dtype != VLG_F32 && in_dtype != VLG_BF16) return set_error(VLG_ERR_DTYPE, "deptree_kbest: in_dtype %d", in_dtype);
    if (B == 0) return 0;
    if (!arc || !heads || !scores) return set_error(VLG_ERR_NULL, "deptree_kbest: null buffer (arc, heads and scores are required)");
    const KbestPlan p = kbest_plan(N, K, kLdsBudget);
    const size_t need = p.ws_stride * (size_t)B;
    if (need > ws_bytes || (need && !ws))
        return set_error(VLG_ERR_WORKSPACE, "deptree_kbest: N=%d K=%d needs a %zu-byte workspace (got %zu); see vlg_deptree_kbest_workspace", N, K,
                         need, ws_bytes);
    const KbestArgs a{arc, lengths, B, N, in_dtype == VLG_BF16 ? 1 : 0, K, heads, scores, count, ws, p, (hipStream_t)stream};
    switch (p.KC) {
        case 1: return launch_kbest_mode<1>(a);
        case 2: return launch_kbest_mode<2>(a);
        case 4: return launch_kbest_mode<4>(a);
        case 8: return launch_kbest_mode<8>(a);
        default: return launch_kbest_mode<16>(a);
    }
}

}  // extern "C"
