// vlg_kbest_kernels.h -- device side and launch frame of the K-best-trees kernels (vlg_kbest.hip: DepTree, vlg_dmv_kbest.hip: DMV1o),
// around the shared bodies of vlg_dp_kbest.h: the wave policy of the walk, the not-a-sentence convention, the entry points' checks,
// the size query and the kernel-image dispatch.  A kernel reads its length, carves, sets up its charts, fills them, counts and hands
// each of its wavefronts' ranks to its walk.  (That last loop -- k = wave, wave + 8 on the wave's stack -- stands in each kernel:
// as a shared function around either walk it moved the SGPR counts and spills of the DepTree images, as the samplers' loop did,
// profiles/kbest_frame_neutrality.md.)
#pragma once
#include <type_traits>

#include "vlg_dp_kernels.h"
#include "vlg_dp_kbest.h"

namespace vlg {

static_assert(kKbestWaves == kThreads / 64, "the walk's stacks are carved for the workgroup's wavefronts");

// the walk's wave operations (its control flow is wave-uniform)
struct KbestX : DevX {
    static constexpr int kWave = 64;
    __device__ __forceinline__ int lane() const { return (int)(threadIdx.x & 63); }
};

// Block b is not a sentence (len outside 1 ... N - 1, block-uniform): the convention of the decode kernels.  The heads of its K ranks
// are 0, their scores NaN, its count 0.
__device__ __forceinline__ void kbest_no_sentence(int N, int K, long long* __restrict__ heads, float* __restrict__ scores,
                                                  int* __restrict__ count) {
    const int b = blockIdx.x, B = gridDim.x, tid = threadIdx.x;
    for (int k = 0; k < K; ++k) {
        for (int i = tid; i < N; i += kThreads) heads[((size_t)k * B + b) * N + i] = 0;
        if (tid == 0) scores[(size_t)k * B + b] = __uint_as_float(0x7fc00000u);
    }
    if (tid == 0 && count) count[b] = 0;
}

// what both launches take behind their potentials; p is kbest_check's (KC = 0: nothing to launch)
struct KbestArgs {
    const int64_t* lengths;
    int B, N, bf16, K;
    int64_t* heads;
    float* scores;
    int32_t* count;
    void* ws;
    hipStream_t s;
    KbestPlan p;
};

static bool kbest_in_range(int N, int K) { return N >= 2 && N <= 255 && K >= 1 && K <= kKbestMaxK; }

// the workspace of a batch, 0 for arguments the entry point refuses
template <typename Layout>
static size_t kbest_workspace(int B, int N, int K) {
    if (B < 1 || !kbest_in_range(N, K)) return 0;
    return kbest_plan_of<Layout>(N, K, kLdsBudget).ws_stride * (size_t)B;
}

// The checks of the entry point vlg_<op>, in the order its callers see them, and the plan of the launch.  `required`: the names of
// the entry's required pointers; `buffers`: they are all set.
template <typename Layout>
static int kbest_check(const char* op, int in_dtype, const char* required, bool buffers, size_t ws_bytes, KbestArgs& a) {
    a.p = KbestPlan{0, 0, 0, 0};
    if (int e = check_dp_args(op, a.B, a.N, VLG_F32, VLG_SR_MAX)) return e;   // the shape; the dtype's turn is behind K
    if (a.K < 1 || a.K > kKbestMaxK) return set_error(VLG_ERR_SHAPE, "%s: need 1 <= K <= %d (got %d)", op, kKbestMaxK, a.K);
    if (in_dtype != VLG_F32 && in_dtype != VLG_BF16) return set_error(VLG_ERR_DTYPE, "%s: in_dtype %d", op, in_dtype);
    if (a.B == 0) return 0;
    if (!buffers) return set_error(VLG_ERR_NULL, "%s: null buffer (%s are required)", op, required);
    const KbestPlan p = kbest_plan_of<Layout>(a.N, a.K, kLdsBudget);
    const size_t need = p.ws_stride * (size_t)a.B;
    if (need > ws_bytes || (need && !a.ws))
        return set_error(VLG_ERR_WORKSPACE, "%s: N=%d K=%d needs a %zu-byte workspace (got %zu); see vlg_%s_workspace", op, a.N, a.K, need,
                         ws_bytes, op);
    a.bf16 = in_dtype == VLG_BF16 ? 1 : 0;
    a.p = p;
    return 0;
}

// the launch of kernel(pot..., bf16, lengths, N, K, heads, scores, count, ws, ws_stride), one workgroup per sentence
template <typename Kern, typename... Pot>
static int launch_kbest(const char* name, Kern kernel, const KbestArgs& a, Pot... pot) {
    return launch(name, kernel, dim3(a.B), dim3(kThreads), a.p.lds_bytes, a.s, pot..., a.bf16, a.lengths, a.N, a.K, (long long*)a.heads, a.scores,
                  (int*)a.count, (char*)a.ws, a.p.ws_stride);
}

// go(KC, MODE) for the code image and the placement of the plan
template <int V>
using KbestConst = std::integral_constant<int, V>;

template <int KC, typename Go>
static int kbest_mode(int mode, const Go& go) {
    if (mode == 0) return go(KbestConst<KC>{}, KbestConst<0>{});
    return mode == 1 ? go(KbestConst<KC>{}, KbestConst<1>{}) : go(KbestConst<KC>{}, KbestConst<2>{});
}

template <typename Go>
static int kbest_dispatch(const KbestPlan& p, const Go& go) {
    switch (p.KC) {
        case 1: return kbest_mode<1>(p.mode, go);
        case 2: return kbest_mode<2>(p.mode, go);
        case 4: return kbest_mode<4>(p.mode, go);
        case 8: return kbest_mode<8>(p.mode, go);
        default: return kbest_mode<16>(p.mode, go);
    }
}

}  // namespace vlg
