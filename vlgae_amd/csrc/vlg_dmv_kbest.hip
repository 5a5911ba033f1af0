// vlg_dmv_kbest.hip -- the K best dependency trees of the valence DMV on the device (vlg_dmv1o_kbest) and the adjoint of their scores
// (vlg_dmv1o_tree_counts), include/vlgae_amd.h: the gfx950 kernels around vlg_dmv_kbest.h.  The reference has no counterpart: on a
// DMV1o its `kmax` / `topk` stop in KMaxSemiring.sum (semirings.py:251).
//
// vlg_dmv1o_kbest: one workgroup per sentence, one launch.  It fills the K-best charts (dmv_kbest_fill: one barrier per span width;
// the lanes of a span's group merge their splits' candidates in registers, then K group arg-max rounds extract the cell -- three
// merges per span and direction).  Behind the last barrier the charts are read-only and the eight wavefronts part ways: wave v walks
// ranks v and v + 8 top-down over the packed back-pointers.  No atomics, one writer per output element.  Placement (dmv_kbest_plan):
// everything in LDS, else the back-pointer charts in the workspace, else the value charts too.
//
// vlg_dmv1o_tree_counts: one workgroup per sentence; lane c owns column c of cnt_attach, lane h row h of cnt_dec, and the trees are
// taken in order -- no atomics, bit-reproducible.
#include "vlg_dp_kernels.h"
#include "vlg_dmv_kbest.h"

namespace vlg {

static_assert(kKbestWaves == kThreads / 64, "the walk's stacks are carved for the workgroup's wavefronts");

// the walk's wave operations (its control flow is wave-uniform)
struct DmvKbestX : DevX {
    static constexpr int kWave = 64;
    __device__ __forceinline__ int lane() const { return (int)(threadIdx.x & 63); }
};

template <int KC, int MODE>
__global__ __launch_bounds__(kThreads) void dmv1o_kbest_kernel(const void* __restrict__ dec, const void* __restrict__ attach, int bf16,
                                                               const int64_t* __restrict__ lengths, int N, int K, long long* __restrict__ heads,
                                                               float* __restrict__ scores, int* __restrict__ count, char* ws, size_t ws_stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x, B = gridDim.x, tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int len = (int)lengths[b];
    if (len < 1 || len > N - 1) {   // not a sentence (block-uniform): the convention of vlg_dmv1o_decode
        for (int k = 0; k < K; ++k) {
            for (int i = tid; i < N; i += kThreads) heads[((size_t)k * B + b) * N + i] = 0;
            if (tid == 0) scores[(size_t)k * B + b] = __uint_as_float(0x7fc00000u);
        }
        if (tid == 0 && count) count[b] = 0;
        return;
    }
    char* wsb = ws + (size_t)b * ws_stride;
    const DmvKbestLayout L(N, KC, MODE);
    DmvKbCtx c;
    c.Ne = len + 1;
    c.len = len;
    c.P = chart_pitch(N);
    c.cells = N * c.P;
    c.C = region_ptr<float>(L.C, smem, wsb);
    c.T = region_ptr<float>(L.T, smem, wsb);
    c.A = region_ptr<float>(L.A, smem, wsb);
    c.bT = region_ptr<unsigned short>(L.bT, smem, wsb);
    c.bC = region_ptr<unsigned short>(L.bC, smem, wsb);
    DmvKbestX x;
    dmv_kbest_fill<KC>(c, DmvKbPot{dec, attach, (size_t)b * N * 8, (size_t)b * N * N * 2, bf16}, N, tid, kThreads, x);
    // (the width loop ends with its barrier: the charts are complete and nothing writes them from here on)
    if (tid == 0 && count) count[b] = dmv_kbest_count(c, K);
    int* stack = region_ptr<int>(L.stack, smem, wsb) + wave * kKbestStack;
    for (int k = wave; k < K; k += kKbestWaves)
        dmv_kbest_walk<KC>(c, k, N, stack, heads + ((size_t)k * B + b) * N, scores + (size_t)k * B + b, x);
}

struct DmvKbestArgs {
    const void *dec, *attach;
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
static int launch_dmv_kbest(const DmvKbestArgs& a) {
    return launch("dmv1o_kbest_kernel", dmv1o_kbest_kernel<KC, MODE>, dim3(a.B), dim3(kThreads), a.p.lds_bytes, a.s, a.dec, a.attach, a.bf16,
                  a.lengths, a.N, a.K, (long long*)a.heads, a.scores, (int*)a.count, (char*)a.ws, a.p.ws_stride);
}

template <int KC>
static int launch_dmv_kbest_mode(const DmvKbestArgs& a) {
    if (a.p.mode == 0) return launch_dmv_kbest<KC, 0>(a);
    return a.p.mode == 1 ? launch_dmv_kbest<KC, 1>(a) : launch_dmv_kbest<KC, 2>(a);
}

static bool dmv_kbest_in_range(int N, int K) { return N >= 2 && N <= 255 && K >= 1 && K <= kKbestMaxK; }

// ---- tree counts ------------------------------------------------------------------------------------------------------------------
constexpr int kCountThreads = 256;   // one lane per position: N <= 255

__global__ __launch_bounds__(kCountThreads) void dmv1o_tree_counts_kernel(const long long* __restrict__ heads, const int64_t* __restrict__ lengths,
                                                                          const int* __restrict__ count, const float* __restrict__ weight, int T,
                                                                          int N, float* __restrict__ cnt_dec, float* __restrict__ cnt_attach) {
    __shared__ int hs[256];
    const int b = blockIdx.x, B = gridDim.x, tid = threadIdx.x;
    float* ca = cnt_attach + (size_t)b * N * N * 2;
    for (int i = tid; i < N * N * 2; i += kCountThreads) ca[i] = 0.f;
    float acc[8];
#pragma unroll
    for (int z = 0; z < 8; ++z) acc[z] = 0.f;
    const int len = (int)lengths[b];
    if (len >= 1 && len <= N - 1) {   // (block-uniform)
        const int live = count ? min(count[b], T) : T;
        for (int t = 0; t < live; ++t) {
            __syncthreads();   // the zero fill / the lanes still reading the tree before
            if (tid < N) {
                const long long h = tid >= 1 && tid <= len ? heads[((size_t)t * B + b) * N + tid] : -1;
                hs[tid] = h >= 0 && h <= len && h != tid ? (int)h : -1;
            }
            __syncthreads();
            if (tid < N) dmv_tree_counts_lane(hs, len, N, tid, weight ? weight[(size_t)t * B + b] : 1.f, ca, acc);
        }
    }
    if (tid < N) {
#pragma unroll
        for (int z = 0; z < 8; ++z) cnt_dec[((size_t)b * N + tid) * 8 + z] = acc[z];
    }
}

}  // namespace vlg

extern "C" {

size_t vlg_dmv1o_kbest_workspace(int B, int N, int K) {
    if (B < 1 || !vlg::dmv_kbest_in_range(N, K)) return 0;
    return vlg::dmv_kbest_plan(N, K, vlg::kLdsBudget).ws_stride * (size_t)B;
}

int vlg_dmv1o_kbest(const void* dec, const void* attach, const int64_t* lengths, int B, int N, int in_dtype, int K, int64_t* heads,
                    float* scores, int32_t* count, void* ws, size_t ws_bytes, void* stream) {
    using namespace vlg;
    if (int e = check_dp_args("dmv1o_kbest", B, N, VLG_F32, VLG_SR_MAX)) return e;   // the shape; the dtype's turn is behind K
    if (K < 1 || K > kKbestMaxK) return set_error(VLG_ERR_SHAPE, "dmv1o_kbest: need 1 <= K <= %d (got %d)", kKbestMaxK, K);
    if (in_dtype != VLG_F32 && in_dtype != VLG_BF16) return set_error(VLG_ERR_DTYPE, "dmv1o_kbest: in_dtype %d", in_dtype);
    if (B == 0) return 0;
    if (!dec || !attach || !lengths || !heads || !scores)
        return set_error(VLG_ERR_NULL, "dmv1o_kbest: null buffer (dec, attach, lengths, heads and scores are required)");
    const KbestPlan p = dmv_kbest_plan(N, K, kLdsBudget);
    const size_t need = p.ws_stride * (size_t)B;
    if (need > ws_bytes || (need && !ws))
        return set_error(VLG_ERR_WORKSPACE, "dmv1o_kbest: N=%d K=%d needs a %zu-byte workspace (got %zu); see vlg_dmv1o_kbest_workspace", N, K, need,
                         ws_bytes);
    const DmvKbestArgs a{dec, attach, lengths, B, N, in_dtype == VLG_BF16 ? 1 : 0, K, heads, scores, count, ws, p, (hipStream_t)stream};
    switch (p.KC) {
        case 1: return launch_dmv_kbest_mode<1>(a);
        case 2: return launch_dmv_kbest_mode<2>(a);
        case 4: return launch_dmv_kbest_mode<4>(a);
        case 8: return launch_dmv_kbest_mode<8>(a);
        default: return launch_dmv_kbest_mode<16>(a);
    }
}

int vlg_dmv1o_tree_counts(const int64_t* heads, const int64_t* lengths, const int32_t* count, const float* weight, int T, int B, int N,
                          float* cnt_dec, float* cnt_attach, void* stream) {
    using namespace vlg;
    if (int e = check_dp_args("dmv1o_tree_counts", B, N, VLG_F32, VLG_SR_MAX)) return e;
    if (T < 0) return set_error(VLG_ERR_SHAPE, "dmv1o_tree_counts: need T >= 0 (got %d)", T);
    if (B == 0) return 0;
    if (!lengths || !cnt_dec || !cnt_attach || (T > 0 && !heads))
        return set_error(VLG_ERR_NULL, "dmv1o_tree_counts: null buffer (heads, lengths, cnt_dec and cnt_attach are required)");
    return launch("dmv1o_tree_counts_kernel", dmv1o_tree_counts_kernel, dim3(B), dim3(kCountThreads), 0, (hipStream_t)stream, (const long long*)heads,
                  lengths, (const int*)count, weight, T, N, cnt_dec, cnt_attach);
}

}  // extern "C"
