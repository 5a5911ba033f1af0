// vlg_dmv_kbest.hip -- the K best dependency trees of the valence DMV on the device (vlg_dmv1o_kbest) and the adjoint of their scores
// (vlg_dmv1o_tree_counts), include/vlgae_amd.h: the gfx950 kernels around vlg_dmv_kbest.h.  The reference has no counterpart: on a
// DMV1o its `kmax` / `topk` stop in KMaxSemiring.sum (semirings.py:251).
//
// vlg_dmv1o_kbest: one workgroup per sentence, one launch.  It fills the K-best charts (dmv_kbest_fill: one barrier per span width;
// the lanes of a span's group merge their splits' candidates in registers, then K group arg-max rounds extract the cell -- three
// merges per span and direction).  Behind the last barrier the charts are read-only and the eight wavefronts part ways: wave v walks
// ranks v and v + 8 top-down over the packed back-pointers.  No atomics, one writer per output element.  Placement (kbest_plan_of):
// everything in LDS, else the back-pointer charts in the workspace, else the value charts too.  The frame shared with vlg_kbest.hip is
// vlg_kbest_kernels.h.
//
// vlg_dmv1o_tree_counts: one workgroup per sentence; lane c owns column c of cnt_attach, lane h row h of cnt_dec, and the trees are
// taken in order -- no atomics, bit-reproducible.
#include "vlg_kbest_kernels.h"
#include "vlg_dmv_kbest.h"

namespace vlg {

template <int KC, int MODE>
__global__ __launch_bounds__(kThreads) void dmv1o_kbest_kernel(const void* __restrict__ dec, const void* __restrict__ attach, int bf16,
                                                               const int64_t* __restrict__ lengths, int N, int K, long long* __restrict__ heads,
                                                               float* __restrict__ scores, int* __restrict__ count, char* ws, size_t ws_stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x, B = gridDim.x, tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int len = (int)lengths[b];
    if (len < 1 || len > N - 1) return kbest_no_sentence(N, K, heads, scores, count);   // the convention of vlg_dmv1o_decode
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
    KbestX x;
    dmv_kbest_fill<KC>(c, DmvKbPot{dec, attach, (size_t)b * N * 8, (size_t)b * N * N * 2, bf16}, N, tid, kThreads, x);
    // (the width loop ends with its barrier: the charts are complete and nothing writes them from here on)
    if (tid == 0 && count) count[b] = dmv_kbest_count(c, K);
    int* stack = region_ptr<int>(L.stack, smem, wsb) + wave * kKbestStack;
    for (int k = wave; k < K; k += kKbestWaves)
        dmv_kbest_walk<KC>(c, k, N, stack, heads + ((size_t)k * B + b) * N, scores + (size_t)k * B + b, x);
}

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

size_t vlg_dmv1o_kbest_workspace(int B, int N, int K) { return vlg::kbest_workspace<vlg::DmvKbestLayout>(B, N, K); }

int vlg_dmv1o_kbest(const void* dec, const void* attach, const int64_t* lengths, int B, int N, int in_dtype, int K, int64_t* heads,
                    float* scores, int32_t* count, void* ws, size_t ws_bytes, void* stream) {
    using namespace vlg;
    KbestArgs a{lengths, B, N, 0, K, heads, scores, count, ws, (hipStream_t)stream};
    const int e = kbest_check<DmvKbestLayout>("dmv1o_kbest", in_dtype, "dec, attach, lengths, heads and scores",
                                              dec && attach && lengths && heads && scores, ws_bytes, a);
    if (e || !a.p.KC) return e;
    return kbest_dispatch(a.p, [&](auto kc, auto mode) {
        return launch_kbest("dmv1o_kbest_kernel", dmv1o_kbest_kernel<decltype(kc)::value, decltype(mode)::value>, a, dec, attach);
    });
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
