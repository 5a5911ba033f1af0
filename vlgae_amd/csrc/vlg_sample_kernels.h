// vlg_sample_kernels.h -- device side and launch frame of the tree samplers (vlg_sample.hip: DepTree, vlg_dmv_sample.hip: DMV1o),
// around the shared rule of vlg_sample_common.h: the wave policy of the walk, the counter-based uniforms, the grid's filling rule,
// the not-a-sentence convention, the entry points' checks and the kernel-image dispatch.  A sampler's kernel reads its length,
// carves, runs its inside pass, reads log Z and hands each of its wavefronts' samples to its walk.  (That last loop -- s = first +
// wave, + 8, ..., TableU or PhiloxU per sample -- stands in each kernel: handing the walk to a shared loop as a functor moved SGPR
// counts and spills of both kernels in every form tried, profiles/sampler_frame_neutrality.md.)
#pragma once
#include <type_traits>

#include "vlg_dp_kernels.h"
#include "vlg_rng.h"
#include "vlg_sample_common.h"

namespace vlg {

constexpr int kSampleWaves = kThreads / 64;
// Workgroups that fill the device once: kSampleCUs x the workgroups of this N that share a CU -- as many as its LDS holds, at most
// kSampleBlocksPerCU (a workgroup is eight of a CU's wavefront slots).  The walk is a chain of dependent LDS reads and cross-lane steps: further
// workgroups on the CU hide its latencies (DepTree, B = 256, N = 41, S = 64: 462 us with one per CU, 366 us with two).
constexpr int kSampleCUs = 256, kSampleBlocksPerCU = 4;

// the wave operations of the walk on a wavefront whose 64 lanes are all active (the walk's control flow is wave-uniform)
struct SampleX : DevX {
    static constexpr int kWave = 64;
    __device__ __forceinline__ int lane() const { return (int)(threadIdx.x & 63); }
    __device__ __forceinline__ float wave_max(float v) {
        allreduce_max<1>(&v, 64);
        return v;
    }
    // Inclusive prefix sum over the 64 lanes without LDS traffic: a shift-and-add scan inside each row of 16 lanes (DPP row_shr 1, 2, 4, 8; a lane
    // without a source adds 0), then the row totals carried on: row_bcast:15 hands lane 15 of rows 0 and 2 to rows 1 and 3, row_bcast:31 lane 31
    // to rows 2 and 3.  (The partial sums are rounded in another order than a sequential sum: see sample_draw's w > 0.)
    __device__ __forceinline__ float wave_scan(float v) {
#define VLG_SCAN_STEP(CTRL, ROWS) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROWS, 0xf, false))
        VLG_SCAN_STEP(0x111, 0xf);   // row_shr:1
        VLG_SCAN_STEP(0x112, 0xf);   // row_shr:2
        VLG_SCAN_STEP(0x114, 0xf);   // row_shr:4
        VLG_SCAN_STEP(0x118, 0xf);   // row_shr:8
        VLG_SCAN_STEP(0x142, 0xa);   // row_bcast:15 -> rows 1, 3
        VLG_SCAN_STEP(0x143, 0xc);   // row_bcast:31 -> rows 2, 3
#undef VLG_SCAN_STEP
        return v;
    }
    __device__ __forceinline__ float wave_last(float v) {   // the last lane's value: the total of an inclusive scan
        return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
    }
    __device__ __forceinline__ int ballot_first(bool p) {   // lowest lane where p holds, -1 if none
        const unsigned long long m = __ballot(p);
        return m ? (int)__ffsll((long long)m) - 1 : -1;
    }
    __device__ __forceinline__ int ballot_last(bool p) {    // highest such lane
        const unsigned long long m = __ballot(p);
        return m ? 63 - (int)__clzll((long long)m) : -1;
    }
};

// the uniforms of one (sample, sentence) from the counter-based generator (vlg_rng.h)
struct PhiloxU {
    uint2 key;
    uint32_t s, b, step;
    __device__ __forceinline__ float get(int kind, int lo, int hi) const {
        const uint4 r = philox4x32_10(make_uint4((uint32_t)(kind << 16 | hi << 8 | lo), s, b, step), key);
        return (float)(r.x >> 8) * (1.0f / 16777216.0f);   // 24 bits: exact in fp32, < 1
    }
};

// Block (b, y) of the (B, Y) grid is not a sentence (len outside 1 ... N - 1, block-uniform): the convention of the decode kernels.
// logZ[b] = NaN from block y = 0; the heads of the block's samples s0 ... s1 - 1 are 0, their logp NaN.
__device__ __forceinline__ void sample_no_sentence(int N, int s0, int s1, long long* __restrict__ heads, float* __restrict__ logp,
                                                   float* __restrict__ logZ) {
    const int b = blockIdx.x, B = gridDim.x, tid = threadIdx.x;
    const float nan = __uint_as_float(0x7fc00000u);
    if (blockIdx.y == 0 && tid == 0 && logZ) logZ[b] = nan;
    for (int s = s0; s < s1; ++s) {
        for (int i = tid; i < N; i += kThreads) heads[((size_t)s * B + b) * N + i] = 0;
        if (tid == 0 && logp) logp[(size_t)s * B + b] = nan;
    }
}

// Blocks per sentence: enough that B Y workgroups fill the device once, never more than the samples can feed (a wavefront owns whole
// samples: ceil(S / 8) blocks have one each).  Every further block repeats the inside pass, so Y = 1 as soon as B alone fills the device.
static int sample_blocks(const DpPlan& p, size_t stack_bytes, int B, int S) {
    size_t per_cu = kLdsBudget / (p.lds_bytes + stack_bytes);
    per_cu = per_cu < 1 ? 1 : per_cu > (size_t)kSampleBlocksPerCU ? (size_t)kSampleBlocksPerCU : per_cu;
    if (p.ws_stride) per_cu = 1;   // charts in the workspace: every block needs its own slice of it (0.5 MB at N = 255), and its inside pass is the slow one
    const int fill = kSampleCUs * (int)per_cu;
    const int want = B >= fill ? 1 : fill / B, cap = (S + kSampleWaves - 1) / kSampleWaves;
    return want < cap ? want : cap;
}

// what every sampler's launch takes behind its potentials; Y ... image are sample_check's
struct SampleArgs {
    const int64_t* lengths;
    int B, N, S;
    const uint64_t* rng;
    unsigned site;
    const float* u;
    int64_t* heads;
    float *logp, *logZ;
    void* ws;
    hipStream_t s;
    int Y, image;   // blocks per sentence (0: nothing to launch), the kernel's MODE
    size_t ws_stride, lds_charts;
};

// The checks of a sampler's entry point `op`, in the order its callers see them, and the plan of the launch: the inside pass's
// placement (dp_plan<Layout>, forward, Log) with the walk's stacks behind its LDS.  `buffers`: the entry's required pointers are set.
template <typename Layout>
static int sample_check(const char* op, size_t stack_bytes, int in_dtype, bool buffers, size_t ws_bytes, SampleArgs& a) {
    a.Y = 0;
    if (int e = check_dp_args(op, a.B, a.N, VLG_F32, VLG_SR_LOG)) return e;   // the shape; the dtype's turn is behind S
    if (a.S < 1) return set_error(VLG_ERR_SHAPE, "%s: need S >= 1 samples (got %d)", op, a.S);
    if (in_dtype != VLG_F32 && in_dtype != VLG_BF16) return set_error(VLG_ERR_DTYPE, "%s: in_dtype %d", op, in_dtype);
    if (a.B == 0) return 0;
    if ((a.rng != nullptr) == (a.u != nullptr))
        return set_error(VLG_ERR_NULL, "%s: pass exactly one of rng (counter-based draws) and u (explicit uniforms)", op);
    if (!buffers) return set_error(VLG_ERR_NULL, "%s: null buffer", op);
    const DpPlan p = dp_plan<Layout>(a.N, false, false);
    if (p.lds_bytes + stack_bytes > kLdsBudget)
        return set_error(VLG_ERR_SHAPE, "%s: N=%d leaves no LDS for the walk's stacks", op, a.N);   // (not reached for N <= 255)
    const int Y = sample_blocks(p, stack_bytes, a.B, a.S);
    if (int e = check_dp_workspace(op, a.N, p, (size_t)a.B * Y, a.ws, ws_bytes)) return e;   // one slice per block of the (B, Y) grid
    a.Y = Y;
    a.image = p.image;
    a.ws_stride = p.ws_stride;
    a.lds_charts = p.lds_bytes;
    return 0;
}

// the launch of kernel(pot..., lengths, N, S, per_block, rng, site, u, heads, logp, logZ, ws, ws_stride, lds_charts) on the (B, Y) grid
template <typename K, typename... Pot>
static int launch_sample(const char* name, K kernel, size_t stack_bytes, const SampleArgs& a, Pot... pot) {
    return launch(name, kernel, dim3(a.B, a.Y), dim3(kThreads), a.lds_charts + stack_bytes, a.s, pot..., a.lengths, a.N, a.S,
                  (a.S + a.Y - 1) / a.Y, a.rng, a.site, a.u, (long long*)a.heads, a.logp, a.logZ, (char*)a.ws, a.ws_stride, a.lds_charts);
}

// go(MODE, In) for the image of the plan and the input type: a forward-only layout has two placements, everything in LDS (0, or the
// short image) and the charts in the workspace (1 ... 3 are one)
template <int MODE>
using SampleMode = std::integral_constant<int, MODE>;

template <typename In, typename Go>
static int sample_image(int image, const Go& go) {
    if (image == kModeShort) return go(SampleMode<kModeShort>{}, In{});
    return image == 0 ? go(SampleMode<0>{}, In{}) : go(SampleMode<1>{}, In{});
}

template <typename Go>
static int sample_dispatch(int in_dtype, int image, const Go& go) {
    return in_dtype == VLG_F32 ? sample_image<F32In>(image, go) : sample_image<BF16In>(image, go);
}

}  // namespace vlg
