// vlg_dmv_sample.hip -- sampling DMV1o dependency trees on the device (vlg_dmv1o_sample, include/vlgae_amd.h): the gfx950 kernel around
// vlg_dmv_sample.h.  Replaces the reference's `StructDistribution.sample` (src/model/torch_struct/distributions.py:195-217: a Python loop
// over span widths under MultiSampledSemiring plus an autograd pass per ten samples) for DMV1o.
//
// One workgroup per (sentence, share of the samples): it stages the potentials and runs the Log-semiring inside pass exactly as
// vlg_dmv1o_inside does (dmv_run<Log, false> through MergedIO, same chart placement: the short image for N <= kShortN, LDS where the
// charts fit, the VLG_OP_DMV1O_INSIDE workspace otherwise).  Behind the last barrier the charts are read-only and the eight wavefronts
// part ways: each owns whole samples (s = first + wave, + 8, ...), lanes spread over the split points of the cell being drawn.  No
// barrier, no atomics, one writer per output element.  The per-wave stacks sit in dynamic LDS behind DmvLayout's lds_bytes.
//
// Built WITHOUT -ffinite-math-only (vlgae_amd/build.py): the draw compares against a uniform that may be NaN.
#include "vlg_dp_kernels.h"
#include "vlg_dmv_sample.h"
#include "vlg_rng.h"

namespace vlg {

constexpr int kDmvSampleWaves = kThreads / 64;
constexpr size_t kDmvSampleStackBytes = (size_t)kDmvSampleWaves * kDmvSampleStack * sizeof(int);
// the grid's filling rule is vlg_deptree_sample_blocks': kCUs x the workgroups of this N that share a CU (as many as its LDS holds, four
// at most; one where the charts live in the workspace), never more blocks than the samples can feed
constexpr int kDmvSampleCUs = 256, kDmvSampleBlocksPerCU = 4;

// the wave operations of the walk on a wavefront whose 64 lanes are all active (the walk's control flow is wave-uniform): the wave
// max, the DPP scan and the ballots of the DepTree sampler (vlg_sample.hip: SampleX), which that file keeps to itself
struct DmvSampleX : DevX {
    static constexpr int kWave = 64;
    __device__ __forceinline__ int lane() const { return (int)(threadIdx.x & 63); }
    __device__ __forceinline__ float wave_max(float v) {
        allreduce_max<1>(&v, 64);
        return v;
    }
    // inclusive prefix sum over the 64 lanes: shift-and-add inside each row of 16 lanes (DPP row_shr 1, 2, 4, 8; a lane without a
    // source adds 0), then row_bcast:15 hands lane 15 of rows 0 and 2 to rows 1 and 3, row_bcast:31 lane 31 to rows 2 and 3
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

// the uniforms of one (sample, sentence) from the counter-based generator (vlg_rng.h): the DepTree sampler's counter layout
struct DmvPhiloxU {
    uint2 key;
    uint32_t s, b, step;
    __device__ __forceinline__ float get(int kind, int lo, int hi) const {
        const uint4 r = philox4x32_10(make_uint4((uint32_t)(kind << 16 | hi << 8 | lo), s, b, step), key);
        return (float)(r.x >> 8) * (1.0f / 16777216.0f);   // 24 bits: exact in fp32, < 1
    }
};

template <int MODE, typename In>
__global__ __launch_bounds__(kThreads) void dmv1o_sample_kernel(const typename In::T* __restrict__ dec, const typename In::T* __restrict__ attach,
                                                                const int64_t* __restrict__ lengths, int N, int S, int per_block,
                                                                const uint64_t* __restrict__ rng, unsigned site, const float* __restrict__ u,
                                                                long long* __restrict__ heads, float* __restrict__ logp,
                                                                float* __restrict__ logZ, char* __restrict__ ws, size_t ws_stride,
                                                                size_t lds_charts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x, B = gridDim.x, tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: keys, counters and the stack address stay scalar
    const int s0 = blockIdx.y * per_block, s1 = s0 + per_block < S ? s0 + per_block : S;   // this block's samples
    const int len = (int)lengths[b];
    const float nan = __uint_as_float(0x7fc00000u);
    if (len < 1 || len > N - 1) {   // not a sentence (block-uniform): the convention of vlg_dmv1o_decode
        if (blockIdx.y == 0 && tid == 0 && logZ) logZ[b] = nan;
        for (int s = s0; s < s1; ++s) {
            for (int i = tid; i < N; i += kThreads) heads[((size_t)s * B + b) * N + i] = 0;
            if (tid == 0 && logp) logp[(size_t)s * B + b] = nan;
        }
        return;
    }
    char* wsb = ws + ((size_t)blockIdx.y * B + b) * ws_stride;
    const DmvCtx c = carve_dmv<VLG_SR_LOG, MODE, false>(N, len, smem, wsb, false);
    MergedIO<In> io;
    io.dec = dec + (size_t)b * N * 8;
    io.attach = attach + (size_t)b * N * N * 2;
    io.N = N;
    io.gdec = nullptr;
    io.gatt = nullptr;
    io.heads = nullptr;
    DmvSampleX x;
    float lz_unused;   // dmv_run hands logZ to one thread; every wave reads it from the chart instead
    dmv_run<VLG_SR_LOG, false, spans_of(MODE)>(c, io, 1.f, &lz_unused, tid, kThreads, x);
    x.sync();   // the charts are complete and nothing writes them from here on
    const float lz2 = c.C[len + 1].y;   // CR(0,len).NOCHILD, log2 units (dmv.py:65)
    if (blockIdx.y == 0 && tid == 0 && logZ) logZ[b] = lz2 * VLG_LN2;
    int* stack = reinterpret_cast<int*>(smem + lds_charts) + wave * kDmvSampleStack;
    for (int s = s0 + wave; s < s1; s += kDmvSampleWaves) {
        long long* h = heads + ((size_t)s * B + b) * N;
        float* lp = logp ? logp + (size_t)s * B + b : nullptr;
        if (u) {
            const DmvTableU us{u + ((size_t)s * B + b) * 3 * N * N, N};
            dmv_sample_walk<In>(c, io.dec, io.attach, N, stack, us, h, lp, lz2, x);
        } else {
            const DmvPhiloxU us{site_key(rng[0], site), (uint32_t)s, (uint32_t)b, (uint32_t)rng[1]};
            dmv_sample_walk<In>(c, io.dec, io.attach, N, stack, us, h, lp, lz2, x);
        }
    }
}

struct DmvSampleArgs {
    const void *dec, *attach;
    const int64_t* lengths;
    int B, N, S, Y;
    const uint64_t* rng;
    unsigned site;
    const float* u;
    int64_t* heads;
    float *logp, *logZ;
    void* ws;
    size_t ws_stride, lds_charts;
    hipStream_t s;
};

template <int MODE, typename In>
static int launch_dmv_sample(const DmvSampleArgs& a) {
    const size_t lds = a.lds_charts + kDmvSampleStackBytes;
    return launch("dmv1o_sample_kernel", dmv1o_sample_kernel<MODE, In>, dim3(a.B, a.Y), dim3(kThreads), lds, a.s, (const typename In::T*)a.dec,
                  (const typename In::T*)a.attach, a.lengths, a.N, a.S, (a.S + a.Y - 1) / a.Y, a.rng, a.site, a.u, (long long*)a.heads, a.logp,
                  a.logZ, (char*)a.ws, a.ws_stride, a.lds_charts);
}

// the forward-only DmvLayout has two placements: everything in LDS (0, or the short image) and both charts in the workspace (1 ... 3 are one)
template <typename In>
static int launch_dmv_sample_mode(int mode, const DmvSampleArgs& a) {
    if (mode == kModeShort) return launch_dmv_sample<kModeShort, In>(a);
    return mode == 0 ? launch_dmv_sample<0, In>(a) : launch_dmv_sample<1, In>(a);
}

static DpPlan dmv_sample_plan(int N) { return dp_plan<DmvLayout>(N, false, false); }   // the plan of vlg_dmv1o_inside

static int dmv_sample_blocks(const DpPlan& p, int B, int S) {
    size_t per_cu = kLdsBudget / (p.lds_bytes + kDmvSampleStackBytes);
    per_cu = per_cu < 1 ? 1 : per_cu > (size_t)kDmvSampleBlocksPerCU ? (size_t)kDmvSampleBlocksPerCU : per_cu;
    if (p.ws_stride) per_cu = 1;   // charts in the workspace: every block needs its own slice of it, and its inside pass is the slow one
    const int fill = kDmvSampleCUs * (int)per_cu;
    const int want = B >= fill ? 1 : fill / B, cap = (S + kDmvSampleWaves - 1) / kDmvSampleWaves;
    return want < cap ? want : cap;
}

}  // namespace vlg

extern "C" {

int vlg_dmv1o_sample_blocks(int B, int N, int S) {
    if (B < 1 || S < 1 || N < 2 || N > 255) return 1;
    return vlg::dmv_sample_blocks(vlg::dmv_sample_plan(N), B, S);
}

size_t vlg_dmv1o_sample_workspace(int B, int N, int S) {
    if (B < 1 || S < 1 || N < 2 || N > 255) return 0;
    const vlg::DpPlan p = vlg::dmv_sample_plan(N);
    return p.ws_stride * (size_t)B * (size_t)vlg::dmv_sample_blocks(p, B, S);
}

size_t vlg_dmv1o_sample_lds_bytes(int N) {
    if (N < 2 || N > 255) return 0;
    return vlg::dmv_sample_plan(N).lds_bytes + vlg::kDmvSampleStackBytes;
}

int vlg_dmv1o_sample(const void* dec, const void* attach, const int64_t* lengths, int B, int N, int in_dtype, int S, const uint64_t* rng,
                     unsigned site, const float* u, int64_t* heads, float* logp, float* logZ, void* ws, size_t ws_bytes, void* stream) {
    using namespace vlg;
    if (int e = check_dp_args("dmv1o_sample", B, N, VLG_F32, VLG_SR_LOG)) return e;   // the shape; the dtype's turn is behind S
    if (S < 1) return set_error(VLG_ERR_SHAPE, "dmv1o_sample: need S >= 1 samples (got %d)", S);
    if (in_dtype != VLG_F32 && in_dtype != VLG_BF16) return set_error(VLG_ERR_DTYPE, "dmv1o_sample: in_dtype %d", in_dtype);
    if (B == 0) return 0;
    if ((rng != nullptr) == (u != nullptr))
        return set_error(VLG_ERR_NULL, "dmv1o_sample: pass exactly one of rng (counter-based draws) and u (explicit uniforms)");
    if (!dec || !attach || !lengths || !heads) return set_error(VLG_ERR_NULL, "dmv1o_sample: null buffer");
    const DpPlan p = dmv_sample_plan(N);
    const int Y = dmv_sample_blocks(p, B, S);
    if (p.lds_bytes + kDmvSampleStackBytes > kLdsBudget)
        return set_error(VLG_ERR_SHAPE, "dmv1o_sample: N=%d leaves no LDS for the walk's stacks", N);   // (not reached for N <= 255)
    if (int e = check_dp_workspace("dmv1o_sample", N, p, (size_t)B * Y, ws, ws_bytes)) return e;   // one slice per block of the (B, Y) grid
    const DmvSampleArgs a{dec, attach, lengths, B, N, S, Y, rng, site, u, heads, logp, logZ, ws, p.ws_stride, p.lds_bytes, (hipStream_t)stream};
    return in_dtype == VLG_F32 ? launch_dmv_sample_mode<F32In>(p.image, a) : launch_dmv_sample_mode<BF16In>(p.image, a);
}

}  // extern "C"
