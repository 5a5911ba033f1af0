// vlg_dmv_sample.hip -- sampling DMV1o dependency trees on the device (vlg_dmv1o_sample, include/vlgae_amd.h): the gfx950 kernel around
// vlg_dmv_sample.h.  Replaces the reference's `StructDistribution.sample` (src/model/torch_struct/distributions.py:195-217: a Python loop
// over span widths under MultiSampledSemiring plus an autograd pass per ten samples) for DMV1o.
//
// One workgroup per (sentence, share of the samples): it stages the potentials and runs the Log-semiring inside pass exactly as
// vlg_dmv1o_inside does (dmv_run<Log, false> through MergedIO, same chart placement: the short image for N <= kShortN, LDS where the
// charts fit, the VLG_OP_DMV1O_INSIDE workspace otherwise).  Behind the last barrier the charts are read-only and the eight wavefronts
// part ways: each owns whole samples (s = first + wave, + 8, ...), lanes spread over the split points of the cell being drawn.  No
// barrier, no atomics, one writer per output element.  The per-wave stacks sit in dynamic LDS behind DmvLayout's lds_bytes.  The frame
// -- wave policy, uniforms, grid, checks, image dispatch -- is vlg_sample_kernels.h's, shared with the DepTree sampler.
//
// Built WITHOUT -ffinite-math-only (vlgae_amd/build.py): the draw compares against a uniform that may be NaN.
#include "vlg_sample_kernels.h"
#include "vlg_dmv_sample.h"

namespace vlg {

constexpr size_t kDmvSampleStackBytes = (size_t)kSampleWaves * kDmvSampleStack * sizeof(int);

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
    if (len < 1 || len > N - 1) return sample_no_sentence(N, s0, s1, heads, logp, logZ);
    char* wsb = ws + ((size_t)blockIdx.y * B + b) * ws_stride;
    const DmvCtx c = carve_dmv<VLG_SR_LOG, MODE, false>(N, len, smem, wsb, false);
    MergedIO<In> io;
    io.dec = dec + (size_t)b * N * 8;
    io.attach = attach + (size_t)b * N * N * 2;
    io.N = N;
    io.gdec = nullptr;
    io.gatt = nullptr;
    io.heads = nullptr;
    SampleX x;
    float lz_unused;   // dmv_run hands logZ to one thread; every wave reads it from the chart instead
    dmv_run<VLG_SR_LOG, false, spans_of(MODE)>(c, io, 1.f, &lz_unused, tid, kThreads, x);
    x.sync();   // the charts are complete and nothing writes them from here on
    const float lz2 = c.C[len + 1].y;   // CR(0,len).NOCHILD, log2 units (dmv.py:65)
    if (blockIdx.y == 0 && tid == 0 && logZ) logZ[b] = lz2 * VLG_LN2;
    int* stack = reinterpret_cast<int*>(smem + lds_charts) + wave * kDmvSampleStack;
    for (int s = s0 + wave; s < s1; s += kSampleWaves) {
        long long* h = heads + ((size_t)s * B + b) * N;
        float* lp = logp ? logp + (size_t)s * B + b : nullptr;
        if (u) {
            const TableU us{u + ((size_t)s * B + b) * 3 * N * N, N};
            dmv_sample_walk<In>(c, io.dec, io.attach, N, stack, us, h, lp, lz2, x);
        } else {
            const PhiloxU us{site_key(rng[0], site), (uint32_t)s, (uint32_t)b, (uint32_t)rng[1]};
            dmv_sample_walk<In>(c, io.dec, io.attach, N, stack, us, h, lp, lz2, x);
        }
    }
}

static DpPlan dmv_sample_plan(int N) { return dp_plan<DmvLayout>(N, false, false); }   // the plan of vlg_dmv1o_inside

}  // namespace vlg

extern "C" {

int vlg_dmv1o_sample_blocks(int B, int N, int S) {
    if (B < 1 || S < 1 || N < 2 || N > 255) return 1;
    return vlg::sample_blocks(vlg::dmv_sample_plan(N), vlg::kDmvSampleStackBytes, B, S);
}

size_t vlg_dmv1o_sample_workspace(int B, int N, int S) {
    if (B < 1 || S < 1 || N < 2 || N > 255) return 0;
    const vlg::DpPlan p = vlg::dmv_sample_plan(N);
    return p.ws_stride * (size_t)B * (size_t)vlg::sample_blocks(p, vlg::kDmvSampleStackBytes, B, S);
}

size_t vlg_dmv1o_sample_lds_bytes(int N) {
    if (N < 2 || N > 255) return 0;
    return vlg::dmv_sample_plan(N).lds_bytes + vlg::kDmvSampleStackBytes;
}

int vlg_dmv1o_sample(const void* dec, const void* attach, const int64_t* lengths, int B, int N, int in_dtype, int S, const uint64_t* rng,
                     unsigned site, const float* u, int64_t* heads, float* logp, float* logZ, void* ws, size_t ws_bytes, void* stream) {
    using namespace vlg;
    SampleArgs a{lengths, B, N, S, rng, site, u, heads, logp, logZ, ws, (hipStream_t)stream};
    const int e = sample_check<DmvLayout>("dmv1o_sample", kDmvSampleStackBytes, in_dtype, dec && attach && lengths && heads, ws_bytes, a);
    if (e || !a.Y) return e;
    return sample_dispatch(in_dtype, a.image, [&](auto mode, auto in) {
        using In = decltype(in);
        return launch_sample("dmv1o_sample_kernel", dmv1o_sample_kernel<decltype(mode)::value, In>, kDmvSampleStackBytes, a,
                             (const typename In::T*)dec, (const typename In::T*)attach);
    });
}

}  // extern "C"
