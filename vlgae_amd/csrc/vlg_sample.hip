// vlg_sample.hip -- sampling dependency trees on the device (vlg_deptree_sample, include/vlgae_amd.h): the gfx950 kernel around
// vlg_dp_sample.h.  Replaces the reference's `StructDistribution.sample` (src/model/torch_struct/distributions.py:195-217: a Python loop
// over span widths under MultiSampledSemiring plus an autograd pass per ten samples) for DependencyCRF.
//
// One workgroup per (sentence, share of the samples): it loads the arcs and runs the Log-semiring inside pass exactly as
// vlg_deptree_inside does (dep_run, same chart placement: LDS where the charts fit, the VLG_OP_DEPTREE_INSIDE workspace otherwise).
// Behind the last barrier of that pass the charts are read-only and the eight wavefronts part ways: each owns whole samples
// (s = first + wave, + 8, ...), lanes spread over the split points of the cell being drawn.  No barrier, no atomics, one writer per
// output element.  The per-wave stacks sit in dynamic LDS behind DepLayout::lds_bytes.  The frame -- wave policy, uniforms, grid,
// checks, image dispatch -- is vlg_sample_kernels.h's, shared with the DMV1o sampler.
#include "vlg_sample_kernels.h"
#include "vlg_dp_sample.h"

namespace vlg {

constexpr size_t kSampleStackBytes = (size_t)kSampleWaves * kSampleStack * sizeof(int);

template <int MODE, typename In>
__global__ __launch_bounds__(kThreads) void deptree_sample_kernel(const typename In::T* __restrict__ arc, const int64_t* __restrict__ lengths,
                                                                  int N, int S, int per_block, const uint64_t* __restrict__ rng,
                                                                  unsigned site, const float* __restrict__ u, long long* __restrict__ heads,
                                                                  float* __restrict__ logp, float* __restrict__ logZ, char* __restrict__ ws,
                                                                  size_t ws_stride, size_t lds_charts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x, B = gridDim.x, tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: the keys, the counters and the stack address stay scalar
    const int s0 = blockIdx.y * per_block, s1 = s0 + per_block < S ? s0 + per_block : S;   // this block's samples
    const int len = lengths ? (int)lengths[b] : N - 1;
    if (len < 1 || len > N - 1) return sample_no_sentence(N, s0, s1, heads, logp, logZ);
    char* wsb = ws + ((size_t)blockIdx.y * B + b) * ws_stride;
    const DepCtx c = carve_dep<VLG_SR_LOG, MODE, false>(N, len, smem, wsb);
    const typename In::T* arc_b = arc + (size_t)b * N * N;
    SampleX x;
    float lz_unused;   // dep_run hands logZ to one thread; every wave reads it from the chart instead
    dep_run<VLG_SR_LOG, false, In, (MODE == kModeShort ? kSpansShort : kSpansGeneral)>(c, arc_b, N, 1.f, &lz_unused, nullptr, nullptr, tid,
                                                                                     kThreads, x);
    // (the inside pass ends with its barrier: the charts are complete and nothing writes them from here on)
    const float lz2 = c.C[len + 1];   // CR(0,len), log2 units
    if (blockIdx.y == 0 && tid == 0 && logZ) logZ[b] = lz2 * VLG_LN2;
    int* stack = reinterpret_cast<int*>(smem + lds_charts) + wave * kSampleStack;
    for (int s = s0 + wave; s < s1; s += kSampleWaves) {
        long long* h = heads + ((size_t)s * B + b) * N;
        float* lp = logp ? logp + (size_t)s * B + b : nullptr;
        if (u) {
            const TableU us{u + ((size_t)s * B + b) * 3 * N * N, N};
            dep_sample_walk<In>(c, arc_b, N, stack, us, h, lp, lz2, x);
        } else {
            const PhiloxU us{site_key(rng[0], site), (uint32_t)s, (uint32_t)b, (uint32_t)rng[1]};
            dep_sample_walk<In>(c, arc_b, N, stack, us, h, lp, lz2, x);
        }
    }
}

}  // namespace vlg

extern "C" {

int vlg_deptree_sample_blocks(int B, int N, int S) {
    if (B < 1 || S < 1 || N < 2 || N > 255) return 1;
    return vlg::sample_blocks(vlg::dp_plan<vlg::DepLayout>(N, false, false), vlg::kSampleStackBytes, B, S);
}

// ws: one slice per block of the (B, Y) grid, vlg_workspace_bytes(VLG_OP_DEPTREE_INSIDE, B * vlg_deptree_sample_blocks(B, N, S), N, 0)
int vlg_deptree_sample(const void* arc, const int64_t* lengths, int B, int N, int in_dtype, int S, const uint64_t* rng, unsigned site,
                       const float* u, int64_t* heads, float* logp, float* logZ, void* ws, size_t ws_bytes, void* stream) {
    using namespace vlg;
    SampleArgs a{lengths, B, N, S, rng, site, u, heads, logp, logZ, ws, (hipStream_t)stream};
    const int e = sample_check<DepLayout>("deptree_sample", kSampleStackBytes, in_dtype, arc && heads, ws_bytes, a);   // the plan of vlg_deptree_inside
    if (e || !a.Y) return e;
    return sample_dispatch(in_dtype, a.image, [&](auto mode, auto in) {
        using In = decltype(in);
        return launch_sample("deptree_sample_kernel", deptree_sample_kernel<decltype(mode)::value, In>, kSampleStackBytes, a,
                             (const typename In::T*)arc);
    });
}

}  // extern "C"
