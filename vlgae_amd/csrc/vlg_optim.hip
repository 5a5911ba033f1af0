// vlg_optim.hip -- what runs between two training steps, on the device (gfx950): clip_grad_norm_ over every parameter, one plain Adam
// step (no amsgrad, no maximize), the ExponentialLR step behind it and the refresh of the bf16 tensors the training step reads, as TWO
// launches over up to kOptCapacity tensors (vlgae_amd/optim.py; the reference: src/pipeline.py:176-227, config/trainer/train.yaml:14,
// config/model/optimize/linear.yaml):
//
//   opt_sqsum_kernel    grid <= kOptNormGrid   sum of g^2 of the chunks a workgroup walks, in float64, into ITS slot of the workspace;
//                                              thread 0 of workgroup 0 advances the update count k in the device state and writes the
//                                              scalars of update k (lr_k / (1 - beta1^k), sqrt(1 - beta2^k), lr_k), formed in float64.
//                                              Nothing in this launch reads them.
//   opt_update_kernel   grid <= kOptGrid       every workgroup adds the slots in one fixed order (the same bits in every workgroup), forms
//                                              coef = min(1, max_norm / (norm + 1e-6)) and streams its chunks: reads g, p, m, v, writes
//                                              p, m, v and bf16(p) -- 28 bytes per element with a bf16 gradient.
//
// Work split: a tensor of n elements is ceil(n / kOptChunk) chunks, chunks are numbered tensor by tensor, workgroup w takes chunks w, w + grid,
// ...; inside a chunk thread t owns the groups of eight elements t, t + 256 (relative to the chunk's start).  The owner and the order of
// every addition are functions of the element counts alone: the results do not depend on where a tensor lies.  Each array of a group is
// moved with 16-byte accesses when ITS address allows it and element by element otherwise (and in the last, partial group of a tensor):
// nothing needs an alignment beyond the element's own.  No atomics.  Plain vector stores only.
//
// The per-tensor constants (VlgOptTensor: p, m, v, shadow, numel, lr_mult, weight_decay) are read from a device table the caller wrote
// once; the gradients' addresses travel by value in the launch arguments (they change with every eager step).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vlg_common.h"
#include "vlg_launch.h"

namespace vlg {

constexpr int kOptThreads = 256;
constexpr int kOptChunk = 4096;       // elements per chunk: two groups of eight per thread
constexpr int kOptCapacity = 128;     // tensors per launch
constexpr int kOptNormGrid = 512;     // workgroups (= slots) of one squared-sum launch
constexpr int kOptGrid = 2048;        // workgroups of one update launch
constexpr size_t kOptScalarBytes = 256;

struct OptState {        // the caller's 32 bytes of device state
    long long count;     // updates done
    float lr;            // base learning rate: the caller may overwrite it between updates
    float norm, coef, lr_used;   // of the last update: pre-clip norm, clip coefficient, lr * gamma^(k-1)
};

struct OptScalars {      // head of the workspace: written by the squared-sum launch, read by the update launch
    double step_base;    // lr_k / (1 - beta1^k)
    float inv_bc2_sqrt;  // 1 / sqrt(1 - beta2^k)
};

struct OptLaunch {       // one launch's tensors: `count` table rows from row `first`
    const void* grad[kOptCapacity];
    int chunk_start[kOptCapacity + 1];   // first chunk of tensor i within this launch; [count] = the launch's chunk count
    unsigned char gdt[kOptCapacity];     // VLG_F32 / VLG_BF16
    int first, count;
};

struct OptConsts {
    float b1, omb1, b2, omb2, eps;
    double beta1, beta2, gamma, max_norm;   // max_norm <= 0: no clipping
};

namespace {

__device__ __forceinline__ float bf16_to_f32(uint32_t h) { return __uint_as_float(h << 16); }

__device__ __forceinline__ uint32_t f32_to_bf16(float x) {   // round to nearest even; NaN -> 0x7FC0 (what torch's conversion gives)
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// x[0..8) = base[0..n), zeros behind n.  `vec`: base is 16-byte aligned (and then n == 8 takes two 16-byte loads).
__device__ __forceinline__ void load8_f32(const float* __restrict__ base, bool vec, int n, float (&x)[8]) {
    if (vec && n == 8) {
        const float4 a = *reinterpret_cast<const float4*>(base), b = *reinterpret_cast<const float4*>(base + 4);
        x[0] = a.x, x[1] = a.y, x[2] = a.z, x[3] = a.w, x[4] = b.x, x[5] = b.y, x[6] = b.z, x[7] = b.w;
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = k < n ? base[k] : 0.f;
    }
}

__device__ __forceinline__ void store8_f32(float* __restrict__ base, bool vec, int n, const float (&x)[8]) {
    if (vec && n == 8) {
        *reinterpret_cast<float4*>(base) = make_float4(x[0], x[1], x[2], x[3]);
        *reinterpret_cast<float4*>(base + 4) = make_float4(x[4], x[5], x[6], x[7]);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < n) base[k] = x[k];
    }
}

__device__ __forceinline__ void load8_bf16(const uint16_t* __restrict__ base, bool vec, int n, float (&x)[8]) {
    if (vec && n == 8) {
        const uint4 a = *reinterpret_cast<const uint4*>(base);
        const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) x[2 * k] = bf16_to_f32(w[k] & 0xffffu), x[2 * k + 1] = bf16_to_f32(w[k] >> 16);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = k < n ? bf16_to_f32(base[k]) : 0.f;
    }
}

__device__ __forceinline__ void store8_bf16(uint16_t* __restrict__ base, bool vec, int n, const float (&x)[8]) {
    if (vec && n == 8) {
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = f32_to_bf16(x[2 * k]) | (f32_to_bf16(x[2 * k + 1]) << 16);
        *reinterpret_cast<uint4*>(base) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < n) base[k] = (uint16_t)f32_to_bf16(x[k]);
    }
}

__device__ __forceinline__ void load8_grad(const void* __restrict__ g, int dt, long long e, bool vec, int n, float (&x)[8]) {
    if (dt == VLG_BF16)
        load8_bf16(reinterpret_cast<const uint16_t*>(g) + e, vec, n, x);
    else
        load8_f32(reinterpret_cast<const float*>(g) + e, vec, n, x);
}

// the tensor of chunk c: the last i with chunk_start[i] <= c (the same in every lane)
__device__ __forceinline__ int tensor_of_chunk(const OptLaunch& L, int c) {
    int lo = 0, hi = L.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (L.chunk_start[mid] <= c)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ double ipow(double b, long long e) {   // b^e, e >= 0, by squaring
    double r = 1.0;
    while (e > 0) {
        if (e & 1) r *= b;
        b *= b;
        e >>= 1;
    }
    return r;
}

// sum over the workgroup, the same order on every call: lanes by xor-shuffles, then the four waves in order
__device__ __forceinline__ double block_sum(double s, double* lds) {
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) s += __shfl_xor(s, w, 64);
    const int t = threadIdx.x;
    if ((t & 63) == 0) lds[t >> 6] = s;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

}  // namespace

__global__ __launch_bounds__(kOptThreads) void opt_sqsum_kernel(const VlgOptTensor* __restrict__ table, OptLaunch L, OptConsts C, int advance,
                                                                OptState* __restrict__ state, OptScalars* __restrict__ scalars,
                                                                double* __restrict__ slots) {
    __shared__ double lds[4];
    const int t = threadIdx.x;
    if (advance && blockIdx.x == 0 && t == 0) {
        const long long k = state->count + 1;
        state->count = k;
        const double lr_k = (double)state->lr * ipow(C.gamma, k - 1);
        state->lr_used = (float)lr_k;
        scalars->step_base = lr_k / (1.0 - ipow(C.beta1, k));
        scalars->inv_bc2_sqrt = (float)(1.0 / sqrt(1.0 - ipow(C.beta2, k)));
    }
    const int n_chunks = L.chunk_start[L.count];
    double acc = 0.0;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int i = tensor_of_chunk(L, c);
        const long long n = table[L.first + i].numel, lo = (long long)(c - L.chunk_start[i]) * kOptChunk;
        const void* g = L.grad[i];
        const int dt = L.gdt[i];
        const bool vec = aligned16(g);
#pragma unroll
        for (int j = 0; j < kOptChunk / (8 * kOptThreads); ++j) {
            const long long e = lo + 8 * (j * kOptThreads + t);
            if (e >= n) break;
            const int cnt = n - e < 8 ? (int)(n - e) : 8;
            float x[8];
            load8_grad(g, dt, e, vec, cnt, x);
#pragma unroll
            for (int k = 0; k < 8; ++k) acc = fma((double)x[k], (double)x[k], acc);
        }
    }
    const double s = block_sum(acc, lds);
    if (t == 0) slots[blockIdx.x] = s;
}

__global__ __launch_bounds__(kOptThreads) void opt_update_kernel(const VlgOptTensor* __restrict__ table, OptLaunch L, OptConsts C, int report,
                                                                 OptState* __restrict__ state, const OptScalars* __restrict__ scalars,
                                                                 const double* __restrict__ slots, int n_slots) {
    __shared__ double lds[4];
    const int t = threadIdx.x;
    double part = 0.0;
    for (int i = t; i < n_slots; i += kOptThreads) part += slots[i];
    const double norm = sqrt(block_sum(part, lds));
    double coef_d = 1.0;
    if (C.max_norm > 0.0) {
        coef_d = C.max_norm / (norm + 1e-6);
        coef_d = coef_d > 1.0 ? 1.0 : coef_d;   // a NaN norm stays NaN, as torch's clamp leaves it
    }
    const float coef = (float)coef_d;
    if (report && blockIdx.x == 0 && t == 0) {
        state->norm = (float)norm;
        state->coef = coef;
    }
    const double step_base = scalars->step_base;
    const float inv_bc2 = scalars->inv_bc2_sqrt;
    const int n_chunks = L.chunk_start[L.count];
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int i = tensor_of_chunk(L, c);
        const VlgOptTensor T = table[L.first + i];
        const long long n = T.numel, lo = (long long)(c - L.chunk_start[i]) * kOptChunk;
        const void* g = L.grad[i];
        const int dt = L.gdt[i];
        float* p = reinterpret_cast<float*>(T.param);
        uint16_t* sh = reinterpret_cast<uint16_t*>(T.shadow);
        const bool vg = aligned16(g), vp = aligned16(p), vm = aligned16(T.exp_avg), vv = aligned16(T.exp_avg_sq), vs = aligned16(sh);
        const float step = (float)(step_base * (double)T.lr_mult), wd = T.weight_decay;
#pragma unroll
        for (int j = 0; j < kOptChunk / (8 * kOptThreads); ++j) {
            const long long e = lo + 8 * (j * kOptThreads + t);
            if (e >= n) break;
            const int cnt = n - e < 8 ? (int)(n - e) : 8;
            float gx[8], px[8], mx[8], vx[8];
            load8_grad(g, dt, e, vg, cnt, gx);
            load8_f32(p + e, vp, cnt, px);
            load8_f32(T.exp_avg + e, vm, cnt, mx);
            load8_f32(T.exp_avg_sq + e, vv, cnt, vx);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                float gk = coef * gx[k];
                if (wd != 0.f) gk += wd * px[k];
                mx[k] = C.b1 * mx[k] + C.omb1 * gk;
                vx[k] = C.b2 * vx[k] + C.omb2 * (gk * gk);
                px[k] -= step * (mx[k] / (sqrtf(vx[k]) * inv_bc2 + C.eps));
            }
            store8_f32(p + e, vp, cnt, px);
            store8_f32(T.exp_avg + e, vm, cnt, mx);
            store8_f32(T.exp_avg_sq + e, vv, cnt, vx);
            if (sh) store8_bf16(sh + e, vs, cnt, px);
        }
    }
}

namespace {

inline long long opt_chunks(long long numel) { return (numel + kOptChunk - 1) / kOptChunk; }

// slots of the squared-sum launches over `count` tensors (one per workgroup), or -1 when an element count is not positive / the chunk
// count leaves int
long long opt_slots(const long long* numel, int count) {
    long long slots = 0;
    for (int first = 0; first < count; first += kOptCapacity) {
        long long chunks = 0;
        for (int i = first; i < count && i < first + kOptCapacity; ++i) {
            if (numel[i] <= 0) return -1;
            chunks += opt_chunks(numel[i]);
            if (chunks > 0x7fffffffLL) return -1;
        }
        slots += chunks < kOptNormGrid ? chunks : kOptNormGrid;
    }
    return slots;
}

inline size_t opt_ws_bytes(long long slots) { return (kOptScalarBytes + (size_t)slots * sizeof(double) + 255) & ~(size_t)255; }

}  // namespace

}  // namespace vlg

int vlg_adam_clip_plan(const VlgOptTensor* items, int count) {
    using namespace vlg;
    if (count < 0) return set_error(VLG_ERR_SHAPE, "adam_clip_plan: count=%d", count);
    if (count == 0) return 0;
    if (!items) return set_error(VLG_ERR_ARG, "adam_clip_plan: null table");
    for (int i = 0; i < count; ++i) {
        const VlgOptTensor& T = items[i];
        if (!T.param || !T.exp_avg || !T.exp_avg_sq) return set_error(VLG_ERR_ARG, "adam_clip_plan: tensor %d: null param / exp_avg / exp_avg_sq", i);
        if (T.numel <= 0) return set_error(VLG_ERR_SHAPE, "adam_clip_plan: tensor %d: numel=%lld", i, T.numel);
        if (!(T.lr_mult >= 0.f) || !(T.weight_decay >= 0.f) || isinf(T.lr_mult) || isinf(T.weight_decay))
            return set_error(VLG_ERR_SHAPE, "adam_clip_plan: tensor %d: lr_mult=%g weight_decay=%g (finite, >= 0)", i, T.lr_mult, T.weight_decay);
        if (((uintptr_t)T.param | (uintptr_t)T.exp_avg | (uintptr_t)T.exp_avg_sq) & 3)
            return set_error(VLG_ERR_ARG, "adam_clip_plan: tensor %d: param / exp_avg / exp_avg_sq must be 4-byte aligned", i);
        if ((uintptr_t)T.shadow & 1) return set_error(VLG_ERR_ARG, "adam_clip_plan: tensor %d: the bf16 shadow must be 2-byte aligned", i);
    }
    return 0;
}

size_t vlg_adam_clip_workspace(const long long* numel, int count) {
    using namespace vlg;
    if (!numel || count <= 0) return 0;
    const long long slots = opt_slots(numel, count);
    return slots < 0 ? 0 : opt_ws_bytes(slots);
}

int vlg_adam_clip_step(const VlgOptTensor* table, const long long* numel, const void* const* grads, const int* grad_dtypes, int count,
                       const VlgAdamHyper* hyper, void* state, void* ws, size_t ws_bytes, void* stream) {
    using namespace vlg;
    if (count < 0) return set_error(VLG_ERR_SHAPE, "adam_clip_step: count=%d", count);
    if (count == 0) return 0;
    if (!table || !numel || !grads || !grad_dtypes || !hyper || !state || !ws) return set_error(VLG_ERR_ARG, "adam_clip_step: null argument");
    if (((uintptr_t)state | (uintptr_t)ws | (uintptr_t)table) & 7) return set_error(VLG_ERR_ARG, "adam_clip_step: table / state / workspace must be 8-byte aligned");
    const VlgAdamHyper& H = *hyper;
    if (!(H.beta1 >= 0.0 && H.beta1 < 1.0) || !(H.beta2 >= 0.0 && H.beta2 < 1.0) || !(H.eps >= 0.0) || isinf(H.eps) || !(H.gamma > 0.0) || isinf(H.gamma) ||
        H.max_norm != H.max_norm)
        return set_error(VLG_ERR_SHAPE, "adam_clip_step: beta1=%g beta2=%g (in [0, 1)) eps=%g (>= 0) gamma=%g (> 0) max_norm=%g", H.beta1, H.beta2, H.eps,
                         H.gamma, H.max_norm);
    for (int i = 0; i < count; ++i) {
        if (grad_dtypes[i] != VLG_F32 && grad_dtypes[i] != VLG_BF16) return set_error(VLG_ERR_DTYPE, "adam_clip_step: gradient %d: dtype %d", i, grad_dtypes[i]);
        if (numel[i] <= 0) return set_error(VLG_ERR_SHAPE, "adam_clip_step: tensor %d: numel=%lld", i, numel[i]);
        if (!grads[i]) return set_error(VLG_ERR_ARG, "adam_clip_step: gradient %d is null", i);
        if ((uintptr_t)grads[i] & (grad_dtypes[i] == VLG_BF16 ? 1 : 3))
            return set_error(VLG_ERR_ARG, "adam_clip_step: gradient %d must be aligned to its element (%d bytes)", i, grad_dtypes[i] == VLG_BF16 ? 2 : 4);
    }
    const long long n_slots = opt_slots(numel, count);
    if (n_slots < 0) return set_error(VLG_ERR_SHAPE, "adam_clip_step: too many chunks in one launch");
    if (ws_bytes < opt_ws_bytes(n_slots))
        return set_error(VLG_ERR_WORKSPACE, "adam_clip_step: workspace %zu bytes, need %zu (vlg_adam_clip_workspace)", ws_bytes, opt_ws_bytes(n_slots));

    OptConsts C;
    C.b1 = (float)H.beta1, C.omb1 = (float)(1.0 - H.beta1), C.b2 = (float)H.beta2, C.omb2 = (float)(1.0 - H.beta2), C.eps = (float)H.eps;
    C.beta1 = H.beta1, C.beta2 = H.beta2, C.gamma = H.gamma, C.max_norm = (H.max_norm > 0.0 && !isinf(H.max_norm)) ? H.max_norm : 0.0;
    OptState* st = reinterpret_cast<OptState*>(state);
    OptScalars* sc = reinterpret_cast<OptScalars*>(ws);
    double* slots = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + kOptScalarBytes);

    // every squared-sum launch first, then every update launch: the update needs the whole norm
    for (int pass = 0; pass < 2; ++pass) {
        long long slot0 = 0;
        for (int first = 0; first < count; first += kOptCapacity) {
            OptLaunch L;
            L.first = first, L.count = count - first < kOptCapacity ? count - first : kOptCapacity;
            int chunks = 0;
            for (int i = 0; i < kOptCapacity; ++i) {
                const bool live = i < L.count;
                L.grad[i] = live ? grads[first + i] : nullptr;
                L.gdt[i] = live ? (unsigned char)grad_dtypes[first + i] : 0;
                L.chunk_start[i] = chunks;
                if (live) chunks += (int)opt_chunks(numel[first + i]);
            }
            L.chunk_start[kOptCapacity] = chunks;
            L.chunk_start[L.count] = chunks;
            if (pass == 0) {
                const int grid = chunks < kOptNormGrid ? chunks : kOptNormGrid;
                if (int rc = launch("opt_sqsum_kernel", opt_sqsum_kernel, dim3(grid), dim3(kOptThreads), 0, (hipStream_t)stream, table, L, C,
                                    first == 0 ? 1 : 0, st, sc, slots + slot0))
                    return rc;
                slot0 += grid;
            } else {
                const int grid = chunks < kOptGrid ? chunks : kOptGrid;
                if (int rc = launch("opt_update_kernel", opt_update_kernel, dim3(grid), dim3(kOptThreads), 0, (hipStream_t)stream, table, L, C,
                                    first == 0 ? 1 : 0, st, (const OptScalars*)sc, (const double*)slots, (int)n_slots))
                    return rc;
            }
        }
    }
    return 0;
}
