// vlg_batch.hip -- the per-batch data of one training step, on the device (gfx950): what vlgae_amd/train_step.py derives from a batch's
// lengths, tags and box masks before the chain runs, as ONE launch at the start of the step (train_step.build(batch_on_device=True)):
// nothing of a batch's contents is then read on the host, and one built step serves every batch of its shape:
//
//   vmask [B,V] u8          encoders.factor_mask: box | strict upper triangle of box (x) box | box | 1        (joint.py:140-170)
//   pen [B,Q,S] f32         align.grounding_prior: rows q = 1..L, pen[b,q,s] = sum over the named factors f != s (obj, rel, attr, in
//                           that order) of scale where f's POS set holds tag[b,q-1], else 0                     (joint.py:446-470)
//   num_token               sum_b lengths[b] as float32                                                          (var_pool.py:18)
//   coef[2], seed_max [B]   [alpha, -(1 - alpha)] / (num_token + 1e-12); coef[1] once per sentence            (fn.py:50-56)
//
// One workgroup per sentence.  Every workgroup sums the B lengths itself (an integer sum: exact in any order) -- no atomics, no second
// launch, the same bits on every run; workgroup 0 writes the scalars.  The float arithmetic is the one torch's ops do, in the same
// order, in IEEE single precision (the library is built without fast-math): every value equals the torch formulation bit for bit.
// Plain vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vlg_common.h"
#include "vlg_launch.h"

namespace vlg {

constexpr int kBatchThreads = 256;

struct PosSets {
    const int64_t* ids[3];   // obj, rel, attr
    int n[3];
    int seg[3];              // segment of the factor in the layout, -1 = absent
};

__device__ __forceinline__ bool pos_hit(const int64_t* ids, int n, int64_t t) {
    for (int i = 0; i < n; ++i)
        if (ids[i] == t) return true;
    return false;
}

__global__ __launch_bounds__(kBatchThreads) void batch_prepare_kernel(const int64_t* __restrict__ lengths, const int64_t* __restrict__ tag,
                                                                      const uint8_t* __restrict__ box_mask, int B, int L, int R, int Q, int V,
                                                                      int off_rel, int off_attr, PosSets pos, int S, float scale, float c_mt,
                                                                      float c_max, float eps, uint8_t* __restrict__ vmask, float* __restrict__ pen,
                                                                      float* __restrict__ num_token, float* __restrict__ coef,
                                                                      float* __restrict__ seed_max) {
    __shared__ long long part[kBatchThreads];
    const int b = blockIdx.x, t = threadIdx.x;
    long long s = 0;
    for (int i = t; i < B; i += kBatchThreads) s += lengths[i];
    part[t] = s;
    __syncthreads();
    for (int w = kBatchThreads / 2; w > 0; w >>= 1) {
        if (t < w) part[t] += part[t + w];
        __syncthreads();
    }
    if (t == 0) {
        const float nt = (float)part[0];   // lengths.sum().to(float32)
        const float den = nt + eps;        // + 1e-12 (a float32 operand, as torch converts the scalar)
        const float c1 = c_max / den;
        seed_max[b] = c1;
        if (b == 0) {
            num_token[0] = nt;
            coef[0] = c_mt / den;
            coef[1] = c1;
        }
    }
    const uint8_t* bm = box_mask + (size_t)b * R;
    uint8_t* vm = vmask + (size_t)b * V;
    const int rel_end = off_rel >= 0 ? off_rel + R * R : -1, attr_end = off_attr >= 0 ? off_attr + R : -1;
    for (int v = t; v < V; v += kBatchThreads) {
        uint8_t m = 1;                                   // the image column
        if (v < R) {
            m = bm[v] != 0;
        } else if (v < rel_end) {                        // rel (i, j): both boxes, j > i (triu(1))
            const int k = v - off_rel, i = k / R, j = k - i * R;
            m = j > i && bm[i] != 0 && bm[j] != 0;
        } else if (v < attr_end) {
            m = bm[v - off_attr] != 0;
        }
        vm[v] = m;
    }
    if (pen) {
        float* pb = pen + (size_t)b * Q * S;
        const int64_t* tb = tag + (size_t)b * L;
        for (int e = t; e < Q * S; e += kBatchThreads) {
            const int q = e / S, sg = e - q * S;
            float acc = 0.f;
            if (q >= 1 && q <= L) {
                const int64_t tg = tb[q - 1];
#pragma unroll
                for (int f = 0; f < 3; ++f)
                    if (pos.seg[f] >= 0 && pos.seg[f] != sg) acc += pos_hit(pos.ids[f], pos.n[f], tg) ? scale : 0.f;
            }
            pb[e] = acc;
        }
    }
}

}  // namespace vlg

int vlg_step_batch_prepare(const int64_t* lengths, const int64_t* tag, const uint8_t* box_mask, int B, int L, int R, int Q, int add_rel,
                           int add_attr, int add_image, const int64_t* pos_obj, int n_obj, const int64_t* pos_rel, int n_rel,
                           const int64_t* pos_attr, int n_attr, float prior_scale, double alpha, uint8_t* vmask, float* pen,
                           float* num_token, float* coef, float* seed_max, void* stream) {
    using namespace vlg;
    if (B < 0) return set_error(VLG_ERR_SHAPE, "step_batch_prepare: B=%d", B);
    if (B == 0) return 0;
    if (L < 1 || R < 1 || R > 4096) return set_error(VLG_ERR_SHAPE, "step_batch_prepare: L=%d R=%d (1 <= R <= 4096)", L, R);
    if (!lengths || !box_mask || !vmask || !num_token || !coef || !seed_max) return set_error(VLG_ERR_ARG, "step_batch_prepare: null buffer");
    if (n_obj < 0 || n_rel < 0 || n_attr < 0 || (n_obj && !pos_obj) || (n_rel && !pos_rel) || (n_attr && !pos_attr))
        return set_error(VLG_ERR_ARG, "step_batch_prepare: POS sets n=%d/%d/%d without their ids", n_obj, n_rel, n_attr);
    if (pen && !tag) return set_error(VLG_ERR_ARG, "step_batch_prepare: the prior table needs the tags");
    if (pen && Q < L + 1) return set_error(VLG_ERR_SHAPE, "step_batch_prepare: Q=%d < L + 1 = %d", Q, L + 1);
    const int off_rel = add_rel ? R : -1;
    const int off_attr = add_attr ? R + (add_rel ? R * R : 0) : -1;
    const int V = R + (add_rel ? R * R : 0) + (add_attr ? R : 0) + (add_image ? 1 : 0);
    // segments in factor order obj | rel | attr | img (encoders.factor_layout); only the first three have POS sets
    const int S = 1 + (add_rel != 0) + (add_attr != 0) + (add_image != 0);
    const PosSets pos{{pos_obj, pos_rel, pos_attr}, {n_obj, add_rel ? n_rel : 0, add_attr ? n_attr : 0},
                      {0, add_rel ? 1 : -1, add_attr ? 1 + (add_rel != 0) : -1}};
    // the two coefficients as torch.tensor([alpha, -(1.0 - alpha)], dtype=float32) rounds them: double arithmetic, one rounding
    const float c_mt = (float)alpha, c_max = (float)(-(1.0 - alpha)), eps = (float)1e-12;
    return launch("batch_prepare_kernel", batch_prepare_kernel, dim3(B), dim3(kBatchThreads), 0, (hipStream_t)stream, lengths, tag, box_mask, B, L, R, Q, V,
                  off_rel, off_attr, pos, S, prior_scale, c_mt, c_max, eps, vmask, pen, num_token, coef, seed_max);
}
