// vlg_eval.hip -- the metric update of one evaluation batch, on the device (gfx950): what Pipeline.validation_step hands to
// `metric.update(predict, y, mask)` (src/pipeline.py:132-143) as integer counts -- DependencyParsingMetric, FactorImageMatchingMetric and
// BoxRelMatchingMetric of src/utility/metric.py.  The reference walks nested Python lists with about B*L tiny device operations per batch;
// every input is a device tensor already (heads, gold arcs, the decoder's top-5 columns and factor2img, the region boxes, the gold
// scene-graph boxes), so nothing here needs the host:
//
//   eval_sentence_kernel  one workgroup per sentence: partial counts of the sentence into its workspace row (plain vector stores)
//   eval_reduce_kernel    one workgroup: adds the B rows in a fixed order INTO the running int64 counters; one thread adds the batch's
//                         float32 loss to the float64 loss sum (batch order = stream order: the reference's Python sum of `.item()`s)
//
// Counts are integers (exact in any order); the only float arithmetic is the IoU, done in IEEE single precision in the operation order
// of `_one_by_one_iou` (metric.py:228-250) with explicitly rounded operations, so that no multiply-add contraction changes a bit:
//   area = (x2 - x1) * (y2 - y1);  wh = max(min(rb) - max(lt), 0);  inter = w * h;  union = area1 + area2 - inter;  inter / union > 0.5
// (0 / 0 is NaN and compares false, as in the reference).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vlg_common.h"
#include "vlg_launch.h"

namespace vlg {

constexpr int kEvalThreads = 256, kEvalTop = 5;
// partial counts of one sentence (workspace row, int64 each)
enum { kPCorrect = 0, kPMask, kPF2iCorrect, kPF2iTotal, kPObj, kPAttr, kPRel, kPRRel, kPTotObj, kPTotAttr, kPTotRel, kPUcm, kPSlots = 16 };

struct EvalArgs {
    const int64_t* pred;      // [B, ld_pred]
    int ld_pred;
    const int64_t* gold;      // [B,L]
    const uint8_t* mask;      // [B,L] or null (the length mask)
    const int64_t* lengths;   // [B]
    const int32_t* f2i;       // [B,Q] or null
    const int32_t* top5;      // [B,Q,5] or null
    const float* vis_box;     // [B,R,4] or null (then no box metric)
    const float* sg_box;      // [B,L,8]
    const int64_t* sg_type;   // [B,L]
    const uint8_t* sg_mask;   // [B,L]
    int B, L, Q, R, V, off_rel, off_attr;
    long long* ws;            // [B][kPSlots]
};

__device__ __forceinline__ float box_area(const float* b) { return __fmul_rn(__fsub_rn(b[2], b[0]), __fsub_rn(b[3], b[1])); }

// _one_by_one_iou(pred, gold) > 0.5 for one pair of boxes (x1, y1, x2, y2)
__device__ __forceinline__ bool iou_above_half(const float* p, const float* g) {
    const float area1 = box_area(p), area2 = box_area(g);
    const float ltx = fmaxf(p[0], g[0]), lty = fmaxf(p[1], g[1]), rbx = fminf(p[2], g[2]), rby = fminf(p[3], g[3]);
    float w = __fsub_rn(rbx, ltx), h = __fsub_rn(rby, lty);
    w = w < 0.f ? 0.f : w;   // clamp(min=0)
    h = h < 0.f ? 0.f : h;
    const float inter = __fmul_rn(w, h);
    const float uni = __fsub_rn(__fadd_rn(area1, area2), inter);
    return __fdiv_rn(inter, uni) > 0.5f;
}

__global__ __launch_bounds__(kEvalThreads) void eval_sentence_kernel(EvalArgs p) {
    __shared__ int acc[kPSlots];
    const int b = blockIdx.x, t0 = threadIdx.x, L = p.L;
    if (t0 < kPSlots) acc[t0] = 0;
    __syncthreads();
    const uint8_t* mk = p.mask ? p.mask + (size_t)b * L : nullptr;   // null: vp.mask, the length mask (pipeline.py:139)
    const long long len = p.lengths[b];
    const int n_b = len < 0 ? 0 : (len > L ? L : (int)len);
    const int64_t* pr = p.pred + (size_t)b * p.ld_pred;
    const int64_t* gd = p.gold + (size_t)b * L;
    // ---- parsing (metric.py:29-39) and the number of scored tokens ----
    int n_mask = 0, n_ok = 0;
    for (int t = t0; t < L; t += kEvalThreads)
        if (mk ? mk[t] != 0 : t < n_b) {
            ++n_mask;
            n_ok += pr[t] == gd[t];
        }
    if (n_mask) atomicAdd(&acc[kPMask], n_mask);   // LDS integer adds: exact in any order
    if (n_ok) atomicAdd(&acc[kPCorrect], n_ok);
    // ---- factor -> image (metric.py:70-80 on the kept rows of txt_mask, joint.py:248-249) ----
    if (p.f2i) {
        const int32_t* f = p.f2i + (size_t)b * p.Q;
        int hit = 0;
        for (int i = t0; i < 2 * n_b; i += kEvalThreads) {
            const int q = i < n_b ? 1 + i : L + 2 + (i - n_b);   // words 1..n_b, arcs N+1..N+n_b (N = L + 1)
            hit += f[q] == b;
        }
        if (hit) atomicAdd(&acc[kPF2iCorrect], hit);
        if (t0 == 0) acc[kPF2iTotal] = 2 * n_b;
    }
    __syncthreads();
    if (t0 == 0) acc[kPUcm] = acc[kPCorrect] == acc[kPMask];   // every masked word correct; an empty mask counts (metric.py:38)
    // ---- box / relation (metric.py:122-193) ----
    if (p.vis_box) {
        const int m_b = acc[kPMask];   // the FIRST m_b words are scored, whatever positions the mask removed
        const int K = p.V < kEvalTop ? p.V : kEvalTop, R = p.R;
        const float* boxes = p.vis_box + (size_t)b * R * 4;
        int c_obj = 0, c_attr = 0, c_rel = 0, c_rrel = 0, n_obj = 0, n_attr = 0, n_rel = 0;
        for (int t = t0; t < L; t += kEvalThreads) {
            const long long gt = p.sg_type[(size_t)b * L + t];
            n_obj += gt == 1;
            n_attr += gt == 2;
            n_rel += gt == 3;
            if (t >= m_b || !p.sg_mask[(size_t)b * L + t]) continue;   // pred_mask & gold_mask (metric.py:173)
            const float* g0 = p.sg_box + ((size_t)b * L + t) * 8;
            const float* g1 = g0 + 4;
            const int32_t* cols = p.top5 + ((size_t)b * p.Q + (t + 1)) * kEvalTop;
            bool any_oa = false, any_rel = false, any_rrel = false;
            int type0 = 0;
            for (int k = 0; k < K; ++k) {
                const int col = cols[k];
                int type = 0, i = 0, j = 0;   // the image factor (and anything outside the layout): type 0, boxes (0, 0)
                if (col >= 0 && col < R) {
                    type = 1; i = j = col;
                } else if (p.off_rel >= 0 && col >= p.off_rel && col < p.off_rel + R * R) {
                    type = 3; i = (col - p.off_rel) / R; j = (col - p.off_rel) - i * R;
                } else if (p.off_attr >= 0 && col >= p.off_attr && col < p.off_attr + R) {
                    type = 2; i = j = col - p.off_attr;
                }
                if (k == 0) type0 = type;
                const float* bi = boxes + (size_t)i * 4;
                const float* bj = boxes + (size_t)j * 4;
                const bool first = iou_above_half(bi, g0);
                if (type < 3) any_oa |= first;                                                       // metric.py:176-177
                else {
                    any_rel |= first && iou_above_half(bj, g1);                                     // :179
                    any_rrel |= iou_above_half(bi, g1) && iou_above_half(bj, g0);                   // :180-185 (gold pair swapped)
                }
            }
            const bool oa = any_oa && gt > 0 && type0 > 0;                                           // :178
            c_obj += oa && gt == 1;
            c_attr += oa && gt == 2;
            c_rel += any_rel && gt == 3;
            c_rrel += any_rrel && gt == 3;
        }
        if (c_obj) atomicAdd(&acc[kPObj], c_obj);
        if (c_attr) atomicAdd(&acc[kPAttr], c_attr);
        if (c_rel) atomicAdd(&acc[kPRel], c_rel);
        if (c_rrel) atomicAdd(&acc[kPRRel], c_rrel);
        if (n_obj) atomicAdd(&acc[kPTotObj], n_obj);
        if (n_attr) atomicAdd(&acc[kPTotAttr], n_attr);
        if (n_rel) atomicAdd(&acc[kPTotRel], n_rel);
    }
    __syncthreads();
    if (t0 < kPSlots) p.ws[(size_t)b * kPSlots + t0] = acc[t0];
}

// counters[k] += sum over sentences; thread (part, slot) adds sentences part, part + 16, ...; the 16 parts are then added in order.
__global__ __launch_bounds__(kEvalThreads) void eval_reduce_kernel(const long long* __restrict__ ws, int B, int has_f2i, int has_box,
                                                                   const float* __restrict__ loss, long long* __restrict__ counters) {
    __shared__ long long part[16][kPSlots + 1];
    const int slot = threadIdx.x & 15, pt = threadIdx.x >> 4;
    long long s = 0;
    for (int b = pt; b < B; b += 16) s += ws[(size_t)b * kPSlots + slot];
    part[pt][slot] = s;
    __syncthreads();
    if (threadIdx.x < kPSlots) {
        long long tot = 0;
        for (int k = 0; k < 16; ++k) tot += part[k][threadIdx.x];
        part[0][threadIdx.x] = tot;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long* tot = part[0];
        counters[VLG_EVAL_CORRECT_ARCS] += tot[kPCorrect];
        counters[VLG_EVAL_TOTAL] += tot[kPMask];
        counters[VLG_EVAL_N_UCM] += tot[kPUcm];
        counters[VLG_EVAL_N] += B;
        if (has_f2i) {
            counters[VLG_EVAL_F2I_CORRECT] += tot[kPF2iCorrect];
            counters[VLG_EVAL_F2I_TOTAL] += tot[kPF2iTotal];
        }
        if (has_box) {
            counters[VLG_EVAL_CORRECT_OBJ] += tot[kPObj];
            counters[VLG_EVAL_CORRECT_ATTR] += tot[kPAttr];
            counters[VLG_EVAL_CORRECT_REL] += tot[kPRel];
            counters[VLG_EVAL_CORRECT_R_REL] += tot[kPRRel];
            counters[VLG_EVAL_TOTAL_OBJ] += tot[kPTotObj];
            counters[VLG_EVAL_TOTAL_ATTR] += tot[kPTotAttr];
            counters[VLG_EVAL_TOTAL_REL] += tot[kPTotRel];
            counters[VLG_EVAL_PROCESSED_TOKEN] += tot[kPMask];
        }
        counters[VLG_EVAL_N_BATCHES] += 1;
        if (loss) {
            double* sum = reinterpret_cast<double*>(counters + VLG_EVAL_LOSS_SUM);
            *sum = *sum + (double)loss[0];
        }
    }
}

}  // namespace vlg

size_t vlg_eval_metrics_workspace(int B) {
    if (B < 1) return 0;
    return ((size_t)B * vlg::kPSlots * sizeof(long long) + 255) & ~(size_t)255;
}

int vlg_eval_metrics(const int64_t* pred_arc, int ld_pred, const int64_t* gold_arc, const uint8_t* mask, const int64_t* lengths,
                     const int32_t* factor2img, const int32_t* top5, const float* vis_box, const float* sg_box, const int64_t* sg_type,
                     const uint8_t* sg_mask, const float* loss, int B, int L, int Q, int R, int add_rel, int add_attr, int add_image,
                     void* ws, size_t ws_bytes, int64_t* counters, void* stream) {
    using namespace vlg;
    if (B < 0 || L < 1) return set_error(VLG_ERR_SHAPE, "eval_metrics: B=%d L=%d", B, L);
    if (B == 0) return 0;
    if (ld_pred < L) return set_error(VLG_ERR_SHAPE, "eval_metrics: ld_pred=%d < L=%d", ld_pred, L);
    if (!pred_arc || !gold_arc || !lengths || !counters) return set_error(VLG_ERR_ARG, "eval_metrics: null buffer");
    const int n_box_args = (vis_box != nullptr) + (sg_box != nullptr) + (sg_type != nullptr) + (sg_mask != nullptr);
    if (n_box_args != 0 && (n_box_args != 4 || !top5))
        return set_error(VLG_ERR_ARG, "eval_metrics: vis_box, sg_box, sg_type, sg_mask and top5 go together");
    if ((factor2img || n_box_args) && Q != 2 * (L + 1))
        return set_error(VLG_ERR_SHAPE, "eval_metrics: Q=%d, expected 2 (L + 1) = %d query rows", Q, 2 * (L + 1));
    if (n_box_args && (R < 1 || R > 4096)) return set_error(VLG_ERR_SHAPE, "eval_metrics: R=%d (1 <= R <= 4096)", R);
    if (!ws || ws_bytes < vlg_eval_metrics_workspace(B))
        return set_error(VLG_ERR_WORKSPACE, "eval_metrics: needs a %zu-byte workspace (got %zu)", vlg_eval_metrics_workspace(B), ws_bytes);
    const int off_rel = add_rel ? R : -1;
    const int off_attr = add_attr ? R + (add_rel ? R * R : 0) : -1;
    const int V = R + (add_rel ? R * R : 0) + (add_attr ? R : 0) + (add_image ? 1 : 0);
    const EvalArgs a{pred_arc, ld_pred, gold_arc, mask, lengths, factor2img, n_box_args ? top5 : nullptr, vis_box, sg_box, sg_type, sg_mask,
                     B, L, Q, R, V, off_rel, off_attr, static_cast<long long*>(ws)};
    hipStream_t s = (hipStream_t)stream;
    if (int rc = launch("eval_sentence_kernel", eval_sentence_kernel, dim3(B), dim3(kEvalThreads), 0, s, a)) return rc;
    return launch("eval_reduce_kernel", eval_reduce_kernel, dim3(1), dim3(kEvalThreads), 0, s, static_cast<const long long*>(ws), B, factor2img != nullptr,
                  n_box_args != 0, loss, reinterpret_cast<long long*>(counters));
}
