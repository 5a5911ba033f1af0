// vlg_label.hip -- labeled arc potentials [B,N,N,L] around the DepTree DP (vlg_label_fold, vlg_label_expand, vlg_label_draw,
// include/vlgae_amd.h).  Replaces what the reference does in torch ops around its DP for the labeled event shape (deptree.py:33-41:
// `semiring.sum` over the label axis in front of the DP, autograd behind it spreading the arc gradient over the labels).
//
// The DP does not change: fold reduces the label axis to the [B,N,N] arc scores it reads, expand spreads an arc-level gradient back
// over the labels, draw labels the arcs of sampled trees.  fold and expand stream phi once each; everything else they touch is
// [B,N,N].  No atomics: every output element has one writer.
//
// Layout (fold, expand).  A ROW is the L labels of one (b, head, child): L consecutive elements, as few as 2 bytes.  A lane group of G
// lanes (a power of two, inside one wavefront) owns one row; consecutive groups own consecutive rows, so the loads of a wavefront cover
// 64 / G consecutive rows -- contiguous memory.  A lane holds up to KS SLOTS of E consecutive elements: slot k of lane j is elements
// [(j + k G) E, (j + k G) E + E).  Two images:
//   vector   L sizeof(elem) a multiple of 16 and every base pointer 16-byte aligned: E = 16 / sizeof(elem) (one 16-byte load per
//            slot of phi), KS = 2
//   element  otherwise: E = 1, KS = 4
// G = the smallest power of two with G KS E >= L (label_plan below; the table is in DESIGN.md).  The max / sum over a row are DPP
// butterflies over the group (vlg_dp_kernels.h: butterfly), as the DP's reductions are.
// Cells the DP never reads -- child 0, head = child, head or child beyond the length -- are not loaded.
#include "vlg_dp_kernels.h"
#include "vlg_label_draw.h"
#include "vlg_rows.h"
#include "vlg_sample_kernels.h"

namespace vlg {

constexpr int kLabelThreads = 256;
#define VLG_MINUS_INF (-__builtin_inff())

struct LabelPlan {
    int E, KS, G, lgG;
    bool vec;
};

static LabelPlan label_plan(int L, int in_dtype, bool aligned) {
    const int es = in_dtype == VLG_BF16 ? 2 : 4;
    LabelPlan p;
    p.vec = aligned && (L * es) % 16 == 0;
    p.E = p.vec ? 16 / es : 1;
    p.KS = p.vec ? 2 : 4;
    const int need = (L + p.KS * p.E - 1) / (p.KS * p.E);   // lanes that hold the row
    p.G = 1;
    p.lgG = 0;
    while (p.G < need) { p.G <<= 1; ++p.lgG; }
    return p;
}

// E consecutive elements as floats
template <typename In, int E>
__device__ __forceinline__ void ld_slot(const typename In::T* p, float (&o)[E]) {
    if constexpr (E == 1) o[0] = In::ld(p, 0);
    else if constexpr (E == 4) load4(p, o);
    else load8(p, o);
}
template <typename T, int E>
__device__ __forceinline__ void st_slot(T* p, const float (&v)[E]) {
    if constexpr (E == 1) stf(p, 0, v[0]);
    else if constexpr (E == 4) store4(p, v);
    else store8(p, v);
}

// a label takes part iff it is above the clamp floor of the DP's load stage (NaN does not): the others have probability 0
__device__ __forceinline__ bool label_allowed(float x) { return x > VLG_POT_FLOOR; }

// which row this lane works on, and whether the DP reads its cell
struct LabelRow {
    int b, q, j;      // sentence, cell h N + c, lane within the group
    bool in, live;    // a row of the tensor; a cell the DP reads
    size_t row;       // b N N + q
};

__device__ __forceinline__ LabelRow label_row(const int64_t* __restrict__ lengths, int N, int lgG, int tps) {
    LabelRow r;
    const int tid = threadIdx.x, G = 1 << lgG;
    r.b = blockIdx.x / tps;
    const int tile = blockIdx.x - r.b * tps;
    r.q = tile * (kLabelThreads >> lgG) + (tid >> lgG);
    r.j = tid & (G - 1);
    r.in = r.q < N * N;
    const int h = r.q / N, c = r.q - h * N;
    const long long len = lengths ? lengths[r.b] : N - 1;
    r.live = r.in && len >= 1 && len <= N - 1 && c >= 1 && h != c && h <= len && c <= len;
    r.row = (size_t)r.b * N * N + (r.in ? r.q : 0);
    return r;
}

// ---- fold ----------------------------------------------------------------------------------------------------------------------------
// arc = logsumexp_l phi (Log) / max_l phi (Max); best = the lowest label attaining the maximum; dbar = sum_l p_l (v_l - v_sub_l).
template <typename In, typename VIn, int E, int KS>
__global__ __launch_bounds__(kLabelThreads) void label_fold_kernel(const typename In::T* __restrict__ phi, const typename VIn::T* __restrict__ v,
                                                                   const typename VIn::T* __restrict__ v_sub,
                                                                   const int64_t* __restrict__ lengths, int N, int L, int lgG, int tps, int sr,
                                                                   float* __restrict__ arc, unsigned char* __restrict__ best,
                                                                   float* __restrict__ dbar) {
    const LabelRow r = label_row(lengths, N, lgG, tps);
    const int G = 1 << lgG;
    const size_t base = r.row * (size_t)L;
    float x[KS][E];
    float m = VLG_MINUS_INF;
    int am = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < KS; ++k) {
        const int e0 = (r.j + k * G) * E;
        const bool ok = r.live && e0 < L;
        if (ok) ld_slot<In, E>(phi + base + e0, x[k]);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            x[k][e] = ok && label_allowed(x[k][e]) ? x[k][e] : VLG_MINUS_INF;
            if (x[k][e] > m) { m = x[k][e]; am = e0 + e; }   // ascending label order within the lane: the first maximum
        }
    }
    float M[1] = {m};
    butterfly<kOpMax, 1>(M, G);
    const bool some = M[0] > VLG_MINUS_INF;   // (group-uniform)
    if (best) {
        int a[1] = {some && m == M[0] ? am : 0x7fffffff};
        butterfly<kOpMinI, 1>(a, G);
        if (r.in && r.j == 0) best[r.row] = (unsigned char)(r.live && some ? a[0] : 0);
    }
    float out = M[0], db = 0.f;
    if (sr == VLG_SR_LOG) {
        float acc[2] = {0.f, 0.f};   // sum_l w_l, sum_l w_l d_l
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const int e0 = (r.j + k * G) * E;
            const bool ok = r.live && e0 < L && some;
            float d[E];
#pragma unroll
            for (int e = 0; e < E; ++e) d[e] = 0.f;
            if (ok && v) {
                ld_slot<VIn, E>(v + base + e0, d);
                if (v_sub) {
                    float s[E];
                    ld_slot<VIn, E>(v_sub + base + e0, s);
#pragma unroll
                    for (int e = 0; e < E; ++e) d[e] -= s[e];
                }
            }
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const bool al = ok && x[k][e] > VLG_MINUS_INF;
                const float w = al ? VLG_EXP((x[k][e] - M[0]) * VLG_LOG2E) : 0.f;
                acc[0] += w;
                acc[1] += al ? w * d[e] : 0.f;   // the direction counts only where the label is allowed
            }
        }
        butterfly<kOpAdd, 2>(acc, G);
        if (some) {
            out = M[0] + VLG_LOG(acc[0]) * VLG_LN2;
            db = acc[1] / acc[0];
        }
    }
    if (r.in && r.j == 0) {
        arc[r.row] = r.live ? out : VLG_NEGINF;
        if (dbar) dbar[r.row] = r.live ? db : 0.f;
    }
}

// ---- expand --------------------------------------------------------------------------------------------------------------------------
// out_l = scale p_l (g1 + g2 (d_l - dbar))   (mode 0)      out_l = scale g1 p_l   (mode 1)
// p_l = exp(phi_l - arc) (Log) / [l == best] (Max).  No reduction: arc, best and dbar are the fold's.
template <typename In, typename VIn, typename Out, int E, int KS>
__global__ __launch_bounds__(kLabelThreads) void label_expand_kernel(const typename In::T* __restrict__ phi, const typename VIn::T* __restrict__ v,
                                                                     const typename VIn::T* __restrict__ v_sub,
                                                                     const int64_t* __restrict__ lengths, int N, int L, int lgG, int tps, int sr,
                                                                     int mode, const float* __restrict__ arc,
                                                                     const unsigned char* __restrict__ best, const float* __restrict__ g1,
                                                                     const float* __restrict__ g2, const float* __restrict__ dbar,
                                                                     const float* __restrict__ scale, int scale_stride, Out* __restrict__ out) {
    const LabelRow r = label_row(lengths, N, lgG, tps);
    if (!r.in) return;
    const int G = 1 << lgG;
    const size_t base = r.row * (size_t)L;
    float a = VLG_MINUS_INF, ga = 0.f, gb = 0.f, db = 0.f;
    int bl = -1;
    if (r.live) {
        a = arc[r.row];
        ga = g1[r.row];
        if (scale) ga *= scale[(size_t)r.b * scale_stride];
        if (mode == 0 && g2) {
            gb = g2[r.row];
            if (scale) gb *= scale[(size_t)r.b * scale_stride];
            if (dbar) db = dbar[r.row];
        }
        if (sr == VLG_SR_MAX) bl = best[r.row];
    }
    const bool some = r.live && a > VLG_MINUS_INF;   // NaN, -inf: a row without an allowed label
#pragma unroll
    for (int k = 0; k < KS; ++k) {
        const int e0 = (r.j + k * G) * E;
        if (e0 >= L) continue;
        float o[E];
#pragma unroll
        for (int e = 0; e < E; ++e) o[e] = 0.f;
        if (some) {
            float x[E], d[E];
            ld_slot<In, E>(phi + base + e0, x);
#pragma unroll
            for (int e = 0; e < E; ++e) d[e] = 0.f;
            if (mode == 0 && g2 && v) {
                ld_slot<VIn, E>(v + base + e0, d);
                if (v_sub) {
                    float s[E];
                    ld_slot<VIn, E>(v_sub + base + e0, s);
#pragma unroll
                    for (int e = 0; e < E; ++e) d[e] -= s[e];
                }
            }
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const bool al = label_allowed(x[e]);
                float p;
                if (sr == VLG_SR_MAX) p = e0 + e == bl ? 1.f : 0.f;
                else p = al ? VLG_EXP(fminf(x[e] - a, 0.f) * VLG_LOG2E) : 0.f;
                o[e] = p == 0.f ? 0.f : p * (ga + (al ? gb * (d[e] - db) : 0.f));
            }
        }
        st_slot<Out, E>(out + base + e0, o);
    }
}

// ---- draw ----------------------------------------------------------------------------------------------------------------------------
// One wavefront per (sample, sentence), four per workgroup; the body is vlg_label_draw.h's.
constexpr int kDrawWaves = kLabelThreads / 64;

template <typename In>
__global__ __launch_bounds__(kLabelThreads) void label_draw_kernel(const typename In::T* __restrict__ phi, const float* __restrict__ arc,
                                                                   const long long* __restrict__ heads, const int64_t* __restrict__ lengths,
                                                                   int B, int N, int L, int S, const uint64_t* __restrict__ rng, unsigned site,
                                                                   const float* __restrict__ u_label, long long* __restrict__ labels,
                                                                   float* __restrict__ logp) {
    __shared__ float stage_all[kDrawWaves][kLabelStage];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long pair = (long long)blockIdx.x * kDrawWaves + wave;   // s B + b
    if (pair >= (long long)S * B) return;
    const int s = (int)(pair / B), b = (int)(pair - (long long)s * B);
    const size_t sb = (size_t)pair * N;
    SampleX x;
    const int lane = x.lane();
    const int len = lengths ? (int)lengths[b] : N - 1;
    if (len < 1 || len > N - 1) {   // not a sentence: the tree sampler wrote heads 0 and logp NaN
        for (int i = lane; i < N; i += 64) labels[sb + i] = 0;
        return;
    }
    const typename In::T* phi_b = phi + (size_t)b * N * N * L;
    const float* arc_b = arc ? arc + (size_t)b * N * N : nullptr;
    float* lp = logp && arc ? logp + pair : nullptr;
    if (u_label) {
        const LabelTableU us{u_label + sb};
        label_draw_walk<In>(phi_b, arc_b, N, L, len, heads + sb, us, stage_all[wave], labels + sb, lp, x);
    } else {
        const PhiloxU us{site_key(rng[0], site), (uint32_t)s, (uint32_t)b, (uint32_t)rng[1]};
        label_draw_walk<In>(phi_b, arc_b, N, L, len, heads + sb, us, stage_all[wave], labels + sb, lp, x);
    }
}

// ---- launch --------------------------------------------------------------------------------------------------------------------------
static int check_label_args(const char* who, int B, int N, int L, int in_dtype, int semiring) {
    if (int e = check_dp_args(who, B, N, in_dtype, semiring)) return e;
    if (L < 1 || L > kLabelMax) return set_error(VLG_ERR_SHAPE, "%s: need 1 <= L <= %d labels (got %d)", who, kLabelMax, L);
    return 0;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// tiles per sentence and the grid; 0 if the grid does not fit: a launch is refused beyond 2^32 - 1 threads, so with 256 lanes per
// workgroup the largest grid is 2^24 - 1 workgroups
constexpr long long kLabelMaxGrid = (1LL << 24) - 1;
static long long label_grid(int B, int N, const LabelPlan& p, int& tps) {
    const int rpb = kLabelThreads / p.G;
    tps = (N * N + rpb - 1) / rpb;
    const long long grid = (long long)B * tps;
    return grid > kLabelMaxGrid ? 0 : grid;
}

struct FoldArgs {
    const void *phi, *v, *v_sub;
    const int64_t* lengths;
    int N, L, lgG, tps, sr;
    float* arc;
    unsigned char* best;
    float* dbar;
    unsigned grid;
    hipStream_t s;
};

template <typename In, typename VIn, int E, int KS>
static int launch_fold(const FoldArgs& a) {
    return launch("label_fold_kernel", label_fold_kernel<In, VIn, E, KS>, dim3(a.grid), dim3(kLabelThreads), 0, a.s, (const typename In::T*)a.phi,
                  (const typename VIn::T*)a.v, (const typename VIn::T*)a.v_sub, a.lengths, a.N, a.L, a.lgG, a.tps, a.sr, a.arc, a.best, a.dbar);
}

template <typename In, int EV>
static int launch_fold_v(bool vec, int v_dtype, const FoldArgs& a) {
    if (v_dtype == VLG_F32) return vec ? launch_fold<In, F32In, EV, 2>(a) : launch_fold<In, F32In, 1, 4>(a);
    return vec ? launch_fold<In, BF16In, EV, 2>(a) : launch_fold<In, BF16In, 1, 4>(a);
}

struct ExpandArgs {
    const void *phi, *v, *v_sub;
    const int64_t* lengths;
    int N, L, lgG, tps, sr, mode;
    const float* arc;
    const unsigned char* best;
    const float *g1, *g2, *dbar, *scale;
    int scale_stride;
    void* out;
    unsigned grid;
    hipStream_t s;
};

template <typename In, typename VIn, typename Out, int E, int KS>
static int launch_expand(const ExpandArgs& a) {
    return launch("label_expand_kernel", label_expand_kernel<In, VIn, Out, E, KS>, dim3(a.grid), dim3(kLabelThreads), 0, a.s,
                  (const typename In::T*)a.phi, (const typename VIn::T*)a.v, (const typename VIn::T*)a.v_sub, a.lengths, a.N, a.L, a.lgG, a.tps,
                  a.sr, a.mode, a.arc, a.best, a.g1, a.g2, a.dbar, a.scale, a.scale_stride, (Out*)a.out);
}

template <typename In, typename Out, int EV>
static int launch_expand_v(bool vec, int v_dtype, const ExpandArgs& a) {
    if (v_dtype == VLG_F32) return vec ? launch_expand<In, F32In, Out, EV, 2>(a) : launch_expand<In, F32In, Out, 1, 4>(a);
    return vec ? launch_expand<In, BF16In, Out, EV, 2>(a) : launch_expand<In, BF16In, Out, 1, 4>(a);
}

}  // namespace vlg

extern "C" {

int vlg_label_lanes(int L, int in_dtype) {
    if (L < 1 || L > vlg::kLabelMax || (in_dtype != VLG_F32 && in_dtype != VLG_BF16)) return 0;
    const vlg::LabelPlan p = vlg::label_plan(L, in_dtype, true);
    return p.G | (p.vec ? 0x100 : 0);
}

int vlg_label_fold(const void* phi, const void* v, const void* v_sub, const int64_t* lengths, int B, int N, int L, int in_dtype, int v_dtype,
                   int semiring, float* arc, unsigned char* best, float* dbar, void* stream) {
    using namespace vlg;
    if (int e = check_label_args("label_fold", B, N, L, in_dtype, semiring)) return e;
    if (v_dtype != VLG_F32 && v_dtype != VLG_BF16) return set_error(VLG_ERR_DTYPE, "label_fold: v_dtype %d", v_dtype);
    if (B == 0) return 0;
    if (!phi || !arc) return set_error(VLG_ERR_ARG, "label_fold: null buffer (phi and arc are required)");
    if (dbar && semiring != VLG_SR_LOG) return set_error(VLG_ERR_ARG, "label_fold: dbar is the Log semiring's");
    if (v_sub && !v) return set_error(VLG_ERR_ARG, "label_fold: v_sub without v");
    const LabelPlan p = label_plan(L, in_dtype, aligned16(phi) && aligned16(v) && aligned16(v_sub));
    int tps;
    const long long grid = label_grid(B, N, p, tps);
    if (!grid) return set_error(VLG_ERR_SHAPE, "label_fold: B=%d N=%d L=%d needs more than 2^24 - 1 workgroups", B, N, L);
    const FoldArgs a{phi, dbar ? v : nullptr, dbar ? v_sub : nullptr, lengths, N, L, p.lgG, tps, semiring, arc, best, dbar, (unsigned)grid,
                     (hipStream_t)stream};
    return in_dtype == VLG_F32 ? launch_fold_v<F32In, 4>(p.vec, v_dtype, a) : launch_fold_v<BF16In, 8>(p.vec, v_dtype, a);
}

int vlg_label_expand(const void* phi, const void* v, const void* v_sub, const int64_t* lengths, int B, int N, int L, int in_dtype, int v_dtype,
                     int out_dtype, int semiring, int mode, const float* arc, const unsigned char* best, const float* g1, const float* g2,
                     const float* dbar, const float* scale, int scale_stride, void* out, void* stream) {
    using namespace vlg;
    if (int e = check_label_args("label_expand", B, N, L, in_dtype, semiring)) return e;
    if (v_dtype != VLG_F32 && v_dtype != VLG_BF16) return set_error(VLG_ERR_DTYPE, "label_expand: v_dtype %d", v_dtype);
    if (out_dtype != VLG_F32 && out_dtype != in_dtype) return set_error(VLG_ERR_DTYPE, "label_expand: out_dtype %d (float32 or the input's)", out_dtype);
    if (mode != 0 && mode != 1) return set_error(VLG_ERR_ARG, "label_expand: mode %d", mode);
    if (scale_stride != 0 && scale_stride != 1) return set_error(VLG_ERR_ARG, "label_expand: scale_stride %d", scale_stride);
    if (B == 0) return 0;
    if (!phi || !arc || !g1 || !out) return set_error(VLG_ERR_ARG, "label_expand: null buffer (phi, arc, g1 and out are required)");
    if (semiring == VLG_SR_MAX && !best) return set_error(VLG_ERR_ARG, "label_expand: the Max semiring needs best");
    if (v_sub && !v) return set_error(VLG_ERR_ARG, "label_expand: v_sub without v");
    const bool dir = mode == 0 && g2 && v;
    const LabelPlan p = label_plan(L, in_dtype, aligned16(phi) && aligned16(out) && (!dir || (aligned16(v) && aligned16(v_sub))));
    int tps;
    const long long grid = label_grid(B, N, p, tps);
    if (!grid) return set_error(VLG_ERR_SHAPE, "label_expand: B=%d N=%d L=%d needs more than 2^24 - 1 workgroups", B, N, L);
    const ExpandArgs a{phi, dir ? v : nullptr, dir ? v_sub : nullptr, lengths, N, L, p.lgG, tps, semiring, mode, arc, best, g1, g2, dbar, scale,
                       scale_stride, out, (unsigned)grid, (hipStream_t)stream};
    if (in_dtype == VLG_F32) return launch_expand_v<F32In, float, 4>(p.vec, v_dtype, a);
    return out_dtype == VLG_F32 ? launch_expand_v<BF16In, float, 8>(p.vec, v_dtype, a) : launch_expand_v<BF16In, uint16_t, 8>(p.vec, v_dtype, a);
}

int vlg_label_draw(const void* phi, const float* arc, const int64_t* heads, const int64_t* lengths, int B, int N, int L, int S, int in_dtype,
                   const uint64_t* rng, unsigned site, const float* u_label, int64_t* labels, float* logp, void* stream) {
    using namespace vlg;
    if (int e = check_label_args("label_draw", B, N, L, in_dtype, VLG_SR_LOG)) return e;
    if (S < 1) return set_error(VLG_ERR_SHAPE, "label_draw: need S >= 1 samples (got %d)", S);
    if (B == 0) return 0;
    if ((rng != nullptr) == (u_label != nullptr))
        return set_error(VLG_ERR_ARG, "label_draw: pass exactly one of rng (counter-based draws) and u_label (explicit uniforms)");
    if (!phi || !heads || !labels) return set_error(VLG_ERR_ARG, "label_draw: null buffer (phi, heads and labels are required)");
    if (logp && !arc) return set_error(VLG_ERR_ARG, "label_draw: logp needs the folded arc scores");
    const long long grid = ((long long)S * B + kDrawWaves - 1) / kDrawWaves;
    if (grid > kLabelMaxGrid) return set_error(VLG_ERR_SHAPE, "label_draw: S=%d B=%d needs more than 2^24 - 1 workgroups", S, B);
    if (in_dtype == VLG_F32)
        return launch("label_draw_kernel", label_draw_kernel<F32In>, dim3((unsigned)grid), dim3(kLabelThreads), 0, (hipStream_t)stream,
                      (const float*)phi, arc, (const long long*)heads, lengths, B, N, L, S, rng, site, u_label, (long long*)labels, logp);
    return launch("label_draw_kernel", label_draw_kernel<BF16In>, dim3((unsigned)grid), dim3(kLabelThreads), 0, (hipStream_t)stream,
                  (const uint16_t*)phi, arc, (const long long*)heads, lengths, B, N, L, S, rng, site, u_label, (long long*)labels, logp);
}

}  // extern "C"
