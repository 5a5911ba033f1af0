// vlg_rules1o.hip -- the gold tree's DMV1o rule counts on the device (gfx950): what the parser's rule-supervised initialisation epochs
// train on (src/model/ldndmv.py:262-275, `init_method: 'y'`).  The reference builds the counts on the host, per sentence, with
// generate_rule_1o (src/model/dmv_helper/good_init_nn.py:34-77, wired at ldndmv.py:153-159), pads them as float64 arrays
// (LinearPadder / SquarePadder) and takes enll = -(dec_rule . dec) - (attach_rule . attach) - (root_rule . root).  Here:
//
//   gold_rules_kernel        the three padded tables, bit-equal to generate_rule_1o + the padders (f32 or f64)
//   gold_score_kernel        per-sentence score sum(counts . potentials) read off the ROOT-MERGED potentials (md[:,1:] = dec,
//                            ma[:,1:,1:] = attach, ma[:,0,1:,NOCHILD] = root; distributions.py:253-265), only where a count is nonzero
//   gold_score_grad_kernel   its adjoint g[b] * counts in the merged layout, every element written (no memset, no scatter)
//
// Counting rules (dmv.py:7-12: HASCHILD 0, NOCHILD 1, LEFT 0, RIGHT 1, GO 0, STOP 1).  Word c of a sentence of n words has head
// h = arc[c] - 1 (-1 = the root); it is a LEFT child when c < h, else a RIGHT child; its valence is NOCHILD when it is h's outermost
// child on that side (leftmost left child / rightmost right child), else HASCHILD:
//   h >= 0:     attach[h,c,v] += 1, dec[h,dir,v,GO] += 1
//   every c:    dec[c,LEFT,  c has no left child  ? NOCHILD : HASCHILD, STOP] += 1, the same for RIGHT
//   root:       root[c0] = 1 for the FIRST c0 with arc = 0
//   h == -1:    dec[n-1, RIGHT, c == n-1 ? NOCHILD : HASCHILD, GO] += 1 -- the reference indexes decision[-1] (its valence test reads
//               right_most_child[-1], which is always n-1); reproduced exactly
// Non-projective trees, cycles, several roots and self-loops are counted as above (the reference's projectivity filter drops nothing:
// task/dep.py:72 discards its result).  A sentence with an arc outside [0, n], without any 0, or whose length is outside [1, width] is
// INVALID (the reference raises or mis-indexes): zero counts, score NaN -- the convention of vlg_dmv1o_rules.
//
// One workgroup per sentence, n <= 254 words (one thread per word): the arc vector, the outermost children and the count rows live in
// LDS; every reduction runs in a fixed order (no atomics): the same bits on every run.  Plain vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vlg_common.h"
#include "vlg_launch.h"

namespace vlg {

constexpr int kGoldThreads = 256;
constexpr int kGoldMaxWords = 254;   // N = n + 1 <= 255, as for the DP

struct GoldTree {
    int head[kGoldThreads];          // head of word c (-1 = root); valid for c < n
    int val[kGoldThreads];           // valence of word c's attachment (HASCHILD 0 / NOCHILD 1)
    int lmc[kGoldThreads], rmc[kGoldThreads];
    float dec[kGoldThreads][8];      // dec counts of word h, [dir][val][decision]
    int n;                           // 0 for an invalid sentence
    int c0;                          // first root child
    int wave_c0[kGoldThreads / 64];  // first root child per wavefront
};

// Everything the three kernels need from one sentence, in LDS.  `width` = the largest length the caller's layout holds.
__device__ __forceinline__ void gold_tree(const int64_t* __restrict__ arc, int ld_arc, const int64_t* __restrict__ lengths, int width,
                                          GoldTree& s) {
    const int b = blockIdx.x, t = threadIdx.x;
    const long long nl = lengths[b];
    const int n0 = (nl >= 1 && nl <= width && nl <= ld_arc) ? (int)nl : 0;
    bool bad = false, root = false;
    if (t < n0) {
        const long long a = arc[(size_t)b * ld_arc + t];
        bad = a < 0 || a > n0;
        root = a == 0;
        s.head[t] = bad ? -1 : (int)a - 1;
    }
    const unsigned long long roots = __ballot(root);   // the first root child: per wavefront here, across them below
    if ((t & 63) == 0) s.wave_c0[t >> 6] = roots ? (t & ~63) + __ffsll((long long)roots) - 1 : kGoldThreads;
    const int any_bad = __syncthreads_or(bad);
    const int any_root = __syncthreads_or(root);
    const int n = (n0 > 0 && !any_bad && any_root) ? n0 : 0;
    // outermost children of word t (itself when it has none on that side; a self-loop changes neither)
    int lm = t, rm = t;
    if (t < n) {
#pragma unroll 8
        for (int c = 0; c < n; ++c) {
            if (s.head[c] != t) continue;
            if (c < t) lm = c < lm ? c : lm;
            else rm = c > rm ? c : rm;
        }
        s.lmc[t] = lm;
        s.rmc[t] = rm;
    }
    if (t == 0) {
        int c0 = kGoldThreads;
#pragma unroll
        for (int w = 0; w < kGoldThreads / 64; ++w) c0 = s.wave_c0[w] < c0 ? s.wave_c0[w] : c0;
        s.c0 = n > 0 ? c0 : -1;
        s.n = n;
    }
    __syncthreads();
    if (t < n) {
        float* cnt = s.dec[t];   // word t's own row (a register array indexed by (dir, valence) would live in scratch)
#pragma unroll
        for (int k = 0; k < 8; ++k) cnt[k] = 0.f;
        // GO decisions of word t as a head (second pass: the outermost children are known now)
#pragma unroll 8
        for (int c = 0; c < n; ++c) {
            const int h = s.head[c];
            if (h == t) {
                const int d = c < t ? 0 : 1;
                const int v = (d == 0 ? lm == c : rm == c) ? 1 : 0;
                cnt[d * 4 + v * 2] += 1.f;
            } else if (h == -1 && t == n - 1) {   // decision[-1][RIGHT][...][GO] of every root child
                cnt[4 + (c == n - 1 ? 2 : 0)] += 1.f;
            }
        }
        cnt[0 * 4 + (lm == t ? 1 : 0) * 2 + 1] += 1.f;   // STOP, LEFT
        cnt[1 * 4 + (rm == t ? 1 : 0) * 2 + 1] += 1.f;   // STOP, RIGHT
        const int h = s.head[t];
        s.val[t] = h < 0 ? 0 : ((t < h ? s.lmc[h] == t : s.rmc[h] == t) ? 1 : 0);
    }
    __syncthreads();
}

// count of attach[h, c, v] (h, c word indices) -- one attachment per child
__device__ __forceinline__ float attach_count(const GoldTree& s, int h, int c, int v) {
    return (c < s.n && s.head[c] == h && s.val[c] == v) ? 1.f : 0.f;
}

template <typename T> struct Vec2;
template <> struct Vec2<float> { using type = float2; };
template <> struct Vec2<double> { using type = double2; };

template <typename T>
__global__ __launch_bounds__(kGoldThreads) void gold_rules_kernel(const int64_t* __restrict__ arc, int ld_arc, const int64_t* __restrict__ lengths,
                                                                  int L, T* __restrict__ dec_rule, T* __restrict__ attach_rule,
                                                                  T* __restrict__ root_rule) {
    __shared__ GoldTree s;
    gold_tree(arc, ld_arc, lengths, L, s);
    using V2 = typename Vec2<T>::type;
    const size_t b = blockIdx.x;
    const int n = s.n;
    for (int h = threadIdx.x; h < L; h += kGoldThreads) {
        V2* row = reinterpret_cast<V2*>(dec_rule + (b * L + h) * 8);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            V2 w;
            w.x = h < n ? (T)s.dec[h][2 * k] : (T)0;
            w.y = h < n ? (T)s.dec[h][2 * k + 1] : (T)0;
            row[k] = w;
        }
        root_rule[b * L + h] = (T)(h == s.c0 ? 1 : 0);
    }
    V2* att = reinterpret_cast<V2*>(attach_rule + b * L * L * 2);
    for (int p = threadIdx.x; p < L * L; p += kGoldThreads) {
        const int h = p / L, c = p - h * L;
        V2 w;
        w.x = (T)attach_count(s, h, c, 0);
        w.y = (T)attach_count(s, h, c, 1);
        att[p] = w;
    }
}

struct F32Load {
    using T = float;
    static __device__ __forceinline__ float ld(const float* p, size_t i) { return p[i]; }
};
struct BF16Load {
    using T = uint16_t;
    static __device__ __forceinline__ float ld(const uint16_t* p, size_t i) { return __uint_as_float((unsigned)p[i] << 16); }
};

template <typename In>
__global__ __launch_bounds__(kGoldThreads) void gold_score_kernel(const typename In::T* __restrict__ md, const typename In::T* __restrict__ ma,
                                                                  const int64_t* __restrict__ arc, int ld_arc, const int64_t* __restrict__ lengths,
                                                                  int N, float* __restrict__ score) {
    __shared__ GoldTree s;
    __shared__ double part[kGoldThreads / 64];
    gold_tree(arc, ld_arc, lengths, N - 1, s);
    const size_t b = blockIdx.x;
    const int t = threadIdx.x;
    double acc = 0.0;
    if (t < s.n) {   // word t: its dec row, its own attachment, the root arc if it is the first root child
        const size_t r = (b * N + 1 + t) * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float c = s.dec[t][k];
            if (c != 0.f) acc += (double)c * (double)In::ld(md, r + k);
        }
        const int h = s.head[t];
        if (h >= 0) acc += (double)In::ld(ma, ((b * N + 1 + h) * N + 1 + t) * 2 + s.val[t]);
        if (t == s.c0) acc += (double)In::ld(ma, (b * N * N + 1 + t) * 2 + 1);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);   // (the same butterfly on every run: fixed order)
    if ((t & 63) == 0) part[t >> 6] = acc;
    __syncthreads();
    if (t == 0) score[b] = s.n > 0 ? (float)(((part[0] + part[1]) + part[2]) + part[3]) : __builtin_nanf("");
}

template <typename Out> struct Store;
template <> struct Store<float> {
    static __device__ __forceinline__ void row8(float* p, const float* v) {
        reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
    }
    static __device__ __forceinline__ void pair(float* p, float a, float b) { *reinterpret_cast<float2*>(p) = make_float2(a, b); }
};
template <> struct Store<__bf16> {
    static __device__ __forceinline__ unsigned bits(float x) { const __bf16 h = (__bf16)x; return (unsigned)__builtin_bit_cast(uint16_t, h); }
    static __device__ __forceinline__ void row8(__bf16* p, const float* v) {
        uint4 w;
        w.x = bits(v[0]) | (bits(v[1]) << 16);
        w.y = bits(v[2]) | (bits(v[3]) << 16);
        w.z = bits(v[4]) | (bits(v[5]) << 16);
        w.w = bits(v[6]) | (bits(v[7]) << 16);
        *reinterpret_cast<uint4*>(p) = w;
    }
    static __device__ __forceinline__ void pair(__bf16* p, float a, float b) { *reinterpret_cast<unsigned*>(p) = bits(a) | (bits(b) << 16); }
};

template <typename Out>
__global__ __launch_bounds__(kGoldThreads) void gold_score_grad_kernel(const int64_t* __restrict__ arc, int ld_arc, const int64_t* __restrict__ lengths,
                                                                       int N, const float* __restrict__ g, int g_stride, Out* __restrict__ grad_md,
                                                                       Out* __restrict__ grad_ma) {
    __shared__ GoldTree s;
    gold_tree(arc, ld_arc, lengths, N - 1, s);
    const size_t b = blockIdx.x;
    const float gs = g[b * g_stride];
    for (int r = threadIdx.x; r < N; r += kGoldThreads) {   // merged dec row r = word r - 1; row 0 (the root) has no count
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = gs * ((r >= 1 && r - 1 < s.n) ? s.dec[r - 1][k] : 0.f);
        Store<Out>::row8(grad_md + (b * N + r) * 8, v);
    }
    Out* ga = grad_ma + b * N * N * 2;
    for (int p = threadIdx.x; p < N * N; p += kGoldThreads) {   // merged attach (head row, child column); column 0 is never a child
        const int hr = p / N, cc = p - hr * N;
        float c0 = 0.f, c1 = 0.f;
        if (cc >= 1) {
            if (hr == 0) c1 = cc - 1 == s.c0 ? 1.f : 0.f;
            else {
                c0 = attach_count(s, hr - 1, cc - 1, 0);
                c1 = attach_count(s, hr - 1, cc - 1, 1);
            }
        }
        Store<Out>::pair(ga + (size_t)p * 2, gs * c0, gs * c1);
    }
}

}  // namespace vlg

extern "C" {

int vlg_dmv1o_gold_rules(const int64_t* arc, int ld_arc, const int64_t* lengths, int B, int L, int out_dtype, void* dec_rule, void* attach_rule,
                         void* root_rule, void* stream) {
    using namespace vlg;
    if (B < 0 || L < 1 || L > kGoldMaxWords || ld_arc < 1)
        return set_error(VLG_ERR_SHAPE, "dmv1o_gold_rules: need B >= 0, 1 <= L <= %d and ld_arc >= 1 (got B=%d L=%d ld_arc=%d)", kGoldMaxWords,
                         B, L, ld_arc);
    if (out_dtype != VLG_F32 && out_dtype != VLG_F64) return set_error(VLG_ERR_DTYPE, "dmv1o_gold_rules: out_dtype %d (VLG_F32 or VLG_F64)", out_dtype);
    if (B == 0) return 0;
    if (!arc || !lengths || !dec_rule || !attach_rule || !root_rule) return set_error(VLG_ERR_ARG, "dmv1o_gold_rules: null buffer");
    hipStream_t s = (hipStream_t)stream;
    if (out_dtype == VLG_F32)
        return launch("gold_rules_kernel", gold_rules_kernel<float>, dim3(B), dim3(kGoldThreads), 0, s, arc, ld_arc, lengths, L, (float*)dec_rule,
                      (float*)attach_rule, (float*)root_rule);
    else
        return launch("gold_rules_kernel", gold_rules_kernel<double>, dim3(B), dim3(kGoldThreads), 0, s, arc, ld_arc, lengths, L, (double*)dec_rule,
                      (double*)attach_rule, (double*)root_rule);
}

int vlg_dmv1o_gold_score(const void* merged_dec, const void* merged_attach, const int64_t* arc, int ld_arc, const int64_t* lengths, int B, int N,
                         int in_dtype, float* score, void* stream) {
    using namespace vlg;
    if (B < 0 || N < 2 || N > kGoldMaxWords + 1 || ld_arc < 1)
        return set_error(VLG_ERR_SHAPE, "dmv1o_gold_score: need B >= 0, 2 <= N <= 255 and ld_arc >= 1 (got B=%d N=%d ld_arc=%d)", B, N, ld_arc);
    if (in_dtype != VLG_F32 && in_dtype != VLG_BF16) return set_error(VLG_ERR_DTYPE, "dmv1o_gold_score: in_dtype %d", in_dtype);
    if (B == 0) return 0;
    if (!merged_dec || !merged_attach || !arc || !lengths || !score) return set_error(VLG_ERR_ARG, "dmv1o_gold_score: null buffer");
    hipStream_t s = (hipStream_t)stream;
    if (in_dtype == VLG_F32)
        return launch("gold_score_kernel", gold_score_kernel<F32Load>, dim3(B), dim3(kGoldThreads), 0, s, (const float*)merged_dec, (const float*)merged_attach,
                      arc, ld_arc, lengths, N, score);
    else
        return launch("gold_score_kernel", gold_score_kernel<BF16Load>, dim3(B), dim3(kGoldThreads), 0, s, (const uint16_t*)merged_dec,
                      (const uint16_t*)merged_attach, arc, ld_arc, lengths, N, score);
}

int vlg_dmv1o_gold_score_backward(const int64_t* arc, int ld_arc, const int64_t* lengths, int B, int N, const float* g, int g_stride,
                                  int out_dtype, void* grad_dec, void* grad_attach, void* stream) {
    using namespace vlg;
    if (B < 0 || N < 2 || N > kGoldMaxWords + 1 || ld_arc < 1 || (g_stride != 0 && g_stride != 1))
        return set_error(VLG_ERR_SHAPE, "dmv1o_gold_score_backward: need B >= 0, 2 <= N <= 255, ld_arc >= 1, g_stride 0 or 1 (got B=%d N=%d "
                         "ld_arc=%d g_stride=%d)", B, N, ld_arc, g_stride);
    if (out_dtype != VLG_F32 && out_dtype != VLG_BF16) return set_error(VLG_ERR_DTYPE, "dmv1o_gold_score_backward: out_dtype %d", out_dtype);
    if (B == 0) return 0;
    if (!arc || !lengths || !g || !grad_dec || !grad_attach) return set_error(VLG_ERR_ARG, "dmv1o_gold_score_backward: null buffer");
    hipStream_t s = (hipStream_t)stream;
    if (out_dtype == VLG_F32)
        return launch("gold_score_grad_kernel", gold_score_grad_kernel<float>, dim3(B), dim3(kGoldThreads), 0, s, arc, ld_arc, lengths, N, g, g_stride,
                      (float*)grad_dec, (float*)grad_attach);
    else
        return launch("gold_score_grad_kernel", gold_score_grad_kernel<__bf16>, dim3(B), dim3(kGoldThreads), 0, s, arc, ld_arc, lengths, N, g, g_stride,
                      (__bf16*)grad_dec, (__bf16*)grad_attach);
}

}  // extern "C"
