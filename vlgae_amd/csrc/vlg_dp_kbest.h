// vlg_dp_kbest.h -- the K best projective single-root trees of a DepTree CRF (DependencyCRF.kbest_heads / kbest_scores).
//
// Like vlg_dp_sample.h: per-lane / per-group / per-wave bodies written against a policy X, shared by the gfx950 kernel
// (vlg_kbest.hip) and the host emulator of the CPU test-suite (tests/emu/emu_kbest.cpp).  Nothing here is a CPU fallback.
// The valence DMV's kernel (vlg_dmv_kbest.h) takes from here what does not depend on the model: the plan, the candidate lists, the
// walk's entry packing, start, back-pointer checks and finish, and the count.  Each model keeps its span body
// with the KC extraction rounds at its end, its span-width loop, and the loop of its walk, which reads a cell's back-pointer, names
// its children and steps: written once over both they moved SGPR counts and spills of the images or cost the DepTree kernel time
// (profiles/kbest_frame_neutrality.md).
//
// Chart geometry is DepCtx's (vlg_dp_core.h), with KC values per cell instead of one, sorted in descending order; KC is the
// compile-time image that serves the caller's K (kbest_image).  Rank k of cell x lives at chart[k * cells + x] ("rank planes"): the
// lanes of a group read neighbouring cells of one plane, as the single-value kernels do.  Values are plain sums of the clamped input
// potentials in natural units -- additions and comparisons only, so they are exact wherever the partial sums are representable.
//
//   T(lo,hi)[.]   = top-KC over r, p, q of CR(lo,lo+r)[p] + CL(hi,lo+r+1)[q]      r in [0,w)    IL = T + arc[hi,lo], IR = T + arc[lo,hi]
//   CL(hi->lo)[.] = top-KC of CL(lo+r,lo)[p] + IL(hi,lo+r)[q]                     r in [0,w)    (r = 0 reads the IL of this very span)
//   CR(lo->hi)[.] = top-KC of IR(lo,lo+1+r)[p] + CR(lo+1+r,hi)[q]                 r in [0,w)    (r = w-1 reads the IR of this very span)
//   CR(0,w) is empty unless w == len (single root, deptree.py:70-75); a trivial cell C(h,h) has ONE derivation (rank 0, value 0).
//
// TOTAL ORDER.  Candidates of a cell are ordered by (value descending, then the packed back-pointer r << 8 | p << 4 | q ascending).
// Every derivation of a cell is one (r, p, q) triple, so the order is total, the K derivations taken are K different trees also under
// exact ties, and nothing is ever de-duplicated by value or recovered by "first split whose sum matches".  For one split only the pairs
// with (p+1)(q+1) <= KC can reach the top KC: (p,q) is preceded by the (p+1)(q+1) - 1 pairs (p' <= p, q' <= q) of the same split --
// their values are at least as large and their packed pointers smaller, so the order puts them first under ties as well.  That is 8
// pairs at KC = 4, 20 at 8, 50 at 16.  Because the order does not depend on KC, the list of a smaller K is a prefix of a larger K's.
//
// A rank that does not exist (fewer derivations than KC, or only through forbidden arcs) holds a value <= VLG_NEGINF + (a sum of
// potentials): at or below 0.5 VLG_NEGINF, where the output stage stops counting.  Their back-pointers are never walked.
#pragma once
#include "vlg_dp_core.h"

namespace vlg {

constexpr int kKbestMaxK = 16;
constexpr int kKbestStack = 32;       // ints per wavefront: the walk leaves at most 8 cells pending (vlg_dp_sample.h) and checks
constexpr int kKbestWaves = 8;        // wavefronts that share the ranks of one sentence (kThreads / 64)
constexpr int kKbestPadBp = 0xffff;   // back-pointer of a list slot that holds no candidate (r = 255 never occurs: r < w <= 254)

VLG_HOSTDEV int kbest_image(int K) { return K <= 1 ? 1 : K <= 2 ? 2 : K <= 4 ? 4 : K <= 8 ? 8 : 16; }

// ---- placement ------------------------------------------------------------------------------------------------------------------
// 0: everything in LDS   1: the two back-pointer charts in the workspace (written once, read only by the walk)   2: the value charts
// too.  The walk's stacks always sit in LDS.
#if defined(__HIPCC__)
#define VLG_KB_INLINE __host__ __device__ __forceinline__   // inlined into the kernels: the carve stays in scalar registers
#else
#define VLG_KB_INLINE inline
#endif
struct KbestLayout {
    Region C, I, bT, bC, stack;
    size_t lds_bytes, ws_bytes;
    VLG_KB_INLINE KbestLayout(int N, int KC, int mode) {
        const size_t cells = (size_t)N * chart_pitch(N);
        Carver k;
        C = k.take(cells * KC * 4, mode < 2);
        I = k.take(cells * KC * 4, mode < 2);
        bT = k.take(cells * KC * 2, mode < 1);
        bC = k.take(cells * KC * 2, mode < 1);
        stack = k.take((size_t)kKbestWaves * kKbestStack * sizeof(int), true);
        lds_bytes = k.lds;
        ws_bytes = k.ws;
    }
};

struct KbestPlan { int KC, mode; size_t lds_bytes, ws_stride; };   // code image; placement; dynamic LDS; workspace bytes per sentence

// the one place that chooses: the first placement of a Layout (KbestLayout, DmvKbestLayout) that fits the LDS (the launchers, the
// size queries and the emulators all ask here)
template <typename Layout>
VLG_HOSTDEV KbestPlan kbest_plan_of(int N, int K, size_t lds_budget) {
    const int KC = kbest_image(K);
    int mode = 0;
    while (mode < 2 && Layout(N, KC, mode).lds_bytes > lds_budget) ++mode;
    const Layout L(N, KC, mode);
    return KbestPlan{KC, mode, L.lds_bytes, L.ws_bytes};
}

VLG_HOSTDEV KbestPlan kbest_plan(int N, int K, size_t lds_budget) { return kbest_plan_of<KbestLayout>(N, K, lds_budget); }

struct KbCtx {
    int Ne, len, P, cells;   // cells = N * P: the distance between two rank planes
    float* C;
    float* I;                // plane 0 is pre-loaded with the arc scores
    unsigned short* bT;      // back-pointers of T(lo,hi) at [lo][hi] -- serve IL(hi,lo) and IR(lo,hi) alike
    unsigned short* bC;      // back-pointers of the complete cells, indexed as C
};

// potentials of one sentence, fp32 or bf16 (chosen at run time: only the load stage reads them)
struct KbArc {
    const void* p;
    size_t base;
    int bf16;
    VLG_HDM float ld(size_t i) const {
        return bf16 ? BF16In::ld((const uint16_t*)p, base + i) : F32In::ld((const float*)p, base + i);
    }
};

// ---- a lane's candidate list: KC (value, back-pointer) pairs in the total order, in registers (every index is a compile-time constant)
template <int KC>
struct KbList {
    float v[KC];
    int b[KC];
};

VLG_HD bool kb_before(float v, int b, float v2, int b2) { return v > v2 || (v == v2 && b < b2); }

template <int KC>
VLG_HD void kb_clear(KbList<KC>& l) {
#pragma unroll
    for (int j = 0; j < KC; ++j) { l.v[j] = VLG_LOWEST; l.b[j] = kKbestPadBp; }
}

template <int KC>
VLG_HD void kb_insert(KbList<KC>& l, float v, int b) {
#pragma unroll
    for (int j = 0; j < KC; ++j) {
        const bool t = kb_before(v, b, l.v[j], l.b[j]);
        const float ov = l.v[j];
        const int ob = l.b[j];
        l.v[j] = t ? v : ov;
        l.b[j] = t ? b : ob;
        v = t ? ov : v;   // the displaced pair moves on: it precedes everything below it
        b = t ? ob : b;
    }
}

// the candidates of split r: a[p] + b[q] over the pairs that can reach the top KC
template <int KC>
VLG_HD void kb_split(KbList<KC>& l, const float* a, const float* b, int r) {
#pragma unroll
    for (int p = 0; p < KC; ++p) {
#pragma unroll
        for (int q = 0; q < KC; ++q) {
            if ((p + 1) * (q + 1) <= KC) {
                const float v = a[p] + b[q];
                const int bp = r << 8 | p << 4 | q;
                if (kb_before(v, bp, l.v[KC - 1], l.b[KC - 1])) kb_insert<KC>(l, v, bp);
            }
        }
    }
}

// One span, one direction (dir 0: T -> IL(j,i) -> CL(j,i); dir 1: T -> IR(i,j) -> CR(i,j)), by the G lanes of its group: phase 0
// merges T, phase 1 the complete cell.  Both directions need T; each computes it (same lanes, same order: same bits), dir 0 stores
// its back-pointers.  Phase 1 reads the IL / IR of this very span at one split (r = 0 | w-1): the lane that owns that split is the
// one that stores the span's cells, so it reads back its own stores and no other lane of the width reads them.  Every extracted rank
// goes straight to the charts: only the list and one split's operands live in registers.
template <int KC, typename X>
VLG_HD void kbest_span(const KbCtx& c, int w, int G, int D, bool live, int rr, int dir, X& x) {
    const int P = c.P, cells = c.cells, DW = D + VLG_MUL24(w, P);
    const int kO = dir == 0 ? DW : D + w + 1;   // own slot: IL(j,i) / CL(j,i) | IR(i,j) / CR(i,j)
    const float aX = c.I[kO];                   // arc score, staged at load
    const bool writer = live && rr == (dir == 0 ? 0 : (w - 1) & (G - 1));
    const bool masked = dir == 1 && D == 0 && w != c.len;   // deptree.py:71-72
#pragma unroll 1
    for (int phase = 0; phase < 2; ++phase) {
        const float *pa, *pb;   // operand p of split r at pa[r sa + k cells], operand q at pb[r sb + k cells]
        int sa = 1, sb = 1;
        if (phase == 0) { pa = c.C + D + 1; pb = c.C + DW + 1; }                    // CR(i,i+r), CL(j,i+r+1)
        else if (dir == 0) { pa = c.C + D; sa = P; pb = c.I + DW; }                 // CL(i+r,i), IL(j,i+r)
        else { pa = c.I + D + 2; pb = c.C + D + P + w + 1; sb = P; }                // IR(i,i+1+r), CR(i+1+r,j)
        KbList<KC> l;
        kb_clear<KC>(l);
#pragma unroll 1
        for (int r = rr; r < w; r += G) {
            float a[KC], b[KC];
            const int oa = VLG_MUL24(r, sa), ob = VLG_MUL24(r, sb);
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                a[k] = pa[oa + k * cells];
                b[k] = pb[ob + k * cells];
            }
            kb_split<KC>(l, a, b, r);
        }
        // KC extraction rounds: the group's best list head (value, then the smaller back-pointer) leaves its lane's list
        float* const ov = phase == 0 ? c.I + kO : c.C + kO;
        unsigned short* const ob = phase == 0 ? c.bT + D + w : c.bC + kO;
        const bool st_bp = writer && (phase == 1 || dir == 0);
        const float add = phase == 0 ? aX : 0.f;   // deptree.py:58,62
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            float m = l.v[0];
            int am = l.b[0];
            x.template allreduce_argmax<1>(&m, &am, G);
            if (l.b[0] == am && l.v[0] == m) {
#pragma unroll
                for (int j = 0; j + 1 < KC; ++j) { l.v[j] = l.v[j + 1]; l.b[j] = l.b[j + 1]; }
                l.v[KC - 1] = VLG_LOWEST;
                l.b[KC - 1] = kKbestPadBp;
            }
            const float v = (m < -1e37f || (phase == 1 && masked)) ? VLG_NEGINF : m + add;   // no candidate left: the semiring zero
            if (writer) ov[k * cells] = v;
            if (st_bp) ob[k * cells] = (unsigned short)am;
        }
    }
}

// The charts of one sentence: load stage and the span-width loop, one barrier per width; tid of nt lanes, nt a power of two >= 2.
// The first half of the lanes takes direction 0 of every span, the second half direction 1 (as dep_fw_segment).
template <int KC, typename X>
VLG_HD void kbest_fill(const KbCtx& c, const KbArc& arc, int N, int tid, int nt, X& x) {
    const int Ne = c.Ne, P = c.P, cells = c.cells;
    for (int i = tid; i < Ne * P; i += nt) {
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            c.C[i + k * cells] = VLG_NEGINF;
            c.I[i + k * cells] = VLG_NEGINF;
        }
    }
    x.sync();
    for (int idx = tid; idx < Ne * Ne; idx += nt) {
        const int h = idx / Ne, ch = idx - h * Ne;
        if (ch == h) {
            c.C[h * P + h] = 0.f;   // rank 0 of the trivial cells; their further ranks stay empty
            c.C[h * P + h + 1] = 0.f;
        } else {
            const float a = pot_clamp(arc.ld((size_t)h * N + ch));
            if (ch < h) c.I[h * P + ch] = a;
            else c.I[h * P + ch + 1] = a;
        }
    }
    x.sync();
    const int nd = nt >> 1;
    const bool right = x.uniform(tid >= nd);
    const int t = right ? tid - nd : tid;
    for (int w = 1; w < Ne; ++w) {
        const int spans = Ne - w, lg = group_log2(spans, w, nd, nd), G = 1 << lg;
        const int per = nd >> lg, rr = t & (G - 1), slot = t >> lg;
        for (int base = 0; base < spans; base += per) {
            const bool live = base + slot < spans;
            const int i = live ? base + slot : 0;
            kbest_span<KC>(c, w, G, VLG_MUL24(i, P + 1), live, rr, right ? 1 : 0, x);
        }
        x.sync();
    }
}

// ---- the walk: rank k of one sentence, by one wavefront (its control flow is wave-uniform; lane 0 writes the heads).  heads: the N
// int64 of this (rank, sentence); score: its cell; stack: kKbestStack ints of this wave.  Behind the last barrier of the fill the
// charts are read-only.  A rank that does not exist gets heads 0 and VLG_NEGINF and is not walked.  The walk visits every non-trivial
// cell of the tree once (at most 3 len + 1); width-0 leaves are not pushed.  After 4 N visits, on a back-pointer that does not fit
// its cell or on a full stack it gives up -- heads 0, score NaN -- so that no chart contents can make it spin or read outside the
// charts.  A model's walk (kbest_walk here, dmv_kbest_walk) reads the back-pointer of a cell, names its two children, descends into
// the narrower one and leaves the wider one pending; the entry packing, the start, the checks of a back-pointer and the finish are the
// ones below.  (The descend / push / pop step stands in each walk: as the samplers' sample_order / sample_step it cost the DepTree
// walk 4 us of 105 at B = 256, N = 41, K = 1, profiles/kbest_frame_neutrality.md.)

// walk entries: 0 = IL(hi -> lo), 1 = CL(hi -> lo), 2 = CR(lo -> hi), 3 = IR(lo -> hi), with the rank of the cell's derivation and,
// where the model has one, its valence
VLG_HD int kbest_entry(int kind, int lo, int hi, int rank, int v = 0) { return kind | (lo << 2) | (hi << 10) | (rank << 18) | (v << 22); }
VLG_HD int kbest_entry_width(int e) { return ((e >> 10) & 255) - ((e >> 2) & 255); }

// s: the value of rank k of the root cell.  False where the rank does not exist: heads 0, score VLG_NEGINF.  Else the heads of the
// positions that are no word are 0 -- every word 1 ... len gets its head from the walk: one writer per element.
template <typename X>
VLG_HD bool kbest_walk_begin(float s, int len, int N, long long* heads, float* score, X& x) {
    const bool exists = s > 0.5f * VLG_NEGINF;
    for (int i = x.lane(); i < N; i += X::kWave)
        if (!exists || i == 0 || i > len) heads[i] = 0;
    if (!exists && x.lane() == 0) *score = VLG_NEGINF;
    return exists;
}

// the back-pointer r << 8 | p << 4 | q fits a cell of width w in the image KC
template <int KC>
VLG_HD bool kbest_bp_fits(int bp, int w) { return (bp >> 8) < w && ((bp >> 4) & 15) < KC && (bp & 15) < KC; }

// a child entry of width w names a rank its cell can have: a trivial cell has rank 0 only
VLG_HD bool kbest_child_fits(int e, int w) { return w != 0 || ((e >> 18) & 15) == 0; }

// the end of a walk: the score s, or -- it gave up -- heads 0 and score NaN
VLG_HD void kbest_walk_finish(bool ok, float s, int N, long long* heads, float* score, int lane) {
    if (lane == 0) {
        if (!ok)
            for (int i = 0; i < N; ++i) heads[i] = 0;   // one lane, in program order behind its own stores above
        *score = ok ? s : VLG_BITS2F(0x7fc00000u);
    }
}

template <int KC, typename X>
VLG_HD void kbest_walk(const KbCtx& c, int k, int N, int* stack, long long* heads, float* score, X& x) {
    const int len = c.len, P = c.P, cells = c.cells, lane = x.lane();
    const float s = c.C[len + 1 + k * cells];   // CR(0,len)[k]
    if (!kbest_walk_begin(s, len, N, heads, score, x)) return;
    int top = 0, visits = 0;
    bool ok = true;
    int e = kbest_entry(2, 0, len, k);
    for (;;) {
        const int kind = e & 3, lo = (e >> 2) & 255, hi = (e >> 10) & 255, rk = (e >> 18) & 15;
        if (++visits > 4 * N) { ok = false; break; }
        const int w = hi - lo, D = lo * (P + 1), ko = rk * cells;
        const bool inc = kind == 0 || kind == 3;
        int bp;
        if (inc) {
            if (lane == 0) heads[kind == 0 ? lo : hi] = kind == 0 ? hi : lo;
            bp = c.bT[D + w + ko];
        } else if (kind == 1) {
            bp = c.bC[hi * P + lo + ko];
        } else {
            bp = c.bC[D + w + 1 + ko];
        }
        bp = x.uniform(bp);
        if (!kbest_bp_fits<KC>(bp, w)) { ok = false; break; }
        const int r = bp >> 8, p = (bp >> 4) & 15, q = bp & 15;
        int ea, eb;   // the two children
        if (inc) { ea = kbest_entry(2, lo, lo + r, p); eb = kbest_entry(1, lo + r + 1, hi, q); }
        else if (kind == 1) { ea = kbest_entry(1, lo, lo + r, p); eb = kbest_entry(0, lo + r, hi, q); }
        else { ea = kbest_entry(3, lo, lo + 1 + r, p); eb = kbest_entry(2, lo + 1 + r, hi, q); }
        int wa = kbest_entry_width(ea), wb = kbest_entry_width(eb);
        if (!kbest_child_fits(ea, wa) || !kbest_child_fits(eb, wb)) { ok = false; break; }
        if (wa > wb) { const int te = ea; ea = eb; eb = te; const int tw = wa; wa = wb; wb = tw; }   // ea: the narrower one
        if (wa > 0) {
            if (top >= kKbestStack) { ok = false; break; }
            stack[top++] = eb;   // (wb >= wa > 0)
            e = ea;
        } else if (wb > 0) {
            e = eb;
        } else {
            if (top == 0) break;
            e = x.uniform(stack[--top]);
        }
    }
    kbest_walk_finish(ok, s, N, heads, score, lane);
}

// how many of the first K ranks exist; rank k of the root cell at C[root + k stride]
VLG_HD int kbest_count_at(const float* C, int root, int stride, int K) {
    int n = 0;
    for (int k = 0; k < K; ++k) n += C[root + k * stride] > 0.5f * VLG_NEGINF ? 1 : 0;
    return n;
}
VLG_HD int kbest_count(const KbCtx& c, int K) { return kbest_count_at(c.C, c.len + 1, c.cells, K); }   // CR(0,len)[k]

}  // namespace vlg
