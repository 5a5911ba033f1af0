// vlg_dmv_kbest.h -- the K best projective single-root trees of the valence DMV (DMV1o.kbest_heads / kbest_scores), and the adjoint of
// their scores (the derivation counts of given trees).
//
// The valence-aware sibling of vlg_dp_kbest.h, whose candidate lists, total order, pruning bound, placement scheme, count
// and walk frame (entry packing, start, back-pointer checks, finish) it reuses: per-lane
// / per-group / per-wave bodies written against a policy X, shared by the gfx950 kernels (vlg_dmv_kbest.hip) and the host emulator of
// the CPU test-suite (tests/emu/emu_dmv_kbest.cpp).  Nothing here is a CPU fallback.
//
// Cells carry a valence v (0 HASCHILD, 1 NOCHILD) and KC sorted values each, in rank planes.  Values are plain sums of the clamped
// input potentials in NATURAL units -- additions and comparisons only, no log2 scaling -- so they are exact wherever the partial sums
// are representable.  The rule is dmv.py:47-63 / dmv_sample_terms (vlg_dmv_sample.h), with i = lo, j = hi, r in [0,w):
//   TL(lo,hi)[.]     = top-KC over r, p, q of CR(lo,lo+r).NC[p] + CL(hi,lo+r+1).HC[q]
//   TR(lo,hi)[.]     = top-KC of              CR(lo,lo+r).HC[p] + CL(hi,lo+r+1).NC[q]
//   IL(hi->lo).v     = TL + A[hi][lo][v],  IR(lo->hi).v = TR + A[lo][hi][v],   A[h][c][v] = attach[h,c,v] + dec[h,dir,v,GO]
//   CL(hi->lo).v[.]  = top-KC of CL(lo+r,lo).NC[p] + IL(hi->lo+r).v[q]          (r = 0 reads the TL of this very span)
//   CR(lo->hi).v[.]  = top-KC of IR(lo->lo+1+r).v[p] + CR(lo+1+r,hi).NC[q]      (r = w-1 reads the TR of this very span)
//   CR(0,w) is empty unless w == len (dmv.py:63); a trivial cell C(h,h).v has ONE derivation: rank 0 = dec[h,dir,v,STOP].
// Unlike DepTree the two directions do not share a T (the valences of its operands differ), so each direction has its own T values and
// back-pointers.  Both valences of an incomplete cell keep T's order and T's back-pointers (the added term does not depend on the
// split), so they have no planes of their own: T is kept, A is staged once as one plane pair, and the sum is taken where it is read.
// The complete cells are merged per valence: their added term depends on r, so the merge order differs between the valences.  That is
// six merges per span (DepTree: four, two of them the shared T computed twice); each runs with ONE candidate list in registers -- the
// two valences of a side one after the other -- so an image needs the registers of the DepTree image of the same KC plus one add.
//
// TOTAL ORDER and pruning: vlg_dp_kbest.h's, unchanged -- (value descending, packed r << 8 | p << 4 | q ascending), pairs with
// (p+1)(q+1) <= KC.  The valences of a cell's children follow from its kind (dmv_sample_walk), so the 16-bit pointer needs none.  Every
// tree has exactly one derivation (the valence of every attachment is a function of the tree), so the K results are K different trees,
// also under exact ties.
#pragma once
#include "vlg_dp_kbest.h"

namespace vlg {

// ---- placement: as KbestLayout.  0: everything in LDS   1: the back-pointer charts in the workspace   2: the value charts (C, T and
// the staged A) too.  The walk's stacks always sit in LDS.
struct DmvKbestLayout {
    Region C, T, A, bT, bC, stack;
    size_t lds_bytes, ws_bytes;
    VLG_KB_INLINE DmvKbestLayout(int N, int KC, int mode) {
        const size_t cells = (size_t)N * chart_pitch(N);
        Carver k;
        C = k.take(cells * KC * 8, mode < 2);    // [rank][valence][cell] float
        T = k.take(cells * KC * 4, mode < 2);    // [rank][cell] float: TL(lo,hi) at [hi][lo], TR(lo,hi) at [lo][hi+1]
        A = k.take(cells * 8, mode < 2);         // [valence][cell] float, indexed as T
        bT = k.take(cells * KC * 2, mode < 1);   // indexed as T
        bC = k.take(cells * KC * 4, mode < 1);   // indexed as C
        stack = k.take((size_t)kKbestWaves * kKbestStack * sizeof(int), true);
        lds_bytes = k.lds;
        ws_bytes = k.ws;
    }
};

VLG_HOSTDEV KbestPlan dmv_kbest_plan(int N, int K, size_t lds_budget) { return kbest_plan_of<DmvKbestLayout>(N, K, lds_budget); }

struct DmvKbCtx {
    int Ne, len, P, cells;   // cells = N * P: the distance between two planes
    float* C;                // CL(h->l).v[k] at C[(2 k + v) cells + h P + l], CR(h->r).v[k] at ... + h P + r + 1
    float* T;
    float* A;                // A[v cells + x]
    unsigned short* bT;
    unsigned short* bC;
};

// potentials of one sentence, fp32 or bf16 (chosen at run time: only the load stage reads them)
struct DmvKbPot {
    const void *dec, *attach;
    size_t dec_base, att_base;
    int bf16;
    VLG_HDM float ld(const void* p, size_t i) const {
        return bf16 ? BF16In::ld((const uint16_t*)p, i) : F32In::ld((const float*)p, i);
    }
    VLG_HDM float ld_dec(size_t i) const { return pot_clamp(ld(dec, dec_base + i)); }
    VLG_HDM float ld_attach(size_t i) const { return pot_clamp(ld(attach, att_base + i)); }
};

// One span, one direction (dir 0: TL -> CL(j,i).HC -> CL(j,i).NC; dir 1: TR -> CR(i,j).HC -> CR(i,j).NC), by the G lanes of its
// group: three merges, one candidate list each.  The complete cell reads the T of this very span at one split (r = 0 | w-1): the lane
// that owns that split is the one that stores the span's cells, so it reads back its own stores and no other lane of the width reads
// them.  Every extracted rank goes straight to the charts.
template <int KC, typename X>
VLG_HD void dmv_kbest_span(const DmvKbCtx& c, int w, int G, int D, bool live, int rr, int dir, X& x) {
    const int P = c.P, cells = c.cells, DW = D + VLG_MUL24(w, P);
    const int kO = dir == 0 ? DW : D + w + 1;   // own slot: TL / CL(j,i) | TR / CR(i,j)
    const bool writer = live && rr == (dir == 0 ? 0 : (w - 1) & (G - 1));
    const bool masked = dir == 1 && D == 0 && w != c.len;   // dmv.py:63
#pragma unroll 1
    for (int phase = 0; phase < 3; ++phase) {
        // operand p of split r at pa[r sa + k ka], operand q at pb[r sb + k kb]; phase >= 1 adds A[v] to the incomplete operand
        const int v = phase - 1;
        const float *pa, *pb, *pA = c.A;
        int sa = 1, sb = 1, ka = 2 * cells, kb = 2 * cells;
        if (phase == 0) {                                 // CR(i,i+r).NC | HC, CL(j,i+r+1).HC | NC
            pa = c.C + D + 1 + (dir == 0 ? cells : 0);
            pb = c.C + DW + 1 + (dir == 0 ? 0 : cells);
        } else if (dir == 0) {                            // CL(i+r,i).NC, TL(i+r,j) + A[v][j][i+r]
            pa = c.C + D + cells; sa = P;
            pb = c.T + DW; kb = cells;
            pA = c.A + DW + v * cells;
        } else {                                          // TR(i,i+1+r) + A[v][i][i+1+r], CR(i+1+r,j).NC
            pa = c.T + D + 2; ka = cells;
            pA = c.A + D + 2 + v * cells;
            pb = c.C + D + P + w + 1 + cells; sb = P;
        }
        KbList<KC> l;
        kb_clear<KC>(l);
#pragma unroll 1
        for (int r = rr; r < w; r += G) {
            float a[KC], b[KC];
            const int oa = VLG_MUL24(r, sa), ob = VLG_MUL24(r, sb);
            const float add = phase == 0 ? 0.f : pA[r];
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                a[k] = pa[oa + k * ka];
                b[k] = pb[ob + k * kb];
            }
            if (phase != 0) {
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    if (dir == 0) b[k] += add;
                    else a[k] += add;
                }
            }
            kb_split<KC>(l, a, b, r);
        }
        // KC extraction rounds: the group's best list head (value, then the smaller back-pointer) leaves its lane's list
        float* const ov = phase == 0 ? c.T + kO : c.C + kO + v * cells;
        unsigned short* const ob = phase == 0 ? c.bT + kO : c.bC + kO + v * cells;
        const int ko = phase == 0 ? cells : 2 * cells;
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
            const float val = (m < -1e37f || (phase != 0 && masked)) ? VLG_NEGINF : m;   // no candidate left: the semiring zero
            if (writer) {
                ov[k * ko] = val;
                ob[k * ko] = (unsigned short)am;
            }
        }
    }
}

// The charts of one sentence: load stage and the span-width loop, one barrier per width; tid of nt lanes, nt a power of two >= 2.
// The first half of the lanes takes direction 0 of every span, the second half direction 1 (as kbest_fill).
template <int KC, typename X>
VLG_HD void dmv_kbest_fill(const DmvKbCtx& c, const DmvKbPot& pot, int N, int tid, int nt, X& x) {
    const int Ne = c.Ne, P = c.P, cells = c.cells;
    for (int i = tid; i < Ne * P; i += nt) {
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            c.C[i + 2 * k * cells] = VLG_NEGINF;
            c.C[i + (2 * k + 1) * cells] = VLG_NEGINF;
            c.T[i + k * cells] = VLG_NEGINF;
        }
        c.A[i] = VLG_NEGINF;
        c.A[i + cells] = VLG_NEGINF;
    }
    x.sync();
    for (int idx = tid; idx < Ne * Ne; idx += nt) {
        const int h = idx / Ne, ch = idx - h * Ne;
        if (ch == h) {   // rank 0 of the trivial cells: the STOP of h towards the side, per valence; their further ranks stay empty
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                c.C[v * cells + h * P + h] = pot.ld_dec((size_t)h * 8 + dec_idx(0, v, 1));
                c.C[v * cells + h * P + h + 1] = pot.ld_dec((size_t)h * 8 + dec_idx(1, v, 1));
            }
        } else {
            const int dir = ch < h ? 0 : 1, at = h * P + ch + dir;
#pragma unroll
            for (int v = 0; v < 2; ++v)
                c.A[v * cells + at] = pot.ld_attach(((size_t)h * N + ch) * 2 + v) + pot.ld_dec((size_t)h * 8 + dec_idx(dir, v, 0));
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
            dmv_kbest_span<KC>(c, w, G, VLG_MUL24(i, P + 1), live, rr, right ? 1 : 0, x);
        }
        x.sync();
    }
}

// Rank k of one sentence, by one wavefront: kbest_walk with valences, around the same start, checks and finish.
template <int KC, typename X>
VLG_HD void dmv_kbest_walk(const DmvKbCtx& c, int k, int N, int* stack, long long* heads, float* score, X& x) {
    const int len = c.len, P = c.P, cells = c.cells, lane = x.lane();
    const float s = c.C[len + 1 + (2 * k + 1) * cells];   // CR(0,len).NC[k]
    if (!kbest_walk_begin(s, len, N, heads, score, x)) return;
    int top = 0, visits = 0;
    bool ok = true;
    int e = kbest_entry(2, 0, len, k, 1);
    for (;;) {
        const int kind = e & 3, lo = (e >> 2) & 255, hi = (e >> 10) & 255, rk = (e >> 18) & 15, v = (e >> 22) & 1;
        if (++visits > 4 * N) { ok = false; break; }
        const int w = hi - lo, D = lo * (P + 1);
        const bool inc = kind == 0 || kind == 3;
        int bp;
        if (inc) {
            if (lane == 0) heads[kind == 0 ? lo : hi] = kind == 0 ? hi : lo;
            bp = c.bT[(kind == 0 ? hi * P + lo : D + w + 1) + rk * cells];
        } else {
            bp = c.bC[(kind == 1 ? hi * P + lo : D + w + 1) + (2 * rk + v) * cells];
        }
        bp = x.uniform(bp);
        if (!kbest_bp_fits<KC>(bp, w)) { ok = false; break; }
        const int r = bp >> 8, p = (bp >> 4) & 15, q = bp & 15;
        int ea, eb;   // the two children, their valences by the parent's kind (dmv_sample_walk)
        if (kind == 0) { ea = kbest_entry(2, lo, lo + r, p, 1); eb = kbest_entry(1, lo + r + 1, hi, q, 0); }
        else if (kind == 3) { ea = kbest_entry(2, lo, lo + r, p, 0); eb = kbest_entry(1, lo + r + 1, hi, q, 1); }
        else if (kind == 1) { ea = kbest_entry(1, lo, lo + r, p, 1); eb = kbest_entry(0, lo + r, hi, q, v); }
        else { ea = kbest_entry(3, lo, lo + 1 + r, p, v); eb = kbest_entry(2, lo + 1 + r, hi, q, 1); }
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

// how many of the first K ranks exist
VLG_HD int dmv_kbest_count(const DmvKbCtx& c, int K) { return kbest_count_at(c.C, c.len + 1 + c.cells, 2 * c.cells, K); }   // CR(0,len).NC[k]

// ---- the adjoint of the scores: derivation counts of given trees ------------------------------------------------------------------
// Lane i of one tree of one sentence.  hs [N]: the tree's heads, -1 where the entry is outside 0 ... len or names the word itself
// (such a word attaches nowhere).  As the child c = i it adds wt to its own column of cnt_attach [N][N][2]: the farthest child of a
// side attaches with NOCHILD, the others with HASCHILD.  As the head h = i it adds the GO / STOP counts of both sides to acc [8]
// (its row of cnt_dec, dec_idx order): STOP is NOCHILD only when the side has no child; the root has a right side only.
VLG_HD void dmv_tree_counts_lane(const int* hs, int len, int N, int i, float wt, float* cnt_attach, float* acc) {
    if (i > len) return;
    if (i >= 1 && hs[i] >= 0) {
        const int h = hs[i];
        bool farthest = true;
        if (i < h) { for (int c = 1; c < i; ++c) farthest &= hs[c] != h; }
        else { for (int c = i + 1; c <= len; ++c) farthest &= hs[c] != h; }
        cnt_attach[((size_t)h * N + i) * 2 + (farthest ? 1 : 0)] += wt;
    }
    int nl = 0, nr = 0;
    for (int c = 1; c < i; ++c) nl += hs[c] == i ? 1 : 0;
    for (int c = i + 1; c <= len; ++c) nr += hs[c] == i ? 1 : 0;
    for (int dir = i == 0 ? 1 : 0; dir < 2; ++dir) {
        const int n = dir == 0 ? nl : nr;
        if (n > 0) {
            acc[dec_idx(dir, 1, 0)] += wt;                      // the farthest child: NOCHILD, GO
            if (n > 1) acc[dec_idx(dir, 0, 0)] += wt * (float)(n - 1);
        }
        acc[dec_idx(dir, n > 0 ? 0 : 1, 1)] += wt;              // STOP
    }
}

}  // namespace vlg
