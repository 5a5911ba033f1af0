// vlg_dmv_sample.h -- drawing a projective single-root tree from the DMV1o inside charts (DMV1o.sample_heads).
//
// The valence-aware sibling of vlg_dp_sample.h: the work of the lanes of ONE wavefront, written against a policy X, shared by the
// gfx950 kernel (vlg_dmv_sample.hip) and the host emulator of the CPU test-suite (tests/emu/emu_dmv_sample.cpp), whose policy
// supplies sequential versions of the wave operations (a "wavefront" of one lane).  Nothing here is a CPU fallback.
//
// After the Log-semiring inside pass (dmv_run<Log, false>, unchanged) C and I hold, in log2 units and for both valences (.x HASCHILD,
// .y NOCHILD), the inside value of every cell, the single-root masking included.  A sample is a top-down expansion from
// CR(0,len).NOCHILD (dmv.py:65).  A cell carries a valence v; the recurrences are dmv_fw_span's / dmv_walk's:
//   draw kind 0  IL(hi -> lo).v               r in [lo,hi)   t_r = CR(lo,r).NC + CL(hi,r+1).HC     (dmv.py:50-52)
//                IR(lo -> hi).v               r in [lo,hi)   t_r = CR(lo,r).HC + CL(hi,r+1).NC     (:54-56)
//   draw kind 1  CL(hi -> lo).v               r in [lo,hi)   t_r = CL(r,lo).NC + IL(hi -> r).v     (:58-59)
//   draw kind 2  CR(lo -> hi).v               r in (lo,hi]   t_r = IR(lo -> r).v + CR(r,hi).NC     (:61-62)
// with the two cells of t_r as children.  The weights of a kind-0 cell do not depend on v but on the direction.  The draw itself is
// vlg_sample_common.h's sample_draw, the one the DepTree sampler calls, over float2 charts: float pointers with a stride of two.
// u is the cell's uniform, keyed (kind, lo, hi) as there: a derivation holds a span (kind, lo, hi) at most once, in one direction and
// with one valence, so neither goes into the key.
//
// The tree's score is summed from the INPUT potentials: attach[h,c,v] + dec[h,dir,v,GO] when the walk enters I(h -> c).v, and
// dec[h,dir,v,STOP] for every width-0 complete cell C(h,h).v towards dir.  Such a leaf is never pushed -- its STOP term is added where
// its parent is split -- so vlg_dp_sample.h's stack argument holds: the walk descends into the narrower child, at most 7 cells are
// ever pending for N <= 255, and kDmvSampleStack ints per wave do.  (Sixteen, not the DepTree sampler's 32: the forward-only DmvLayout
// keeps both charts in LDS up to N = 99 and leaves 672 bytes there; eight stacks of 16 ints are 512.)
#pragma once
#include "vlg_dp_core.h"
#include "vlg_sample_common.h"

namespace vlg {

constexpr int kDmvSampleStack = 16;   // ints per wavefront; the walk needs 7 (above) and checks

// The terms of walk cell (kind, lo, hi, v) as two strided float walks over the float2 charts (component = valence).
VLG_HD void dmv_sample_terms(const DmvCtx& c, int kind, int lo, int hi, int v, const float*& a, int& sa, const float*& b, int& sb) {
    const int P = c.P;
    const float* Cf = reinterpret_cast<const float*>(c.C);
    const float* If = reinterpret_cast<const float*>(c.I);
    sa = sb = 2;
    if (kind == 0) {          // IL: CR(lo,r).NC at [lo][r+1].y, CL(hi,r+1).HC at [hi][r+1].x
        a = Cf + 2 * (lo * P + lo + 1) + 1;
        b = Cf + 2 * (hi * P + lo + 1);
    } else if (kind == 3) {   // IR: CR(lo,r).HC, CL(hi,r+1).NC
        a = Cf + 2 * (lo * P + lo + 1);
        b = Cf + 2 * (hi * P + lo + 1) + 1;
    } else if (kind == 1) {   // CL(r,lo).NC at [r][lo].y, IL(hi,r).v at [hi][r]
        a = Cf + 2 * (lo * P + lo) + 1;
        sa = 2 * P;
        b = If + 2 * (hi * P + lo) + v;
    } else {                  // IR(lo,r).v at [lo][r+1], CR(r,hi).NC at [r][hi+1].y
        a = If + 2 * (lo * P + lo + 2) + v;
        b = Cf + 2 * ((lo + 1) * P + hi + 1) + 1;
        sb = 2 * P;
    }
}

// One sample of one sentence, by one wavefront.  heads: the N int64 of this (sample, sentence); logp: its cell or null; lz2: the
// sentence's log-partition in log2 units (CR(0,len).NC); stack: kDmvSampleStack ints of this wave.  dec [N][2][2][2] / attach [N][N][2]
// are this sentence's input potentials.  The walk visits each non-trivial cell of the tree once (at most 3 len + 1 of them); after
// 4 N visits, or on a full stack, it gives up -- heads 0, logp NaN -- so that no chart contents can make it spin.
template <typename In, typename U, typename X>
VLG_HD void dmv_sample_walk(const DmvCtx& c, const typename In::T* dec, const typename In::T* attach, int N, int* stack, const U& us,
                            long long* heads, float* logp, float lz2, X& x) {
    const int len = c.len, lane = x.lane();
    for (int i = lane; i < N; i += X::kWave)
        if (i == 0 || i > len) heads[i] = 0;   // every word 1 ... len gets its head from the walk: one writer per element
    int top = 0, visits = 0;
    float score = 0.f;
    bool ok = true;
    // The potentials of the score stay RAW and in flight for one visit: loaded where the walk meets them, converted and added where the
    // next ones are loaded (and behind the loop), so a global load's latency lies under a draw instead of in front of it.
    using T = typename In::T;
    T raw_att = T(), raw_go = T(), raw_stop_a = T(), raw_stop_b = T();
    bool has_arc = false, has_stop_a = false, has_stop_b = false;
    int e = sample_entry(2, 0, len, 1);
    for (;;) {
        const int kind = entry_kind(e), lo = entry_lo(e), hi = entry_hi(e), v = entry_v(e);
        if (++visits > 4 * N) { ok = false; break; }
        const int dk = kind == 3 ? 0 : kind;
        if (dk == 0) {
            const int h = kind == 0 ? hi : lo, ch = kind == 0 ? lo : hi, dir = kind == 0 ? 0 : 1;
            if (lane == 0) heads[ch] = h;
            if (has_arc) score += In::ld(&raw_att, 0) + In::ld(&raw_go, 0);
            raw_att = attach[((size_t)h * N + ch) * 2 + v];
            raw_go = dec[(size_t)h * 8 + dec_idx(dir, v, 0)];
            has_arc = true;
        }
        // (a cell with one split has nothing to draw: whatever u is, the rule takes it -- no uniform is generated for it)
        int k = 0;
        if (hi - lo > 1) {
            const float *a, *b;
            int sa, sb;
            dmv_sample_terms(c, kind, lo, hi, v, a, sa, b, sb);
            k = x.uniform(sample_draw(a, sa, b, sb, hi - lo, us.get(dk, lo, hi), x));
        }
        int ea, eb, wa, wb;   // the two children
        if (kind == 0) { ea = sample_entry(2, lo, lo + k, 1); eb = sample_entry(1, lo + k + 1, hi, 0); }
        else if (kind == 3) { ea = sample_entry(2, lo, lo + k, 0); eb = sample_entry(1, lo + k + 1, hi, 1); }
        else if (kind == 1) { ea = sample_entry(1, lo, lo + k, 1); eb = sample_entry(0, lo + k, hi, v); }
        else { ea = sample_entry(3, lo, lo + 1 + k, v); eb = sample_entry(2, lo + 1 + k, hi, 1); }
        sample_order(ea, eb, wa, wb);
        if (has_stop_a) score += In::ld(&raw_stop_a, 0);
        if (has_stop_b) score += In::ld(&raw_stop_b, 0);
        has_stop_a = wa == 0;
        has_stop_b = wb == 0;
        if (has_stop_a) {   // a width-0 complete cell C(h,h).v (an incomplete cell is >= 1 wide): the STOP of h towards CL's / CR's side
            const int h = entry_lo(ea), dir = entry_kind(ea) == 1 ? 0 : 1;
            raw_stop_a = dec[(size_t)h * 8 + dec_idx(dir, entry_v(ea), 1)];
        }
        if (has_stop_b) {
            const int h = entry_lo(eb), dir = entry_kind(eb) == 1 ? 0 : 1;
            raw_stop_b = dec[(size_t)h * 8 + dec_idx(dir, entry_v(eb), 1)];
        }
        if (!sample_step(stack, kDmvSampleStack, top, ea, eb, wa, wb, e, ok, x)) break;
    }
    if (has_arc) score += In::ld(&raw_att, 0) + In::ld(&raw_go, 0);
    if (has_stop_a) score += In::ld(&raw_stop_a, 0);
    if (has_stop_b) score += In::ld(&raw_stop_b, 0);
    sample_finish(ok, score, lz2, N, heads, logp, lane);
}

}  // namespace vlg
