// vlg_dp_sample.h -- drawing a projective single-root tree from the DepTree inside charts (DependencyCRF.sample_heads).
//
// Like the phase bodies of vlg_dp_core.h this is the work of the lanes of ONE wavefront, written against a policy X, and shared by the
// gfx950 kernel (vlg_sample.hip) and the host emulator of the CPU test-suite (tests/emu/emu_sample.cpp), whose policy supplies
// sequential versions of the wave operations (a "wavefront" of one lane).  Nothing here is a CPU fallback.
//
// After the Log-semiring inside pass (dep_fw_all, unchanged) C and I hold, in log2 units, the inside value of every cell, the
// single-root masking included.  A sample is a top-down expansion from CR(0,len) (deptree.py:74-75).  Three kinds of cell are
// non-trivial, keyed (kind, lo, hi), lo < hi:
//   kind 0  incomplete span [lo,hi], either direction   r in [lo,hi)   t_r = CR(lo,r) + CL(hi,r+1)    (deptree.py:53-62)
//   kind 1  CL(hi -> lo)                                r in [lo,hi)   t_r = CL(r,lo) + I(hi -> r)     (:64-66)
//   kind 2  CR(lo -> hi)                                r in (lo,hi]   t_r = I(lo -> r) + CR(r,hi)     (:67-69)
// (only one of the two arcs between lo and hi can occur in a tree, so one key serves both directions of kind 0).
// The draw rule and the keying of the cell's uniform are vlg_sample_common.h's (sample_draw), shared with the DMV1o sampler.
//
// The walk keeps its pending siblings on a stack.  It descends into the NARROWER child and leaves the wider one pending: a pending
// cell is then at least as wide as everything above it and its parent at most half as wide as the pending cell's parent below it, so
// at most 7 cells are ever pending for N <= 255 (a parent that leaves a sibling pending is >= 2 wide) and kSampleStack ints per wave
// do.  (The order of the visits does not matter to the result: the draws are keyed by cell.)  That keeps the per-wave stacks at 1 KiB
// per workgroup: with 2 N + 4 ints each, as dep_walk's stack has, they would not fit behind the charts for N = 139 ... 142, where
// DepLayout still places both charts in LDS.
#pragma once
#include "vlg_dp_core.h"
#include "vlg_sample_common.h"

namespace vlg {

constexpr int kSampleStack = 32;   // ints per wavefront; the walk needs 7 (above) and checks

// The terms of cell (draw kind, lo, hi) as two strided walks over the charts: t_k = a[k sa] + b[k sb], r = lo + k for kinds 0 and 1,
// lo + 1 + k for kind 2.
VLG_HD void dep_sample_terms(const DepCtx& c, int kind, int lo, int hi, const float*& a, int& sa, const float*& b, int& sb) {
    const int P = c.P;
    sa = sb = 1;
    if (kind == 0) { a = c.C + lo * P + lo + 1; b = c.C + hi * P + lo + 1; }                 // CR(lo,r) at [lo][r+1], CL(hi,r+1) at [hi][r+1]
    else if (kind == 1) { a = c.C + lo * P + lo; sa = P; b = c.I + hi * P + lo; }            // CL(r,lo) at [r][lo],   IL(hi,r) at [hi][r]
    else { a = c.I + lo * P + lo + 2; b = c.C + (lo + 1) * P + hi + 1; sb = P; }             // IR(lo,r) at [lo][r+1], CR(r,hi) at [r][hi+1]
}

// One sample of one sentence, by one wavefront.  heads: the N int64 of this (sample, sentence); logp: its cell or null; lz2: the
// sentence's log-partition in log2 units (C[len + 1]); stack: kSampleStack ints of this wave.  The tree's score is summed from the
// INPUT potentials (one In::ld per arc).  The walk visits each non-trivial cell of the tree once (at most 3 len + 1 of them); after
// 4 N visits it gives up -- heads 0, logp NaN -- so that no chart contents can make it spin.
template <typename In, typename U, typename X>
VLG_HD void dep_sample_walk(const DepCtx& c, const typename In::T* arc, int N, int* stack, const U& us, long long* heads, float* logp,
                            float lz2, X& x) {
    const int len = c.len, lane = x.lane();
    for (int i = lane; i < N; i += X::kWave)
        if (i == 0 || i > len) heads[i] = 0;   // every word 1 ... len gets its head from the walk: one writer per element
    int top = 0, visits = 0;
    float score = 0.f;
    bool ok = true;
    int e = sample_entry(2, 0, len);
    for (;;) {
        const int kind = entry_kind(e), lo = entry_lo(e), hi = entry_hi(e);
        if (++visits > 4 * N) { ok = false; break; }
        const int dk = kind == 3 ? 0 : kind;
        if (dk == 0) {
            const int h = kind == 0 ? hi : lo, ch = kind == 0 ? lo : hi;
            if (lane == 0) heads[ch] = h;
            score += In::ld(arc, (size_t)h * N + ch);
        }
        // (a cell with one split has nothing to draw: whatever u is, the rule takes it -- no uniform is generated for it)
        int k = 0;
        if (hi - lo != 1) {
            const float *a, *b;
            int sa, sb;
            dep_sample_terms(c, dk, lo, hi, a, sa, b, sb);
            k = x.uniform(sample_draw(a, sa, b, sb, hi - lo, us.get(dk, lo, hi), x));
        }
        int ea, eb, wa, wb;   // the two children; lo == hi: a trivial cell, nothing to draw
        if (dk == 0) { ea = sample_entry(2, lo, lo + k); eb = sample_entry(1, lo + k + 1, hi); }
        else if (dk == 1) { ea = sample_entry(1, lo, lo + k); eb = sample_entry(0, lo + k, hi); }
        else { ea = sample_entry(3, lo, lo + 1 + k); eb = sample_entry(2, lo + 1 + k, hi); }
        sample_order(ea, eb, wa, wb);
        if (!sample_step(stack, kSampleStack, top, ea, eb, wa, wb, e, ok, x)) break;
    }
    sample_finish(ok, score, lz2, N, heads, logp, lane);
}

}  // namespace vlg
