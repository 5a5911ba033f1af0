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
// The draw: w_r = 2^(t_r - max t), cum = running sum in increasing r, total = the last cum; taken is the SMALLEST r with
// cum_r > u total (strict), else -- u within an ulp of 1, or NaN -- the largest r with w_r > 0.  A split of weight 0 is never taken:
// in a sequential sum cum_r = cum_(r-1) there, and the wave's parallel scan, whose partial sums are rounded in another order, also asks
// for w_r > 0 outright.  u is the cell's uniform: a function of (state, sentence, sample, kind, lo, hi) alone -- not of the order the
// cells are visited in, of the wave that walks the sample or of the grid.
//
// The walk keeps its pending siblings on a stack.  It descends into the NARROWER child and leaves the wider one pending: a pending
// cell is then at least as wide as everything above it and its parent at most half as wide as the pending cell's parent below it, so
// at most 7 cells are ever pending for N <= 255 (a parent that leaves a sibling pending is >= 2 wide) and kSampleStack ints per wave
// do.  (The order of the visits does not matter to the result: the draws are keyed by cell.)  That keeps the per-wave stacks at 1 KiB
// per workgroup: with 2 N + 4 ints each, as dep_walk's stack has, they would not fit behind the charts for N = 139 ... 142, where
// DepLayout still places both charts in LDS.
#pragma once
#include "vlg_dp_core.h"

namespace vlg {

constexpr int kSampleStack = 32;   // ints per wavefront; the walk needs 7 (above) and checks

// walk entries: 0 = IL(hi -> lo), 1 = CL(hi -> lo), 2 = CR(lo -> hi), 3 = IR(lo -> hi); the draw kind of both incomplete cells is 0
VLG_HD int sample_entry(int kind, int lo, int hi) { return kind | (lo << 2) | (hi << 10); }

// the uniforms of one (sample, sentence) from the explicit table u [S,B,3,N,N]
struct TableU {
    const float* u;   // at [s][b]
    int N;
    VLG_HDM float get(int kind, int lo, int hi) const { return u[((size_t)kind * N + lo) * N + hi]; }
};

// One draw: the index k (r = lo + k for kinds 0 and 1, lo + 1 + k for kind 2) of the split taken in cell (kind, lo, hi) under u.
// Every lane of the wave returns the same k.  X::kWave lanes spread over the hi - lo terms, 'kWave' at a time.
template <typename X>
VLG_HD int dep_sample_draw(const DepCtx& c, int kind, int lo, int hi, float u, X& x) {
    constexpr int W = X::kWave;
    const int P = c.P, n = hi - lo, lane = x.lane();
    const float *a, *b;
    int sa = 1, sb = 1;
    if (kind == 0) { a = c.C + lo * P + lo + 1; b = c.C + hi * P + lo + 1; }                 // CR(lo,r) at [lo][r+1], CL(hi,r+1) at [hi][r+1]
    else if (kind == 1) { a = c.C + lo * P + lo; sa = P; b = c.I + hi * P + lo; }            // CL(r,lo) at [r][lo],   IL(hi,r) at [hi][r]
    else { a = c.I + lo * P + lo + 2; b = c.C + (lo + 1) * P + hi + 1; sb = P; }             // IR(lo,r) at [lo][r+1], CR(r,hi) at [r][hi+1]
    if (n <= W) {   // one chunk (always, for N <= 65 on the device): the terms stay in registers -- the same operations as the loops below
        const bool in = lane < n;
        const float t = in ? a[lane * sa] + b[lane * sb] : VLG_LOWEST;
        const float m1 = x.wave_max(t), w1 = in ? VLG_EXP(t - m1) : 0.f, cum = x.wave_scan(w1);
        int pick = x.ballot_first(cum > u * x.wave_last(cum) && w1 > 0.f);
        if (pick < 0) pick = x.ballot_last(w1 > 0.f);
        return pick < 0 ? 0 : pick;
    }
    float m = VLG_LOWEST;
    for (int k = lane; k < n; k += W) m = fmaxf(m, a[k * sa] + b[k * sb]);
    m = x.wave_max(m);
    // the weights of the chunk at k0 and their running sum behind `carry`; w = 0 past the last term
    auto chunk = [&](int k0, float carry, float& w) {
        const int k = k0 + lane;
        w = k < n ? VLG_EXP(a[k * sa] + b[k * sb] - m) : 0.f;
        return carry + x.wave_scan(w);
    };
    float total = 0.f, w;
    for (int k0 = 0; k0 < n; k0 += W) total = x.wave_last(chunk(k0, total, w));
    const float thr = u * total;
    float carry = 0.f;
    int pick = -1, last = -1;   // carried over the chunks: the split taken, the largest k of weight > 0 so far
    for (int k0 = 0; k0 < n && pick < 0; k0 += W) {
        const float cum = chunk(k0, carry, w);
        const int f = x.ballot_first(cum > thr && w > 0.f), l = x.ballot_last(w > 0.f);
        if (f >= 0) pick = k0 + f;
        if (l >= 0) last = k0 + l;
        carry = x.wave_last(cum);
    }
    if (pick < 0) pick = last;
    return pick < 0 ? 0 : pick;   // (no term of weight > 0: only a damaged chart; the walk's visit bound ends it)
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
        const int kind = e & 3, lo = (e >> 2) & 255, hi = (e >> 10) & 255;
        if (++visits > 4 * N) { ok = false; break; }
        const int dk = kind == 3 ? 0 : kind;
        if (dk == 0) {
            const int h = kind == 0 ? hi : lo, ch = kind == 0 ? lo : hi;
            if (lane == 0) heads[ch] = h;
            score += In::ld(arc, (size_t)h * N + ch);
        }
        // (a cell with one split has nothing to draw: whatever u is, the rule takes it -- no uniform is generated for it)
        const int k = hi - lo == 1 ? 0 : x.uniform(dep_sample_draw(c, dk, lo, hi, us.get(dk, lo, hi), x));
        int ea, eb;   // the two children; lo == hi: a trivial cell, nothing to draw
        if (dk == 0) { ea = sample_entry(2, lo, lo + k); eb = sample_entry(1, lo + k + 1, hi); }
        else if (dk == 1) { ea = sample_entry(1, lo, lo + k); eb = sample_entry(0, lo + k, hi); }
        else { ea = sample_entry(3, lo, lo + 1 + k); eb = sample_entry(2, lo + 1 + k, hi); }
        int wa = ((ea >> 10) & 255) - ((ea >> 2) & 255), wb = ((eb >> 10) & 255) - ((eb >> 2) & 255);
        if (wa > wb) { const int t = ea; ea = eb; eb = t; const int tw = wa; wa = wb; wb = tw; }   // ea: the narrower one
        if (wa > 0) {
            if (top >= kSampleStack) { ok = false; break; }
            stack[top++] = eb;   // (wb >= wa > 0)
            e = ea;
        } else if (wb > 0) {
            e = eb;
        } else {
            if (top == 0) break;
            e = x.uniform(stack[--top]);
        }
    }
    if (lane == 0) {
        if (!ok)
            for (int i = 0; i < N; ++i) heads[i] = 0;   // one lane, in program order behind its own stores above
        if (logp) *logp = ok ? score - lz2 * VLG_LN2 : VLG_BITS2F(0x7fc00000u);
    }
}

}  // namespace vlg
