// vlg_sample_common.h -- what the on-device tree samplers share (vlg_dp_sample.h: DepTree, vlg_dmv_sample.h: DMV1o): the draw rule,
// the explicit uniform table, the packing of a walk entry, and the walk's order / step / finish.  Like those two headers it is the
// work of the lanes of ONE wavefront, written against a policy X, and shared by the gfx950 kernels (whose policy and launch frame
// are vlg_sample_kernels.h) and the host emulators of the CPU test-suite (tests/emu/emu_sample_common.h: a "wavefront" of one lane).
// Nothing here is a CPU fallback.  A sampler adds: its chart type, the terms of a cell, the children of a cell, the potentials that
// enter the score, and its stack depth.
#pragma once
#include "vlg_dp_core.h"

namespace vlg {

// walk entries: kind 0 = IL(hi -> lo), 1 = CL(hi -> lo), 2 = CR(lo -> hi), 3 = IR(lo -> hi), with a valence v where the model has
// one; the draw kind of both incomplete cells is 0
VLG_HD int sample_entry(int kind, int lo, int hi, int v = 0) { return kind | (lo << 2) | (hi << 10) | (v << 18); }
VLG_HD int entry_kind(int e) { return e & 3; }
VLG_HD int entry_lo(int e) { return (e >> 2) & 255; }
VLG_HD int entry_hi(int e) { return (e >> 10) & 255; }
VLG_HD int entry_v(int e) { return (e >> 18) & 1; }
VLG_HD int entry_width(int e) { return entry_hi(e) - entry_lo(e); }

// the uniforms of one (sample, sentence) from the explicit table u [S,B,3,N,N]
struct TableU {
    const float* u;   // at [s][b]
    int N;
    VLG_HDM float get(int kind, int lo, int hi) const { return u[((size_t)kind * N + lo) * N + hi]; }
};

// One draw: the index k of the split taken among the n terms t_k = a[k sa] + b[k sb] (log2 units) under u.  Every lane of the wave
// returns the same k.  X::kWave lanes spread over the terms, 'kWave' at a time.
// The rule: w_k = 2^(t_k - max t), cum = running sum in increasing k, total = the last cum; taken is the SMALLEST k with
// cum_k > u total (strict), else -- u within an ulp of 1, or NaN -- the largest k with w_k > 0.  A split of weight 0 is never taken:
// in a sequential sum cum_k = cum_(k-1) there, and the wave's parallel scan, whose partial sums are rounded in another order, also asks
// for w_k > 0 outright.  u is the cell's uniform: a function of (state, sentence, sample, kind, lo, hi) alone -- not of the order the
// cells are visited in, of the wave that walks the sample or of the grid.
template <typename X>
VLG_HD int sample_draw(const float* a, int sa, const float* b, int sb, int n, float u, X& x) {
    constexpr int W = X::kWave;
    const int lane = x.lane();
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

// The two children of a cell, ordered so that ea is the narrower one (widths wa <= wb).
VLG_HD void sample_order(int& ea, int& eb, int& wa, int& wb) {
    wa = entry_width(ea);
    wb = entry_width(eb);
    if (wa > wb) { const int t = ea; ea = eb; eb = t; const int tw = wa; wa = wb; wb = tw; }
}

// The walk's next cell e: the narrower child, the wider one left pending on the stack of `depth` ints; else the wider child; else
// (both children trivial) the last pending cell.  False where the walk ends: nothing pending, or -- ok = false -- the stack is full.
template <typename X>
VLG_HD bool sample_step(int* stack, int depth, int& top, int ea, int eb, int wa, int wb, int& e, bool& ok, X& x) {
    if (wa > 0) {
        if (top >= depth) { ok = false; return false; }
        stack[top++] = eb;   // (wb >= wa > 0)
        e = ea;
    } else if (wb > 0) {
        e = eb;
    } else {
        if (top == 0) return false;
        e = x.uniform(stack[--top]);
    }
    return true;
}

// The end of a walk: logp = score - logZ, or -- the walk gave up -- heads 0 and logp NaN.
VLG_HD void sample_finish(bool ok, float score, float lz2, int N, long long* heads, float* logp, int lane) {
    if (lane == 0) {
        if (!ok)
            for (int i = 0; i < N; ++i) heads[i] = 0;   // one lane, in program order behind its own stores above
        if (logp) *logp = ok ? score - lz2 * VLG_LN2 : VLG_BITS2F(0x7fc00000u);
    }
}

}  // namespace vlg
