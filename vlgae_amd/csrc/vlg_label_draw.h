// vlg_label_draw.h -- drawing the labels of a sampled dependency tree (vlg_label_draw, include/vlgae_amd.h).
//
// Like vlg_dp_sample.h this is the work of the lanes of ONE wavefront, written against the sampler's policy X, and shared by the
// gfx950 kernel (vlg_label.hip) and the host emulator of the CPU test-suite (tests/emu/emu_label.cpp: a "wavefront" of one lane).
// Nothing here is a CPU fallback.
//
// Given the heads of one (sample, sentence), word c = 1 ... len takes its label from softmax_l phi[head(c), c, :]: the draw rule is
// sample_draw of vlg_sample_common.h with the L labels as its terms, in label order, under the word's uniform (the table
// u_label[s,b,c], or the sampler's counter with the free draw kind 3 keyed (head, child)).  The row is staged in log2 units in
// `stage` (kLabelStage floats of this wave, the last one a 0 that serves as the rule's second operand with stride 0); a label that
// is -inf or below the clamp floor has weight 0 and is never drawn while another label of the row is allowed.
// One wave owns the whole (sample, sentence): its words are drawn one after the other, so the sum of (phi_label - arc) that turns the
// tree's log-probability into the labeled tree's has one writer and one order.
#pragma once
#include "vlg_dp_core.h"
#include "vlg_sample_common.h"

namespace vlg {

constexpr int kLabelMax = 255;                // labels per arc
constexpr int kLabelStage = kLabelMax + 1;    // floats per wave: the row, then the 0 at [kLabelMax]

// the uniforms of one (sample, sentence) from the explicit table u_label [S,B,N] (kind, head unused: one draw per word)
struct LabelTableU {
    const float* u;   // at [s][b]
    VLG_HDM float get(int, int child, int) const { return u[child]; }
};

// heads, labels: the N int64 of this (sample, sentence); phi: the sentence's [N,N,L]; arc: its folded [N,N] (read only when logp is
// given); logp: the sample's cell or null -- it holds the tree's score minus logZ, or NaN where the tree sampler gave up.
// A tree the sampler gave up on has heads 0 throughout, which no tree of two or more words has: its labels are 0 and logp stays NaN.
template <typename In, typename U, typename X>
VLG_HD void label_draw_walk(const typename In::T* phi, const float* arc, int N, int L, int len, const long long* heads, const U& us,
                            float* stage, long long* labels, float* logp, X& x) {
    constexpr int W = X::kWave;
    const int lane = x.lane();
    bool any = false;
    for (int i = 1 + lane; i <= len; i += W) any = any || heads[i] != 0;
    const bool ok = x.uniform(len == 1 || x.ballot_first(any) >= 0);
    for (int i = lane; i < N; i += W)
        if (i == 0 || i > len || !ok) labels[i] = 0;   // every word of a drawn tree gets its label below: one writer per element
    if (!ok) return;
    if (lane == 0) stage[kLabelMax] = 0.f;
    float add = 0.f;
    for (int c = 1; c <= len; ++c) {
        const int h = x.uniform((int)heads[c]);
        if (h < 0 || h > len || h == c) {   // not an arc of a tree (foreign heads): no row to read
            if (lane == 0) labels[c] = 0;
            continue;
        }
        const typename In::T* row = phi + ((size_t)h * N + c) * L;
        int k = 0;
        if (L > 1) {   // (one label: nothing to draw, no uniform is generated)
            for (int l = lane; l < L; l += W) stage[l] = pot_clamp(In::ld(row, l)) * VLG_LOG2E;
            x.lockstep();
            k = x.uniform(sample_draw(stage, 1, stage + kLabelMax, 0, L, us.get(3, c, h), x));
            x.lockstep();
        }
        if (lane == 0) labels[c] = k;
        if (logp) add += In::ld(row, k) - arc[(size_t)h * N + c];
    }
    if (logp && lane == 0) *logp += add;
}

}  // namespace vlg
