// sched_short.cpp -- the outside pass's group-size rule and lane map of the short-sentence image.  TEST INFRASTRUCTURE ONLY.
//
// A stand-alone program (its own main) against vlgae_amd/csrc/vlg_dp_core.h.  For every sentence of the short image, Ne = 2 ... 41, at
// the kernels' 256 lanes (four wavefronts) per direction, and every width w of it, it checks what dmv_bw_segment_p rests on:
//   * bw_sched (the rule solved for w) and bw_piece_of (the rule) name the same table entry, and G does not fall as w grows;
//   * the width's spans fit: Ne - w <= waves (64 / G), with at least one group per wavefront;
//   * the piece's term count TM = bw_terms(k) covers the width, ceil(w / G) <= TM <= 2 (1 at G = 64), and G TM <= 64 -- the reach
//     tests/emu/emu_short.cpp sizes its slack for;
//   * the lane map bw_lane<G>: every (span, split point) of the width belongs to exactly one (lane, term); the lanes of a group are G
//     consecutive lanes of ONE wavefront with the residues 0 ... G - 1; a lane that is dealt no group has a slot past every span.
// It is built with -fsanitize=address,undefined by tests/test_dmv_short_sched_host.py.
#include <cstdio>
#include <vector>

#include "../../vlgae_amd/csrc/vlg_dp_core.h"

namespace {

constexpr int kLanesPerDir = 256;
int failures = 0;

void fail(int Ne, int w, const char* what) {
    if (++failures <= 20) std::printf("FAIL Ne %d w %d: %s\n", Ne, w, what);
}

template <int K>
void check_width(int Ne, int w, int waves) {
    constexpr int G = vlg::bw_group(K), TM = vlg::bw_terms(K), GW = 64 / G;
    static_assert(GW >= 1 && TM >= 1 && TM <= 2 && G * TM <= 64 && (G != 64 || TM == 1), "a piece of the table");
    const int spans = Ne - w;
    if (spans > waves * GW) fail(Ne, w, "more spans than groups");
    if ((w + G - 1) / G > TM) fail(Ne, w, "the width needs more terms than the piece runs");
    std::vector<int> owners((size_t)spans * w, 0), members((size_t)spans, 0), wave_of((size_t)spans, -1), residues((size_t)spans * G, 0);
    for (int t = 0; t < kLanesPerDir; ++t) {
        const vlg::BwLane ln = vlg::bw_lane<G>(t);
        if (ln.rr < 0 || ln.rr >= G) fail(Ne, w, "residue out of range");
        if (ln.wslot != (t >> 6) * GW) fail(Ne, w, "wslot is not the wavefront's first span");
        if (ln.slot == vlg::kBwNoSlot) {
            if ((t & 63) < GW * G) fail(Ne, w, "a lane inside a whole group is idle");
            if (ln.slot < vlg::kShortN) fail(Ne, w, "an idle lane's slot is not past every span");
            continue;
        }
        if ((t & 63) >= GW * G) fail(Ne, w, "a lane past the last whole group of its wavefront is dealt a span");
        if (ln.slot < ln.wslot || ln.slot >= ln.wslot + GW) fail(Ne, w, "slot outside its wavefront's range");
        if (ln.slot >= spans) continue;   // a group without a span at this width
        ++members[ln.slot];
        ++residues[(size_t)ln.slot * G + ln.rr];
        if (wave_of[ln.slot] < 0) wave_of[ln.slot] = t >> 6;
        else if (wave_of[ln.slot] != (t >> 6)) fail(Ne, w, "a group crosses a multiple of 64");
        for (int u = 0; u < TM; ++u) {
            const int r = ln.rr + u * G;
            if (r >= 64) fail(Ne, w, "a term reaches split point 64");
            if (r < w) ++owners[(size_t)ln.slot * w + r];
        }
    }
    for (int s = 0; s < spans; ++s) {
        if (members[s] != G) fail(Ne, w, "a span's group does not have G lanes");
        for (int q = 0; q < G; ++q)
            if (residues[(size_t)s * G + q] != 1) fail(Ne, w, "a residue of a group is missing or doubled");
        for (int r = 0; r < w; ++r)
            if (owners[(size_t)s * w + r] != 1) fail(Ne, w, "a (span, split point) is not owned exactly once");
    }
}

void check_piece(int k, int Ne, int w, int waves) {
    switch (k) {
        case 0: check_width<0>(Ne, w, waves); break;
        case 1: check_width<1>(Ne, w, waves); break;
        case 2: check_width<2>(Ne, w, waves); break;
        case 3: check_width<3>(Ne, w, waves); break;
        case 4: check_width<4>(Ne, w, waves); break;
        case 5: check_width<5>(Ne, w, waves); break;
        case 6: check_width<6>(Ne, w, waves); break;
        default: fail(Ne, w, "piece index outside the table");
    }
}
static_assert(vlg::kBwPieces == 7, "check_piece names every entry of the table");

}  // namespace

int main() {
    const int waves = vlg::bw_waves(kLanesPerDir);
    if (waves != kLanesPerDir / 64) { std::printf("FAIL: %d wavefronts per direction\n", waves); return 1; }
    int widths = 0;
    for (int Ne = 2; Ne <= vlg::kShortN; ++Ne) {
        const vlg::BwSched sc = vlg::bw_sched(Ne, waves);
        if (sc.first[0] != 1 || sc.first[vlg::kBwPieces] != Ne) fail(Ne, 0, "the pieces do not span 1 ... Ne - 1");
        for (int k = 0; k < vlg::kBwPieces; ++k)
            if (sc.first[k] > sc.first[k + 1]) fail(Ne, 0, "piece edges not ascending");
        int prev = 0;
        for (int w = 1; w < Ne; ++w, ++widths) {
            int k = 0;
            while (k + 1 < vlg::kBwPieces && sc.first[k + 1] <= w) ++k;
            if (k != vlg::bw_piece_of(Ne, w, waves)) fail(Ne, w, "bw_sched and bw_piece_of disagree");
            if (vlg::bw_group(k) < vlg::bw_group(prev)) fail(Ne, w, "G falls as w grows");
            prev = k;
            check_piece(k, Ne, w, waves);
        }
    }
    // the table of DESIGN.md section 2 at Ne = 41
    const int want[7][3] = {{1, 8, 4}, {9, 16, 8}, {17, 20, 10}, {21, 24, 12}, {25, 32, 16}, {33, 36, 32}, {37, 40, 64}};
    for (const auto& row : want)
        for (int w = row[0]; w <= row[1]; ++w)
            if (vlg::bw_group(vlg::bw_piece_of(41, w, waves)) != row[2]) fail(41, w, "not the documented group size");
    std::printf("%d widths of %d sentences: %d failures\n", widths, vlg::kShortN - 1, failures);
    return failures == 0 ? 0 : 1;
}
