// plan_short.cpp -- the stationary cells of the short image's outside pass (vlg_dp_core.h: dmv_bw_segment_p).  TEST INFRASTRUCTURE ONLY.
//
// A stand-alone program (its own main) against vlgae_amd/csrc/vlg_dp_core.h.  Since round 11 a lane of the outside pass reads xa,
// the cell CR(i, i + r) of its split point, once per piece, and keeps that cell's adjoint word in a register over the widths of the
// piece: loaded at the piece's start, summed, written through with every contribution.  That is the parent's read-modify-write
// through LDS exactly if (1) the addresses are stationary over the piece and (2) nobody else stores to the word while the lane holds
// it.  For every tensor width N = 2 ... 41 (every chart pitch), every sentence Ne <= N, both directions, every piece and every lane
// this program
//   * checks that the reference index formulas (dmv_bw_addr) give the same vXA / aXA at EVERY width of a piece as at its first, and
//     that BwAddr's steps reproduce dmv_bw_addr's other addresses at every width (the value set one width ahead);
//   * replays the pass on counters: a chart of integers in place of gCi, every lane's register copy loaded where the kernel loads it,
//     +1 where the kernel adds a weight, stored where the kernel stores.  Every word must have ONE writer per piece -- (lane, term,
//     walk) -- and when the span that owns a cell reads it as `gb` (CR(i, i + r) at width r, CL(j, k) at width j - k) the word in the
//     chart must hold every contribution: Ne - 1 - i - r per component for CR(i, i + r), k for CL(j, k).  At the end of the pass the
//     width-0 cells the count write-out reads are checked the same way.
// It is built with -fsanitize=address,undefined by tests/test_dmv_short_plan_host.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../vlgae_amd/csrc/vlg_dp_core.h"

namespace {

constexpr int kLanesPerDir = 256;
int failures = 0;
long long checked_addr = 0, checked_reads = 0;

void fail(int N, int Ne, int w, const char* what) {
    if (++failures <= 20) std::printf("FAIL N %d Ne %d w %d: %s\n", N, Ne, w, what);
}

struct PlanX {
    template <typename T>
    T* pin(T* p) { return p; }
    bool uniform(bool v) { return v; }
    int uniform(int v) { return v; }
};

bool same_addr(const vlg::BwAddr& a, const vlg::BwAddr& b, bool vals) {
    if (vals) return a.vC == b.vC && a.vI == b.vI && a.vS == b.vS && a.vSU == b.vSU && a.vUU == b.vUU && a.vVV == b.vVV && a.vXA == b.vXA && a.vXB == b.vXB;
    return a.aGc == b.aGc && a.aGi == b.aGi && a.aI == b.aI && a.aUU == b.aUU && a.aVV == b.aVV && a.aXA == b.aXA && a.aXB == b.aXB;
}

struct Sim {
    int N, Ne, P;
    std::vector<unsigned char> arena;   // never dereferenced through the addresses: it only keeps the pointer arithmetic inside one object
    vlg::DmvCtx c;
    std::vector<int> mem;               // the chart gCi as counters, one per 4-byte word
    std::vector<int> owner;             // per word, in the current piece: the (direction, lane, term) that holds it in a register, -2 = stored through the chart, -1 = untouched
    size_t words;

    Sim(int N_, int Ne_) : N(N_), Ne(Ne_), P(vlg::chart_pitch(N_)) {
        const vlg::DmvLayout L(N, true, false, 0, false);
        const size_t slack = 64 * 1024;   // tests/emu/emu_short.cpp: far_read_bytes(41) <= 64 KB
        arena.assign(L.lds_bytes + slack, 0);
        char* A = reinterpret_cast<char*>(arena.data());
        std::memset(&c, 0, sizeof c);
        c.Ne = Ne; c.len = Ne - 1; c.P = P;
        c.C = (float2*)(A + L.C.off); c.I = (float2*)(A + L.I.off); c.C2 = c.C; c.I2 = c.I;
        c.S = (float*)(A + L.S.off);
        c.gCc = (float*)(A + L.gCc.off); c.gCi = (float2*)(A + L.gCi.off); c.gI = (float2*)(A + L.gI.off);
        words = (size_t)2 * N * P;
        mem.assign(words, 0);
        owner.assign(words, -1);
    }
    // word index of a gCi byte address, or -1 when it lies outside the chart's Ne rows (a dead lane's shadow)
    long word_of(const char* p) const {
        const long off = p - reinterpret_cast<const char*>(c.gCi);
        if (off < 0 || off % 4 || (size_t)(off / 4) >= words) return -1;
        return off / 4;
    }

    template <int K>
    void piece(int w0, int w1) {
        constexpr int G = vlg::bw_group(K), TM = vlg::bw_terms(K);
        if (w1 <= w0) return;
        PlanX x;
        std::fill(owner.begin(), owner.end(), -1);
        struct Lane { vlg::BwAddr a; int slot, rr, D; int reg[TM]; };
        std::vector<Lane> lanes((size_t)2 * kLanesPerDir);
        for (int dir = 0; dir < 2; ++dir)
            for (int t = 0; t < kLanesPerDir; ++t) {
                Lane& ln = lanes[(size_t)dir * kLanesPerDir + t];
                const vlg::BwLane b = vlg::bw_lane<G>(t);
                ln.slot = b.slot; ln.rr = b.rr;
                ln.D = b.slot < Ne - w0 ? b.slot * (P + 1) : 0;
                ln.a = vlg::dmv_bw_addr<G>(c, w1 - 1, ln.D, ln.rr, dir == 1, x);
                ln.a.step_vals();
                for (int u = 0; u < TM; ++u) {   // the register copy, loaded at the piece's start
                    const long wd = word_of(ln.a.aXA + u * G * 8);
                    ln.reg[u] = wd >= 0 ? mem[wd] : 0;
                }
            }
        for (int w = w1 - 1; w >= w0; --w) {
            const int spans = Ne - w;
            // every lane reads before any lane stores (one barrier per width; the groups' lockstep is inside it)
            for (int dir = 0; dir < 2; ++dir)
                for (int t = 0; t < kLanesPerDir; ++t) {
                    Lane& ln = lanes[(size_t)dir * kLanesPerDir + t];
                    const vlg::BwAddr ref = vlg::dmv_bw_addr<G>(c, w, ln.D, ln.rr, dir == 1, x);
                    if (!same_addr(ln.a, ref, false)) fail(N, Ne, w, "a stepped adjoint address differs from dmv_bw_addr's");
                    if (w >= 1) {   // the value set runs one width ahead
                        const vlg::BwAddr refv = vlg::dmv_bw_addr<G>(c, w - 1, ln.D, ln.rr, dir == 1, x);
                        if (!same_addr(ln.a, refv, true)) fail(N, Ne, w, "a stepped value address differs from dmv_bw_addr's one width ahead");
                    }
                    ++checked_addr;
                    if (ln.slot >= spans) continue;
                    // the own cell, read as gb: complete with every contribution of the wider spans
                    const int i = ln.slot, j = i + w;
                    const long own = word_of(ln.a.aGi);
                    if (own < 0) { fail(N, Ne, w, "a live span's own gCi cell lies outside the chart"); continue; }
                    const int want = dir == 1 ? Ne - 1 - j : i;   // CR(i, j): spans (i, j') with j' > j   |   CL(j, i): spans (i', j) with i' < i
                    if (ln.rr == 0) {
                        if (mem[own] != want || mem[own + 1] != want) fail(N, Ne, w, "the own cell's adjoint is read before it is complete (or after too much)");
                        ++checked_reads;
                    }
                }
            for (int dir = 0; dir < 2; ++dir)
                for (int t = 0; t < kLanesPerDir; ++t) {
                    Lane& ln = lanes[(size_t)dir * kLanesPerDir + t];
                    if (ln.slot >= spans) continue;
                    for (int u = 0; u < TM; ++u) {
                        const int r = ln.rr + u * G;
                        if (r >= w) continue;
                        const int me = (dir * kLanesPerDir + t) * 2 + u;
                        const long wa = word_of(ln.a.aXA + u * G * 8), wb = word_of(ln.a.aXB + u * G * 8);
                        if (wa < 0 || wb < 0) { fail(N, Ne, w, "a live term stores outside the chart"); continue; }
                        if (owner[wa] != -1 && owner[wa] != me) fail(N, Ne, w, "a stationary word has a second writer inside the piece");
                        if (owner[wb] >= 0) fail(N, Ne, w, "a read-modify-write through the chart hits a word that a lane holds in a register");
                        owner[wa] = me;
                        owner[wb] = -2;         // the moving walk xb: other spans' lanes add to the same word at other widths, through the chart
                        ln.reg[u] += 1;         // gxa[u] += ws
                        mem[wa] = ln.reg[u];    // written through
                        mem[wb] += 1;           // read-modify-write through the chart
                    }
                }
            for (Lane& ln : lanes) { ln.a.step_vals(); ln.a.step_adj(); }
        }
    }

    void run() {
        const vlg::BwSched bs = vlg::bw_sched(Ne, vlg::bw_waves(kLanesPerDir));
        piece<6>(bs.first[6], bs.first[7]);
        piece<5>(bs.first[5], bs.first[6]);
        piece<4>(bs.first[4], bs.first[5]);
        piece<3>(bs.first[3], bs.first[4]);
        piece<2>(bs.first[2], bs.first[3]);
        piece<1>(bs.first[1], bs.first[2]);
        piece<0>(bs.first[0], bs.first[1]);
        // the width-0 cells the count write-out reads: CL(h, h) at (h, h), CR(h, h) at (h, h + 1)
        for (int h = 0; h < Ne; ++h)
            for (int dir = 0; dir < 2; ++dir) {
                const size_t wd = (size_t)2 * (h * P + h + dir);
                const int want = dir == 1 ? Ne - 1 - h : h;
                if (mem[wd] != want || mem[wd + 1] != want) fail(N, Ne, 0, "a width-0 cell does not hold every contribution at the end of the pass");
                ++checked_reads;
            }
    }
};
static_assert(vlg::kBwPieces == 7, "Sim::run names every entry of the table");

}  // namespace

int main() {
    int sentences = 0;
    for (int N = 2; N <= vlg::kShortN; ++N)
        for (int Ne = 2; Ne <= N; ++Ne, ++sentences) {
            Sim s(N, Ne);
            s.run();
        }
    std::printf("%d (N, Ne) pairs, %lld lane-width address sets, %lld own-cell reads: %d failures\n", sentences, checked_addr, checked_reads, failures);
    return failures == 0 ? 0 : 1;
}
