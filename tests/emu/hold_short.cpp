// hold_short.cpp -- the cells the short image keeps in registers over a piece since round 12 (vlg_dp_core.h: dmv_bw_dir_p's BwHeld,
// dmv_fw_piece_p's FwHeld).  TEST INFRASTRUCTURE ONLY.
//
// A stand-alone program (its own main) against vlgae_amd/csrc/vlg_dp_core.h, beside plan_short.cpp (round 11: xa and its gCi word).
// For every tensor width N = 2 ... 41 (every chart pitch), every sentence Ne <= N, both directions, every piece and every lane:
//
// OUTSIDE pass.  The left direction keeps its column walk (uu, and the gCc word through aUU), the right direction its row walk (vv,
// and the gI cell through aVV).  That is the parent's read-modify-write through LDS exactly if
//   * dmv_bw_addr names the same vUU / aUU (left), vVV / aVV (right) at EVERY width of a piece;
//   * a counter replay of gCc and gI -- an integer per cell, every holder's register loaded where the kernel loads it, +1 where the
//     kernel adds a weight, stored where it stores; every walk that moves read in the width's first half and stored back in its second
//     half, as the kernel does -- finds ONE holder (lane, term) per held word and piece, the chart and the register in agreement
//     before every add, no read-modify-write through the chart on a held word, and as the only other store to a held word the right
//     direction's own-cell store at w = r + 1, after which the holder adds nothing;
//   * every read through the chart finds all contributions: `ga` (the own gCc cell at the span's width), `gi_old` (the own gI cell,
//     w = r + 1 for its holder), and at the end of the pass every gI cell (the attach counts and the GO-count row sums) and the
//     width-0 cells of gCc (the STOP counts).  Contributions, by the recurrences: gCc[CL(k, i)] Ne - 1 - k, gCc[CR(k, j)] k,
//     gI[IL(j, k)] k, gI[IR(i, k)] Ne - 1 - k.
//
// INSIDE pass.  For every segment of make_sched as dmv_fw_all runs it, every piece TU, direction, lane and term u < TU - 1:
//   * eA names CR(i, i + r), eU (left) CL(i + r, i), eV (right) IR(i, i + 1 + r), r = rr + u G -- cells of width r, r, r + 1, all
//     below the piece's first width: written before the piece begins;
//   * FwAddr<DIR>::step() leaves those addresses unchanged from the piece's first width to its last.
// It is built with -fsanitize=address,undefined by tests/test_dmv_short_hold_host.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../vlgae_amd/csrc/vlg_dp_core.h"

namespace {

constexpr int kLanesPerDir = 256;
int failures = 0;
long long checked_addr = 0, checked_reads = 0, checked_held = 0, checked_fw = 0;

void fail(int N, int Ne, int w, const char* what) {
    if (++failures <= 20) std::printf("FAIL N %d Ne %d w %d: %s\n", N, Ne, w, what);
}

struct PlanX {
    template <typename T>
    T* pin(T* p) { return p; }
    bool uniform(bool v) { return v; }
    int uniform(int v) { return v; }
};

struct Sim {
    int N, Ne, P;
    std::vector<unsigned char> arena;   // never dereferenced through the addresses: it only keeps the pointer arithmetic inside one object
    vlg::DmvCtx c;
    size_t cells;
    // counters, one per chart cell (both components of a gI cell take their weights together)
    std::vector<int> memC, memI;
    std::vector<int> ownC, ownI;        // per cell, in the current piece: the (direction, lane, term) that holds it, -2 = stored through the chart, -1 = untouched
    std::vector<char> closedI;          // a held gI cell whose own-cell store has happened: its holder must add nothing more
    std::vector<int> own_stores;        // per gI cell: how often a span stored its complete adjoint there

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
        cells = (size_t)N * P;
        memC.assign(cells, 0); memI.assign(cells, 0);
        ownC.assign(cells, -1); ownI.assign(cells, -1);
        closedI.assign(cells, 0);
        own_stores.assign(cells, 0);
    }
    // cell index of a byte address in a chart of `size`-byte cells at `base`, or -1 outside the chart's N rows (a dead lane's shadow)
    long cell_of(const char* p, const void* base, int size) const {
        const long off = p - reinterpret_cast<const char*>(base);
        if (off < 0 || off % size || (size_t)(off / size) >= cells) return -1;
        return off / size;
    }
    long cellC(const char* p) const { return cell_of(p, c.gCc, 4); }
    long cellI(const char* p) const { return cell_of(p, c.gI, 8); }

    // ---- outside pass -------------------------------------------------------------------------------------------------------------
    template <int K>
    void bw_piece(int w0, int w1) {
        constexpr int G = vlg::bw_group(K), TM = vlg::bw_terms(K);
        if (w1 <= w0) return;
        PlanX x;
        std::fill(ownC.begin(), ownC.end(), -1);
        std::fill(ownI.begin(), ownI.end(), -1);
        std::fill(closedI.begin(), closedI.end(), 0);
        struct Lane { vlg::BwAddr a, first; int slot, rr, D; int reg[TM]; int old_mov[TM]; int old_own; };
        std::vector<Lane> lanes((size_t)2 * kLanesPerDir);
        for (int dir = 0; dir < 2; ++dir)
            for (int t = 0; t < kLanesPerDir; ++t) {
                Lane& ln = lanes[(size_t)dir * kLanesPerDir + t];
                const vlg::BwLane b = vlg::bw_lane<G>(t);
                ln.slot = b.slot; ln.rr = b.rr;
                ln.D = b.slot < Ne - w0 ? b.slot * (P + 1) : 0;
                ln.a = vlg::dmv_bw_addr<G>(c, w1 - 1, ln.D, ln.rr, dir == 1, x);
                ln.first = ln.a;
                ln.a.step_vals();
                for (int u = 0; u < TM; ++u) {   // the register copy, loaded at the piece's start (dmv_bw_load_held)
                    const long cl = dir == 0 ? cellC(ln.a.aUU + u * ln.a.gp4) : cellI(ln.a.aVV + u * G * 8);
                    ln.reg[u] = cl >= 0 ? (dir == 0 ? memC[cl] : memI[cl]) : 0;
                }
            }
        for (int w = w1 - 1; w >= w0; --w) {
            const int spans = Ne - w;
            // first half of every body: the reads (one barrier per width; the groups' lockstep is inside it)
            for (int dir = 0; dir < 2; ++dir)
                for (int t = 0; t < kLanesPerDir; ++t) {
                    Lane& ln = lanes[(size_t)dir * kLanesPerDir + t];
                    // the stationary walk of the direction: the reference formulas at this width and one width ahead (the value set)
                    const vlg::BwAddr ref = vlg::dmv_bw_addr<G>(c, w, ln.D, ln.rr, dir == 1, x);
                    const vlg::BwAddr refv = vlg::dmv_bw_addr<G>(c, w > 0 ? w - 1 : 0, ln.D, ln.rr, dir == 1, x);
                    if (dir == 0) {
                        if (ref.aUU != ln.first.aUU || ref.vUU != ln.first.vUU || refv.vUU != ln.first.vUU) fail(N, Ne, w, "left: the column walk moves inside a piece");
                        if (ln.a.aUU != ln.first.aUU || ln.a.vUU != ln.first.vUU) fail(N, Ne, w, "left: BwAddr's steps move the column walk");
                    } else {
                        if (ref.aVV != ln.first.aVV || ref.vVV != ln.first.vVV || refv.vVV != ln.first.vVV) fail(N, Ne, w, "right: the row walk moves inside a piece");
                        if (ln.a.aVV != ln.first.aVV || ln.a.vVV != ln.first.vVV) fail(N, Ne, w, "right: BwAddr's steps move the row walk");
                    }
                    if (ref.gp4 != ln.first.gp4 || ref.gp8 != ln.first.gp8) fail(N, Ne, w, "the term stride changes inside a piece");
                    ++checked_addr;
                    if (ln.slot >= spans) continue;
                    const int i = ln.slot, j = i + w;
                    const long oc = cellC(ln.a.aGc), oi = cellI(ln.a.aI);
                    if (oc < 0 || oi < 0) { fail(N, Ne, w, "a live span's own cell lies outside the chart"); continue; }
                    if (oc != (dir == 0 ? (long)j * P + i : (long)i * P + j + 1) || oi != oc) fail(N, Ne, w, "the own cell is not CL(j, i) | CR(i, j)");
                    // ga and gi_old, read by every lane of the group: complete with every contribution of the wider spans
                    if (memC[oc] != (dir == 0 ? Ne - 1 - j : i)) fail(N, Ne, w, "ga: the own gCc cell is read before it is complete (or after too much)");
                    if (memI[oi] != (dir == 0 ? i : Ne - 1 - j)) fail(N, Ne, w, "gi_old: the own gI cell is read before it is complete (or after too much)");
                    checked_reads += 2;
                    ln.old_own = memI[oi];
                    for (int u = 0; u < TM; ++u) {   // the read half of the moving walk's read-modify-write
                        const long cl = dir == 0 ? cellI(ln.a.aVV + u * G * 8) : cellC(ln.a.aUU + u * ln.a.gp4);
                        ln.old_mov[u] = cl >= 0 ? (dir == 0 ? memI[cl] : memC[cl]) : 0;
                    }
                }
            // second half: the stores
            for (int dir = 0; dir < 2; ++dir)
                for (int t = 0; t < kLanesPerDir; ++t) {
                    Lane& ln = lanes[(size_t)dir * kLanesPerDir + t];
                    if (ln.slot >= spans) continue;
                    const int selfr = dir == 0 ? 0 : w - 1;
                    for (int u = 0; u < TM; ++u) {
                        const int r = ln.rr + u * G;
                        if (r >= w) continue;
                        const int me = (dir * kLanesPerDir + t) * 2 + u;
                        const long cu = cellC(ln.a.aUU + u * ln.a.gp4), cv = cellI(ln.a.aVV + u * G * 8);
                        if (cu < 0 || cv < 0) { fail(N, Ne, w, "a live term stores outside the chart"); continue; }
                        if (dir == 0) {
                            // held: gCc[CL(i + r, i)]
                            if (cu != (long)(ln.slot + r) * P + ln.slot) fail(N, Ne, w, "left: the held word is not gCc[CL(i + r, i)]");
                            if (ownC[cu] != -1 && ownC[cu] != me) fail(N, Ne, w, "left: a held gCc word has a second writer inside the piece");
                            if (ln.reg[u] != memC[cu]) fail(N, Ne, w, "left: the chart and the holder's register disagree");
                            ownC[cu] = me;
                            memC[cu] = ++ln.reg[u];   // guu[u] += w0 + w1, written through
                            ++checked_held;
                            // moving: gI[IL(j, i + r)], r != 0, through the chart
                            if (r != selfr) {
                                if (ownI[cv] >= 0) fail(N, Ne, w, "left: a read-modify-write through the chart hits a gI cell that a lane holds");
                                ownI[cv] = -2;
                                memI[cv] = ln.old_mov[u] + 1;
                            }
                        } else {
                            // held: gI[IR(i, i + 1 + r)], not at r == selfr (its own cell at this width)
                            if (cv != (long)ln.slot * P + ln.slot + r + 2) fail(N, Ne, w, "right: the held word is not gI[IR(i, i + 1 + r)]");
                            if (r != selfr) {
                                if (ownI[cv] != -1 && ownI[cv] != me) fail(N, Ne, w, "right: a held gI cell has a second writer inside the piece");
                                if (closedI[cv]) fail(N, Ne, w, "right: the holder adds to its cell after the span's own-cell store");
                                if (ln.reg[u] != memI[cv]) fail(N, Ne, w, "right: the chart and the holder's register disagree");
                                ownI[cv] = me;
                                memI[cv] = ++ln.reg[u];   // gvv[u] += (w0, w1), written through
                                ++checked_held;
                            }
                            // moving: gCc[CR(i + 1 + r, j)] through the chart
                            if (ownC[cu] >= 0) fail(N, Ne, w, "right: a read-modify-write through the chart hits a gCc word that a lane holds");
                            ownC[cu] = -2;
                            memC[cu] = ln.old_mov[u] + 1;
                        }
                    }
                    if (ln.rr == 0) {   // the own-cell store: gi = gi_old + the same-width term, the count of contributions unchanged
                        const long oi = cellI(ln.a.aI);
                        if (oi < 0) continue;
                        if (memI[oi] != ln.old_own) fail(N, Ne, w, "the own gI cell changed between gi_old and the own-cell store");
                        if (ownI[oi] >= 0) {   // a held cell: only the right direction's, at the holder's w = r + 1
                            const int hold = ownI[oi] / 2, hu = ownI[oi] % 2, hdir = hold / kLanesPerDir;
                            const Lane& hl = lanes[(size_t)hold];
                            if (dir != 1 || hdir != 1) fail(N, Ne, w, "an own-cell store hits a held cell outside the right direction");
                            if (hl.rr + hu * G != w - 1 || hl.slot != ln.slot) fail(N, Ne, w, "an own-cell store hits a held cell at a width other than r + 1 of its holder");
                            if (hl.reg[hu] != memI[oi]) fail(N, Ne, w, "the own-cell store overwrites a contribution the chart does not hold");
                        }
                        closedI[oi] = 1;
                        ++own_stores[oi];
                        memI[oi] = ln.old_own;
                    }
                }
            for (Lane& ln : lanes) { ln.a.step_vals(); ln.a.step_adj(); }
        }
    }

    void run_bw() {
        const vlg::BwSched bs = vlg::bw_sched(Ne, vlg::bw_waves(kLanesPerDir));
        bw_piece<6>(bs.first[6], bs.first[7]);
        bw_piece<5>(bs.first[5], bs.first[6]);
        bw_piece<4>(bs.first[4], bs.first[5]);
        bw_piece<3>(bs.first[3], bs.first[4]);
        bw_piece<2>(bs.first[2], bs.first[3]);
        bw_piece<1>(bs.first[1], bs.first[2]);
        bw_piece<0>(bs.first[0], bs.first[1]);
        // what the count write-out reads: every gI cell (attach counts, GO-count row sums), the width-0 cells of gCc (STOP counts)
        for (int h = 0; h < Ne; ++h) {
            for (int k = 0; k < Ne; ++k) {
                if (k == h) continue;
                const size_t cl = (size_t)h * P + (k < h ? k : k + 1);
                const int want = k < h ? k : Ne - 1 - k;   // IL(h, k): spans (i', h), i' < k  |  IR(h, k): spans (h, j), j > k
                if (memI[cl] != want) fail(N, Ne, 0, "a gI cell does not hold every contribution at the end of the pass");
                if (own_stores[cl] != 1) fail(N, Ne, 0, "a gI cell has not taken exactly one own-cell store");
                ++checked_reads;
            }
            if (memC[(size_t)h * P + h] != Ne - 1 - h) fail(N, Ne, 0, "gCc[CL(h, h)] does not hold every contribution at the end of the pass");
            if (memC[(size_t)h * P + h + 1] != h) fail(N, Ne, 0, "gCc[CR(h, h)] does not hold every contribution at the end of the pass");
            checked_reads += 2;
        }
    }

    // ---- inside pass --------------------------------------------------------------------------------------------------------------
    // the width at which the inside pass writes the cell at a byte address in C / I (0: the load stage), -1 outside the chart
    int produced_at(const char* p, const void* base) const {
        const long cl = cell_of(p - (p - reinterpret_cast<const char*>(base)) % 8, base, 8);
        if (cl < 0) return -1;
        const int row = (int)(cl / P), col = (int)(cl % P);
        return col <= row ? row - col : col - 1 - row;   // CL(row, col) | IL(row, col);  CR(row, col - 1) | IR(row, col - 1)
    }

    template <int DIR, int LG, int TM>
    void fw_dir(int w0, int w1) {
        constexpr int G = 1 << LG;
        PlanX x;
        for (int t = 0; t < kLanesPerDir; ++t) {
            const int rr = t & (G - 1), slot = t >> LG;
            const int D = slot < Ne - w0 ? slot * (P + 1) : 0;   // dmv_fw_dir_p
            vlg::FwAddr<DIR> a = vlg::dmv_fw_addr<DIR, G, false>(c, w0, D, rr, x);
            for (int k = 1; k <= TM; ++k) {   // dmv_fw_dir_p's pieces
                const int lo = (k - 1) * G + 1, hi = k == TM ? w1 : k * G + 1;
                const int wa = w0 > lo ? w0 : lo, wb = w1 < hi ? w1 : hi;
                const vlg::FwAddr<DIR> first = a;
                for (int w = wa; w < wb; ++w) {
                    for (int u = 0; u < k - 1; ++u) {
                        const int r = rr + u * G;
                        const char* eS = DIR == 0 ? a.eU + u * a.gp8 : a.eV + u * G * 8;
                        const char* fS = DIR == 0 ? first.eU + u * first.gp8 : first.eV + u * G * 8;
                        if (a.eA != first.eA || eS != fS) fail(N, Ne, w, "inside: step() moves a held address");
                        if (slot < Ne - w) {   // a live lane: the cells and their producing widths
                            const int i = slot;
                            const long ca = cell_of(a.eA + u * G * 8 - (DIR == 0 ? 4 : 0), c.C, 8);
                            const long cs = DIR == 0 ? cell_of(eS - 4, c.C, 8) : cell_of(eS, c.I, 8);
                            if (ca != (long)i * P + i + r + 1) fail(N, Ne, w, "inside: eA is not CR(i, i + r)");
                            if (cs != (DIR == 0 ? (long)(i + r) * P + i : (long)i * P + i + r + 2)) fail(N, Ne, w, "inside: eU | eV is not CL(i + r, i) | IR(i, i + 1 + r)");
                            const int pa = produced_at(a.eA + u * G * 8, c.C), ps = produced_at(eS, DIR == 0 ? (const void*)c.C : (const void*)c.I);
                            if (pa != r || ps != (DIR == 0 ? r : r + 1)) fail(N, Ne, w, "inside: a held cell has an unexpected width");
                            if (pa < 0 || pa >= wa || ps < 0 || ps >= wa) fail(N, Ne, w, "inside: a held cell is written inside the piece");
                        }
                        ++checked_fw;
                    }
                    a.step();
                }
            }
        }
    }
    template <int LG, int TM>
    void fw_segment(int w0, int w1) {
        if (w1 <= w0) return;
        fw_dir<0, LG, TM>(w0, w1);
        fw_dir<1, LG, TM>(w0, w1);
    }
    template <int LG>
    void fw_segment(int w0, int w1) { fw_segment<LG, vlg::short_tmax(LG, vlg::kShortN, VLG_DP_LANES_FW)>(w0, w1); }

    void run_fw() {   // dmv_fw_all, the short image
        const vlg::Sched sc = vlg::make_sched(Ne, kLanesPerDir, VLG_DP_LANES_FW);
        fw_segment<0, 2>(sc.first[0], sc.first[2]);
        fw_segment<2>(sc.first[2], sc.first[3]);
        fw_segment<3>(sc.first[3], sc.first[4]);
        fw_segment<4>(sc.first[4], sc.first[5]);
        fw_segment<5>(sc.first[5], sc.first[6]);
        fw_segment<6>(sc.first[6], sc.first[7]);
    }
};
static_assert(vlg::kBwPieces == 7, "Sim::run_bw names every entry of the table");

}  // namespace

int main() {
    int sentences = 0;
    for (int N = 2; N <= vlg::kShortN; ++N)
        for (int Ne = 2; Ne <= N; ++Ne, ++sentences) {
            Sim s(N, Ne);
            s.run_bw();
            s.run_fw();
        }
    std::printf("%d (N, Ne) pairs, %lld lane-width address sets, %lld chart reads, %lld held adds, %lld held inside terms: %d failures\n", sentences,
                checked_addr, checked_reads, checked_held, checked_fw, failures);
    return failures == 0 ? 0 : 1;
}
