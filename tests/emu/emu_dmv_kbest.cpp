// emu_dmv_kbest.cpp -- HOST EMULATOR of the DMV1o k-best workgroup and of the tree-counts workgroup (vlgae_amd/csrc/vlg_dmv_kbest.hip).
// TEST INFRASTRUCTURE ONLY.
//
// The charts are filled by the SAME bodies the gfx950 kernel runs (vlg_dmv_kbest.h: dmv_kbest_fill / dmv_kbest_span) under the token
// barrier of emu_dp.cpp, `nt` host threads as lanes; behind it the same walk (dmv_kbest_walk) extracts every rank under a host policy
// whose "wavefront" is one lane.  The charts and the walk's stacks are carved as the kernel carves them (DmvKbestLayout, at the
// placement mode the caller asks for: the spilled modes run at any N, with a second arena as the workspace), with the canary of
// emu_dp.cpp behind each arena.  The workspace arena is pre-filled with a NaN pattern: nothing may depend on what it held.  The tree
// counts run dmv_tree_counts_lane lane after lane, tree after tree.
//
// Built two ways: as a shared library for ctypes calls (tests/test_dmv_kbest_host.py), and, with -DEMU_DMV_KBEST_MAIN, as a
// stand-alone program for the sanitizers, which replays a case file written by the test.
#include "emu_dp.cpp"

#include "emu_kbest_common.h"
#include "../../vlgae_amd/csrc/vlg_dmv_kbest.h"

#include <cstdio>

namespace {

// plant: -1, or a 16-bit value written over the back-pointer of rank 0 of the root cell before the walks (the walk's give-up rules)
template <int KC>
void dmv_kbest_one(const vlg::DmvKbPot& pot, int len, int b, int B, int N, int K, int mode, int plant, long long* heads, float* scores,
                   int32_t* count, int nt, int order) {
    const vlg::DmvKbestLayout L(N, KC, mode);
    KbArenas m(L.lds_bytes, L.ws_bytes);
    vlg::DmvKbCtx c;
    c.Ne = len + 1; c.len = len; c.P = vlg::chart_pitch(N); c.cells = N * c.P;
    c.C = m.at<float>(L.C); c.T = m.at<float>(L.T); c.A = m.at<float>(L.A);
    c.bT = m.at<unsigned short>(L.bT); c.bC = m.at<unsigned short>(L.bC);
    run_workgroup(nt, order, [&](int tid, HostX& x) { vlg::dmv_kbest_fill<KC>(c, pot, N, tid, nt, x); });
    if (count) count[b] = vlg::dmv_kbest_count(c, K);
    if (plant >= 0) c.bC[len + 1 + c.cells] = (unsigned short)plant;   // CR(0,len).NC[0]
    kbest_each_rank(b, B, N, K, m.at<int>(L.stack), heads, scores,
                    [&](int k, int* stack, long long* h, float* s, KbSeqX& x) { vlg::dmv_kbest_walk<KC>(c, k, N, stack, h, s, x); });
    m.check();
}

int dmv_kbest_batch(const void* dec, const void* attach, const int64_t* lengths, int B, int N, int in_dtype, int K, int mode, const int* plant,
                    long long* heads, float* scores, int32_t* count, int nt, int order) {
    if (K < 1 || K > vlg::kKbestMaxK || N < 2 || N > 255) return -1;
    const vlg::KbestPlan p = vlg::dmv_kbest_plan(N, K, vlg::kLdsBudget);
    if (mode < 0) mode = p.mode;
    for (int b = 0; b < B; ++b) {
        const int len = (int)lengths[b];
        if (kbest_no_sentence(len, b, B, N, K, heads, scores, count)) continue;
        const vlg::DmvKbPot pot{dec, attach, (size_t)b * N * 8, (size_t)b * N * N * 2, in_dtype};
        kbest_image_switch(p.KC, [&](auto kc) {
            dmv_kbest_one<decltype(kc)::value>(pot, len, b, B, N, K, mode, plant ? plant[b] : -1, heads, scores, count, nt, order);
        });
    }
    return 0;
}

}  // namespace

// heads [K,B,N], scores [K,B], count [B] (optional); mode: the DmvKbestLayout placement to emulate (any N), or -1 for the plan's own
extern "C" int emu_dmv1o_kbest(const void* dec, const void* attach, const int64_t* lengths, int B, int N, int in_dtype, int K, int mode,
                               long long* heads, float* scores, int32_t* count, int nt, int order) {
    return dmv_kbest_batch(dec, attach, lengths, B, N, in_dtype, K, mode, nullptr, heads, scores, count, nt, order);
}

// the same with plant [B]: per sentence -1, or the value that replaces the back-pointer of rank 0 of its root cell behind the fill
extern "C" int emu_dmv1o_kbest_planted(const void* dec, const void* attach, const int64_t* lengths, int B, int N, int in_dtype, int K,
                                       int mode, const int* plant, long long* heads, float* scores, int32_t* count, int nt, int order) {
    return dmv_kbest_batch(dec, attach, lengths, B, N, in_dtype, K, mode, plant, heads, scores, count, nt, order);
}

extern "C" void emu_dmv_kbest_plan(int N, int K, long long* out) { kbest_plan_export<vlg::DmvKbestLayout>(N, K, out); }

// vlg_dmv1o_tree_counts: the kernel's frame around dmv_tree_counts_lane, one lane after the other
extern "C" int emu_dmv1o_tree_counts(const long long* heads, const int64_t* lengths, const int32_t* count, const float* weight, int T, int B,
                                     int N, float* cnt_dec, float* cnt_attach) {
    if (N < 2 || N > 255 || T < 0) return -1;
    for (int b = 0; b < B; ++b) {
        float* ca = cnt_attach + (size_t)b * N * N * 2;
        for (int i = 0; i < N * N * 2; ++i) ca[i] = 0.f;
        std::vector<float> acc((size_t)N * 8, 0.f);
        const int len = (int)lengths[b];
        if (len >= 1 && len <= N - 1) {
            const int live = count ? std::min((int)count[b], T) : T;
            for (int t = 0; t < live; ++t) {
                std::vector<int> hs(N);
                for (int i = 0; i < N; ++i) {
                    const long long h = i >= 1 && i <= len ? heads[((size_t)t * B + b) * N + i] : -1;
                    hs[i] = h >= 0 && h <= len && h != i ? (int)h : -1;
                }
                for (int i = 0; i < N; ++i)
                    vlg::dmv_tree_counts_lane(hs.data(), len, N, i, weight ? weight[(size_t)t * B + b] : 1.f, ca, acc.data() + (size_t)i * 8);
            }
        }
        for (int i = 0; i < N * 8; ++i) cnt_dec[(size_t)b * N * 8 + i] = acc[i];
    }
    return 0;
}

#ifdef EMU_DMV_KBEST_MAIN
// emu_dmv_kbest CASEFILE: int32 B, N, K, mode; int64 lengths[B]; float dec[B N 8]; float attach[B N N 2]; float expect_scores[K B];
// int64 expect_heads[K B N]; float expect_cnt_dec[B N 8]; float expect_cnt_attach[B N N 2] (the counts of all K ranks, weight 1).
// Exit status 0 iff everything comes back exactly and no canary tripped.
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[4];
    if (std::fread(hdr, sizeof(int), 4, f) != 4) return 2;
    const int B = hdr[0], N = hdr[1], K = hdr[2], mode = hdr[3];
    std::vector<int64_t> lengths(B);
    std::vector<float> dec((size_t)B * N * 8), att((size_t)B * N * N * 2), es((size_t)K * B), scores((size_t)K * B);
    std::vector<float> ecd(dec.size()), eca(att.size()), cd(dec.size(), -1.f), ca(att.size(), -1.f);
    std::vector<long long> eh((size_t)K * B * N), heads((size_t)K * B * N, -1);
    std::vector<int32_t> count(B);
    auto rd = [&](void* p, size_t esz, size_t n) { return std::fread(p, esz, n, f) == n; };
    bool ok = rd(lengths.data(), 8, lengths.size()) && rd(dec.data(), 4, dec.size()) && rd(att.data(), 4, att.size()) && rd(es.data(), 4, es.size()) &&
              rd(eh.data(), 8, eh.size()) && rd(ecd.data(), 4, ecd.size()) && rd(eca.data(), 4, eca.size());
    std::fclose(f);
    if (!ok) return 2;
    if (emu_dmv1o_kbest(dec.data(), att.data(), lengths.data(), B, N, 0, K, mode, heads.data(), scores.data(), count.data(), 8, 2) != 0) return 2;
    if (emu_dmv1o_tree_counts(heads.data(), lengths.data(), count.data(), nullptr, K, B, N, cd.data(), ca.data()) != 0) return 2;
    int bad = 0;
    for (size_t i = 0; i < heads.size(); ++i) bad += heads[i] != eh[i];
    for (size_t i = 0; i < scores.size(); ++i) bad += std::memcmp(&scores[i], &es[i], 4) != 0;
    for (size_t i = 0; i < cd.size(); ++i) bad += cd[i] != ecd[i];
    for (size_t i = 0; i < ca.size(); ++i) bad += ca[i] != eca[i];
    std::printf("emu_dmv_kbest: B=%d N=%d K=%d mode=%d mismatches=%d canary_trips=%d\n", B, N, K, mode, bad, emu_canary_trips());
    return bad == 0 && emu_canary_trips() == 0 ? 0 : 1;
}
#endif
