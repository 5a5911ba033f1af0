// emu_kbest.cpp -- HOST EMULATOR of the k-best-trees workgroup (vlgae_amd/csrc/vlg_kbest.hip).  TEST INFRASTRUCTURE ONLY.
//
// The charts are filled by the SAME bodies the gfx950 kernel runs (vlg_dp_kbest.h: kbest_fill / kbest_span) under the token barrier
// of emu_dp.cpp, `nt` host threads as lanes; behind it the same walk (kbest_walk) extracts every rank under a host policy whose
// "wavefront" is one lane.  The charts and the walk's stacks are carved as the kernel carves them (KbestLayout, at the placement
// mode the caller asks for: the spilled modes run at any N, with a second arena as the workspace), with the canary of emu_dp.cpp
// behind each arena.  The workspace arena is pre-filled with a NaN pattern: nothing may depend on what it held.
//
// Built two ways: as part of a shared library for ctypes calls (tests/test_kbest_host.py), and, with -DEMU_KBEST_MAIN, as a
// stand-alone program for the sanitizers, which replays a case file written by the test.
#include "emu_dp.cpp"

#include "emu_kbest_common.h"

#include <cstdio>

namespace {

// plant: -1, or a 16-bit value written over the back-pointer of rank 0 of the root cell before the walks (the walk's give-up rules)
template <int KC>
void kbest_one(const vlg::KbArc& arc, int len, int b, int B, int N, int K, int mode, int plant, long long* heads, float* scores,
               int32_t* count, int nt, int order) {
    const vlg::KbestLayout L(N, KC, mode);
    KbArenas m(L.lds_bytes, L.ws_bytes);
    vlg::KbCtx c;
    c.Ne = len + 1; c.len = len; c.P = vlg::chart_pitch(N); c.cells = N * c.P;
    c.C = m.at<float>(L.C); c.I = m.at<float>(L.I);
    c.bT = m.at<unsigned short>(L.bT); c.bC = m.at<unsigned short>(L.bC);
    run_workgroup(nt, order, [&](int tid, HostX& x) { vlg::kbest_fill<KC>(c, arc, N, tid, nt, x); });
    if (count) count[b] = vlg::kbest_count(c, K);
    if (plant >= 0) c.bC[len + 1] = (unsigned short)plant;   // CR(0,len)[0]
    kbest_each_rank(b, B, N, K, m.at<int>(L.stack), heads, scores,
                    [&](int k, int* stack, long long* h, float* s, KbSeqX& x) { vlg::kbest_walk<KC>(c, k, N, stack, h, s, x); });
    m.check();
}

int kbest_batch(const void* arc, const int64_t* lengths, int B, int N, int in_dtype, int K, int mode, const int* plant, long long* heads,
                float* scores, int32_t* count, int nt, int order) {
    if (K < 1 || K > vlg::kKbestMaxK || N < 2 || N > 255) return -1;
    const vlg::KbestPlan p = vlg::kbest_plan(N, K, vlg::kLdsBudget);
    if (mode < 0) mode = p.mode;
    for (int b = 0; b < B; ++b) {
        const int len = lengths ? (int)lengths[b] : N - 1;
        if (kbest_no_sentence(len, b, B, N, K, heads, scores, count)) continue;
        const vlg::KbArc a{arc, (size_t)b * N * N, in_dtype};
        kbest_image_switch(p.KC, [&](auto kc) {
            kbest_one<decltype(kc)::value>(a, len, b, B, N, K, mode, plant ? plant[b] : -1, heads, scores, count, nt, order);
        });
    }
    return 0;
}

}  // namespace

// heads [K,B,N], scores [K,B], count [B] (optional); mode: the KbestLayout placement to emulate (any N), or -1 for the plan's own
extern "C" int emu_deptree_kbest(const void* arc, const int64_t* lengths, int B, int N, int in_dtype, int K, int mode, long long* heads,
                                 float* scores, int32_t* count, int nt, int order) {
    return kbest_batch(arc, lengths, B, N, in_dtype, K, mode, nullptr, heads, scores, count, nt, order);
}

// the same with plant [B]: per sentence -1, or the value that replaces the back-pointer of rank 0 of its root cell behind the fill
extern "C" int emu_deptree_kbest_planted(const void* arc, const int64_t* lengths, int B, int N, int in_dtype, int K, int mode,
                                         const int* plant, long long* heads, float* scores, int32_t* count, int nt, int order) {
    return kbest_batch(arc, lengths, B, N, in_dtype, K, mode, plant, heads, scores, count, nt, order);
}

extern "C" void emu_kbest_plan(int N, int K, long long* out) { kbest_plan_export<vlg::KbestLayout>(N, K, out); }

#ifdef EMU_KBEST_MAIN
// emu_kbest CASEFILE: int32 B, N, K, mode; int64 lengths[B]; float arc[B N N]; float expect_scores[K B]; int64 expect_heads[K B N].
// Exit status 0 iff scores and heads come back exactly and no canary tripped.
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[4];
    if (std::fread(hdr, sizeof(int), 4, f) != 4) return 2;
    const int B = hdr[0], N = hdr[1], K = hdr[2], mode = hdr[3];
    std::vector<int64_t> lengths(B);
    std::vector<float> arc((size_t)B * N * N), es((size_t)K * B), scores((size_t)K * B);
    std::vector<long long> eh((size_t)K * B * N), heads((size_t)K * B * N, -1);
    std::vector<int32_t> count(B);
    bool ok = std::fread(lengths.data(), 8, lengths.size(), f) == lengths.size() && std::fread(arc.data(), 4, arc.size(), f) == arc.size() &&
              std::fread(es.data(), 4, es.size(), f) == es.size() && std::fread(eh.data(), 8, eh.size(), f) == eh.size();
    std::fclose(f);
    if (!ok) return 2;
    if (emu_deptree_kbest(arc.data(), lengths.data(), B, N, 0, K, mode, heads.data(), scores.data(), count.data(), 8, 2) != 0) return 2;
    int bad = 0;
    for (size_t i = 0; i < heads.size(); ++i) bad += heads[i] != eh[i];
    for (size_t i = 0; i < scores.size(); ++i) bad += std::memcmp(&scores[i], &es[i], 4) != 0;
    std::printf("emu_kbest: B=%d N=%d K=%d mode=%d mismatches=%d canary_trips=%d\n", B, N, K, mode, bad, emu_canary_trips());
    return bad == 0 && emu_canary_trips() == 0 ? 0 : 1;
}
#endif
