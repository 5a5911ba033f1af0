// emu_short.cpp -- the SHORT-SENTENCE code image of the DMV1o kernel bodies on the host.  TEST INFRASTRUCTURE ONLY.
//
// The phase emulator (emu_dp.cpp) instantiates the general and the long-sentence images of vlg_dp_core.h; the short image
// (kSpansShort: per-segment addresses, the one-width-ahead value reads of the outside pass) is otherwise compiled for the device
// alone.  This stand-alone program runs dmv_run<Log, true, kSpansShort> and dmv_run<Log, true, kSpansGeneral> on the same merged
// potentials, with 512 host threads as the lanes of the workgroup, and demands identical bits in logZ and in both count tensors:
// every length 1 ... 40, as N = 41 and as N = len + 1.  It is built with -fsanitize=address,undefined
// (tests/test_short_image_host.py) and must finish clean.
//
// Like the device's policy (DevX) and unlike emu_dp.cpp's HostX it says kChartsInLds = true: reads of split points past a span's
// width, and of lanes whose span starts later in the segment, are not clamped.  On the device they fall into LDS; here the working
// set is carved -- with the kernel's DmvLayout, mode 0 -- out of one arena followed by slack that is zero before a run and must
// be zero after it (nothing is ever stored through such an address), large enough for the farthest of those reads.
//
// The lanes run free between barriers (no serialisation order: intra-phase races are emu_dp.cpp's subject); a barrier is a
// pthread barrier, and the group all-reduces replay the device's butterfly tree through an exchange buffer, as HostX does.
#include <pthread.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "../../vlgae_amd/csrc/vlg_dp_core.h"

namespace {

constexpr int kLanes = 512;

struct ShortX {
    static constexpr bool kSkipDeadWaves = false;   // an all-reduce is a barrier here: every lane takes part
    static constexpr bool kChartsInLds = true;      // unclamped reads, as on the device (arena + slack)
    pthread_barrier_t* bar;
    int tid;
    float* xf;   // [kLanes][8]

    void sync() { pthread_barrier_wait(bar); }
    void lockstep() { sync(); }
    bool uniform(bool v) { return v; }
    int uniform(int v) { return v; }
    template <typename T>
    T* pin(T* p) { return p; }
    void settle(float&) {}
    template <int n, typename Op>
    void butterfly(float* v, int G, Op op) {
        if (G == 1) return;   // uniform over the workgroup
        for (int k = 0; k < n; ++k) xf[tid * 8 + k] = v[k];
        sync();
        const int base = tid & ~(G - 1);
        for (int k = 0; k < n; ++k) {
            float cur[64], nxt[64];
            for (int t = 0; t < G; ++t) cur[t] = xf[(base + t) * 8 + k];
            for (int s = 1; s < G; s <<= 1) {   // lane t combines with lane t ^ 1, then t ^ 2, ...: the device's tree
                for (int t = 0; t < G; ++t) nxt[t] = op(cur[t], cur[t ^ s]);
                for (int t = 0; t < G; ++t) cur[t] = nxt[t];
            }
            v[k] = cur[tid - base];
        }
        sync();
    }
    template <int n>
    void allreduce_max(float* v, int G) { butterfly<n>(v, G, [](float a, float b) { return fmaxf(a, b); }); }
    template <int n>
    void allreduce_sum(float* v, int G) { butterfly<n>(v, G, [](float a, float b) { return a + b; }); }
    // the Log semiring never calls these (dmv_run compiles its Max branches all the same)
    template <int n>
    void allreduce_argmax(float*, int*, int) { std::abort(); }
    void group_bcast2(float*, int, int, int) { std::abort(); }
    void group_bcast4(float*, int, int, int) { std::abort(); }
};

// How far past the START of a chart an unclamped read can reach, in bytes (8-byte cells; the 4-byte charts reach half as far).  The
// cell indices of vlg_dp_core.h's address table are all below  D + w P + r P + P + w + 2  with D <= (N - 1)(P + 1) the diagonal cell
// of the last row, w <= N - 1 the width and r < 64 the split point of a lane's last term (G TM <= 64 in every segment of the short
// image; the general image's r = rr + u G stays below T G < w + G, which is at most 64 for N <= 41 too).  The last chart of the carve is such a chart, so this also bounds the reach past
// the carve's end, whatever DmvLayout puts behind it.
constexpr size_t far_read_bytes(int N) {
    const size_t P = (size_t)((N + 1) | 1), n = (size_t)N;   // vlg::chart_pitch, which is not constexpr (Run::prepare checks the two agree)
    return 8 * ((n - 1) * (P + 1) + (n - 1) * P + 64 * P + P + n + 2) + 8;
}
constexpr size_t kSlack = 64 * 1024;
static_assert(far_read_bytes(vlg::kShortN) <= kSlack, "the slack behind the arena does not cover the farthest unclamped read");   // 50.6 KB at N = 41

struct Case {
    int len, N;
    std::vector<float> dec, attach;
};

struct Out {
    float logZ;
    std::vector<float> gdec, gatt;
};

// one sentence through one image, on the lanes' threads (called by every lane; lane 0 owns set-up and checks)
struct Run {
    std::vector<unsigned char> arena;
    vlg::DmvCtx c;
    vlg::MergedIO<vlg::F32In> io;
    size_t used = 0;
    void prepare(const Case& k, Out& o) {
        const vlg::DmvLayout L(k.N, true, false, 0, false);
        used = L.lds_bytes;
        if (vlg::chart_pitch(k.N) != ((k.N + 1) | 1) || far_read_bytes(k.N) > kSlack) std::abort();
        arena.assign(used + kSlack, 0);
        std::memset(arena.data(), 0xA5, used);   // the kernel's own cells: whatever the last launch left there
        char* A = reinterpret_cast<char*>(arena.data());
        c.walk = false;
        c.Ne = k.len + 1; c.len = k.len; c.P = vlg::chart_pitch(k.N);
        c.C = (float2*)(A + L.C_in.off); c.I = (float2*)(A + L.I_in.off); c.C2 = (float2*)(A + L.C.off); c.I2 = (float2*)(A + L.I.off);
        c.S = (float*)(A + L.S.off); c.bpS = (unsigned char*)(A + L.bpS.off); c.bpC = (unsigned char*)(A + L.bpC.off);
        c.gCc = (float*)(A + L.gCc.off); c.gCi = (float2*)(A + L.gCi.off); c.gI = (float2*)(A + L.gI.off);
        c.decs = (float*)(A + L.decs.off); c.gdecs = (float*)(A + L.gdecs.off);
        o.logZ = NAN;
        o.gdec.assign((size_t)k.N * 8, NAN);
        o.gatt.assign((size_t)k.N * k.N * 2, NAN);
        io.dec = k.dec.data(); io.attach = k.attach.data(); io.N = k.N;
        io.gdec = o.gdec.data(); io.gatt = o.gatt.data(); io.heads = nullptr;
    }
    bool slack_untouched() const {
        for (size_t i = used; i < arena.size(); ++i)
            if (arena[i] != 0) return false;
        return true;
    }
};

bool same_bits(const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

}  // namespace

int main() {
    std::vector<Case> cases;
    std::mt19937 rng(20240607);
    std::normal_distribution<float> nrm(0.f, 1.f);
    std::uniform_real_distribution<float> uni(0.05f, 1.f);
    for (int pass = 0; pass < 2; ++pass)
        for (int len = 1; len <= 40; ++len) {
            Case k;
            k.len = len;
            k.N = pass == 0 ? 41 : len + 1;
            k.dec.resize((size_t)k.N * 8);
            k.attach.resize((size_t)k.N * k.N * 2);
            for (float& x : k.dec) x = std::log(uni(rng));
            for (float& x : k.attach) x = nrm(rng);
            cases.push_back(std::move(k));
        }

    pthread_barrier_t bar;
    pthread_barrier_init(&bar, nullptr, kLanes);
    std::vector<float> xf((size_t)kLanes * 8);
    Run run;
    Out out_short, out_general;
    int failures = 0;
    std::vector<std::thread> lanes;
    for (int tid = 0; tid < kLanes; ++tid)
        lanes.emplace_back([&, tid] {
            ShortX x;
            x.bar = &bar; x.tid = tid; x.xf = xf.data();
            for (const Case& k : cases) {
                for (int image = 0; image < 2; ++image) {
                    Out& o = image == 0 ? out_short : out_general;
                    if (tid == 0) run.prepare(k, o);
                    x.sync();
                    if (image == 0) vlg::dmv_run<VLG_SR_LOG, true, vlg::kSpansShort>(run.c, run.io, 1.f, &o.logZ, tid, kLanes, x);
                    else vlg::dmv_run<VLG_SR_LOG, true, vlg::kSpansGeneral>(run.c, run.io, 1.f, &o.logZ, tid, kLanes, x);
                    x.sync();
                    if (tid == 0 && !run.slack_untouched()) {
                        std::printf("FAIL len %d N %d image %d: a store landed past the kernel's carve\n", k.len, k.N, image);
                        ++failures;
                    }
                }
                if (tid == 0) {
                    const bool ok = std::memcmp(&out_short.logZ, &out_general.logZ, 4) == 0 && same_bits(out_short.gdec, out_general.gdec) &&
                                    same_bits(out_short.gatt, out_general.gatt) && std::isfinite(out_short.logZ);
                    if (!ok) {
                        std::printf("FAIL len %d N %d: short image logZ %.9g, general image logZ %.9g, grad_dec %s, grad_attach %s\n", k.len, k.N,
                                    out_short.logZ, out_general.logZ, same_bits(out_short.gdec, out_general.gdec) ? "same" : "DIFFER",
                                    same_bits(out_short.gatt, out_general.gatt) ? "same" : "DIFFER");
                        ++failures;
                    }
                }
                x.sync();
            }
        });
    for (auto& t : lanes) t.join();
    pthread_barrier_destroy(&bar);
    std::printf("%zu sentences, short image vs general image: %d failures\n", cases.size(), failures);
    return failures == 0 ? 0 : 1;
}
