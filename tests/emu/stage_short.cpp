// stage_short.cpp -- the short image's load stage since round 13 (vlg_dp_core.h: dmv_stage_request / dmv_stage_write).
// TEST INFRASTRUCTURE ONLY.
//
// A stand-alone program (its own main) against vlgae_amd/csrc/vlg_dp_core.h, beside hold_short.cpp.  The stage has no barrier inside
// it -- a lane asks for what its own cells need and stores those cells, once -- so the 512 lanes are run one after the other, in
// forward, reverse and a shuffled order.  For every tensor width N = 2 ... 41 (every chart pitch), every sentence Ne <= N, and the
// three forms the stage is compiled for (MergedIO on fp32 and on bf16 storage: cells of all N rows, whatever the length; RuleIO:
// cells of the sentence's rows, through token[]):
//   * C and I hold, in all Ne P cells, bit for bit what the general image's stage leaves there -- its formulas, written out below with
//     the policy's own accessors: the semiring zero, d = fl(clamp(dec) LOG2E) in the STOP cells, fmaf(clamp(attach), LOG2E, d) in the
//     arc cells;
//   * every one of those cells is stored by exactly one lane, exactly the lane that owns it (q = tid + k nt), and no cell past Ne P
//     is stored at all (the charts are allocated at exactly N P cells: a store past them is a sanitizer error);
//   * dec and attach (rule, root, token) are allocated at exactly their element counts, so a request past a slice is a sanitizer
//     error too; the positions >= Ne, attach's diagonal, and token[] past the sentence hold NaN / +-inf / 3e38 / ids outside the
//     table, which must not reach a cell.
// The count write-out of the same round (dmv_counts_out_short) follows, for the same (N, Ne) and both I/O policies: on adjoint charts
// of exactly N P cells -- dense counts for the Log semiring, the counts of one tree for the Max semiring, with and without the head
// vector; NaN wherever the write-out has nothing to read -- every output (attach, STOP and GO counts, heads; rule-space counts
// through the atomics) must equal, bit for bit, what the other images' write-out leaves: dmv_counts_out, the very statements dmv_run
// executes for them (vlg_dp_counts_body.h).
// It is built with -fsanitize=address,undefined by tests/test_dmv_short_stage_host.py.
#include <pthread.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <thread>
#include <vector>

#include "../../vlgae_amd/csrc/vlg_dp_core.h"

namespace {

constexpr int kLanes = 512;
constexpr uint32_t kSentinel = 0x7fa5a5a5u;   // a NaN pattern no potential produces
int failures = 0;
long long cells_checked = 0, stores_seen = 0, runs = 0;

void fail(const char* form, int N, int Ne, const char* what) {
    if (++failures <= 20) std::printf("FAIL %s N %d Ne %d: %s\n", form, N, Ne, what);
}

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
bool is_sentinel(const float2& v) { return bits(v.x) == kSentinel && bits(v.y) == kSentinel; }
bool same(const float2& a, const float2& b) { return bits(a.x) == bits(b.x) && bits(a.y) == bits(b.y); }

const float kPoison[] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                         -std::numeric_limits<float>::infinity(), 3e38f, -std::numeric_limits<float>::quiet_NaN()};

template <typename T>
T store(float f);
template <>
float store<float>(float f) { return f; }
template <>
uint16_t store<uint16_t>(float f) { return (uint16_t)(bits(f) >> 16); }   // bf16 by truncation: NaN and inf keep their class

// the general image's stage (vlg_dp_core.h: dmv_run, the branch of the other images), cell by cell
template <typename IO>
void reference(const IO& io, int Ne, int P, std::vector<float2>& C, std::vector<float2>& I) {
    const float2 zz = make_float2(VLG_NEGINF, VLG_NEGINF);
    for (int q = 0; q < Ne * P; ++q) C[q] = I[q] = zz;
    for (int h = 0; h < Ne; ++h) {
        float d[8];
        for (int k = 0; k < 8; ++k) d[k] = io.ld_dec(h * 8 + k) * VLG_LOG2E;
        C[h * P + h] = make_float2(d[1], d[3]);
        C[h * P + h + 1] = make_float2(d[5], d[7]);
        for (int ch = 0; ch < Ne; ++ch) {
            if (ch == h) continue;
            const float2 a = io.ld_attach(h, ch);
            if (ch < h) I[h * P + ch] = make_float2(fmaf(a.x, VLG_LOG2E, d[0]), fmaf(a.y, VLG_LOG2E, d[2]));
            else I[h * P + ch + 1] = make_float2(fmaf(a.x, VLG_LOG2E, d[4]), fmaf(a.y, VLG_LOG2E, d[6]));
        }
    }
}

template <typename IO>
void run_stage(const char* form, const IO& io, int N, int Ne, const std::vector<int>& order) {
    const int P = vlg::chart_pitch(N), cells = N * P;
    std::vector<float2> C(cells), I(cells), gotC(cells), gotI(cells), refC(cells), refI(cells);
    const float2 sent = make_float2(from_bits(kSentinel), from_bits(kSentinel));
    std::fill(C.begin(), C.end(), sent);
    std::fill(I.begin(), I.end(), sent);
    std::vector<int> nC(cells, 0), nI(cells, 0);
    vlg::DmvCtx c;
    std::memset(&c, 0, sizeof c);
    c.Ne = Ne; c.len = Ne - 1; c.P = P; c.C = C.data(); c.I = I.data();
    for (int tid : order) {
        for (int k = 0; k < vlg::kStageCells; ++k) {   // a foreign store into a cell this lane owns would sit here now
            const int q = tid + k * kLanes;
            if (q < cells && (!is_sentinel(C[q]) || !is_sentinel(I[q]))) fail(form, N, Ne, "a cell was stored by a lane that does not own it");
        }
        const vlg::ShortStage pre = vlg::dmv_stage_request(io, P, io.stage_rows(Ne), tid, kLanes);
        vlg::dmv_stage_write(c, pre, tid, kLanes);
        for (int k = 0; k < vlg::kStageCells; ++k) {
            const int q = tid + k * kLanes;
            if (q >= cells) continue;
            if (!is_sentinel(C[q])) { ++nC[q]; gotC[q] = C[q]; C[q] = sent; ++stores_seen; }
            if (!is_sentinel(I[q])) { ++nI[q]; gotI[q] = I[q]; I[q] = sent; ++stores_seen; }
        }
    }
    reference(io, Ne, P, refC, refI);
    for (int q = 0; q < cells; ++q) {
        if (!is_sentinel(C[q]) || !is_sentinel(I[q])) fail(form, N, Ne, "a lane stored a cell it does not own");
        const int want = q < Ne * P ? 1 : 0;
        if (nC[q] != want || nI[q] != want) fail(form, N, Ne, want ? "a chart cell of the sentence does not have exactly one writer" : "a cell past Ne P was stored");
        if (want && (!same(gotC[q], refC[q]) || !same(gotI[q], refI[q]))) fail(form, N, Ne, "a chart cell differs from the general image's stage");
        cells_checked += want;
    }
    ++runs;
}

template <typename In>
void merged_case(const char* form, int N, int Ne, std::mt19937& rng, const std::vector<std::vector<int>>& orders) {
    using T = typename In::T;
    std::normal_distribution<float> nrm(0.f, 1.f);
    std::uniform_real_distribution<float> uni(0.05f, 1.f);
    std::vector<T> dec((size_t)N * 8), attach((size_t)N * N * 2);   // exactly the sentence's slices
    for (int h = 0; h < N; ++h)
        for (int k = 0; k < 8; ++k) dec[h * 8 + k] = store<T>(h < Ne ? std::log(uni(rng)) : kPoison[rng() % 5]);
    for (int h = 0; h < N; ++h)
        for (int ch = 0; ch < N; ++ch)
            for (int v = 0; v < 2; ++v) {
                const bool real = h < Ne && ch < Ne && ch != h;
                float a = real ? nrm(rng) : kPoison[rng() % 5];
                if (real && rng() % 11 == 0) a = -std::numeric_limits<float>::infinity();   // a forbidden arc: clamped to the floor
                attach[((size_t)h * N + ch) * 2 + v] = store<T>(a);
            }
    vlg::MergedIO<In> io;
    std::memset(&io, 0, sizeof io);
    io.dec = dec.data(); io.attach = attach.data(); io.N = N;
    for (const auto& o : orders) run_stage(form, io, N, Ne, o);
}

void rules_case(int N, int Ne, std::mt19937& rng, const std::vector<std::vector<int>>& orders) {
    const int L = N - 1, T = L + 1, len = Ne - 1;
    std::normal_distribution<float> nrm(0.f, 1.f);
    std::uniform_real_distribution<float> uni(0.05f, 1.f);
    std::vector<float> rule((size_t)L * T * 4), dec((size_t)L * 8), root((size_t)T);
    std::vector<long long> token((size_t)L);
    std::vector<unsigned char> mask((size_t)L);
    for (int h = 0; h < L; ++h) {
        for (int k = 0; k < 8; ++k) dec[h * 8 + k] = h < len ? std::log(uni(rng)) : kPoison[rng() % 5];
        for (int k = 0; k < T * 4; ++k) rule[(size_t)h * T * 4 + k] = h < len ? nrm(rng) : kPoison[rng() % 5];
        token[h] = h < len ? (long long)(rng() % T) : (h & 1 ? -7 : (long long)T + 1000);   // past the sentence: ids outside the table
        mask[h] = rng() % 7 == 0;
    }
    for (float& r : root) r = std::log(uni(rng));
    vlg::RuleIO<vlg::F32In> io;
    std::memset(&io, 0, sizeof io);
    io.rule = rule.data(); io.dec = dec.data(); io.root = root.data(); io.token = token.data(); io.head_mask = mask.data();
    io.L = L; io.T = T; io.fill = -1e20f;
    for (const auto& o : orders) run_stage("rules f32", io, N, Ne, o);
}

// ---- the count write-out: dmv_counts_out_short against the other images' write-out (dmv_counts_out: the very statements dmv_run
// executes, vlg_dp_counts_body.h) on the same finished adjoint charts ----------------------------------------------------------------
// The write-out has a barrier (decode mode) and a lane-group all-reduce, so here the 512 lanes are host threads that run free between
// barriers, as in emu_short.cpp; a lane order has no meaning for it.
struct OutX {
    static constexpr bool kSkipDeadWaves = false;
    static constexpr bool kChartsInLds = false;
    pthread_barrier_t* bar;
    int tid;
    float* xf;   // [kLanes][8]
    void sync() { pthread_barrier_wait(bar); }
    void lockstep() { sync(); }
    template <int n>
    void allreduce_sum(float* v, int G) {   // the device's butterfly: lane t with t ^ 1, then t ^ 2, ...
        for (int k = 0; k < n; ++k) xf[tid * 8 + k] = v[k];
        sync();
        const int base = tid & ~(G - 1);
        for (int k = 0; k < n; ++k) {
            float cur[64], nxt[64];
            for (int t = 0; t < G; ++t) cur[t] = xf[(base + t) * 8 + k];
            for (int st = 1; st < G; st <<= 1) {
                for (int t = 0; t < G; ++t) nxt[t] = cur[t] + cur[t ^ st];
                for (int t = 0; t < G; ++t) cur[t] = nxt[t];
            }
            v[k] = cur[tid - base];
        }
        sync();
    }
};

struct OutCase {
    int N = 0, Ne = 0, P = 0, cfg = 0;   // cfg 0: Log, dense counts; 1: Max, the counts of one tree; 2: Max with the head vector
    std::vector<float2> gI, gCi;         // exactly N P cells each: a read past a chart is a sanitizer error
    std::vector<float> gCc, gdecs;
    vlg::DmvCtx c;
    std::vector<float> gdec[2], gatt[2], g_rule[2], g_dec[2], g_root[2];   // [0] the short image's outputs, [1] the other images'
    std::vector<long long> heads[2], rheads[2], token;
    std::vector<unsigned char> mask;
    vlg::MergedIO<vlg::F32In> mio[2];
    vlg::RuleIO<vlg::F32In> rio[2];

    void prepare(int N_, int Ne_, int cfg_, std::mt19937& rng) {
        N = N_; Ne = Ne_; cfg = cfg_; P = vlg::chart_pitch(N);
        const int cells = N * P, L = N - 1, T = L + 1;
        const float nan = std::numeric_limits<float>::quiet_NaN();
        std::uniform_real_distribution<float> uni(0.f, 1.f);
        gI.assign(cells, make_float2(nan, nan));   // whatever the write-out must not read stays NaN
        gCi.assign(cells, make_float2(nan, nan));
        gCc.assign(cells, nan);
        gdecs.assign((size_t)N * 4, nan);
        for (int h = 0; h < Ne; ++h) {
            for (int ch = 0; ch < Ne; ++ch) {
                if (ch == h) continue;
                float2& g = gI[h * P + ch + (ch > h ? 1 : 0)];
                g = cfg == 0 ? make_float2(rng() % 5 ? uni(rng) : 0.f, rng() % 7 ? uni(rng) : 0.f) : make_float2(0.f, 0.f);
            }
            for (int dir = 0; dir < 2; ++dir) {
                gCc[h * P + h + dir] = uni(rng);
                gCi[h * P + h + dir] = make_float2(uni(rng), rng() % 3 ? uni(rng) : 0.f);
                for (int v = 0; v < 2; ++v) gdecs[h * 4 + dir * 2 + v] = (float)(rng() % 2);
            }
        }
        if (cfg != 0)   // one head per word, as the back-pointer walk leaves it
            for (int ch = 1; ch < Ne; ++ch) {
                int h = (int)(rng() % (Ne - 1));
                if (h >= ch) ++h;
                float2& g = gI[h * P + ch + (ch > h ? 1 : 0)];
                (rng() % 2 ? g.x : g.y) = 1.f;
            }
        std::memset(&c, 0, sizeof c);
        c.Ne = Ne; c.len = Ne - 1; c.P = P;
        c.gI = gI.data(); c.gCi = gCi.data(); c.gCc = gCc.data(); c.gdecs = gdecs.data();
        token.resize(L);
        std::vector<long long> perm(T);
        for (int k = 0; k < T; ++k) perm[k] = k;
        std::shuffle(perm.begin(), perm.end(), rng);   // a token of its own per word: one atomic add per rule word
        for (int k = 0; k < L; ++k) token[k] = k < Ne - 1 ? perm[k] : -7;
        mask.resize(L);
        for (int k = 0; k < L; ++k) mask[k] = rng() % 7 == 0;
        for (int im = 0; im < 2; ++im) {
            gdec[im].assign((size_t)N * 8, nan);
            gatt[im].assign((size_t)N * N * 2, nan);
            heads[im].assign(N, -1);
            g_rule[im].assign((size_t)L * T * 4, 0.f);   // zero-filled by the caller
            g_root[im].assign(T, 0.f);
            g_dec[im].assign((size_t)L * 8, nan);
            rheads[im].assign(L + 1, -1);
            std::memset(&mio[im], 0, sizeof mio[im]);
            mio[im].N = N; mio[im].gdec = gdec[im].data(); mio[im].gatt = gatt[im].data();
            mio[im].heads = cfg == 2 ? heads[im].data() : nullptr;
            std::memset(&rio[im], 0, sizeof rio[im]);
            rio[im].token = token.data(); rio[im].head_mask = mask.data(); rio[im].L = L; rio[im].T = T; rio[im].fill = -1e20f;
            rio[im].g_rule = g_rule[im].data(); rio[im].g_dec = g_dec[im].data(); rio[im].g_root = g_root[im].data();
            rio[im].heads = cfg == 2 ? rheads[im].data() : nullptr;
        }
    }
    template <typename V>
    static bool eq(const V& a, const V& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0; }
    void check() {
        if (!eq(gdec[0], gdec[1]) || !eq(gatt[0], gatt[1]) || !eq(heads[0], heads[1])) fail("write-out merged", N, Ne, "an output differs from the other images' write-out");
        if (!eq(g_rule[0], g_rule[1]) || !eq(g_dec[0], g_dec[1]) || !eq(g_root[0], g_root[1]) || !eq(rheads[0], rheads[1]))
            fail("write-out rules", N, Ne, "an output differs from the other images' write-out");
        for (float v : gatt[0]) if (v != v) { fail("write-out merged", N, Ne, "a count was not written, or a cell outside the sentence was read"); break; }
        for (float v : gdec[0]) if (v != v) { fail("write-out merged", N, Ne, "a dec count was not written, or a cell outside the sentence was read"); break; }
        for (float v : g_rule[0]) if (v != v) { fail("write-out rules", N, Ne, "a cell outside the sentence was read"); break; }
        ++runs;
    }
};

template <int SR>
void out_lane(OutCase& k, int tid, OutX& x) {
    vlg::dmv_counts_out_short<SR>(k.c, k.mio[0], tid, kLanes, x, nullptr);
    vlg::dmv_counts_out<SR>(k.c, k.mio[1], tid, kLanes, x);
    vlg::dmv_counts_out_short<SR>(k.c, k.rio[0], tid, kLanes, x, nullptr);
    vlg::dmv_counts_out<SR>(k.c, k.rio[1], tid, kLanes, x);
}

void write_out_sweep(std::mt19937& rng) {
    pthread_barrier_t bar;
    pthread_barrier_init(&bar, nullptr, kLanes);
    std::vector<float> xf((size_t)kLanes * 8);
    OutCase k;
    std::vector<std::thread> lanes;
    for (int tid = 0; tid < kLanes; ++tid)
        lanes.emplace_back([&, tid] {
            OutX x;
            x.bar = &bar; x.tid = tid; x.xf = xf.data();
            for (int N = 2; N <= vlg::kShortN; ++N)
                for (int Ne = 2; Ne <= N; ++Ne)
                    for (int cfg = 0; cfg < 3; ++cfg) {
                        if (tid == 0) k.prepare(N, Ne, cfg, rng);
                        x.sync();
                        if (cfg == 0) out_lane<VLG_SR_LOG>(k, tid, x);
                        else out_lane<VLG_SR_MAX>(k, tid, x);
                        x.sync();
                        if (tid == 0) k.check();
                    }
        });
    for (auto& t : lanes) t.join();
    pthread_barrier_destroy(&bar);
}

}  // namespace

int main() {
    std::mt19937 rng(20241301);
    std::vector<std::vector<int>> orders(3, std::vector<int>(kLanes));
    for (int t = 0; t < kLanes; ++t) { orders[0][t] = t; orders[1][t] = kLanes - 1 - t; orders[2][t] = t; }
    std::shuffle(orders[2].begin(), orders[2].end(), rng);
    int pairs = 0;
    for (int N = 2; N <= vlg::kShortN; ++N)
        for (int Ne = 2; Ne <= N; ++Ne, ++pairs) {
            merged_case<vlg::F32In>("merged f32", N, Ne, rng, orders);
            merged_case<vlg::BF16In>("merged bf16", N, Ne, rng, orders);
            rules_case(N, Ne, rng, orders);
        }
    const long long stage_runs = runs;
    runs = 0;
    write_out_sweep(rng);
    std::printf("%d (N, Ne) pairs, %lld stage runs, %lld write-out comparisons, %lld chart cells, %lld stores: %d failures\n", pairs, stage_runs, runs,
                cells_checked, stores_seen, failures);
    return failures == 0 ? 0 : 1;
}
