// vlg_dmv_expect.h -- the DMV1o inside-outside pass in dual numbers (vlg_dmv1o_expect, include/vlgae_amd.h): expected scores, entropy,
// cross-entropy and KL of DMV1o with their exact gradients (the reference's StructDistribution.entropy / cross_entropy / kl / risk,
// src/model/torch_struct/distributions.py:79-114, which run the Python width loop of dmv.py:18-69 under EntropySemiring /
// CrossEntropySemiring / RiskSemiring plus autograd).  The sibling of vlg_dp_expect.h for the valence DMV: the placement rule, the
// direction load, the adjoint weight and the lane plan of a width are that header's.
//
// Like the phase bodies of vlg_dp_core.h this is the work of ONE thread (tid of nt) between barriers, written against a policy X,
// and shared by the gfx950 kernel (vlg_dmv_expect.hip) and the host emulator of the CPU test-suite (tests/emu/emu_dmv_expect.cpp).
// Nothing here is a CPU fallback.
//
// Every chart cell of DMV1o (notation: dmv_fw_span / dmv_bw_span, vlg_dp_core.h; .x HASCHILD, .y NOCHILD) carries a value and a
// TANGENT: its derivative along a direction d = (v_dec - v_sub_dec, v_attach - v_sub_attach) in potential space.  Values are kept in
// log2 units as in the family; tangents are in natural units and need no rescaling (their recurrences are linear, the weights p_r are
// ratios).
//   load     a component of d is forced to 0 where its own potential is forbidden (at or below the semiring zero DMV1o.merge writes:
//            the test is against 0.5 VLG_NEGINF, which also catches bf16's rounding of -1e12, -inf and NaN) and outside the sentence;
//            elsewhere d must be finite (the caller's contract).  Incomplete slot (h -> c, val): value (attach[h,c,val] +
//            dec[h,dir,val,GO]) log2 e, tangent d_att[h,c,val] + d_dec[h,dir,val,GO].  C(h,h) towards dir: dec[h,dir,val,STOP] and its d.
//   inside   three reductions per (span, direction) as in dmv_fw_span: S, C.HC, C.NC; each X = log sum_r exp t_r has
//            X' = sum_r p_r t_r', p_r = 2^(t_r - X).  I.v = staged.v + S, I'.v = staged'.v + S'.  The same-width term is folded in as
//            expect_fw_span does.  The masked root cell (dmv.py:63) has value VLG_NEGINF and tangent 0.
//            logZ = CR(0,len).NC ln 2, ev = its tangent = <mu, d>.
//   outside  seed (1, 0) at CR(0,len).NC; every adjoint carries its tangent through expect_adj.  mu_attach / hv_attach = gI and its
//            tangent; the STOP entries of mu_dec / hv_dec = the diagonal cells' adjoint and its tangent; the GO entries = the row sums
//            of gI / gI' in a fixed summation tree.  hv = (Hessian of logZ) d.
// Work decomposition, ownership of every read-modify-write target and the one barrier per width are those of dmv_fw_span /
// dmv_bw_span: left and right chains on the two halves of the workgroup, no atomics; the tangent charts sit beside the charts they
// differentiate and are written by the same lane.  Split points go through one general loop (no per-T unrolled bodies, no
// short-sentence image); the lane-group size of a width is a run-time value (group_log2).
#pragma once
#include "vlg_dp_core.h"
#include "vlg_dp_expect.h"

namespace vlg {

struct DmvExpectCtx {
    int Ne, len, P;
    float2 *C, *I;             // values (log2 units); I pre-loaded with attach + dec[...,GO]
    float* S;                  // SL(i,j) at S[j*P+i], SR(i,j) at S[i*P+j] (outside pass only)
    float2 *Cd, *Id;           // their tangents (natural units)
    float* Sd;
    float* gCc;                // adjoints, split as in DmvCtx
    float2 *gCi, *gI;
    float* gCcd;               // their tangents
    float2 *gCid, *gId;
    float *decs, *decsd;       // staged dec [Ne][8] (log2 units) and its tangent
};

// The placement rule of vlg_dp_expect.h over DMV1o's cells: two valences in a C / I / gCi / gI cell (80 bytes of charts per chart cell
// with an outside pass, 32 without), and the staged dec pair [N][8] and its direction behind them.
using DmvExpectLayout = ExpectLayoutOf<8, 32>;

template <typename At>
VLG_HD DmvExpectCtx dmv_expect_carve(const DmvExpectLayout& L, int N, int len, const At& at) {
    DmvExpectCtx c;
    c.Ne = len + 1;
    c.len = len;
    c.P = chart_pitch(N);
    c.C = (float2*)at(L.C);
    c.I = (float2*)at(L.I);
    c.S = (float*)at(L.S);
    c.Cd = (float2*)at(L.Cd);
    c.Id = (float2*)at(L.Id);
    c.Sd = (float*)at(L.Sd);
    c.gCc = (float*)at(L.gCc);
    c.gCi = (float2*)at(L.gCi);
    c.gI = (float2*)at(L.gI);
    c.gCcd = (float*)at(L.gCcd);
    c.gCid = (float2*)at(L.gCid);
    c.gId = (float2*)at(L.gId);
    c.decs = (float*)at(L.decs);
    c.decsd = (float*)at(L.decsd);
    return c;
}

// "forbidden": at or below the semiring zero DMV1o.merge writes.  bf16 rounds -1e12 to a smaller magnitude, so the test is against
// half of it; -inf, everything below the clamp floor and NaN (the comparison is false) are covered too.
VLG_HD bool dmv_expect_allowed(float pot) { return pot > 0.5f * VLG_NEGINF; }

// Inside, one span, one direction: DIR 0 = SL -> IL(j,i) -> CL(j,i), DIR 1 = SR -> IR(i,j) -> CR(i,j) (see dmv_fw_span, TU == 0).
template <bool GRAD, int DIR, typename X>
VLG_HD void dmv_expect_fw_span(const DmvExpectCtx& c, int w, int G, int D, bool live, int rr, X& x) {
    // Every multiply-add of the value pass is written out (fmaf) and the compiler may fuse no other: the forward-only image and the
    // inside-outside image then compute logZ and ev with the same operations in the same order -- the same bits, which tree_kl relies on.
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int P = c.P, DW = D + VLG_MUL24(w, P);
    const float *Cf = reinterpret_cast<const float*>(c.C), *Cdf = reinterpret_cast<const float*>(c.Cd);
    const int eA = 2 * (D + 1) + (DIR == 0 ? 1 : 0);                  // CR(i, i+r):   .NC for SL, .HC for SR
    const int eB = 2 * (DW + 1) + (DIR == 0 ? 0 : 1);                 // CL(j, i+r+1): .HC for SL, .NC for SR
    const int eU = DIR == 0 ? 2 * D + 1 : 2 * (D + P + w + 1) + 1;    // CL(i+r, i).NC | CR(i+1+r, j).NC   (stride 2P)
    const int eV = DIR == 0 ? DW : D + 2;                             // IL(j, i+r) | IR(i, i+1+r)
    const int kO = DIR == 0 ? DW : D + w + 1;                         // own slot
    const int kX = DIR == 0 ? 2 * D + 1 : 2 * (DW + w + 1) + 1;       // CL(i,i).NC | CR(j,j).NC: partner of the same-width term
    const float2 aX = c.I[kO], aXd = c.Id[kO];                        // attach + dec[...,GO] and its tangent, staged at load
    const float cX = Cf[kX], cXd = Cdf[kX];
    float m[3] = {VLG_LOWEST, VLG_LOWEST, VLG_LOWEST};
    for (int r = rr; r < w; r += G) {
        m[0] = fmaxf(m[0], Cf[eA + 2 * r] + Cf[eB + 2 * r]);
        if (DIR == 0 ? r >= 1 : r <= w - 2) {
            const float uu = Cf[eU + 2 * VLG_MUL24(r, P)];
            const float2 vv = c.I[eV + r];
            m[1] = fmaxf(m[1], uu + vv.x);
            m[2] = fmaxf(m[2], uu + vv.y);
        }
    }
    x.template allreduce_max<3>(m, G);
    float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // sums of weights of S, C.HC, C.NC; then their weighted tangent sums
    for (int r = rr; r < w; r += G) {
        const float e0 = VLG_EXP(Cf[eA + 2 * r] + Cf[eB + 2 * r] - m[0]);
        s[0] += e0;
        s[3] = fmaf(e0, Cdf[eA + 2 * r] + Cdf[eB + 2 * r], s[3]);
        if (DIR == 0 ? r >= 1 : r <= w - 2) {
            const int ku = eU + 2 * VLG_MUL24(r, P);
            const float uu = Cf[ku], uud = Cdf[ku];
            const float2 vv = c.I[eV + r], vvd = c.Id[eV + r];
            const float e1 = VLG_EXP(uu + vv.x - m[1]), e2 = VLG_EXP(uu + vv.y - m[2]);
            s[1] += e1;
            s[2] += e2;
            s[4] = fmaf(e1, uud + vvd.x, s[4]);
            s[5] = fmaf(e2, uud + vvd.y, s[5]);
        }
    }
    x.template allreduce_sum<6>(s, G);
    const float Sv = m[0] + VLG_LOG(s[0]), Svd = s[3] / s[0];   // (s[0] >= 1: the term at the maximum has weight 1)
    const float2 In = make_float2(aX.x + Sv, aX.y + Sv), Ind = make_float2(aXd.x + Svd, aXd.y + Svd);
    // the same-width term folded in as fold_term does: one exponential of -|m - t| serves both rescales
    float Cv[2], Cvd[2];
    for (int k = 0; k < 2; ++k) {
        const float t = cX + (k == 0 ? In.x : In.y), td = cXd + (k == 0 ? Ind.x : Ind.y);
        const float d = m[1 + k] - t, e = VLG_EXP(-fabsf(d));
        const float Sw = d >= 0.f ? s[1 + k] + e : fmaf(s[1 + k], e, 1.f);
        Cv[k] = fmaxf(m[1 + k], t) + VLG_LOG(Sw);
        Cvd[k] = (d >= 0.f ? fmaf(e, td, s[4 + k]) : fmaf(s[4 + k], e, td)) / Sw;
    }
    if (DIR == 1 && D == 0 && w != c.len) { Cv[0] = Cv[1] = VLG_NEGINF; Cvd[0] = Cvd[1] = 0.f; }   // masked root cell, dmv.py:63
    if (live && rr == 0) {
        c.I[kO] = In;
        c.Id[kO] = Ind;
        c.C[kO] = make_float2(Cv[0], Cv[1]);
        c.Cd[kO] = make_float2(Cvd[0], Cvd[1]);
        if (GRAD) {   // the outside replay's tape
            const int kS = DIR == 0 ? DW : D + w;
            c.S[kS] = Sv;
            c.Sd[kS] = Svd;
        }
    }
}

// Outside, one span, one direction (see dmv_bw_span, TU == 0): every target below is owned by this (span, direction, r) within the
// width -- the left direction owns gI row j, the CL half of gCc and the (.NC of CR(i,.), .HC of CL(j,.)) words of gCi, the right one
// the mirror set -- and the same holds for the tangent charts.
template <int DIR, typename X>
VLG_HD void dmv_expect_bw_span(const DmvExpectCtx& c, int w, int G, int D, bool live, int rr, X& x) {
    const int P = c.P, DW = D + VLG_MUL24(w, P);
    const float *Cf = reinterpret_cast<const float*>(c.C), *Cdf = reinterpret_cast<const float*>(c.Cd);
    float *gCif = reinterpret_cast<float*>(c.gCi), *gCidf = reinterpret_cast<float*>(c.gCid);
    const int eA = 2 * (D + 1) + (DIR == 0 ? 1 : 0);          // CR(i, i+r):   .NC for SL, .HC for SR   (also its gCi word)
    const int eB = 2 * (DW + 1) + (DIR == 0 ? 0 : 1);         // CL(j, i+r+1): .HC for SL, .NC for SR
    const int eU = DIR == 0 ? D : D + P + w + 1;              // cell of CL(i+r, i) | CR(i+1+r, j)   (stride P): value .NC, adjoint gCc
    const int eV = DIR == 0 ? DW : D + 2;                     // IL(j, i+r) | IR(i, i+1+r)
    const int kO = DIR == 0 ? DW : D + w + 1;                 // own slot
    const int kS = DIR == 0 ? DW : D + w;
    const int selfr = DIR == 0 ? 0 : w - 1;                   // the split point whose incomplete span has this same width
    float2 gc = make_float2(0.f, 0.f), gcd = gc;              // total adjoint of CL(j,i) | CR(i,j) and its tangent
    if (!(DIR == 1 && D == 0 && w != c.len)) {                // masked root cell: dmv.py:63
        const float a = c.gCc[kO], ad = c.gCcd[kO];
        const float2 b = c.gCi[kO], bd = c.gCid[kO];
        gc = make_float2(b.x, a + b.y);
        gcd = make_float2(bd.x, ad + bd.y);
    }
    const float2 oc = c.C[kO], ocd = c.Cd[kO], gi_old = c.gI[kO], gi_oldd = c.gId[kO];
    const float Sv = c.S[kS], Svd = c.Sd[kS];
    const int r0 = live ? rr : w;                             // a lane without a span this round only keeps step with the others
    for (int r = r0; r < w; r += G) {
        const int rP = VLG_MUL24(r, P);
        const float a = Cf[2 * (eU + rP) + 1], ad = Cdf[2 * (eU + rP) + 1];
        const float2 v = c.I[eV + r], vd = c.Id[eV + r];
        float q0, q0d, q1, q1d;
        expect_adj(gc.x, gcd.x, a + v.x, ad + vd.x, oc.x, ocd.x, q0, q0d);
        expect_adj(gc.y, gcd.y, a + v.y, ad + vd.y, oc.y, ocd.y, q1, q1d);
        if (r != selfr) {
            const float2 t = c.gI[eV + r], td = c.gId[eV + r];
            c.gI[eV + r] = make_float2(t.x + q0, t.y + q1);
            c.gId[eV + r] = make_float2(td.x + q0d, td.y + q1d);
        }
        c.gCc[eU + rP] += q0 + q1;
        c.gCcd[eU + rP] += q0d + q1d;
    }
    // share of gI(own slot) that comes from this very span's complete cell: every lane of the group evaluates it (see dmv_bw_span)
    const int ks = eU + VLG_MUL24(selfr, P);
    const float su = Cf[2 * ks + 1], sud = Cdf[2 * ks + 1];   // CL(i,i).NC | CR(j,j).NC
    const float2 sv = c.I[kO], svd = c.Id[kO];                // IL(j,i) | IR(i,j): this span's own incomplete value
    float f0, f0d, f1, f1d;
    expect_adj(gc.x, gcd.x, su + sv.x, sud + svd.x, oc.x, ocd.x, f0, f0d);
    expect_adj(gc.y, gcd.y, su + sv.y, sud + svd.y, oc.y, ocd.y, f1, f1d);
    x.lockstep();   // every read of gI(own slot) above precedes its store below (the lanes of a group sit in one wavefront)
    const float2 gi = make_float2(gi_old.x + f0, gi_old.y + f1), gid = make_float2(gi_oldd.x + f0d, gi_oldd.y + f1d);
    const float gs = gi.x + gi.y, gsd = gid.x + gid.y;        // adjoint of SL(i,j) | SR(i,j)
    for (int r = r0; r < w; r += G) {
        float ws, wsd;
        expect_adj(gs, gsd, Cf[eA + 2 * r] + Cf[eB + 2 * r], Cdf[eA + 2 * r] + Cdf[eB + 2 * r], Sv, Svd, ws, wsd);
        gCif[eA + 2 * r] += ws;
        gCif[eB + 2 * r] += ws;
        gCidf[eA + 2 * r] += wsd;
        gCidf[eB + 2 * r] += wsd;
    }
    if (live && rr == 0) {   // == d logZ / d attach[j,i,:] | attach[i,j,:] and its tangent
        c.gI[kO] = gi;
        c.gId[kO] = gid;
    }
}

struct DmvExpectIO {   // one sentence's tensors; every pointer but dec and attach may be null
    const void *dec, *attach, *v_dec, *v_attach, *v_sub_dec, *v_sub_attach;
    float *logZ, *ev, *mu_dec, *mu_attach, *hv_dec, *hv_attach;
};

// One sentence: the body of one workgroup.
template <bool GRAD, typename In, typename VIn, typename X>
VLG_HD void dmv_expect_run(const DmvExpectCtx& c, const DmvExpectIO& io, int N, int tid, int nt, X& x) {
    using T = typename In::T;
    using VT = typename VIn::T;
    const int Ne = c.Ne, P = c.P, len = c.len;
    const T *dec = (const T*)io.dec, *attach = (const T*)io.attach;
    const VT *vd = (const VT*)io.v_dec, *va = (const VT*)io.v_attach, *sd = (const VT*)io.v_sub_dec, *sa = (const VT*)io.v_sub_attach;
    // ---- stage: charts to the semiring zero with tangent 0, dec and its direction into fast memory ----
    const float2 zz = make_float2(VLG_NEGINF, VLG_NEGINF), oo = make_float2(0.f, 0.f);
    for (int i = tid; i < Ne * P; i += nt) {
        c.C[i] = zz;
        c.I[i] = zz;
        c.Cd[i] = oo;
        c.Id[i] = oo;
        if (GRAD) {
            c.gCc[i] = 0.f; c.gCi[i] = oo; c.gI[i] = oo;
            c.gCcd[i] = 0.f; c.gCid[i] = oo; c.gId[i] = oo;
        }
    }
    for (int i = tid; i < Ne * 8; i += nt) {
        const float p = In::ld(dec, i);
        float d = expect_dir<VIn>(vd, sd, i);
        if (!dmv_expect_allowed(p)) d = 0.f;   // a forbidden decision carries no tangent, whatever v holds there
        c.decs[i] = pot_clamp(p) * VLG_LOG2E;
        c.decsd[i] = d;
    }
    x.sync();
    for (int idx = tid; idx < Ne * Ne; idx += nt) {
        const int h = idx / Ne, ch = idx - h * Ne;
        const float *d = c.decs + h * 8, *dd = c.decsd + h * 8;
        if (ch == h) {
            c.C[h * P + h] = make_float2(d[1], d[3]);        // CL(h,h).v = dec[h,LEFT ,v,STOP]
            c.Cd[h * P + h] = make_float2(dd[1], dd[3]);
            c.C[h * P + h + 1] = make_float2(d[5], d[7]);    // CR(h,h).v = dec[h,RIGHT,v,STOP]
            c.Cd[h * P + h + 1] = make_float2(dd[5], dd[7]);
        } else {
            const size_t at = ((size_t)h * N + ch) * 2;
            const float2 a = In::ld2(attach, at);
            float2 t = make_float2(expect_dir<VIn>(va, sa, at), expect_dir<VIn>(va, sa, at + 1));
            if (!dmv_expect_allowed(a.x)) t.x = 0.f;
            if (!dmv_expect_allowed(a.y)) t.y = 0.f;
            const int k = ch < h ? h * P + ch : h * P + ch + 1, go = ch < h ? 0 : 4;   // dec[h,dir,val,GO] at go + 2 val
            c.I[k] = make_float2(fmaf(pot_clamp(a.x), VLG_LOG2E, d[go]), fmaf(pot_clamp(a.y), VLG_LOG2E, d[go + 2]));
            c.Id[k] = make_float2(t.x + dd[go], t.y + dd[go + 2]);
        }
    }
    x.sync();
    // ---- inside ----
    const int nd = nt >> 1;
    const bool right = x.uniform(tid >= nd);
    const int t = right ? tid - nd : tid;
    for (int w = 1; w < Ne; ++w) {
        const int spans = Ne - w;
        const ExpectLanes l(spans, w, nd, t, VLG_DP_LANES_FW);
        for (int base = 0; base < spans; base += l.per) {
            const bool live = base + l.slot < spans;
            if (X::kSkipDeadWaves && (base + ((t & ~63) >> l.lg)) >= spans) continue;
            const int D = VLG_MUL24(live ? base + l.slot : 0, P + 1);
            if (right) dmv_expect_fw_span<GRAD, 1>(c, w, l.G, D, live, l.rr, x);
            else dmv_expect_fw_span<GRAD, 0>(c, w, l.G, D, live, l.rr, x);
        }
        x.sync();
    }
    if (tid == 0) {
        *io.logZ = c.C[len + 1].y * VLG_LN2;   // CR(0,len).NOCHILD, dmv.py:65
        if (io.ev) *io.ev = c.Cd[len + 1].y;
    }
    if (!GRAD) return;
    // ---- outside ----
    if (tid == 0) c.gCc[len + 1] = 1.f;   // seed (1, 0)
    x.sync();
    for (int w = Ne - 1; w >= 1; --w) {
        const int spans = Ne - w;
        const ExpectLanes l(spans, w, nd, t, VLG_DP_LANES_BW);
        for (int base = 0; base < spans; base += l.per) {
            const bool live = base + l.slot < spans;
            if (X::kSkipDeadWaves && (base + ((t & ~63) >> l.lg)) >= spans) continue;
            const int D = VLG_MUL24(live ? base + l.slot : 0, P + 1);
            if (right) dmv_expect_bw_span<1>(c, w, l.G, D, live, l.rr, x);
            else dmv_expect_bw_span<0>(c, w, l.G, D, live, l.rr, x);
        }
        x.sync();
    }
    // ---- expected counts and their tangents out: one writer per element, exact zeros on the diagonal and outside the sentence ----
    if (io.mu_attach || io.hv_attach)
        for (int idx = tid; idx < N * N; idx += nt) {
            const int h = idx / N, ch = idx - h * N;
            float2 g = oo, gd = oo;
            if (h < Ne && ch < Ne && ch != h) {
                const int k = ch < h ? h * P + ch : h * P + ch + 1;
                g = c.gI[k];
                gd = c.gId[k];
            }
            if (io.mu_attach) *reinterpret_cast<float2*>(io.mu_attach + (size_t)idx * 2) = g;
            if (io.hv_attach) *reinterpret_cast<float2*>(io.hv_attach + (size_t)idx * 2) = gd;
        }
    if (!io.mu_dec && !io.hv_dec) return;
    // STOP: the adjoint of the width-0 span (one cell each) and its tangent
    for (int idx = tid; idx < N * 4; idx += nt) {
        const int h = idx >> 2, dir = (idx >> 1) & 1, v = idx & 1;
        float g = 0.f, gd = 0.f;
        if (h < Ne) {
            const int q = h * P + h + dir;
            g = (v == 1 ? c.gCc[q] : 0.f) + reinterpret_cast<const float*>(c.gCi + q)[v];
            gd = (v == 1 ? c.gCcd[q] : 0.f) + reinterpret_cast<const float*>(c.gCid + q)[v];
        }
        const int o = h * 8 + (dir * 2 + v) * 2 + 1;
        if (io.mu_dec) io.mu_dec[o] = g;
        if (io.hv_dec) io.hv_dec[o] = gd;
    }
    // GO: dec[h,dir,v,GO] enters every incomplete span headed by h towards dir, so its count is a row sum of the finished gI chart:
    // four lanes per (h, dir) take every fourth cell and meet in a two-step butterfly -- a fixed summation tree (see dmv_run)
    constexpr int GL = 4;
    for (int base = 0; base < N * 2; base += nt / GL) {
        const int grp = base + tid / GL, rr = tid % GL;
        const int h = grp >> 1, dir = grp & 1;
        float sum[4] = {0.f, 0.f, 0.f, 0.f};
        if (grp < N * 2 && h < Ne) {
            const int r0 = h * P + (dir == 0 ? 0 : h + 2);      // cells (h, ch) for ch < h  |  (h, ch + 1) for ch > h
            const int n = dir == 0 ? h : Ne - 1 - h;
            for (int k = rr; k < n; k += GL) {
                const float2 g = c.gI[r0 + k], gd = c.gId[r0 + k];
                sum[0] += g.x; sum[1] += g.y; sum[2] += gd.x; sum[3] += gd.y;
            }
        }
        x.template allreduce_sum<4>(sum, GL);
        if (grp < N * 2 && rr == 0) {
            const int o = h * 8 + dir * 4;
            if (io.mu_dec) { io.mu_dec[o] = sum[0]; io.mu_dec[o + 2] = sum[1]; }
            if (io.hv_dec) { io.hv_dec[o] = sum[2]; io.hv_dec[o + 2] = sum[3]; }
        }
    }
}

}  // namespace vlg
