// vlg_dp_expect.h -- the DepTree inside-outside pass in dual numbers (vlg_deptree_expect, include/vlgae_amd.h): expected scores,
// entropy, cross-entropy and KL of DependencyCRF with their exact gradients (the reference's StructDistribution.entropy /
// cross_entropy / kl / risk, src/model/torch_struct/distributions.py:79-114, which run the Python width loop under EntropySemiring /
// CrossEntropySemiring / KLDivergenceSemiring plus autograd).
//
// Like the phase bodies of vlg_dp_core.h this is the work of ONE thread (tid of nt) between barriers, written against a policy X,
// and shared by the gfx950 kernel (vlg_expect.hip) and the host emulator of the CPU test-suite (tests/emu/emu_expect.cpp).  Nothing
// here is a CPU fallback.  What the DMV1o pass (vlg_dmv_expect.h) shares with this one also stands here: the placement rule of the
// charts (ExpectLayoutOf), the size of a batch's workspace, the direction load (expect_dir), the adjoint weight (expect_adj) and the
// lane plan of a width (ExpectLanes); the launch frame of both kernels is vlg_expect_kernels.h.  What stayed apart, and why:
// profiles/expect_frame_neutrality.md.
//
// Every chart cell of DepTree (notation: the comment above DepCtx) carries a value and a TANGENT: its derivative along a direction
// v in potential space.  Values are kept in log2 units as in the family; tangents are in natural units and need no rescaling (their
// recurrences are linear and the weights p_r are ratios).
//   load     phi = pot_clamp(arc); tangent of an arc = v[h,c] - v_sub[h,c] (each optional, NULL = 0), forced to 0 where the arc is at
//            the clamp floor (a forbidden arc) and outside the sentence.  Elsewhere v must be finite (the caller's contract).
//   inside   X = log sum_r exp t_r  has  X' = sum_r p_r t_r',  p_r = exp(t_r - X);  I = T + phi  has  I' = T' + tangent(arc);
//            the masked root cell has value zero and tangent 0.  logZ = CR(0,len), ev = CR'(0,len) = <mu, v>.
//   outside  seed (1, 0) at CR(0,len); a cell with adjoint (g, g') hands the operands of term r  (g p_r,  g' p_r + g p_r (t_r' - X')):
//            adj_w and its derivative along v.  The same-width self terms as in dep_self.  mu[h,c] = the adjoint of the arc,
//            hv[h,c] = its tangent = (Hessian of logZ) v.
// Work decomposition, ownership of every read-modify-write target and the one barrier per width are those of dep_fw_span /
// dep_bw_span: the tangent charts sit beside the charts they differentiate and are written by the same lane.  Split points go
// through one general loop (no per-T unrolled bodies); the lane-group size of a width is a run-time value.
#pragma once
#include "vlg_dp_core.h"

namespace vlg {

struct ExpectCtx {
    int Ne, len, P;
    float *C, *I, *S;          // values (log2 units); I pre-loaded with the arc scores; S = T(i,j) at [i][j] (outside pass only)
    float *Cd, *Id, *Sd;       // their tangents (natural units)
    float *gCc, *gCi, *gI;     // adjoints, split as in DepCtx
    float *gCcd, *gCid, *gId;  // their tangents
};

// Where the charts of a dual-number pass live: every chart of the model's Log-semiring set next to its tangent chart.  One placement
// rule for both models (DmvExpectLayout, vlg_dmv_expect.h); W = bytes of a C / I / gCi / gI cell (S and gCc cells have 4), STAGE =
// bytes per word of the staged potentials and their direction behind the charts (always in LDS; 0 = none).
//   grad (mu and / or hv wanted), twelve charts:  0: everything   1: the three adjoint pairs (values, tape and their tangents in the
//     workspace)   2: gCc, gCi and their tangents   3: staging only -- the adjoint pairs stay in LDS longest, as in DepLayout.
//   forward only, four charts (no tape, no adjoints):  0: everything   1: C, I (their tangents in the workspace)   2, 3: staging only.
// (dp_plan's short-sentence image is the same kernel here: the launchers take placement_of(image).)
template <int W, int STAGE>
struct ExpectLayoutOf {
    Region C, I, S, Cd, Id, Sd, gCc, gCi, gI, gCcd, gCid, gId, decs, decsd;
    size_t lds_bytes, ws_bytes;
    VLG_HOSTDEV_M ExpectLayoutOf(int N, bool grad, bool, int mode, bool = false) {
        const size_t cells = (size_t)N * chart_pitch(N), val = cells * W, c4 = grad ? cells * 4 : 0, cw = grad ? val : 0;
        const bool v = mode < 1, ci = grad ? v : mode < 2, a1 = mode < 3, a2 = mode < 2;   // ci: where C and I go
        Carver k;
        C = k.take(val, ci);
        I = k.take(val, ci);
        S = k.take(c4, v);
        Cd = k.take(val, v);
        Id = k.take(val, v);
        Sd = k.take(c4, v);
        gCc = k.take(c4, a1);
        gCcd = k.take(c4, a1);
        gCi = k.take(cw, a1);
        gCid = k.take(cw, a1);
        gI = k.take(cw, a2);
        gId = k.take(cw, a2);
        decs = k.take((size_t)N * STAGE, true);
        decsd = k.take((size_t)N * STAGE, true);
        lds_bytes = k.lds;
        ws_bytes = k.ws;
    }
};
using ExpectLayout = ExpectLayoutOf<4, 0>;

// the workspace of a batch under Layout: what the launchers check and both size queries return
template <typename Layout>
VLG_HOSTDEV size_t expect_workspace_bytes(int B, int N, bool grad) { return dp_plan<Layout>(N, grad, false).ws_stride * (size_t)B; }

// One sentence's context over its layout; at(Region) gives the address of a region (the kernel: LDS or the sentence's slice of the
// workspace; the emulator: its two arenas).
template <typename At>
VLG_HD ExpectCtx expect_carve(const ExpectLayout& L, int N, int len, const At& at) {
    ExpectCtx c;
    c.Ne = len + 1;
    c.len = len;
    c.P = chart_pitch(N);
    c.C = (float*)at(L.C);
    c.I = (float*)at(L.I);
    c.S = (float*)at(L.S);
    c.Cd = (float*)at(L.Cd);
    c.Id = (float*)at(L.Id);
    c.Sd = (float*)at(L.Sd);
    c.gCc = (float*)at(L.gCc);
    c.gCi = (float*)at(L.gCi);
    c.gI = (float*)at(L.gI);
    c.gCcd = (float*)at(L.gCcd);
    c.gCid = (float*)at(L.gCid);
    c.gId = (float*)at(L.gId);
    return c;
}

// Inside, one span, one direction: DIR 0 = T -> IL(j,i) -> CL(j,i), DIR 1 = T -> IR(i,j) -> CR(i,j) (see dep_fw_span).
template <bool GRAD, int DIR, typename X>
VLG_HD void expect_fw_span(const ExpectCtx& c, int w, int G, int D, bool live, int rr, X& x) {
    // Every multiply-add of the value pass is written out (fmaf) and the compiler may fuse no other: the forward-only image and the
    // inside-outside image then compute logZ and ev with the same operations in the same order -- the same bits, which tree_kl relies on.
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int P = c.P, DW = D + VLG_MUL24(w, P);
    const int eA = D + 1, eB = DW + 1;                        // CR(i, i+r), CL(j, i+r+1)
    const int eU = DIR == 0 ? D : D + P + w + 1;              // CL(i+r, i) | CR(i+1+r, j)   (stride P)
    const int eV = DIR == 0 ? DW : D + 2;                     // IL(j, i+r) | IR(i, i+1+r)
    const int kO = DIR == 0 ? DW : D + w + 1;                 // own slot
    const int kX = DIR == 0 ? D : DW + w + 1;                 // CL(i,i) | CR(j,j): partner of the same-width term
    const float aX = c.I[kO], aXd = c.Id[kO];                 // arc score and its tangent, staged at load
    const float cX = c.C[kX], cXd = c.Cd[kX];
    float m[2] = {VLG_LOWEST, VLG_LOWEST};
    for (int r = rr; r < w; r += G) {
        m[0] = fmaxf(m[0], c.C[eA + r] + c.C[eB + r]);
        if (DIR == 0 ? r >= 1 : r <= w - 2) m[1] = fmaxf(m[1], c.C[eU + VLG_MUL24(r, P)] + c.I[eV + r]);
    }
    x.template allreduce_max<2>(m, G);
    float s[4] = {0.f, 0.f, 0.f, 0.f};   // sum of weights of T, of C; weighted tangent sums of T, of C
    for (int r = rr; r < w; r += G) {
        const float e0 = VLG_EXP(c.C[eA + r] + c.C[eB + r] - m[0]);
        s[0] += e0;
        s[2] = fmaf(e0, c.Cd[eA + r] + c.Cd[eB + r], s[2]);
        if (DIR == 0 ? r >= 1 : r <= w - 2) {
            const int ku = eU + VLG_MUL24(r, P);
            const float e1 = VLG_EXP(c.C[ku] + c.I[eV + r] - m[1]);
            s[1] += e1;
            s[3] = fmaf(e1, c.Cd[ku] + c.Id[eV + r], s[3]);
        }
    }
    x.template allreduce_sum<4>(s, G);
    const float T = m[0] + VLG_LOG(s[0]), Td = s[2] / s[0];   // (s[0] >= 1: the term at the maximum has weight 1)
    const float In = aX + T, Ind = aXd + Td;
    // the same-width term folded in as fold_term does: one exponential of -|m - t| serves both rescales
    const float t = cX + In, td = cXd + Ind;
    const float d = m[1] - t, e = VLG_EXP(-fabsf(d));
    const float Sw = d >= 0.f ? s[1] + e : fmaf(s[1], e, 1.f);
    float Cv = fmaxf(m[1], t) + VLG_LOG(Sw);
    float Cvd = (d >= 0.f ? fmaf(e, td, s[3]) : fmaf(s[3], e, td)) / Sw;
    if (DIR == 1 && D == 0 && w != c.len) { Cv = VLG_NEGINF; Cvd = 0.f; }   // masked root cell, deptree.py:71-72
    if (live && rr == 0) {
        c.I[kO] = In;
        c.Id[kO] = Ind;
        c.C[kO] = Cv;
        c.Cd[kO] = Cvd;
        if (GRAD && DIR == 0) { c.S[D + w] = T; c.Sd[D + w] = Td; }   // the outside replay's tape
    }
}

// the direction's component at element i of a pair of tensors shaped like a potential (each may be null = 0)
template <typename VIn>
VLG_HD float expect_dir(const typename VIn::T* v, const typename VIn::T* v_sub, size_t i) {
    return (v ? VIn::ld(v, i) : 0.f) - (v_sub ? VIn::ld(v_sub, i) : 0.f);
}

// weight of a term (value t, tangent td) of a cell (value out, tangent outd) under the adjoint (g, gd): adj_w and its derivative
VLG_HD void expect_adj(float g, float gd, float t, float td, float out, float outd, float& wv, float& wd) {
    const float p = VLG_EXP(fminf(t - out, 0.f));
    wv = g * p;
    wd = fmaf(gd, p, wv * (td - outd));
}

// the self term of IL(j,i) / IR(i,j) and its tangent (see dep_self)
VLG_HD void expect_self(const ExpectCtx& c, int D, int w, int dir, float& wv, float& wd) {
    const int P = c.P, DW = D + VLG_MUL24(w, P);
    const int kO = dir == 0 ? DW : D + w + 1, kX = dir == 0 ? D : DW + w + 1;
    float g = c.gCc[kO] + c.gCi[kO], gd = c.gCcd[kO] + c.gCid[kO];
    if (dir == 1 && D == 0 && w != c.len) { g = 0.f; gd = 0.f; }
    expect_adj(g, gd, c.C[kX] + c.I[kO], c.Cd[kX] + c.Id[kO], c.C[kO], c.Cd[kO], wv, wd);
}

// Outside, one span, one direction (see dep_bw_span): every target below is owned by this (span, r) within the width.
template <int DIR>
VLG_HD void expect_bw_span(const ExpectCtx& c, int w, int G, int D, int rr) {
    const int P = c.P, DW = D + VLG_MUL24(w, P);
    const int eU = DIR == 0 ? D : D + P + w + 1;
    const int eV = DIR == 0 ? DW : D + 2;
    const int eX = DIR == 0 ? D + 1 : DW + 1;
    const int kO = DIR == 0 ? DW : D + w + 1;
    const int selfr = DIR == 0 ? 0 : w - 1;
    float g = c.gCc[kO] + c.gCi[kO], gd = c.gCcd[kO] + c.gCid[kO];
    if (DIR == 1 && D == 0 && w != c.len) { g = 0.f; gd = 0.f; }
    const float oc = c.C[kO], ocd = c.Cd[kO], Tv = c.S[D + w], Tvd = c.Sd[D + w];
    float s0, s0d, s1, s1d;
    expect_self(c, D, w, 0, s0, s0d);
    expect_self(c, D, w, 1, s1, s1d);
    const float gs = c.gI[DW] + c.gI[D + w + 1] + s0 + s1, gsd = c.gId[DW] + c.gId[D + w + 1] + s0d + s1d;
    for (int r = rr; r < w; r += G) {
        const int ku = eU + VLG_MUL24(r, P);
        float wc, wcd, wt, wtd;
        expect_adj(g, gd, c.C[ku] + c.I[eV + r], c.Cd[ku] + c.Id[eV + r], oc, ocd, wc, wcd);
        expect_adj(gs, gsd, c.C[D + 1 + r] + c.C[DW + 1 + r], c.Cd[D + 1 + r] + c.Cd[DW + 1 + r], Tv, Tvd, wt, wtd);
        if (r != selfr) { c.gI[eV + r] += wc; c.gId[eV + r] += wcd; }
        c.gCc[ku] += wc;
        c.gCcd[ku] += wcd;
        c.gCi[eX + r] += wt;
        c.gCid[eX + r] += wtd;
    }
}

// The lane plan of a width on one half of the workgroup (nd lanes, this one is lane t of them; `cap` = VLG_DP_LANES_FW / _BW): groups of
// G = 1 << lg lanes, `per` groups side by side; this lane is lane rr of group `slot`.
struct ExpectLanes {
    int lg, G, per, rr, slot;
    VLG_HDM ExpectLanes(int spans, int w, int nd, int t, int cap)
        : lg(group_log2(spans, w, nd, cap)), G(1 << lg), per(nd >> lg), rr(t & (G - 1)), slot(t >> lg) {}
};

// One sentence: the body of one workgroup.  arc, v, v_sub, mu, hv point at THIS sentence; v, v_sub, ev, mu, hv may be null.
template <bool GRAD, typename In, typename VIn, typename X>
VLG_HD void expect_run(const ExpectCtx& c, const typename In::T* arc, const typename VIn::T* v, const typename VIn::T* v_sub, int N,
                       float* logZ, float* ev, float* mu, float* hv, int tid, int nt, X& x) {
    const int Ne = c.Ne, P = c.P, len = c.len;
    for (int i = tid; i < Ne * P; i += nt) {
        c.C[i] = VLG_NEGINF;
        c.I[i] = VLG_NEGINF;
        c.Cd[i] = 0.f;
        c.Id[i] = 0.f;
        if (GRAD) {
            c.gCc[i] = 0.f; c.gCi[i] = 0.f; c.gI[i] = 0.f;
            c.gCcd[i] = 0.f; c.gCid[i] = 0.f; c.gId[i] = 0.f;
        }
    }
    x.sync();
    for (int idx = tid; idx < Ne * Ne; idx += nt) {
        const int h = idx / Ne, ch = idx - h * Ne;
        if (ch == h) {
            c.C[h * P + h] = 0.f;
            c.C[h * P + h + 1] = 0.f;
        } else {
            const size_t at = (size_t)h * N + ch;
            const float a = pot_clamp(In::ld(arc, at));
            float d = expect_dir<VIn>(v, v_sub, at);
            if (!(a > VLG_POT_FLOOR)) d = 0.f;   // a forbidden arc carries no tangent, whatever v holds there
            const int k = ch < h ? h * P + ch : h * P + ch + 1;
            c.I[k] = a * VLG_LOG2E;
            c.Id[k] = d;
        }
    }
    x.sync();
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
            if (right) expect_fw_span<GRAD, 1>(c, w, l.G, D, live, l.rr, x);
            else expect_fw_span<GRAD, 0>(c, w, l.G, D, live, l.rr, x);
        }
        x.sync();
    }
    if (tid == 0) {
        *logZ = c.C[len + 1] * VLG_LN2;   // CR(0,len)
        if (ev) *ev = c.Cd[len + 1];
    }
    if (!GRAD) return;
    if (tid == 0) c.gCc[len + 1] = 1.f;   // seed (1, 0)
    x.sync();
    for (int w = Ne - 1; w >= 1; --w) {
        const int spans = Ne - w;
        const ExpectLanes l(spans, w, nd, t, VLG_DP_LANES_BW);
        for (int base = l.slot; base < spans; base += l.per) {
            const int D = VLG_MUL24(base, P + 1);
            if (right) expect_bw_span<1>(c, w, l.G, D, l.rr);
            else expect_bw_span<0>(c, w, l.G, D, l.rr);
        }
        x.sync();
    }
    for (int idx = tid; idx < N * N; idx += nt) {
        const int h = idx / N, ch = idx - h * N;
        float g = 0.f, gd = 0.f;
        if (h < Ne && ch < Ne && ch != h) {
            const int k = ch < h ? h * P + ch : h * P + ch + 1;
            const int i = ch < h ? ch : h, w = ch < h ? h - ch : ch - h;
            float sv, sd;
            expect_self(c, i * (P + 1), w, ch < h ? 0 : 1, sv, sd);   // + the self term the sweep left out
            g = c.gI[k] + sv;
            gd = c.gId[k] + sd;
        }
        if (mu) mu[idx] = g;
        if (hv) hv[idx] = gd;
    }
}

}  // namespace vlg
