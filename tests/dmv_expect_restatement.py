"""What the DMV1o expectation tests share (test_dmv_expect_host.py, test_dmv_expect_gpu.py): the dual-number inside-outside pass of
vlg_dmv1o_expect restated in numpy, a brute-force form over every tree with its valences, the placement plan, and the comparison with
the family's tolerances (expect_restatement.value_bound / mu_bound / grad_bound).  A helper, not a test.

The rule (normative; the kernel, the host emulator and this file implement it).  Positions 0 ... len, root 0; potentials are root-merged,
dec [N,2,2,2] = [head, dir (0 LEFT, 1 RIGHT), valence (0 HASCHILD, 1 NOCHILD), decision (0 GO, 1 STOP)], attach [N,N,2] = [head, child,
valence]; cells as in dmv.py:18-69 (dmv_sample_restatement.inside64).  Every cell carries a value and a tangent: its derivative along
a direction d = (d_dec, d_att) = v - v_sub in potential space.
    load     potentials are clamped to >= -1e30 (NaN -> -1e30); a component of d is forced to 0 where its own potential is forbidden
             (not above -5e11: at or below the semiring zero -1e12 that DMV1o.merge writes) and outside the sentence.  Incomplete slot
             (h -> c, val): attach[h,c,val] + dec[h,dir,val,GO], tangent d_att[h,c,val] + d_dec[h,dir,val,GO]; C(h,h) towards dir:
             dec[h,dir,val,STOP], tangent d_dec[h,dir,val,STOP].
    inside   X = log sum_r exp t_r  has  X' = sum_r p_r t_r', p_r = exp(t_r - X);  I.v = staged.v + S, I'.v = staged'.v + S';
             the masked root cell CR(0,w), w != len, has value zero and tangent 0;  logZ = CR(0,len).NC, ev = its tangent = <mu, d>.
    outside  seed (1, 0) at CR(0,len).NC; a cell with adjoint (g, g') hands the operands of term r (g p_r, g' p_r + g p_r (t_r' - X'));
             mu_attach = the adjoint of the incomplete cells, mu_dec[..., STOP] = the adjoint of the width-0 cells, mu_dec[..., GO] = the
             sum of mu_attach[h, c, v] over the children c on that side; hv_* = their tangents = (Hessian of logZ) d.
Tolerances: the family's bounds; the GO entries of mu_dec, which are counts and not probabilities, through count_ratio below.
`dual` runs it in any floating dtype: float64 is the reference of every test, float32 (the same sums, one split point after the
other) is the yardstick the tolerances scale with.
"""
import functools

import numpy as np

import dmv_sample_restatement as R
from expect_restatement import grad_bound, mu_bound, value_bound

FLOOR = -1e30
ZERO = -1e12        # the semiring zero of the reference (semirings.py:16): finite, never -inf
FORBIDDEN = -5e11   # a potential not above this carries no direction
HC, NC, LEFT, RIGHT, GO, STOP = 0, 1, 0, 1, 0, 1


def _pair(p):
    return (None, None) if p is None else p


def direction(dec, attach, length, v=None, v_sub=None, dtype=np.float64):
    "the effective direction (d_dec [N,2,2,2], d_att [N,N,2]) of one sentence: v - v_sub, 0 on forbidden entries and outside the sentence"
    N = np.asarray(dec).shape[0]
    out = []
    for pot, a, b in ((dec, _pair(v)[0], _pair(v_sub)[0]), (attach, _pair(v)[1], _pair(v_sub)[1])):
        pot = np.asarray(pot, dtype)
        d = np.zeros(pot.shape, dtype)
        if a is not None:
            d = d + np.asarray(a, dtype)
        if b is not None:
            d = d - np.asarray(b, dtype)
        with np.errstate(invalid="ignore"):
            d = np.where(pot > dtype(FORBIDDEN), d, dtype(0)).astype(dtype)
        out.append(d)
    n = length + 1 if 1 <= length <= N - 1 else 0
    out[0][n:] = 0
    out[1][n:] = 0
    out[1][:, n:] = 0
    return out


def dual(dec, attach, length, v=None, v_sub=None, dtype=np.float64, want_grad=True):
    """(logZ, ev, mu_dec [N,2,2,2], mu_att [N,N,2], hv_dec, hv_att) of one sentence; the last four None unless want_grad.
    Invalid length: (nan, nan, 0, 0, 0, 0)."""
    dtype = np.dtype(dtype).type
    f = dtype
    dec, attach = np.asarray(dec), np.asarray(attach)
    N = dec.shape[0]
    if length < 1 or length > N - 1:
        z = [np.zeros(dec.shape, dtype), np.zeros(attach.shape, dtype), np.zeros(dec.shape, dtype), np.zeros(attach.shape, dtype)]
        return (f(np.nan), f(np.nan), *(z if want_grad else [None] * 4))
    n = length + 1
    dd_full, da_full = direction(dec, attach, length, v, v_sub, dtype)
    with np.errstate(invalid="ignore"):
        d = np.where(dec.astype(dtype) > f(FLOOR), dec.astype(dtype), f(FLOOR))[:n]
        a = np.where(attach.astype(dtype) > f(FLOOR), attach.astype(dtype), f(FLOOR))[:n, :n]
    dd, da = dd_full[:n], da_full[:n, :n]
    k = np.arange(n)
    side = (k[None, :] > k[:, None]).astype(int)                     # [h, c]: 0 = c left of h, 1 = right
    st = a + d[k[:, None], side, :, GO]                              # staged incomplete slots [h, c, v]
    std = da + dd[k[:, None], side, :, GO]
    std[k, k] = 0
    I, Id = np.full((n, n, 2), ZERO, dtype), np.zeros((n, n, 2), dtype)
    CL, CLd = np.full((n, n, 2), ZERO, dtype), np.zeros((n, n, 2), dtype)
    CR, CRd = np.full((n, n, 2), ZERO, dtype), np.zeros((n, n, 2), dtype)
    SL, SLd, SR, SRd = (np.zeros((n, n), dtype) for _ in range(4))   # at [i, j]
    CL[k, k], CLd[k, k] = d[:, LEFT, :, STOP], dd[:, LEFT, :, STOP]
    CR[k, k], CRd[k, k] = d[:, RIGHT, :, STOP], dd[:, RIGHT, :, STOP]

    def lse(t, td):
        "over axis 0 (the split points, added one after the other): value, tangent"
        m = t.max(axis=0)
        e = np.exp(t - m)
        s = np.add.reduce(e, axis=0)
        return m + np.log(s), np.add.reduce((e / s) * td, axis=0)

    for w in range(1, n):
        i = np.arange(n - w)[None, :]
        j = i + w
        r = i + np.arange(w)[:, None]                                # i <= r < j, shape (w, spans)
        i0, j0 = i[0], j[0]
        SL[i0, j0], SLd[i0, j0] = lse(CR[i, r, NC] + CL[j, r + 1, HC], CRd[i, r, NC] + CLd[j, r + 1, HC])
        SR[i0, j0], SRd[i0, j0] = lse(CR[i, r, HC] + CL[j, r + 1, NC], CRd[i, r, HC] + CLd[j, r + 1, NC])
        I[j0, i0], Id[j0, i0] = SL[i0, j0][:, None] + st[j0, i0], SLd[i0, j0][:, None] + std[j0, i0]
        I[i0, j0], Id[i0, j0] = SR[i0, j0][:, None] + st[i0, j0], SRd[i0, j0][:, None] + std[i0, j0]
        for val in (HC, NC):
            CL[j0, i0, val], CLd[j0, i0, val] = lse(CL[r, i, NC] + I[j, r, val], CLd[r, i, NC] + Id[j, r, val])
            CR[i0, j0, val], CRd[i0, j0, val] = lse(I[i, r + 1, val] + CR[r + 1, j, NC], Id[i, r + 1, val] + CRd[r + 1, j, NC])
        if w != length:
            CR[0, w], CRd[0, w] = ZERO, 0                            # dmv.py:63
    logZ, ev = CR[0, length, NC], CRd[0, length, NC]
    if not want_grad:
        return logZ, ev, None, None, None, None
    gCL, gCLd, gCR, gCRd, gI, gId = (np.zeros((n, n, 2), dtype) for _ in range(6))
    gCR[0, length, NC] = 1

    def hand(g, gd, t, td, X, Xd):
        p = np.exp(np.minimum(t - X, 0))
        wv = g * p
        return wv, gd * p + wv * (td - Xd)

    for w in range(n - 1, 0, -1):
        i = np.arange(n - w)[None, :]
        j = i + w
        r = i + np.arange(w)[:, None]
        i0, j0 = i[0], j[0]
        # complete cells first: their r = 0 | w-1 term feeds the incomplete cell of the same width
        g, gd = gCR[i0, j0].copy(), gCRd[i0, j0].copy()
        if w != length:
            g[0], gd[0] = 0, 0                                       # masked root cell
        for val in (HC, NC):
            wv, wd = hand(g[:, val], gd[:, val], I[i, r + 1, val] + CR[r + 1, j, NC], Id[i, r + 1, val] + CRd[r + 1, j, NC],
                          CR[i0, j0, val], CRd[i0, j0, val])
            gI[i, r + 1, val] += wv; gId[i, r + 1, val] += wd
            gCR[r + 1, j, NC] += wv; gCRd[r + 1, j, NC] += wd
            wv, wd = hand(gCL[j0, i0, val], gCLd[j0, i0, val], CL[r, i, NC] + I[j, r, val], CLd[r, i, NC] + Id[j, r, val],
                          CL[j0, i0, val], CLd[j0, i0, val])
            gI[j, r, val] += wv; gId[j, r, val] += wd
            gCL[r, i, NC] += wv; gCLd[r, i, NC] += wd
        gs, gsd = gI[j0, i0, HC] + gI[j0, i0, NC], gId[j0, i0, HC] + gId[j0, i0, NC]          # adjoint of SL(i,j)
        wv, wd = hand(gs, gsd, CR[i, r, NC] + CL[j, r + 1, HC], CRd[i, r, NC] + CLd[j, r + 1, HC], SL[i0, j0], SLd[i0, j0])
        gCR[i, r, NC] += wv; gCRd[i, r, NC] += wd
        gCL[j, r + 1, HC] += wv; gCLd[j, r + 1, HC] += wd
        gs, gsd = gI[i0, j0, HC] + gI[i0, j0, NC], gId[i0, j0, HC] + gId[i0, j0, NC]          # adjoint of SR(i,j)
        wv, wd = hand(gs, gsd, CR[i, r, HC] + CL[j, r + 1, NC], CRd[i, r, HC] + CLd[j, r + 1, NC], SR[i0, j0], SRd[i0, j0])
        gCR[i, r, HC] += wv; gCRd[i, r, HC] += wd
        gCL[j, r + 1, NC] += wv; gCLd[j, r + 1, NC] += wd
    outs = []
    for gi, gl, gr in ((gI, gCL, gCR), (gId, gCLd, gCRd)):
        md, ma = np.zeros((N, 2, 2, 2), dtype), np.zeros((N, N, 2), dtype)
        gi = gi.copy()
        gi[k, k] = 0
        ma[:n, :n] = gi
        md[:n, LEFT, :, STOP], md[:n, RIGHT, :, STOP] = gl[k, k], gr[k, k]
        left = (k[None, :] < k[:, None])[:, :, None]
        md[:n, LEFT, :, GO] = np.where(left, gi, 0).sum(1)
        md[:n, RIGHT, :, GO] = np.where(~left, gi, 0).sum(1)
        outs += [md, ma]
    return logZ, ev, outs[0], outs[1], outs[2], outs[3]


def dual_batch(dec, attach, lengths, v=None, v_sub=None, dtype=np.float64):
    "(logZ [B], ev [B], mu_dec, mu_att, hv_dec, hv_att) stacked over the batch"
    def row(p, b):
        return None if p is None else tuple(None if t is None else t[b] for t in p)
    outs = [dual(dec[b], attach[b], int(lengths[b]), row(v, b), row(v_sub, b), dtype) for b in range(len(dec))]
    return tuple(np.stack([np.asarray(o[k], dtype) for o in outs]) for k in range(6))


@functools.lru_cache(maxsize=None)
def _tree_counts(length):
    "([T,n,2,2,2] dec counts, [T,n,n,2] attach counts) of every projective single-root tree with its valences"
    hs = R.all_trees(length)
    n = length + 1
    zd, za = np.zeros((n, 2, 2, 2)), np.zeros((n, n, 2))
    cs = [R.tree_score(zd, za, h, length)[2:] for h in hs]
    return np.stack([c[0] for c in cs]), np.stack([c[1] for c in cs])


def brute(dec, attach, length, v):
    """By enumeration, no DP: (logZ, ev, mu_dec, mu_att, hv_dec, hv_att, H, gH_dec, gH_att) over positions 0 ... length with
    ev = E[<d, tree>], hv = Cov(tree, <d, tree>), grad H = -Cov(tree, <theta, tree>).  Forbidden entries count as score 0 where no tree
    uses them (merged potentials: no tree does)."""
    n = length + 1
    xd, xa = _tree_counts(length)
    d, a = np.asarray(dec, np.float64)[:n], np.asarray(attach, np.float64)[:n, :n]
    vd, va = direction(dec, attach, length, v)
    vd, va = vd[:n], va[:n, :n]
    s = (xd * np.where(xd > 0, d, 0)).sum((1, 2, 3, 4)) + (xa * np.where(xa > 0, a, 0)).sum((1, 2, 3))
    logZ = np.logaddexp.reduce(s)
    p = np.exp(s - logZ)
    mud, mua = np.tensordot(p, xd, 1), np.tensordot(p, xa, 1)
    sv = (xd * vd).sum((1, 2, 3, 4)) + (xa * va).sum((1, 2, 3))
    ev = p @ sv
    hvd, hva = np.tensordot(p * sv, xd, 1) - mud * ev, np.tensordot(p * sv, xa, 1) - mua * ev
    H = -(p * (s - logZ)).sum()
    gHd, gHa = -(np.tensordot(p * s, xd, 1) - mud * (p @ s)), -(np.tensordot(p * s, xa, 1) - mua * (p @ s))
    return logZ, ev, mud, mua, hvd, hva, H, gHd, gHa


# ---- the placement plan of vlg_dmv1o_expect, restated (DmvExpectLayout / dp_plan, vlgae_amd/csrc/vlg_dmv_expect.h) -------------------
LDS_BUDGET = 160 * 1024


def _align16(x):
    return (x + 15) & ~15


def layout(N, grad, mode):
    """(lds_bytes, ws_bytes) of one sentence.  Per cell of the N x pitch(N) chart: C 8 + I 8 + S 4 + gCc 4 + gCi 8 + gI 8 bytes, each
    with its tangent (80; forward only C, I and their tangents: 32), plus the staged dec and its tangent (2 x 32 N), always in LDS."""
    cells = N * ((N + 1) | 1)
    c8, c4, staging = _align16(cells * 8), _align16(cells * 4), 2 * _align16(N * 32)
    if grad:   # values + tape + their tangents | gCc, gCi pairs | gI pair
        groups = ((4 * c8 + 2 * c4, mode < 1), (2 * c4 + 2 * c8, mode < 3), (2 * c8, mode < 2))
    else:      # C, I | their tangents
        groups = ((2 * c8, mode < 2), (2 * c8, mode < 1))
    lds = staging + sum(b for b, in_lds in groups if in_lds)
    return lds, sum(b for b, in_lds in groups if not in_lds)


def plan(N, grad):
    "(mode, lds_bytes, ws_bytes): the first mode whose LDS part fits"
    for mode in range(4):
        lds, ws = layout(N, grad, mode)
        if lds <= LDS_BUDGET or mode == 3:
            return mode, lds, ws


def boundaries():
    "every N in 3 ... 255 at which the plan of either image changes mode (so that N - 1 and N run different placements)"
    return sorted({N for N in range(3, 256) for grad in (False, True) if plan(N, grad)[0] != plan(N - 1, grad)[0]})


def first_workspace_n(grad=True):
    return next(N for N in range(2, 256) if plan(N, grad)[2] > 0)


# ---- test cases and the comparison shared by the emulator and the GPU tests -----------------------------------------------------------
def ragged(N):
    return np.array([N - 1, 1, max(1, (N - 1) // 2)], np.int64)


def case(N, seed, B=3, scale=0.5):
    "(dec, attach, (v_dec, v_att)) float32: root-merged potentials of random unmerged ones, and a random direction"
    rng = np.random.default_rng(seed)
    ud, ua, ur = R.random_unmerged(rng, B, N - 1, scale)
    dec, attach = R.merge64(ud, ua, ur)
    v = ((0.5 * rng.standard_normal(dec.shape)).astype(np.float32), (0.5 * rng.standard_normal(attach.shape)).astype(np.float32))
    return dec, attach, v


NAMES = ("logZ", "ev", "mu_dec", "mu_att", "hv_dec", "hv_att")
COUNT_FLOOR = 5e-5   # mu_bound's floor


def count_ratio(got, ref64, ref32):
    """Largest error / bound of one sentence's dec counts [N,2,2,2].  The STOP entries are probabilities and keep mu_bound.  The GO entries
    are expected NUMBERS of children, sums of up to len attach marginals that are not bounded by 1 (random potentials reach 10 at N = 81
    and 19 at N = 255), so the floor of 5e-5 is taken relative to the largest GO count of the sentence (float64), never below 1.  From
    the float32 restatement's own error against float64 (first sentence of case(N, seed), seeds 500 + N and 7): its GO error is 3 to 19
    times its STOP / attach error and follows the count -- N = 81: attach 4e-6, STOP 7e-6, GO 3e-5 (largest count 10.3); N = 255: attach
    2e-5, STOP 3e-5, GO 3e-4 (count 18); N = 41: all 2e-6 ... 4e-6 (count 2) -- 6e-6 ... 3e-5 of the count throughout."""
    got, ref64, ref32 = (np.asarray(t, np.float64) for t in (got, ref64, ref32))
    e, e32 = np.abs(got - ref64), np.abs(ref32 - ref64)
    stop = e[..., STOP].max() / mu_bound(e32[..., STOP].max())
    go = e[..., GO].max() / max(COUNT_FLOOR * max(1.0, float(np.abs(ref64[..., GO]).max())), 6.0 * float(e32[..., GO].max()))
    return float(max(stop, go))


def ratios(got, dec, attach, lengths, v=None, v_sub=None, refs=None):
    """Largest error / bound per output of `got` = (logZ, ev, mu_dec, mu_att, hv_dec, hv_att) (entries may be None) over the valid
    sentences of a batch, against the float64 restatement; invalid lengths are checked exactly (NaN values, zero counts) by assertion.
    Bounds: expect_restatement's floors, or 6 x the float32 restatement's own error where that is larger; mu_dec: count_ratio.
    refs: (r64, r32) if known."""
    r64, r32 = refs or (dual_batch(dec, attach, lengths, v, v_sub, np.float64), dual_batch(dec, attach, lengths, v, v_sub, np.float32))
    N = np.asarray(dec).shape[1]
    out = {}
    for b in range(len(lengths)):
        if not 1 <= int(lengths[b]) <= N - 1:
            for k in (0, 1):
                assert got[k] is None or np.isnan(got[k][b]), (k, b, got[k][b])
            for k in (2, 3, 4, 5):
                assert got[k] is None or not np.any(got[k][b]), (k, b)
            continue
        row = lambda p: None if p is None else tuple(None if t is None else t[b] for t in p)
        dd, da = direction(dec[b], attach[b], int(lengths[b]), row(v), row(v_sub))
        weight = np.concatenate([(np.abs(r64[2][b]) * np.abs(dd)).ravel(), (np.abs(r64[3][b]) * np.abs(da)).ravel()])
        e32 = [np.abs(np.asarray(r32[k][b], np.float64) - r64[k][b]).max() for k in range(6)]
        vb = lambda err: value_bound(r64[0][b], weight, np.ones_like(weight), err)
        bounds = (vb(e32[0]), vb(e32[1]), mu_bound(e32[2]), mu_bound(e32[3]), grad_bound(r64[4][b], e32[4]), grad_bound(r64[5][b], e32[5]))
        for k, name in enumerate(NAMES):
            if got[k] is None:
                continue
            g = np.asarray(got[k][b], np.float64)
            assert np.all(np.isfinite(g)), (name, b)
            if k == 2:
                out[name] = max(out.get(name, 0.0), count_ratio(g, r64[2][b], r32[2][b]))
                continue
            err = float(np.abs(g - r64[k][b]).max())
            if bounds[k] == 0.0:   # a direction under which nothing varies: hv is 0 exactly
                assert err == 0.0, (name, b, err)
                continue
            out[name] = max(out.get(name, 0.0), err / bounds[k])
    return out
