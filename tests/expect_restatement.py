"""What the expectation tests share (test_expect_host.py, test_expect_gpu.py): the dual-number inside-outside pass of
vlg_deptree_expect restated in numpy, a brute-force form over every tree, and the tolerances.  A helper, not a test.

The rule (normative; the kernel, the host emulator and this file implement it).  Positions 0 ... len, root 0; cells as in
deptree.py:25-76.  Every cell carries a value and a tangent: its derivative along a direction d = v - v_sub in potential space.
    load     phi = max(arc, -1e30) (NaN -> -1e30); tangent of an arc = d[h,c], forced to 0 where phi is at the floor.
    inside   X = log sum_r exp t_r  has  X' = sum_r p_r t_r', p_r = exp(t_r - X);  I = T + phi  has  I' = T' + d;
             the masked root cell CR(0,w), w != len, has value zero and tangent 0;  logZ = CR(0,len), ev = CR'(0,len) = <mu, d>.
    outside  seed (1, 0) at CR(0,len); a cell with adjoint (g, g') hands the operands of term r (g p_r, g' p_r + g p_r (t_r' - X'));
             mu[h,c] = the adjoint of the arc, hv[h,c] = its tangent = (Hessian of logZ) d.
`dual` runs it in any floating dtype: float64 is the reference of every test, float32 (the same sums, one split point after the
other) is the yardstick the tolerances scale with.
"""
import functools

import numpy as np

import sample_restatement as R

FLOOR = -1e30
ZERO = -1e12   # the semiring zero of the reference (semirings.py:16): finite, never -inf


def dual(arc, length, v=None, v_sub=None, dtype=np.float64, want_grad=True):
    """(logZ, ev, mu [N,N], hv [N,N]) of one sentence; mu, hv None unless want_grad.  Invalid length: (nan, nan, 0, 0)."""
    f = np.dtype(dtype).type
    N = np.asarray(arc).shape[-1]
    if length < 1 or length > N - 1:
        z = np.zeros((N, N), dtype)
        return f(np.nan), f(np.nan), (z if want_grad else None), (z.copy() if want_grad else None)
    n = length + 1
    a = np.asarray(arc, dtype)[:n, :n]
    with np.errstate(invalid="ignore"):
        phi = np.where(a > f(FLOOR), a, f(FLOOR)).astype(dtype)
    d = np.zeros((n, n), dtype)
    if v is not None:
        d = d + np.asarray(v, dtype)[:n, :n]
    if v_sub is not None:
        d = d - np.asarray(v_sub, dtype)[:n, :n]
    with np.errstate(invalid="ignore"):
        d = np.where(phi > f(FLOOR), d, f(0)).astype(dtype)
    d[np.arange(n), np.arange(n)] = 0
    C = np.full((n, n), ZERO, dtype)
    I = np.full((n, n), ZERO, dtype)
    Cd, Id = np.zeros((n, n), dtype), np.zeros((n, n), dtype)
    T, Td = np.zeros((n, n), dtype), np.zeros((n, n), dtype)   # T(i,j) at [i,j]
    C[np.arange(n), np.arange(n)] = 0

    def lse(t, td):
        "over axis 0 (the split points, added one after the other): value, tangent, weights p_r"
        m = t.max(axis=0)
        e = np.exp(t - m)
        s = np.add.reduce(e, axis=0)
        p = e / s
        return m + np.log(s), np.add.reduce(p * td, axis=0), p

    for w in range(1, n):
        i = np.arange(n - w)[None, :]
        j = i + w
        r = i + np.arange(w)[:, None]                                  # i <= r < j, shape (w, spans)
        i0, j0 = i[0], j[0]
        T[i0, j0], Td[i0, j0], _ = lse(C[i, r] + C[j, r + 1], Cd[i, r] + Cd[j, r + 1])
        I[j0, i0], Id[j0, i0] = T[i0, j0] + phi[j0, i0], Td[i0, j0] + d[j0, i0]
        I[i0, j0], Id[i0, j0] = T[i0, j0] + phi[i0, j0], Td[i0, j0] + d[i0, j0]
        C[j0, i0], Cd[j0, i0], _ = lse(C[r, i] + I[j, r], Cd[r, i] + Id[j, r])                  # CL(j,i)
        C[i0, j0], Cd[i0, j0], _ = lse(I[i, r + 1] + C[r + 1, j], Id[i, r + 1] + Cd[r + 1, j])  # CR(i,j)
        if w != length:
            C[0, w], Cd[0, w] = ZERO, 0
    logZ, ev = C[0, length], Cd[0, length]
    if not want_grad:
        return logZ, ev, None, None
    gC, gCd = np.zeros((n, n), dtype), np.zeros((n, n), dtype)
    gI, gId = np.zeros((n, n), dtype), np.zeros((n, n), dtype)
    gC[0, length] = 1

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
        g, gd = gC[i0, j0].copy(), gCd[i0, j0].copy()                  # CR(i,j)
        if w != length:
            g[0], gd[0] = 0, 0                                         # masked root cell
        wv, wd = hand(g, gd, I[i, r + 1] + C[r + 1, j], Id[i, r + 1] + Cd[r + 1, j], C[i0, j0], Cd[i0, j0])
        gI[i, r + 1] += wv; gId[i, r + 1] += wd
        gC[r + 1, j] += wv; gCd[r + 1, j] += wd
        wv, wd = hand(gC[j0, i0], gCd[j0, i0], C[r, i] + I[j, r], Cd[r, i] + Id[j, r], C[j0, i0], Cd[j0, i0])   # CL(j,i)
        gI[j, r] += wv; gId[j, r] += wd
        gC[r, i] += wv; gCd[r, i] += wd
        gs, gsd = gI[j0, i0] + gI[i0, j0], gId[j0, i0] + gId[i0, j0]   # adjoint of T(i,j)
        wv, wd = hand(gs, gsd, C[i, r] + C[j, r + 1], Cd[i, r] + Cd[j, r + 1], T[i0, j0], Td[i0, j0])
        gC[i, r] += wv; gCd[i, r] += wd
        gC[j, r + 1] += wv; gCd[j, r + 1] += wd
    mu, hv = np.zeros((N, N), dtype), np.zeros((N, N), dtype)
    mu[:n, :n], hv[:n, :n] = gI, gId
    return logZ, ev, mu, hv


def dual_batch(arc, lengths, v=None, v_sub=None, dtype=np.float64):
    "(logZ [B], ev [B], mu [B,N,N], hv [B,N,N])"
    outs = [dual(arc[b], int(lengths[b]), None if v is None else v[b], None if v_sub is None else v_sub[b], dtype) for b in range(len(arc))]
    return tuple(np.stack([np.asarray(o[k], dtype) for o in outs]) for k in range(4))


@functools.lru_cache(maxsize=None)
def _trees(length):
    "[T, length+1, length+1] 0/1 arc indicators of every projective single-root tree"
    hs = R.all_trees(length)
    x = np.zeros((len(hs), length + 1, length + 1))
    for k, h in enumerate(hs):
        x[k, h[1:], np.arange(1, length + 1)] = 1
    return x


def brute(arc, length, v):
    """By enumeration, no DP: (logZ, ev, mu, hv, H, grad_H) with ev = E[<v, tree>], hv = Cov(tree, <v, tree>) and
    grad_H = -Cov(tree, <arc, tree>) over positions 0 ... length."""
    n = length + 1
    x = _trees(length)
    a, d = np.asarray(arc, np.float64)[:n, :n], np.asarray(v, np.float64)[:n, :n]
    s = (x * a).sum((1, 2))
    logZ = np.logaddexp.reduce(s)
    p = np.exp(s - logZ)
    mu = np.tensordot(p, x, 1)
    sv = (x * d).sum((1, 2))
    ev = p @ sv
    hv = np.tensordot(p * sv, x, 1) - mu * ev
    H = -(p * (s - logZ)).sum()
    gH = -(np.tensordot(p * s, x, 1) - mu * (p @ s))
    return logZ, ev, mu, hv, H, gH


# ---- tolerances (against the float64 restatement): the floor, or 6 x the float32 restatement's own error when that is larger ----------
def value_bound(logZ64, mu64, v64, err32=0.0):
    "for logZ, ev, H, CE, KL of one sentence: 2e-5 max(1, |logZ|, sum mu |v|)"
    scale = max(1.0, abs(float(logZ64)), float((np.abs(mu64) * np.abs(v64)).sum()))
    return max(2e-5 * scale, 6.0 * float(err32))


def mu_bound(err32=0.0):
    return max(5e-5, 6.0 * float(err32))


def grad_bound(ref64, err32=0.0):
    "for hv and the gradients of one sentence: 1e-4 of the largest float64 magnitude of that output within the sentence"
    return max(1e-4 * float(np.abs(ref64).max()), 6.0 * float(err32))


# ---- the placement plan of vlg_deptree_expect, restated (ExpectLayout / dp_plan, vlgae_amd/csrc/vlg_dp_expect.h) -----------------------
LDS_BUDGET = 160 * 1024


def _align16(x):
    return (x + 15) & ~15


def layout(N, grad, mode):
    "(lds_bytes, ws_bytes) of one sentence: which of the twelve (grad) or four charts of N * pitch(N) floats sit in LDS at this mode"
    chart = _align16(N * ((N + 1) | 1) * 4)
    if grad:   # values + tape + their tangents (6) | gCc, gCi pairs (4) | gI pair (2)
        in_lds = 6 * (mode < 1) + 4 * (mode < 3) + 2 * (mode < 2)
        return in_lds * chart, (12 - in_lds) * chart
    in_lds = 2 * (mode < 2) + 2 * (mode < 1)   # C, I | their tangents
    return in_lds * chart, (4 - in_lds) * chart


def plan(N, grad):
    "(mode, lds_bytes, ws_bytes): the first mode whose LDS part fits"
    for mode in range(4):
        lds, ws = layout(N, grad, mode)
        if lds <= LDS_BUDGET or mode == 3:
            return mode, lds, ws


def boundaries():
    "every N in 3 ... 255 at which the plan of either op changes mode (so that N - 1 and N run different placements)"
    return sorted({N for N in range(3, 256) for grad in (False, True) if plan(N, grad)[0] != plan(N - 1, grad)[0]})


# ---- comparison shared by the emulator and the GPU tests ------------------------------------------------------------------------------
def direction(arc, lengths, v=None, v_sub=None):
    "the effective direction d [B,N,N] in float64: v - v_sub, 0 on forbidden arcs, the diagonal and outside the sentence"
    arc = np.asarray(arc, np.float64)
    B, N, _ = arc.shape
    d = np.zeros((B, N, N)) + (0 if v is None else np.asarray(v, np.float64)) - (0 if v_sub is None else np.asarray(v_sub, np.float64))
    pos = np.arange(N)
    with np.errstate(invalid="ignore"):
        ok = (arc > FLOOR) & (pos[None, :, None] != pos[None, None, :])
    for b in range(B):
        n = int(lengths[b]) + 1 if 1 <= int(lengths[b]) <= N - 1 else 0
        ok[b, n:, :] = False
        ok[b, :, n:] = False
    return np.where(ok, d, 0.0)


def ratios(got, arc, lengths, v=None, v_sub=None, refs=None):
    """Largest error / bound per output of (logZ, ev, mu, hv) `got` (entries may be None) over the valid sentences of a batch, against
    the float64 restatement; invalid lengths are checked exactly (NaN values, zero mu / hv) by assertion.  refs: (r64, r32) if known."""
    r64, r32 = refs or (dual_batch(arc, lengths, v, v_sub, np.float64), dual_batch(arc, lengths, v, v_sub, np.float32))
    d = direction(arc, lengths, v, v_sub)
    N = np.asarray(arc).shape[-1]
    out = {}
    for b in range(len(lengths)):
        if not 1 <= int(lengths[b]) <= N - 1:
            for k in (0, 1):
                assert got[k] is None or np.isnan(got[k][b]), (k, b, got[k][b])
            for k in (2, 3):
                assert got[k] is None or not np.any(got[k][b]), (k, b)
            continue
        bounds = (value_bound(r64[0][b], r64[2][b], d[b], abs(float(r32[0][b]) - r64[0][b])),
                  value_bound(r64[0][b], r64[2][b], d[b], abs(float(r32[1][b]) - r64[1][b])),
                  mu_bound(np.abs(r32[2][b] - r64[2][b]).max()),
                  grad_bound(r64[3][b], np.abs(r32[3][b] - r64[3][b]).max()))
        for k, name in enumerate(("logZ", "ev", "mu", "hv")):
            if got[k] is None:
                continue
            g = np.asarray(got[k][b], np.float64)
            assert np.all(np.isfinite(g)), (name, b)
            err = float(np.abs(g - r64[k][b]).max())
            if k == 3 and bounds[3] == 0.0:   # a direction under which nothing varies: hv is 0 exactly
                assert err == 0.0, (name, b, err)
                continue
            out[name] = max(out.get(name, 0.0), err / bounds[k])
    return out
