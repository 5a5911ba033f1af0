"""What the labeled-potential tests share (test_labeled_host.py, test_labeled_gpu.py): vlg_label_fold / vlg_label_expand / the label
draw restated in numpy, the labeled quantities and their gradient formulas on top of the unlabeled restatements, and a brute force
over every labeled tree.  A helper, not a test.

The rule (normative; the kernels, the host emulator and this file implement it).  phi [N,N,L] head x child x label.
    cells    the DP reads cell (h, c) iff 1 <= c <= len, h <= len, h != c (len valid: 1 ... N - 1).  The others are never loaded:
             arc = -1e12 (the semiring zero), best = 0, dbar = 0, every expanded gradient 0.
    labels   label l of a read cell takes part iff phi_l > -1e30 (NaN does not); the others have p_l = 0.
    fold     arc = log sum_l exp phi_l (Log) / max_l phi_l (Max) over the labels that take part, -inf if none does;
             best = the lowest l attaining the maximum (0 if none takes part);
             dbar = sum_l p_l d_l, p_l = exp(phi_l - arc), d_l = v_l - v_sub_l forced to 0 where the label takes no part.
    expand   out_l = scale p_l (g1 + g2 (d_l - dbar))  |  scale g1 p_l;  Max: p_l = [l == best];  0 in rows where no label takes part.
    draw     sample_restatement.draw over the row's labels in label order (a label that takes no part is read as -1e30: weight 0).
Labeled quantities are the unlabeled ones of `arc` (expect_restatement.dual with the arc-level direction dbar), spread by expand:
    d ev / d phi = p (hv + mu (d - dbar))     d ev / d v = mu p      d H / d phi = -p (hv + mu (phi - phibar))
    d H[p,q] / d phi_p = d KL / d phi_p = -p (hv + mu_p (d - dbar))     d / d phi_q = mu_q q - mu_p p
"""
import itertools

import numpy as np

import expect_restatement as E
import kbest_restatement as K
import sample_restatement as S

FLOOR = -1e30
ZERO = -1e12


def potentials(rng, shape, bf16=False, strict=None):
    """kbest_restatement.potentials (2^-12 grid in +-4, bf16-representable on request) with no two equal labels in a row -- no label
    ties -- wherever that can be had: strict (the default up to 8 labels) insists; beyond that rows are redrawn a few times and a tie
    that stays is the first-index rule's business (a row of 255 bfloat16 values on this grid cannot be tie-free)."""
    x = K.potentials(rng, shape, bf16=bf16)
    L = shape[-1]
    strict = L <= 8 if strict is None else strict
    flat = x.reshape(-1, L)
    for _ in range(200 if strict else 3):
        bad = np.nonzero([len(set(r)) < L for r in flat])[0]
        if not len(bad):
            break
        flat[bad] = K.potentials(rng, (len(bad), L), bf16=bf16)
    else:
        assert not strict, "potentials: label ties left"
    return flat.reshape(shape)


def read_mask(N, length):
    "[N,N] bool: the cells (h, c) the DP reads"
    pos = np.arange(N)
    if not 1 <= length <= N - 1:
        return np.zeros((N, N), bool)
    ok = pos <= length
    return ok[:, None] & (ok & (pos >= 1))[None, :] & (pos[:, None] != pos[None, :])


def takes_part(phi):
    with np.errstate(invalid="ignore"):
        return np.asarray(phi) > FLOOR


def fold(phi, length, semiring="log", v=None, v_sub=None, dtype=np.float64):
    """One sentence: (arc [N,N], best [N,N] uint8, dbar [N,N], p [N,N,L]) in `dtype`; sums run over the labels one after the other
    (float32: the sequential yardstick of the tolerances)."""
    f = np.dtype(dtype).type
    phi = np.asarray(phi, dtype)
    N, _, L = phi.shape
    live = read_mask(N, length)
    part = takes_part(phi) & live[:, :, None]
    x = np.where(part, phi, -np.inf).astype(dtype)
    m = x.max(-1)
    some = np.isfinite(m)
    best = np.where(some, np.argmax(x, -1), 0).astype(np.uint8)
    ms = np.where(some, m, 0).astype(dtype)
    w = np.where(part, np.exp(x - ms[:, :, None]), 0).astype(dtype)
    s = np.zeros((N, N), dtype)
    for l in range(L):
        s = (s + w[:, :, l]).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(some[:, :, None], w / np.where(some, s, 1)[:, :, None], 0).astype(dtype)
        if semiring == "max":
            arc = m
            p = (np.arange(L)[None, None, :] == best[:, :, None]) & some[:, :, None]
            p = p.astype(dtype)
        else:
            arc = (ms + np.log(np.where(some, s, 1))).astype(dtype)
            arc = np.where(some, arc, -np.inf)
    arc = np.where(live, arc, f(ZERO)).astype(dtype)
    d = np.zeros(phi.shape, dtype)
    if v is not None:
        d = d + np.asarray(v, dtype)
    if v_sub is not None:
        d = d - np.asarray(v_sub, dtype)
    with np.errstate(invalid="ignore"):
        d = np.where(part, d, 0).astype(dtype)
    dbar = np.zeros((N, N), dtype)
    for l in range(L):
        dbar = (dbar + p[:, :, l] * d[:, :, l]).astype(dtype)
    return arc, best, dbar, p


def fold_batch(phi, lengths, semiring="log", v=None, v_sub=None, dtype=np.float64):
    outs = [fold(phi[b], int(lengths[b]), semiring, None if v is None else v[b], None if v_sub is None else v_sub[b], dtype)
            for b in range(len(phi))]
    return tuple(np.stack([o[k] for o in outs]) for k in range(4))


def direction(phi, length, v=None, v_sub=None):
    "the effective label-level direction of one sentence, float64: v - v_sub, 0 where the label takes no part or the cell is never read"
    phi = np.asarray(phi, np.float64)
    N = phi.shape[0]
    d = np.zeros(phi.shape) + (0 if v is None else np.asarray(v, np.float64)) - (0 if v_sub is None else np.asarray(v_sub, np.float64))
    with np.errstate(invalid="ignore"):
        return np.where(takes_part(phi) & read_mask(N, length)[:, :, None], d, 0.0)


def expand(p, g1, g2=None, d=None, dbar=None, scale=1.0, mode=0):
    "out [N,N,L] from the fold's p; arc-level g1, g2, dbar [N,N]; d [N,N,L] the effective direction"
    if mode == 1 or g2 is None:
        return scale * p * g1[:, :, None]
    dd = 0 if d is None else d - dbar[:, :, None]
    return scale * p * (g1[:, :, None] + g2[:, :, None] * dd)


def draw_label(row, u):
    "the label the rule draws from one row under u"
    row = np.asarray(row, np.float64)
    with np.errstate(invalid="ignore"):
        t = np.where(row > FLOOR, row, FLOOR)
    return S.draw(t, float(u)) if len(t) > 1 else 0


def steer_label(row, target):
    "(u, p): the midpoint of the target label's interval of the rule, and the label's probability"
    row = np.asarray(row, np.float64)
    w = S.weights(np.where(row > FLOOR, row, FLOOR))
    cum = np.cumsum(w)
    return ((cum[target] - w[target]) + cum[target]) / (2.0 * cum[-1]), w[target] / cum[-1]


# ---- the labeled quantities of one sentence ---------------------------------------------------------------------------------------------
def log_quantities(phi, length, other=None, cost=None, dtype=np.float64):
    """dict of partition, marginals [N,N,L], entropy (+ grad), and -- with `other` -- kl, cross_entropy (+ grads w.r.t. both), with
    `cost` -- risk (+ grads w.r.t. phi and cost): the formulas of the module docstring on expect_restatement.dual."""
    N = np.asarray(phi).shape[0]
    out = {}
    arc, _, phibar, p = fold(phi, length, "log", v=phi, dtype=dtype)
    logZ, ev, mu, hv = E.dual(arc, length, v=phibar, dtype=dtype)
    dphi = direction(phi, length, v=phi).astype(dtype)
    out["partition"], out["arc"], out["p"], out["mu"] = logZ, arc, p, mu
    out["marginals"] = expand(p, mu)
    out["entropy"] = logZ - ev
    out["entropy_grad"] = expand(p, hv, mu, dphi, phibar, scale=-1.0)
    if cost is not None:
        _, _, cbar, _ = fold(phi, length, "log", v=cost, dtype=dtype)
        _, ev, mu, hv = E.dual(arc, length, v=cbar, dtype=dtype)
        dc = direction(phi, length, v=cost).astype(dtype)
        out["risk"] = ev
        out["risk_grad"] = expand(p, hv, mu, dc, cbar)
        out["risk_grad_cost"] = expand(p, mu, mode=1)
    if other is not None:
        arc_q, _, _, q = fold(other, length, "log", dtype=dtype)
        logZ_q, _, mu_q, _ = E.dual(arc_q, length, dtype=dtype)
        gq = expand(q, mu_q, mode=1)
        for name, sub in (("cross_entropy", None), ("kl", phi)):
            _, _, dbar, _ = fold(phi, length, "log", v=other, v_sub=sub, dtype=dtype)
            _, ev, mu_p, hv = E.dual(arc, length, v=dbar, dtype=dtype)
            d = direction(phi, length, v=other, v_sub=sub).astype(dtype)
            out[name] = logZ_q - ev - (logZ if sub is not None else 0)
            out[name + "_grad"] = expand(p, hv, mu_p, d, dbar, scale=-1.0)
            out[name + "_grad_other"] = gq - expand(p, mu_p, mode=1)
    return out


def max_quantities(phi, length):
    """dict of max, heads [N], labels [N], argmax [N,N,L] of one sentence (float64; the best tree of the max-folded arc scores) and
    `unique`: no second tree reaches the same score (label ties inside a row are the first-index rule's and do not count)"""
    phi = np.asarray(phi, np.float64)
    N, _, L = phi.shape
    arc, best, _, _ = fold(phi, length, "max")
    v, h, c = K.kbest_dp(arc, length, 2)
    heads = np.asarray(h[0], np.int64)
    labels = np.zeros(N, np.int64)
    parts = np.zeros((N, N, L))
    for ch in range(1, length + 1):
        labels[ch] = best[heads[ch], ch]
        parts[heads[ch], ch, labels[ch]] = 1
    return dict(max=v[0], heads=heads, labels=labels, argmax=parts, arc=arc, best=best, unique=bool(c < 2 or v[0] > v[1]))


def labeled_score(phi, heads, labels, length):
    phi = np.asarray(phi, np.float64)
    return float(sum(phi[int(heads[c]), c, int(labels[c])] for c in range(1, length + 1)))


# ---- brute force over every labeled tree (length <= 4) ----------------------------------------------------------------------------------
def brute(phi, length):
    "(logZ, marginals [n,n,L], H, best score, best heads, best labels) by enumeration: every tree x every labeling of its arcs"
    phi = np.asarray(phi, np.float64)
    L = phi.shape[-1]
    n = length + 1
    words = np.arange(1, n)
    scores, items = [], []
    for h in S.all_trees(length):
        for lab in itertools.product(range(L), repeat=length):
            scores.append(phi[h[1:], words, list(lab)].sum())
            items.append((h, lab))
    s = np.array(scores)
    logZ = np.logaddexp.reduce(s)
    pr = np.exp(s - logZ)
    marg = np.zeros((n, n, L))
    for w, (h, lab) in zip(pr, items):
        marg[h[1:], words, list(lab)] += w
    with np.errstate(divide="ignore", invalid="ignore"):
        H = -np.where(pr > 0, pr * (s - logZ), 0).sum()
    k = int(np.argmax(s))
    return logZ, marg, H, s[k], items[k][0], np.array((0,) + items[k][1])
