"""What the DMV1o tree-sampling tests share (test_dmv_sample_host.py, test_dmv_sample_gpu.py): the sampling rule of DMV1o.sample_heads
restated in float64 numpy, steering, and the score of a tree in terms of the tree alone.  A helper, not a test.

The rule (normative; the kernel, the host emulator and this file implement it).  Positions 0 ... len, root 0; potentials are root-merged,
dec [N,2,2,2] = [head, dir (0 LEFT, 1 RIGHT), valence (0 HASCHILD, 1 NOCHILD), decision (0 GO, 1 STOP)], attach [N,N,2] = [head, child,
valence].  A sample is a top-down expansion from CR(0,len).NC (dmv.py:65); a cell carries a valence v:
    draw kind 0  IL(hi -> lo).v   r in [lo,hi)   t_r = CR(lo,r).NC + CL(hi,r+1).HC       dmv.py:50-52
                 IR(lo -> hi).v   r in [lo,hi)   t_r = CR(lo,r).HC + CL(hi,r+1).NC       :54-56
    draw kind 1  CL(hi -> lo).v   r in [lo,hi)   t_r = CL(r,lo).NC + IL(hi -> r).v       :58-59
    draw kind 2  CR(lo -> hi).v   r in (lo,hi]   t_r = IR(lo -> r).v + CR(r,hi).NC       :61-62
with the two cells of t_r as children; a width-0 complete cell is a leaf.  The draw is sample_restatement.draw; the uniform of a cell is
read from a table u[kind, lo, hi] -- no valence, no direction: a derivation holds a span at most once.

The score of a tree in terms of the tree alone (tree_score): for head h and direction d, order the children from inner to outer; the
outermost child attaches with NC, every other child with HC (attach[h,c,v] + dec[h,d,v,GO] each); the STOP of (h, d) is HC if there is
a child in that direction, else NC.  The root has a right side only.
"""
import numpy as np

from sample_restatement import _depth, draw, weights  # noqa: F401  (draw: re-exported for the tests)
from sample_restatement import all_trees, floor_pick, is_tree, left_chain, pad_heads, random_tree, right_chain  # noqa: F401

NEG = -np.inf
HC, NC, LEFT, RIGHT, GO, STOP = 0, 1, 0, 1, 0, 1


def merge64(dec, attach, root, one=0.0, zero=-1e12):
    "DMV1o.merge (distributions.py:253-265) for one batch [B,L,...] -> root-merged [B,L+1,...], dtype kept"
    B, L = dec.shape[:2]
    a = np.full((B, L + 1, L + 1, 2), zero, dec.dtype)
    d = np.full((B, L + 1, 2, 2, 2), zero, dec.dtype)
    a[:, 0, 1:, NC] = root
    a[:, 1:, 1:, :] = attach
    d[:, 0, RIGHT] = one
    d[:, 1:] = dec
    return d, a


def inside64(dec, attach, length):
    """The inside charts of dmv.py:19-66 in float64, natural log, vectorised per width: (I, CL, CR), each [n,n,2]: I[h,c,v] the incomplete
    span of arc h -> c, CL[h,l,v] / CR[h,r,v] the complete spans of head h reaching left to l / right to r, single-root masking applied.
    Only positions 0 ... length are used.  logZ = CR[0, length, NC]."""
    n = length + 1
    d = np.asarray(dec, np.float64)[:n]
    a = np.asarray(attach, np.float64)[:n, :n]
    I = np.full((n, n, 2), NEG)
    CL = np.full((n, n, 2), NEG)
    CR = np.full((n, n, 2), NEG)
    k = np.arange(n)
    CL[k, k] = d[:, LEFT, :, STOP]
    CR[k, k] = d[:, RIGHT, :, STOP]
    lse = np.logaddexp.reduce
    with np.errstate(invalid="ignore"):
        for w in range(1, n):
            i = np.arange(n - w)[:, None]
            j = i + w
            r = i + np.arange(w)[None, :]                                     # i <= r < j
            i0, j0 = i[:, 0], j[:, 0]
            sl = lse(CR[i, r, NC] + CL[j, r + 1, HC], axis=1)
            sr = lse(CR[i, r, HC] + CL[j, r + 1, NC], axis=1)
            I[j0, i0] = sl[:, None] + a[j0, i0] + d[j0, LEFT, :, GO]
            I[i0, j0] = sr[:, None] + a[i0, j0] + d[i0, RIGHT, :, GO]
            CL[j0, i0] = lse(CL[r, i, NC][:, :, None] + I[j, r], axis=1)      # CL(r,i).NC + IL(j -> r).v
            CR[i0, j0] = lse(I[i, r + 1] + CR[r + 1, j, NC][:, :, None], axis=1)   # IR(i -> r).v + CR(r,j).NC, i < r <= j
            if w != length:
                CR[0, w] = NEG                                                # dmv.py:63
    return I, CL, CR


def log_partition(charts, length):
    return float(charts[2][0, length, NC])


def terms(charts, kind, right, lo, hi, v):
    """(t, r): the terms of the cell of draw kind `kind` over [lo,hi] with valence v (kind 0: `right` = the arc lo -> hi) and their
    split points, in increasing r."""
    I, CL, CR = charts
    if kind == 2:
        r = np.arange(lo + 1, hi + 1)
        return I[lo, r, v] + CR[r, hi, NC], r
    r = np.arange(lo, hi)
    if kind == 1:
        return CL[r, lo, NC] + I[hi, r, v], r
    return (CR[lo, r, HC] + CL[hi, r + 1, NC], r) if right else (CR[lo, r, NC] + CL[hi, r + 1, HC], r)


def _walk(charts, length, choose):
    """Top-down expansion; choose(kind, lo, hi, right, t, r) -> index into r.  Cells: (wk, lo, hi, v), wk 0 = IL(hi -> lo), 1 = CL,
    2 = CR, 3 = IR(lo -> hi)."""
    heads = np.zeros(length + 1, np.int64)
    todo = [(2, 0, length, NC)]
    while todo:
        wk, lo, hi, v = todo.pop()
        if lo == hi:
            continue
        kind = 0 if wk == 3 else wk
        if kind == 0:
            h, c = (hi, lo) if wk == 0 else (lo, hi)
            heads[c] = h
        t, r = terms(charts, kind, wk == 3, lo, hi, v)
        s = int(r[choose(kind, lo, hi, wk == 3, t, r)])
        if wk == 0:
            todo += [(2, lo, s, NC), (1, s + 1, hi, HC)]
        elif wk == 3:
            todo += [(2, lo, s, HC), (1, s + 1, hi, NC)]
        elif wk == 1:
            todo += [(1, lo, s, NC), (0, s, hi, v)]
        else:
            todo += [(3, lo, s, v), (2, s, hi, NC)]
    return heads


def walk(dec, attach, length, u, charts=None):
    "The tree the rule draws from root-merged potentials under the table u [3,N,N] (float64 arithmetic)."
    charts = charts or inside64(dec, attach, length)
    return _walk(charts, length, lambda kind, lo, hi, right, t, r: draw(t, float(u[kind, lo, hi])))


def steer(dec, attach, length, target=None, pick=None, N=None, charts=None):
    """(u [3,N,N] float32, pmin, heads): the table that makes the rule return one chosen tree, NaN where the walk does not come, the
    smallest conditional probability steered through, and the tree -- sample_restatement.steer with valences.  The tree is either
    `target` or grown by pick(kind, lo, hi, r, p) -> index of the split to take."""
    N = N or np.asarray(attach).shape[-2]
    charts = charts or inside64(dec, attach, length)
    u = np.full((3, N, N), np.nan, np.float32)
    pmin = [1.0]
    if target is not None:
        kids = [[c for c in range(1, length + 1) if target[c] == h] for h in range(length + 1)]
        lext, rext = list(range(length + 1)), list(range(length + 1))   # leftmost / rightmost descendant
        for h in sorted(range(1, length + 1), key=lambda c: -_depth(target, c)):   # children before their heads
            g = target[h]
            lext[g], rext[g] = min(lext[g], lext[h]), max(rext[g], rext[h])

    def choose(kind, lo, hi, right, t, r):
        w = weights(t)
        cum = np.cumsum(w)
        if target is None:
            k = int(pick(kind, lo, hi, r, w / cum[-1]))
        else:
            if kind == 0:
                s = lext[hi] - 1 if right else rext[lo]
            elif kind == 1:
                s = min(c for c in kids[hi] if lo <= c < hi)
            else:
                s = max(c for c in kids[lo] if lo < c <= hi)
            k = int(np.nonzero(r == s)[0][0])
        u[kind, lo, hi] = ((cum[k] - w[k]) + cum[k]) / (2.0 * cum[-1])
        pmin[0] = min(pmin[0], w[k] / cum[-1])
        return k

    got = _walk(charts, length, choose)
    if target is not None:
        assert np.array_equal(got, np.asarray(target)[:length + 1]), "steer: the target is not a projective single-root tree"
    return u, pmin[0], got


def random_unmerged(rng, B, L, scale=0.25):
    "(dec [B,L,2,2,2], attach [B,L,L,2], root [B,L]) float32: scale x randn, what DMV1o.merge takes"
    return ((scale * rng.standard_normal((B, L, 2, 2, 2))).astype(np.float32), (scale * rng.standard_normal((B, L, L, 2))).astype(np.float32),
            (scale * rng.standard_normal((B, L))).astype(np.float32))


def steered_rows(dec, attach, length, count, rng, floor, charts=None):
    """`count` steer() results for one sentence, aimed in turn at the left chain, the right chain, a tree of the root-child sweep (over the
    positions whose root split reaches `floor`; the rest of the tree grows through splits of probability >= 2 floor) and a floor-picked
    random tree -- the targets of the DepTree sampler's tests."""
    charts = charts or inside64(dec, attach, length)
    t, r = terms(charts, 2, True, 0, length, NC)
    root_ok = r[weights(t) / weights(t).sum() >= floor]
    assert root_ok.size >= 1
    rows = []
    for s in range(count):
        if s % 4 == 0:
            row = steer(dec, attach, length, left_chain(length), charts=charts)
        elif s % 4 == 1:
            row = steer(dec, attach, length, right_chain(length), charts=charts)
        elif s % 4 == 2:
            p = int(root_ok[(s // 4) * max(1, root_ok.size // 2) % root_ok.size])
            row = steer(dec, attach, length, pick=floor_pick(rng, 2 * floor, root_child=p, length=length), charts=charts)
            assert row[2][p] == 0
        else:
            row = steer(dec, attach, length, pick=floor_pick(rng, 2 * floor), charts=charts)
        rows.append(row)
    return rows


def tree_score(dec, attach, heads, length):
    """(score, sum of |terms|, dec counts [N,2,2,2], attach counts [N,N,2]) of the tree `heads` under root-merged potentials, float64, from
    the tree alone (module docstring)."""
    d = np.asarray(dec, np.float64)
    a = np.asarray(attach, np.float64)
    cd, ca = np.zeros(d.shape), np.zeros(a.shape)
    heads = np.asarray(heads)
    for h in range(length + 1):
        for direction in ((RIGHT,) if h == 0 else (LEFT, RIGHT)):
            if direction == LEFT:
                kids = [c for c in range(h - 1, 0, -1) if heads[c] == h]          # inner to outer
            else:
                kids = [c for c in range(h + 1, length + 1) if heads[c] == h]
            for k, c in enumerate(kids):
                v = NC if k == len(kids) - 1 else HC
                ca[h, c, v] += 1
                cd[h, direction, v, GO] += 1
            cd[h, direction, HC if kids else NC, STOP] += 1
    md, ma = cd > 0, ca > 0
    terms_ = np.concatenate([(cd[md] * d[md]).ravel(), (ca[ma] * a[ma]).ravel()])
    return float(terms_.sum()), float(np.abs(terms_).sum()), cd, ca
