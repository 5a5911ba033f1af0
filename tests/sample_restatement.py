"""What the tree-sampling tests share (test_sample_host.py, test_sample_gpu.py): the sampling rule of DependencyCRF.sample_heads restated in
float64 numpy, steering, and the trees the tests aim at.  A helper, not a test.

The rule (normative; the kernel, the host emulator and this file implement it).  Positions 0 ... len, root 0.  A sample is a top-down
expansion from CR(0,len) (deptree.py:74-75) over three kinds of non-trivial cell, keyed (kind, lo, hi), lo < hi:
    kind 0  incomplete span [lo,hi], either direction   r in [lo,hi)   t_r = CR(lo,r) + CL(hi,r+1)    deptree.py:53-62
    kind 1  CL(hi -> lo)                                r in [lo,hi)   t_r = CL(r,lo) + I(hi -> r)     :64-66
    kind 2  CR(lo -> hi)                                r in (lo,hi]   t_r = I(lo -> r) + CR(r,hi)     :67-69
with children: two complete cells (kind 0), one complete and one incomplete cell (kinds 1, 2).  A draw: w_r = exp(t_r - max t),
cum = running sum in increasing r, total = last cum; taken is the smallest r with cum_r > u total, else the largest r with w_r > 0.
u is the cell's uniform, read from a table u[kind, lo, hi].

Steering: for a target tree the walk is run in float64 and, at every cell it visits, the table gets the MIDPOINT of the target split's
interval [cum_(r-1), cum_r) / total; unvisited entries stay NaN.  A float32 implementation whose cum / total is off by less than half the
interval's width -- the smallest conditional probability steered through, which `steer` returns -- lands on the same split.
"""
import itertools

import numpy as np

NEG = -np.inf


def inside64(arc, length):
    """The inside charts of deptree.py:48-72 in float64, natural log: I[h, c] (incomplete, arc h -> c), C[h, e] (complete, head h
    reaching to e), single-root masking applied.  Only positions 0 ... length are used."""
    n = length + 1
    a = np.asarray(arc, np.float64)[:n, :n]
    I = np.full((n, n), NEG)
    C = np.full((n, n), NEG)
    C[np.arange(n), np.arange(n)] = 0.0
    with np.errstate(invalid="ignore"):
        for w in range(1, n):
            i = np.arange(n - w)[:, None]
            j = i + w
            r = i + np.arange(w)[None, :]                               # i <= r < j
            t = np.logaddexp.reduce(C[i, r] + C[j, r + 1], axis=1)      # C(i->r) + C(j->r+1)
            i0, j0 = i[:, 0], j[:, 0]
            I[j0, i0] = t + a[j0, i0]
            I[i0, j0] = t + a[i0, j0]
            C[j0, i0] = np.logaddexp.reduce(C[r, i] + I[j, r], axis=1)          # C(r->i) + I(j->r), i <= r < j
            C[i0, j0] = np.logaddexp.reduce(I[i, r + 1] + C[r + 1, j], axis=1)  # I(i->r) + C(r->j), i < r <= j
            if w != length:
                C[0, w] = NEG                                           # deptree.py:71-72
    return I, C


def terms(I, C, kind, lo, hi):
    """(t, r): the terms of cell (kind, lo, hi) and their split points, in increasing r."""
    if kind == 2:
        r = np.arange(lo + 1, hi + 1)
        return I[lo, r] + C[r, hi], r
    r = np.arange(lo, hi)
    return (C[lo, r] + C[hi, r + 1], r) if kind == 0 else (C[r, lo] + I[hi, r], r)


def weights(t):
    with np.errstate(invalid="ignore"):
        w = np.exp(t - np.max(t))
    return np.where(np.isnan(w), 0.0, w)


def draw(t, u):
    """Index into t of the split the rule takes under uniform u."""
    w = weights(t)
    cum = np.cumsum(w)
    hit = np.nonzero(cum > u * cum[-1])[0]
    return int(hit[0]) if hit.size else int(np.nonzero(w > 0)[0][-1])


def _walk(I, C, length, choose):
    """Top-down expansion; choose(kind, lo, hi, head_is_lo, t, r) -> index into r.  Cells: (wk, lo, hi), wk 0 = I(hi -> lo), 1 = CL,
    2 = CR, 3 = I(lo -> hi)."""
    heads = np.zeros(length + 1, np.int64)
    todo = [(2, 0, length)]
    while todo:
        wk, lo, hi = todo.pop()
        if lo == hi:
            continue
        kind = 0 if wk == 3 else wk
        if kind == 0:
            h, c = (hi, lo) if wk == 0 else (lo, hi)
            heads[c] = h
        t, r = terms(I, C, kind, lo, hi)
        s = int(r[choose(kind, lo, hi, wk == 3, t, r)])
        if kind == 0:
            todo += [(2, lo, s), (1, s + 1, hi)]
        elif kind == 1:
            todo += [(1, lo, s), (0, s, hi)]
        else:
            todo += [(3, lo, s), (2, s, hi)]
    return heads


def walk(arc, length, u):
    """The tree the rule draws from arc scores [N,N] under the table u [3,N,N] (float64 arithmetic)."""
    I, C = inside64(arc, length)
    return _walk(I, C, length, lambda kind, lo, hi, right, t, r: draw(t, float(u[kind, lo, hi])))


def steer(arc, length, target=None, pick=None, N=None, charts=None):
    """(u [3,N,N] float32, pmin, heads): the table that makes the rule return one chosen tree, NaN where the walk does not come, the
    smallest conditional probability steered through, and the tree.  The tree is either `target` (heads over positions 0 ... length of a
    projective single-root tree) or grown by pick(kind, lo, hi, r, p) -> index of the split to take, p = the splits' conditional
    probabilities (float64).  charts: inside64(arc, length), if the caller has it."""
    N = N or np.asarray(arc).shape[-1]
    I, C = charts or inside64(arc, length)
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
            if kind == 0:     # head hi: CR(lo, .) is all of lo's right side; head lo: CL(hi, .) is all of hi's left side
                s = lext[hi] - 1 if right else rext[lo]
            elif kind == 1:   # the leftmost child of hi inside the span
                s = min(c for c in kids[hi] if lo <= c < hi)
            else:             # the rightmost child of lo inside the span
                s = max(c for c in kids[lo] if lo < c <= hi)
            k = int(np.nonzero(r == s)[0][0])
        u[kind, lo, hi] = ((cum[k] - w[k]) + cum[k]) / (2.0 * cum[-1])
        pmin[0] = min(pmin[0], w[k] / cum[-1])
        return k

    got = _walk(I, C, length, choose)
    if target is not None:
        assert np.array_equal(got, np.asarray(target)[:length + 1]), "steer: the target is not a projective single-root tree"
    return u, pmin[0], got


def _depth(heads, c):
    d = 0
    while c != 0:
        c, d = heads[c], d + 1
    return d


def floor_pick(rng, floor, root_child=None, length=None):
    """pick() for `steer`: uniformly among the splits whose conditional probability is at least `floor` (the likeliest split if none
    is); root_child: the root's child is that position (the split of CR(0,length)) whatever its probability."""
    def pick(kind, lo, hi, r, p):
        if root_child is not None and kind == 2 and lo == 0 and hi == length:
            return int(np.nonzero(r == root_child)[0][0])
        ok = np.nonzero(p >= floor)[0]
        return int(rng.choice(ok)) if ok.size else int(np.argmax(p))
    return pick


# ---- trees --------------------------------------------------------------------------------------------------------------------------------
def left_chain(length):
    "root -> last word, every other word headed by its right neighbour"
    h = np.zeros(length + 1, np.int64)
    h[1:length] = np.arange(2, length + 1)
    return h


def right_chain(length):
    "root -> word 1, every other word headed by its left neighbour"
    h = np.zeros(length + 1, np.int64)
    h[1:] = np.arange(0, length)
    return h


def root_child_at(length, p):
    "root -> word p; the words left of p hang off p in a chain to the left, those right of it in a chain to the right"
    h = np.zeros(length + 1, np.int64)
    for c in range(1, p):
        h[c] = c + 1
    for c in range(p + 1, length + 1):
        h[c] = c - 1
    return h


def random_tree(length, rng):
    "a random projective single-root tree (not uniform over trees; every tree has positive probability)"
    h = np.zeros(length + 1, np.int64)

    def fill(head, lo, hi):   # the words lo ... hi (all on one side of head) become descendants of head
        while lo <= hi:
            end = int(rng.integers(lo, hi + 1))          # one child's subtree covers lo ... end
            c = int(rng.integers(lo, end + 1))
            h[c] = head
            fill(c, lo, c - 1)
            fill(c, c + 1, end)
            lo = end + 1

    p = int(rng.integers(1, length + 1))
    h[p] = 0
    fill(p, 1, p - 1)
    fill(p, p + 1, length)
    return h


def is_tree(heads, length):
    """heads[0 ... length] is a projective single-root spanning tree of the sentence (and 0 elsewhere)."""
    heads = np.asarray(heads)
    if heads[0] != 0 or np.any(heads[length + 1:] != 0):
        return False
    h = heads[:length + 1]
    if np.any(h[1:] < 0) or np.any(h[1:] > length) or np.any(h[1:] == np.arange(1, length + 1)) or np.sum(h[1:] == 0) != 1:
        return False
    for c in range(1, length + 1):   # every word reaches the root
        k, steps = c, 0
        while k != 0:
            k, steps = h[k], steps + 1
            if steps > length:
                return False
    for c in range(1, length + 1):   # no crossing arcs; nothing spans the root's arc
        a, b = min(c, h[c]), max(c, h[c])
        for d in range(1, length + 1):
            x, y = min(d, h[d]), max(d, h[d])
            if a < x < b < y or x < a < y < b:
                return False
    return True


def all_trees(length):
    "every projective single-root tree over `length` words, as head vectors (1, 2, 7, 30, 143, ... of them)"
    out = []
    for hs in itertools.product(range(length + 1), repeat=length):
        h = np.array((0,) + hs, np.int64)
        if is_tree(h, length):
            out.append(h)
    return out


def tree_score(arc, heads, length):
    "sum of the arc scores on the tree, float64; also the sum of their magnitudes"
    a = np.asarray(arc, np.float64)
    c = np.arange(1, length + 1)
    v = a[np.asarray(heads)[c], c]
    return float(v.sum()), float(np.abs(v).sum())


def pad_heads(h, N):
    out = np.zeros(N, np.int64)
    out[:len(h)] = h
    return out
