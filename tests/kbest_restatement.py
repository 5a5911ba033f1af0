"""K-best projective single-root trees, restated in numpy float64 for the tests of vlg_deptree_kbest (tests/test_kbest_host.py,
tests/test_kbest_gpu.py).  TEST INFRASTRUCTURE ONLY.

  kbest_dp     the k-best Eisner DP (cell rule of vlgae_amd/csrc/vlg_dp_kbest.h) under the total order (value descending, then
               split r, rank p, rank q ascending), by default WITHOUT the kernel's per-split pruning: every (p, q) pair is a candidate
  brute_force  every projective single-root tree of a sentence of length <= 6, scored and sorted
  tree_score, is_tree

On potentials whose partial sums are exactly representable in float32 the float64 values here are the kernel's, bit for bit.
"""
import itertools

import numpy as np

NEGINF = -1e12
POT_FLOOR = -1e30   # VLG_POT_FLOOR: potentials are clamped to it as they enter (NaN too)


def clamp(arc):
    a = np.asarray(arc, np.float64)
    return np.where(a > POT_FLOOR, a, POT_FLOOR)


def _pairs(K, prune):
    """(p, q) pairs in ascending (p, q) order: all K x K, or only those with (p+1)(q+1) <= K (the kernel's pruning bound)"""
    pq = [(p, q) for p in range(K) for q in range(K) if not prune or (p + 1) * (q + 1) <= K]
    return np.array([p for p, _ in pq]), np.array([q for _, q in pq])


def _merge(A, B, K, pairs):
    """top K of A[r,p] + B[r,q] over (r, p, q), ties by ascending (r, p, q): values [K] and pointers [K,3]"""
    pp, qq = pairs
    flat = (A[:, pp] + B[:, qq]).reshape(-1)   # flat index order == (r, p, q) order
    idx = np.arange(flat.size)
    if flat.size > 8 * K:   # everything at or above the K-th largest value (all of its ties included), then the exact order among those
        idx = np.flatnonzero(flat >= np.partition(flat, flat.size - K)[flat.size - K])
    order = idx[np.argsort(-flat[idx], kind="stable")][:K]   # stable: the smaller (r, p, q) first among equals
    r, j = np.divmod(order, pp.size)
    return flat[order], np.stack([r, pp[j], qq[j]], -1)


def kbest_dp(arc, length, K, prune=False):
    """arc [N,N] (head, child), root at 0.  Returns (values [K] float64, heads [K,N] int64, count): rank k exists iff
    values[k] > 0.5 * NEGINF; the others have value NEGINF and heads 0.  prune: only for speed at large N (the unpruned form is the
    independent check of the bound at every smaller size)."""
    arc = clamp(arc)
    N, n = arc.shape[0], length + 1
    neg = -np.inf
    pairs = _pairs(K, prune)
    CL, CR, IL, IR = (np.full((n, n, K), neg) for _ in range(4))   # CL[hi,lo], CR[lo,hi], IL[hi,lo] (hi -> lo), IR[lo,hi]
    bT, bL, bR = (np.zeros((n, n, K, 3), np.int64) for _ in range(3))   # T(lo,hi) at [lo,hi]; CL at [hi,lo]; CR at [lo,hi]
    for h in range(n):
        CL[h, h, 0] = CR[h, h, 0] = 0.0
    for w in range(1, n):
        for lo in range(n - w):
            hi, r = lo + w, np.arange(w)
            t, bT[lo, hi] = _merge(CR[lo, lo + r], CL[hi, lo + r + 1], K, pairs)
            IL[hi, lo] = t + arc[hi, lo]
            IR[lo, hi] = t + arc[lo, hi]
            CL[hi, lo], bL[hi, lo] = _merge(CL[lo + r, lo], IL[hi, lo + r], K, pairs)
            v, bR[lo, hi] = _merge(IR[lo, lo + 1 + r], CR[lo + 1 + r, hi], K, pairs)
            CR[lo, hi] = v if (lo != 0 or w == length) else neg   # single root
    values = CR[0, length].copy()
    exists = values > 0.5 * NEGINF
    heads = np.zeros((K, N), np.int64)
    for k in np.flatnonzero(exists):
        stack = [(2, 0, length, int(k))]
        while stack:
            kind, lo, hi, rk = stack.pop()
            if lo == hi:
                assert rk == 0
                continue
            if kind in (0, 3):
                h, c = (hi, lo) if kind == 0 else (lo, hi)
                heads[k, c] = h
                r, p, q = bT[lo, hi, rk]
                stack += [(2, lo, lo + r, int(p)), (1, lo + r + 1, hi, int(q))]
            elif kind == 1:
                r, p, q = bL[hi, lo, rk]
                stack += [(1, lo, lo + r, int(p)), (0, lo + r, hi, int(q))]
            else:
                r, p, q = bR[lo, hi, rk]
                stack += [(3, lo, lo + 1 + r, int(p)), (2, lo + 1 + r, hi, int(q))]
    values[~exists] = NEGINF
    return values, heads, int(exists.sum())


def is_tree(heads, length):
    """heads [N]: a projective tree over words 1 ... length with exactly one child of the root 0, zeros elsewhere"""
    heads = [int(h) for h in heads]
    if heads[0] != 0 or any(h != 0 for h in heads[length + 1:]):
        return False
    words = range(1, length + 1)
    if any(not (0 <= heads[c] <= length) or heads[c] == c for c in words):
        return False
    if sum(heads[c] == 0 for c in words) != 1:
        return False
    for c in words:   # every word reaches the root
        seen, x = 0, c
        while x != 0:
            x, seen = heads[x], seen + 1
            if seen > length:
                return False
    for c in words:   # projective: no two arcs cross (the root's arc included)
        a, b = sorted((heads[c], c))
        for d in words:
            e, f = sorted((heads[d], d))
            if a < e < b < f or e < a < f < b:
                return False
    return True


def tree_score(arc, heads, length):
    arc = clamp(arc)
    return float(sum(arc[int(heads[c]), c] for c in range(1, length + 1)))


def brute_force(arc, length):
    """(scores descending [T], heads [T,N]) over every projective single-root tree, length <= 6"""
    assert 1 <= length <= 6
    N = np.asarray(arc).shape[0]
    trees = []
    for hs in itertools.product(range(length + 1), repeat=length):
        heads = np.zeros(N, np.int64)
        heads[1:length + 1] = hs
        if is_tree(heads, length):
            trees.append((tree_score(arc, heads, length), heads))
    trees.sort(key=lambda t: -t[0])
    return np.array([t[0] for t in trees]), np.stack([t[1] for t in trees])


TREE_COUNTS = {1: 1, 2: 2, 3: 7, 4: 30, 5: 143, 6: 728}


def potentials(rng, shape, bf16=False):
    """The tests' potentials: on the 2^-12 grid, clipped to +-4, so that every partial sum of a tree of up to 254 arcs is an exact
    float32 (at most 22 bits).  bf16: randn rounded to bfloat16 first, so the values are bf16-representable as well."""
    x = np.clip(rng.standard_normal(shape), -4, 4)
    if bf16:
        u = x.astype(np.float32).view(np.uint32)
        u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16).astype(np.uint32)
        x = u.view(np.float32).astype(np.float64)
    x = np.clip(np.round(x * 4096) / 4096, -4, 4)
    if bf16:
        f = x.astype(np.float32)
        assert np.array_equal(f.view(np.uint32) & 0xFFFF, np.zeros_like(f, np.uint32)), "not bf16-representable"
    return x


def tied_share(ref):
    """Share of the existing (sentence, rank) pairs, over the first K' - 1 ranks of the reference values ref[b] = (values [K'], ...),
    whose value is tied with a neighbour: those are the pairs check_kbest cannot compare heads on.  A property of the potentials
    alone -- the same for every K served from this reference."""
    tied = total = 0
    for v, _, c in ref:
        for k in range(min(c, len(v) - 1)):
            total += 1
            tied += not ((k == 0 or v[k - 1] > v[k]) and v[k] > v[k + 1])
    return tied / max(total, 1)


def check_kbest(arc, lengths, K, heads, scores, count, ref, tie_cap=0.25):
    """The checks every k-best result gets.  arc [B,N,N] float64 (exactly representable recipe), heads [K,B,N], scores [K,B] float32,
    count [B]; ref[b] = (values, heads, count) of kbest_dp at some K' > K.  Scores bit for bit; heads equal where the rank's value is
    strictly separated from both neighbours among the K + 1 reference values; every returned tree valid, distinct, and its tree_score
    equal to the reported score; absent ranks NEGINF / 0.  Returns (compared, tied) rank counts; tie_cap (None: no cap) bounds
    tied_share(ref), the share of (sentence, rank) pairs of these potentials that are left out as tied."""
    compared = tied = 0
    for b, L in enumerate(lengths):
        v, h, c = ref[b]
        assert len(v) > K
        n = min(c, K)
        assert count[b] == n, (b, count[b], n)
        want = v[:K].astype(np.float32)
        assert np.array_equal(scores[:, b].view(np.uint32), want.view(np.uint32)), (b, scores[:, b], want)
        assert np.all(scores[n:, b] == np.float32(NEGINF)) and not heads[n:, b].any()
        assert np.all(np.diff(scores[:, b]) <= 0)
        for k in range(n):
            assert is_tree(heads[k, b], L), (b, k, heads[k, b])
            assert np.float32(tree_score(arc[b], heads[k, b], L)) == scores[k, b], (b, k)
            if (k == 0 or v[k - 1] > v[k]) and v[k] > v[k + 1]:
                assert np.array_equal(heads[k, b], h[k]), (b, k)
                compared += 1
            else:
                tied += 1
        assert len({tuple(x) for x in heads[:n, b]}) == n, b
    if tie_cap is not None:
        assert tied_share(ref) <= tie_cap, (tied_share(ref), compared, tied)
    return compared, tied
