"""K-best projective single-root trees of the valence DMV, restated in numpy float64 for the tests of vlg_dmv1o_kbest and
vlg_dmv1o_tree_counts (tests/test_dmv_kbest_host.py, tests/test_dmv_kbest_gpu.py).  TEST INFRASTRUCTURE ONLY.

  dmv_kbest_dp   the k-best DMV DP (cell rule of vlgae_amd/csrc/vlg_dmv_kbest.h) under the total order (value descending, then split r,
                 rank p, rank q ascending), by default WITHOUT the kernel's per-split pruning
  brute_force    every projective single-root tree of a sentence of <= 6 words, scored by dmv_sample_restatement.tree_score
  tree_counts    sum_t weight[t] * (derivation counts of tree t): vlg_dmv1o_tree_counts restated, lane by lane
  check_dmv_kbest, potentials, tied_share

Potentials are root-merged: dec [N,2,2,2] = [head, dir (0 LEFT, 1 RIGHT), valence (0 HASCHILD, 1 NOCHILD), decision (0 GO, 1 STOP)],
attach [N,N,2] = [head, child, valence].  On potentials whose partial sums are exactly representable in float32 the float64 values
here are the kernel's, bit for bit.
"""
import numpy as np

from dmv_sample_restatement import GO, HC, LEFT, NC, RIGHT, STOP, tree_score
from kbest_restatement import NEGINF, TREE_COUNTS, _merge, _pairs, clamp, is_tree, tied_share  # noqa: F401  (re-exported for the tests)
from sample_restatement import all_trees  # noqa: F401


def dmv_kbest_dp(dec, attach, length, K, prune=False):
    """Returns (values [K] float64, heads [K,N] int64, count): rank k exists iff values[k] > 0.5 * NEGINF; the others have value
    NEGINF and heads 0.  prune: only for speed at large N (the unpruned form is the independent check of the bound)."""
    d, a = clamp(dec), clamp(attach)
    N, n = a.shape[0], length + 1
    neg = -np.inf
    pairs = _pairs(K, prune)
    CL, CR = (np.full((n, n, 2, K), neg) for _ in range(2))   # CL[hi,lo,v], CR[lo,hi,v]
    TL, TR = (np.full((n, n, K), neg) for _ in range(2))      # TL[hi,lo], TR[lo,hi]
    bTL, bTR = (np.zeros((n, n, K, 3), np.int64) for _ in range(2))
    bL, bR = (np.zeros((n, n, 2, K, 3), np.int64) for _ in range(2))
    A = a + np.where(np.arange(N)[None, :, None] < np.arange(N)[:, None, None], d[:, LEFT, :, GO][:, None, :], d[:, RIGHT, :, GO][:, None, :])
    for h in range(n):
        CL[h, h, :, 0] = d[h, LEFT, :, STOP]
        CR[h, h, :, 0] = d[h, RIGHT, :, STOP]
    for w in range(1, n):
        for lo in range(n - w):
            hi, r = lo + w, np.arange(w)
            TL[hi, lo], bTL[hi, lo] = _merge(CR[lo, lo + r, NC], CL[hi, lo + r + 1, HC], K, pairs)
            TR[lo, hi], bTR[lo, hi] = _merge(CR[lo, lo + r, HC], CL[hi, lo + r + 1, NC], K, pairs)
            for v in (HC, NC):
                CL[hi, lo, v], bL[hi, lo, v] = _merge(CL[lo + r, lo, NC], TL[hi, lo + r] + A[hi, lo + r, v][:, None], K, pairs)
                val, bR[lo, hi, v] = _merge(TR[lo, lo + 1 + r] + A[lo, lo + 1 + r, v][:, None], CR[lo + 1 + r, hi, NC], K, pairs)
                CR[lo, hi, v] = val if (lo != 0 or w == length) else neg   # single root, dmv.py:63
    values = CR[0, length, NC].copy()
    exists = values > 0.5 * NEGINF
    heads = np.zeros((K, N), np.int64)
    for k in np.flatnonzero(exists):
        stack = [(2, 0, length, int(k), NC)]
        while stack:
            kind, lo, hi, rk, v = stack.pop()
            if lo == hi:
                assert rk == 0
                continue
            if kind == 0:
                heads[k, lo] = hi
                r, p, q = bTL[hi, lo, rk]
                stack += [(2, lo, lo + r, int(p), NC), (1, lo + r + 1, hi, int(q), HC)]
            elif kind == 3:
                heads[k, hi] = lo
                r, p, q = bTR[lo, hi, rk]
                stack += [(2, lo, lo + r, int(p), HC), (1, lo + r + 1, hi, int(q), NC)]
            elif kind == 1:
                r, p, q = bL[hi, lo, v, rk]
                stack += [(1, lo, lo + r, int(p), NC), (0, lo + r, hi, int(q), v)]
            else:
                r, p, q = bR[lo, hi, v, rk]
                stack += [(3, lo, lo + 1 + r, int(p), v), (2, lo + 1 + r, hi, int(q), NC)]
    values[~exists] = NEGINF
    return values, heads, int(exists.sum())


def score(dec, attach, heads, length):
    "tree_score on the clamped potentials: (score, sum of |terms|)"
    s, sabs, _, _ = tree_score(clamp(dec), clamp(attach), heads, length)
    return s, sabs


def brute_force(dec, attach, length):
    """(scores descending [T], heads [T,N]) over every projective single-root tree, length <= 6"""
    assert 1 <= length <= 6
    N = np.asarray(attach).shape[0]
    trees = []
    for t in all_trees(length):
        heads = np.zeros(N, np.int64)
        heads[:length + 1] = np.asarray(t)[:length + 1]
        assert is_tree(heads, length)
        trees.append((score(dec, attach, heads, length)[0], heads))
    trees.sort(key=lambda t: -t[0])
    return np.array([t[0] for t in trees]), np.stack([t[1] for t in trees])


def tree_counts(heads, lengths, count, weight, N):
    """vlg_dmv1o_tree_counts restated: heads [T,B,N]; count [B] or None; weight [T,B] or None -> (cnt_dec [B,N,2,2,2], cnt_attach
    [B,N,N,2]) float32, accumulated in float32 in the order of t.  Entries outside 0 ... len, or naming the word itself, attach nowhere."""
    T, B = heads.shape[:2]
    cd, ca = np.zeros((B, N, 2, 2, 2), np.float32), np.zeros((B, N, N, 2), np.float32)
    for b in range(B):
        L = int(lengths[b])
        if not 1 <= L <= N - 1:
            continue
        for t in range(T if count is None else min(int(count[b]), T)):
            wt = np.float32(1.0 if weight is None else weight[t, b])
            hs = [int(h) if (1 <= c <= L and 0 <= h <= L and h != c) else -1 for c, h in enumerate(heads[t, b])]
            for h in range(L + 1):
                for direction in ((RIGHT,) if h == 0 else (LEFT, RIGHT)):
                    kids = [c for c in (range(h - 1, 0, -1) if direction == LEFT else range(h + 1, L + 1)) if hs[c] == h]
                    for i, c in enumerate(kids):
                        ca[b, h, c, NC if i == len(kids) - 1 else HC] += wt
                    if kids:
                        cd[b, h, direction, NC, GO] += wt
                        if len(kids) > 1:
                            cd[b, h, direction, HC, GO] += wt * np.float32(len(kids) - 1)
                    cd[b, h, direction, HC if kids else NC, STOP] += wt
    return cd, ca


def _grid(x, bf16):
    if bf16:
        u = x.astype(np.float32).view(np.uint32)
        u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16).astype(np.uint32)
        x = u.view(np.float32).astype(np.float64)
    x = np.clip(np.round(x * 4096) / 4096, -2, 2)
    if bf16:
        f = x.astype(np.float32)
        assert not (f.view(np.uint32) & 0xFFFF).any(), "not bf16-representable"
    return x


def potentials(rng, B, N, bf16=False):
    """(dec [B,N,2,2,2], attach [B,N,N,2]) float64 on the 2^-12 grid, clipped to +-2: a tree of N <= 255 has at most 1017 terms, so
    |sum| < 2^11 and every partial sum is an exact float32 (at most 23 bits).  bf16: randn rounded to bfloat16 first, so the values are
    bf16-representable as well.  Root-merged in shape only: every entry is an ordinary score (the root's rows too)."""
    return _grid(np.clip(rng.standard_normal((B, N, 2, 2, 2)), -2, 2), bf16), _grid(np.clip(rng.standard_normal((B, N, N, 2)), -2, 2), bf16)


def check_dmv_kbest(dec, attach, lengths, K, heads, scores, count, ref, tie_cap=0.25):
    """The checks every k-best result gets (kbest_restatement.check_kbest for the DMV).  dec / attach float64 of the exactly
    representable recipe, heads [K,B,N], scores [K,B] float32, count [B]; ref[b] = (values, heads, count) of dmv_kbest_dp at some
    K' > K.  Scores bit for bit; heads equal where the rank's value is strictly separated from both neighbours among the K + 1
    reference values; every returned tree valid, distinct, and its tree_score equal to the reported score; absent ranks NEGINF / 0.
    Returns (compared, tied); tie_cap (None: no cap) bounds tied_share(ref)."""
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
            assert np.float32(score(dec[b], attach[b], heads[k, b], L)[0]) == scores[k, b], (b, k)
            if (k == 0 or v[k - 1] > v[k]) and v[k] > v[k + 1]:
                assert np.array_equal(heads[k, b], h[k]), (b, k)
                compared += 1
            else:
                tied += 1
        assert len({tuple(x) for x in heads[:n, b]}) == n, b
    if tie_cap is not None:
        assert tied_share(ref) <= tie_cap, (tied_share(ref), compared, tied)
    return compared, tied
