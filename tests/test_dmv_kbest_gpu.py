"""GPU: the k best trees of the valence DMV (vlg_dmv1o_kbest, DMV1o.kbest_heads / kbest_scores) and the adjoint of their scores
(vlg_dmv1o_tree_counts) on an MI355X -- the reference-made fixtures, brute force over every tree of short sentences, every chart
placement and both sides of every LDS <-> workspace boundary for every code image, N = 255, rank 0 against vlg_dmv1o_decode, unrounded
potentials, forbidden potentials, exact ties, bad lengths, independence of the batch, tree counts and the gradient of the scores, the
Python surface and capture into a HIP graph.

Potentials are the exactly-representable recipe of tests/dmv_kbest_restatement.py (2^-12 grid, |x| <= 2): a tree of N <= 255 has at most
1017 terms, so every partial sum has at most 23 bits, float32 scores are exact and compared BIT FOR BIT with the float64 restatement.
Heads are compared where the rank's value is strictly separated from both neighbours among the K + 1 reference values.  Tie cap: the
share of (sentence, rank) pairs left out as tied is a property of the potentials -- taken over the 16 ranks of the case's reference
values -- and is held to a quarter at every (N, dtype) used here (confirmed with the restatement alone before any kernel ran).

Every call goes through the C ABI with the outputs inside guard bands and the workspace pre-filled with NaN bit patterns.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dmv_kbest_restatement as R
from conftest import GOLDEN, load
from dmv_sample_restatement import merge64, tree_score

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 5, 8, 9, 16)
GUARD = 64
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    from vlgae_amd.build import build_library
    build_library()
    return torch.device("cuda")


def _guarded(shape, dtype, fill, device):
    n = int(np.prod(shape))
    return torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=device)


def _unguard(t, shape, fill):
    a = t.cpu().numpy()
    edge = np.concatenate([a[:GUARD], a[-GUARD:]])
    assert np.all(np.isnan(edge)) if isinstance(fill, float) and np.isnan(fill) else np.all(edge == fill)
    return a[GUARD:-GUARD].reshape(shape)


def kbest(dec, attach, lengths, K):
    """vlg_dmv1o_kbest on CUDA tensors (f32 or bf16) -> numpy heads [K,B,N], scores [K,B], count [B]; guards checked"""
    from vlgae_amd import _C
    L = _C.lib()
    B, N = attach.shape[:2]
    dt, d = _C.in_dtype(dec)
    _, a = _C.in_dtype(attach)
    ln = torch.as_tensor(lengths, dtype=torch.int64).to(dec.device)
    heads = _guarded((K, B, N), torch.int64, -7, dec.device)
    scores = _guarded((K, B), torch.float32, float("nan"), dec.device)
    count = _guarded((B,), torch.int32, -7, dec.device)
    nb = L.vlg_dmv1o_kbest_workspace(B, N, K)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=dec.device) if nb else None   # 0xffffffff: a NaN; 0xffff: no back-pointer
    off = lambda t, esz: ctypes.c_void_p(t.data_ptr() + GUARD * esz)
    _C.check(L.vlg_dmv1o_kbest(_C.ptr(d), _C.ptr(a), _C.ptr(ln), B, N, dt, K, off(heads, 8), off(scores, 4), off(count, 4), _C.ptr(ws), nb,
                               _C.stream_of(dec)), "dmv1o_kbest")
    torch.cuda.synchronize()
    return _unguard(heads, (K, B, N), -7), _unguard(scores, (K, B), float("nan")), _unguard(count, (B,), -7)


def counts(heads, lengths, count, weight, dev):
    """vlg_dmv1o_tree_counts on numpy inputs -> numpy cnt_dec [B,N,2,2,2], cnt_attach [B,N,N,2]; NaN-prefilled outputs inside guards"""
    from vlgae_amd import _C
    L = _C.lib()
    T, B, N = heads.shape
    h = torch.from_numpy(np.ascontiguousarray(heads, np.int64)).to(dev)
    ln = torch.as_tensor(lengths, dtype=torch.int64).to(dev)
    c = None if count is None else torch.from_numpy(np.ascontiguousarray(count, np.int32)).to(dev)
    w = None if weight is None else torch.from_numpy(np.ascontiguousarray(weight, np.float32)).to(dev)
    cd = _guarded((B, N, 2, 2, 2), torch.float32, float("nan"), dev)
    ca = _guarded((B, N, N, 2), torch.float32, float("nan"), dev)
    off = lambda t: ctypes.c_void_p(t.data_ptr() + GUARD * 4)
    _C.check(L.vlg_dmv1o_tree_counts(_C.ptr(h), _C.ptr(ln), _C.ptr(c), _C.ptr(w), T, B, N, off(cd), off(ca), _C.stream_of(h)), "dmv1o_tree_counts")
    torch.cuda.synchronize()
    return _unguard(cd, (B, N, 2, 2, 2), float("nan")), _unguard(ca, (B, N, N, 2), float("nan"))


def to_dev(x, dev, bf16=False):
    t = torch.from_numpy(np.asarray(x, np.float32)).to(dev)
    return t.to(torch.bfloat16) if bf16 else t


def ragged(N):
    return [N - 1, 1, max(1, (N - 1) // 2)]


@functools.lru_cache(maxsize=None)
def case(N, bf16, B=3):
    """potentials, lengths and the float64 restatement at K' = 17, computed once per (N, dtype) and shared by every K"""
    lengths = ragged(N)[:B] if B == 3 else [N - 1, 1]
    for draw in range(8):
        rng = np.random.default_rng(6000 + 2 * N + bf16 + 1000 * draw)
        dec, attach = R.potentials(rng, B, N, bf16=bf16)
        ref = [R.dmv_kbest_dp(dec[b], attach[b], L, 17, prune=N > 45) for b, L in enumerate(lengths)]   # (the bound is checked unpruned on the CPU)
        # The potentials are drawn again until they meet the tie cap: a property of the inputs and the float64 restatement alone,
        # decided before the kernel runs; check_dmv_kbest asserts the cap all the same.
        if R.tied_share(ref) <= 0.25:
            break
    return dec, attach, lengths, ref


# the largest N with everything in LDS / with only the back-pointers in the workspace, per code image (also pinned in test_dmv_kbest_host.py)
PLACEMENT = {1: (78, 89), 2: (60, 70), 4: (44, 52), 8: (32, 38), 16: (22, 28)}


def image(K):
    return next(c for c in (1, 2, 4, 8, 16) if K <= c)


def plan(N, K):
    "(mode 0 / 1 / 2 as the size query shows it) -- 0: no workspace; 1: back-pointers only; 2: values too"
    from vlgae_amd import _C
    need = _C.lib().vlg_dmv1o_kbest_workspace(1, N, K)
    KC, cells = image(K), N * ((N + 1) | 1)
    al = lambda x: (x + 15) & ~15
    bp = al(cells * KC * 2) + al(cells * KC * 4)
    return {0: 0, bp: 1, bp + al(cells * KC * 8) + al(cells * KC * 4) + al(cells * 8): 2}[need]


# ---- fixtures, brute force --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("dmvkbest_B3_N6_s0", "dmvkbest_B4_N5_s1"))
def test_reference_fixtures(dev, name):
    g = load(f"{GOLDEN}/{name}.npz")
    K = 16
    heads, scores, count = kbest(to_dev(g["dec"], dev), to_dev(g["attach"], dev), g["lengths"], K)
    n_cmp = 0
    for b, L in enumerate(g["lengths"]):
        nt = int(g["ntrees"][b])
        n = min(nt, K)
        v = g["values"][:, b]
        assert count[b] == n
        assert np.array_equal(scores[:n, b], v[:n].astype(np.float32))
        assert np.all(scores[n:, b] == np.float32(R.NEGINF)) and not heads[n:, b].any()
        for k in range(n):
            if (k == 0 or v[k - 1] > v[k]) and (k + 1 == nt or v[k] > v[k + 1]):
                assert np.array_equal(heads[k, b], g["heads"][k, b]), (b, k)
                n_cmp += 1
    assert n_cmp >= 0.75 * sum(min(K, int(t)) for t in g["ntrees"])


def test_reference_argmax_fixture(dev):
    g = load(f"{GOLDEN}/dmvkbest_B2_N41_s2.npz")
    heads, scores, count = kbest(to_dev(g["dec"], dev), to_dev(g["attach"], dev), g["lengths"], 2)
    assert np.array_equal(scores[0], g["values"][0].astype(np.float32)) and np.array_equal(heads[0], g["heads"][0])
    assert np.all(scores[1] < scores[0]) and list(count) == [2, 2]


def test_every_tree_of_short_sentences(dev):
    rng = np.random.default_rng(11)
    dec, attach = R.potentials(rng, 4, 7)
    lengths = [1, 2, 3, 6]
    heads, scores, count = kbest(to_dev(dec, dev), to_dev(attach, dev), lengths, 16)
    for b, L in enumerate(lengths):
        s, h = R.brute_force(dec[b], attach[b], L)
        assert len(s) == R.TREE_COUNTS[L]
        n = min(16, len(s))
        assert count[b] == n
        assert np.array_equal(scores[:n, b], s[:n].astype(np.float32))
        assert np.all(scores[n:, b] == np.float32(R.NEGINF)) and not heads[n:, b].any()
        assert len({tuple(x) for x in heads[:n, b]}) == n
        for k in range(n):
            assert R.is_tree(heads[k, b], L) and np.float32(R.score(dec[b], attach[b], heads[k, b], L)[0]) == scores[k, b]
            if (k == 0 or s[k - 1] > s[k]) and (k + 1 == len(s) or s[k] > s[k + 1]):
                assert np.array_equal(heads[k, b], h[k])


# ---- placements ----------------------------------------------------------------------------------------------------------------------------
def test_placement_table_matches_the_size_query(dev):
    for KC, (a, b) in PLACEMENT.items():
        assert [plan(n, KC) for n in (2, a, a + 1, b, b + 1, 255)] == [0, 0, 1, 1, 2, 2], KC


def _placement_cases():
    for K in KS:
        a, b = PLACEMENT[image(K)]
        for N in (2, a, a + 1, b, b + 1):   # the first and last N of each mode (the last of all, 255: test_longest_sentence)
            yield K, N


@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("K,N", list(_placement_cases()))
def test_every_placement(dev, K, N, bf16):
    dec, attach, lengths, ref = case(N, bf16)
    heads, scores, count = kbest(to_dev(dec, dev, bf16), to_dev(attach, dev, bf16), lengths, K)
    compared, tied = R.check_dmv_kbest(dec, attach, lengths, K, heads, scores, count, ref)
    print(f"N={N} K={K} {'bf16' if bf16 else 'f32'} placement {plan(N, K)}: heads compared {compared}, tied {tied}")


@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("K", (1, 16))
def test_longest_sentence(dev, K, bf16):
    "N = 255: the 8-bit split field at its limit, everything in the workspace"
    dec, attach, lengths, ref = case(255, bf16, B=2)
    heads, scores, count = kbest(to_dev(dec, dev, bf16), to_dev(attach, dev, bf16), lengths, K)
    R.check_dmv_kbest(dec, attach, lengths, K, heads, scores, count, ref)


# ---- rank 0 against the existing decode, unrounded potentials ---------------------------------------------------------------------------
def _sum_bound(dec, attach, heads, L):
    "n 2^-24 sum |terms|, n = 4 len + 1: the standard bound of an n-term float32 sum"
    return (4 * L + 1) * U * R.score(dec, attach, heads, L)[1]


def test_rank_zero_is_the_decode(dev):
    """vlg_dmv1o_decode sums the same 4 len + 1 terms in log2 units: every term times log2(e) (one rounding each, plus the constant's),
    an n-term float32 sum, and one product with ln 2 (its rounding and the constant's) -- (n + 3) 2^-24 sum |terms| to first order, next
    to the k-best kernel's own (n - 1) 2^-24 sum |terms|.  Score within (2 n + 4) 2^-24 sum |terms|; heads equal where the float64 gap to
    rank 1 exceeds that."""
    from vlgae_amd.torch_struct import DMV1o
    N = 41
    rng = np.random.default_rng(8)
    dec = rng.standard_normal((3, N, 2, 2, 2)).astype(np.float32).astype(np.float64)
    attach = rng.standard_normal((3, N, N, 2)).astype(np.float32).astype(np.float64)
    lengths = ragged(N)
    dist = DMV1o([to_dev(dec, dev), to_dev(attach, dev)], torch.tensor(lengths, device=dev))
    heads, scores, count = dist.kbest_heads(2, return_scores=True)
    heads, scores = heads.cpu().numpy(), scores.cpu().numpy()
    hd, mx = dist.argmax_heads.cpu().numpy(), dist.max.cpu().numpy().reshape(-1)
    for b, L in enumerate(lengths):
        v, h, _ = R.dmv_kbest_dp(dec[b], attach[b], L, 2)
        bound = (2 * (4 * L + 1) + 4) * U * R.score(dec[b], attach[b], h[0], L)[1]
        print(f"b={b} len={L}: |scores[0] - max| = {abs(float(scores[0, b]) - float(mx[b])):.3g}, bound {bound:.3g}, gap {v[0] - v[1]:.3g}")
        assert abs(float(scores[0, b]) - float(mx[b])) <= bound, b
        if v[0] - v[1] > bound:
            assert np.array_equal(heads[0, b], hd[b]) and np.array_equal(heads[0, b], h[0]), b


@pytest.mark.parametrize("N", (41, 100))
def test_unrounded_float32_potentials(dev, N):
    rng = np.random.default_rng(N)
    dec = rng.standard_normal((3, N, 2, 2, 2)).astype(np.float32).astype(np.float64)
    attach = rng.standard_normal((3, N, N, 2)).astype(np.float32).astype(np.float64)
    lengths, K = ragged(N), 8
    heads, scores, count = kbest(to_dev(dec, dev), to_dev(attach, dev), lengths, K)
    n_cmp = 0
    for b, L in enumerate(lengths):
        v, h, c = R.dmv_kbest_dp(dec[b], attach[b], L, K + 1, prune=N > 45)
        n = min(c, K)
        assert count[b] == n
        bounds = np.array([max(_sum_bound(dec[b], attach[b], heads[k, b], L), _sum_bound(dec[b], attach[b], h[k], L)) for k in range(n)])
        for k in range(n):
            assert R.is_tree(heads[k, b], L)
            assert abs(R.score(dec[b], attach[b], heads[k, b], L)[0] - float(scores[k, b])) <= _sum_bound(dec[b], attach[b], heads[k, b], L), (b, k)
            print(f"N={N} b={b} k={k}: |score - float64| = {abs(float(scores[k, b]) - v[k]):.3g}, bound {bounds[k]:.3g}")
            assert abs(float(scores[k, b]) - v[k]) <= bounds.max(), (b, k)
            if (k == 0 or v[k - 1] - v[k] > 2 * bounds.max()) and v[k] - v[k + 1] > 2 * bounds.max():
                assert np.array_equal(heads[k, b], h[k]), (b, k)
                n_cmp += 1
        assert len({tuple(x) for x in heads[:n, b]}) == n and np.all(np.diff(scores[:, b]) <= 0)
    assert n_cmp > 0


# ---- forbidden potentials, ties, bad lengths -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", (float("-inf"), -1e20))
def test_forbidden_arcs(dev, fill):
    N, K = 9, 8
    dec, attach = R.potentials(np.random.default_rng(2), 1, N)
    dec, base = dec[0], attach[0]
    chain = np.full((N, N, 2), fill)                   # only the right chain 0 -> 1 -> 2 -> ... is allowed
    for c in range(1, N):
        chain[c - 1, c] = base[c - 1, c]
    orphan = base.copy()                               # word 4 has no head at all
    orphan[:, 4] = fill
    nostop = dec.copy()                                # word 3 may not stop to its right
    nostop[3, 1, :, 1] = fill
    d, a = np.stack([dec, dec, nostop, dec]), np.stack([chain, orphan, base, base])
    heads, scores, count = kbest(to_dev(d, dev), to_dev(a, dev), [N - 1] * 4, K)
    assert list(count) == [1, 0, 0, K]
    want = np.concatenate([[0], np.arange(N - 1)])
    assert np.array_equal(heads[0, 0], want) and scores[0, 0] == np.float32(R.score(dec, base, want, N - 1)[0])
    assert np.all(scores[1:, 0] == np.float32(R.NEGINF)) and not heads[1:, 0].any()
    assert np.all(scores[:, 1:3] == np.float32(R.NEGINF)) and not heads[:, 1:3].any()
    ref = R.dmv_kbest_dp(dec, base, N - 1, K + 1)
    R.check_dmv_kbest(d[3:], a[3:], [N - 1], K, heads[:, 3:], scores[:, 3:], count[3:], [ref])


def test_merged_potentials(dev):
    "DMV1o.merge's layout: -1e12 in the root's left decisions and HASCHILD attachments, and on every arc into the root"
    B, L, K = 3, 7, 16
    dec, attach = R.potentials(np.random.default_rng(5), B, L)
    root = R.potentials(np.random.default_rng(6), B, L)[0][:, :, 0, 0, 0]
    md, ma = merge64(dec, attach, root)
    lengths = [L, 2, 4]
    heads, scores, count = kbest(to_dev(md, dev), to_dev(ma, dev), lengths, K)
    ref = [R.dmv_kbest_dp(md[b], ma[b], n, K + 1) for b, n in enumerate(lengths)]
    assert [r[2] for r in ref] == [K + 1, 2, K + 1]
    R.check_dmv_kbest(md, ma, lengths, K, heads, scores, count, ref)


def test_exact_ties_give_distinct_trees(dev):
    N, K = 9, 16
    heads, scores, count = kbest(torch.zeros((1, N, 2, 2, 2), device=dev), torch.zeros((1, N, N, 2), device=dev), [N - 1], K)
    assert count[0] == K and np.all(scores == 0.0) and not np.signbit(scores).any()
    assert all(R.is_tree(h, N - 1) for h in heads[:, 0])
    assert len({tuple(h) for h in heads[:, 0]}) == K


def test_invalid_lengths_leave_the_others_alone(dev):
    N, K = 12, 5
    dec, attach, lengths, ref = case(N, False)
    pick = [0, 0, 1, 0, 2]
    heads, scores, count = kbest(to_dev(dec[pick], dev), to_dev(attach[pick], dev), [lengths[0], 0, lengths[1], N, lengths[2]], K)
    for b in (1, 3):
        assert count[b] == 0 and not heads[:, b].any() and np.all(np.isnan(scores[:, b]))
    keep = [0, 2, 4]
    R.check_dmv_kbest(dec, attach, lengths, K, heads[:, keep], scores[:, keep], count[keep], ref)
    alone = kbest(to_dev(dec, dev), to_dev(attach, dev), lengths, K)
    assert np.array_equal(alone[0], heads[:, keep]) and np.array_equal(alone[1].view(np.uint32), scores[:, keep].view(np.uint32))
    heads, scores, count = kbest(to_dev(dec[:2], dev), to_dev(attach[:2], dev), [-3, lengths[1]], K)
    assert count[0] == 0 and not heads[:, 0].any() and np.all(np.isnan(scores[:, 0]))
    R.check_dmv_kbest(dec[1:2], attach[1:2], lengths[1:2], K, heads[:, 1:], scores[:, 1:], count[1:], ref[1:2])


# ---- independence, reproducibility, prefix -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (30, 41))
def test_batch_independence_reruns_and_prefix(dev, N):
    dec, attach, lengths, _ = case(N, False)
    d, a = to_dev(np.concatenate([dec, dec[::-1]]), dev), to_dev(np.concatenate([attach, attach[::-1]]), dev)   # B = 6
    ln = lengths + lengths[::-1]
    h16, s16, c16 = kbest(d, a, ln, 16)
    h16b, s16b, c16b = kbest(d, a, ln, 16)
    assert np.array_equal(h16, h16b) and np.array_equal(s16.view(np.uint32), s16b.view(np.uint32)) and np.array_equal(c16, c16b)
    assert np.array_equal(h16[:, :3], h16[:, :2:-1]) and np.array_equal(s16[:, :3].view(np.uint32), s16[:, :2:-1].view(np.uint32))
    h1, s1, c1 = kbest(d[:1], a[:1], ln[:1], 16)                       # alone against inside the batch
    assert np.array_equal(h1[:, 0], h16[:, 0]) and np.array_equal(s1[:, 0].view(np.uint32), s16[:, 0].view(np.uint32)) and c1[0] == c16[0]
    h5, s5, c5 = kbest(d, a, ln, 5)                                    # another code image, another placement
    assert np.array_equal(s5.view(np.uint32), s16[:5].view(np.uint32)) and np.array_equal(h5, h16[:5])
    assert np.array_equal(c5, np.minimum(c16, 5))


# ---- tree counts and the gradient of the scores -----------------------------------------------------------------------------------------------
def test_tree_counts_kernel(dev):
    "every tree of 5 words in one call, each alone and all weighted by powers of two; bad entries; count; an invalid length"
    N, L = 8, 5
    trees = R.all_trees(L)
    T = len(trees)
    heads = np.zeros((T, 3, N), np.int64)
    for t, h in enumerate(trees):
        heads[t, :, :L + 1] = h
    heads[1, 1, 2], heads[2, 1, 3], heads[3, 1, 4] = 2, L + 1, -5   # names itself / outside the sentence / negative
    heads[:, :, L + 1:] = 1 << 40                                   # padding is never read as a word
    w = (2.0 ** np.random.default_rng(0).integers(-3, 4, (T, 3))).astype(np.float32)
    for count, weight, lengths in ((None, None, [L, L, L]), (np.array([7, T, 0], np.int32), w, [L, L, L]), (None, w, [L, 0, N])):
        cd, ca = counts(heads, lengths, count, weight, dev)
        want = R.tree_counts(heads, lengths, count, weight, N)
        assert np.array_equal(cd.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(ca.view(np.uint32), want[1].view(np.uint32))
    dec, attach = R.potentials(np.random.default_rng(1), 1, N)
    one = np.stack([np.stack([h]) for h in heads[:, 0]])            # [T,1,N]: tree t as sentence 0 of its own call
    for t in range(0, T, 13):
        cd, ca = counts(one[t:t + 1], [L], None, None, dev)
        _, _, wd, wa = tree_score(dec[0], attach[0], one[t, 0], L)
        assert np.array_equal(cd[0], wd) and np.array_equal(ca[0], wa), t


def test_scores_gradient_is_the_tree_counts(dev):
    from vlgae_amd.torch_struct import DMV1o
    N, K = 12, 5
    dec, attach, lengths, ref = case(N, False)
    d, a = to_dev(dec, dev).requires_grad_(True), to_dev(attach, dev).requires_grad_(True)
    dist = DMV1o([d, a], torch.tensor(lengths, device=dev))
    heads, scores, count = dist.kbest_heads(K, return_scores=True)
    heads, count = heads.cpu().numpy(), count.cpu().numpy()
    assert list(count) == [K, 1, K]   # the sentence of one word has one tree: its ranks 1 ... are absent
    ks = dist.kbest_scores(K)
    assert torch.equal(ks.detach(), scores) and ks.requires_grad
    for k in range(K):
        gd, ga = torch.autograd.grad(ks[k].sum(), (d, a), retain_graph=True)
        gd, ga = gd.cpu().numpy(), ga.cpu().numpy()
        for b, L in enumerate(lengths):
            if k < count[b]:
                _, _, wd, wa = tree_score(dec[b], attach[b], heads[k, b], L)
                assert np.array_equal(gd[b], wd) and np.array_equal(ga[b], wa), (k, b)
            else:
                assert not gd[b].any() and not ga[b].any(), (k, b)   # an absent rank: zero gradient
    w = (2.0 ** np.random.default_rng(0).integers(-3, 4, (K, 3))).astype(np.float32)
    w[::2] *= -1
    gd, ga = torch.autograd.grad((torch.from_numpy(w).to(dev) * ks).sum(), (d, a))
    want = R.tree_counts(heads, lengths, count, w, N)
    assert np.array_equal(gd.cpu().numpy().view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(ga.cpu().numpy().view(np.uint32), want[1].view(np.uint32))


# ---- Python surface --------------------------------------------------------------------------------------------------------------------------
def test_python_api(dev):
    from vlgae_amd.torch_struct import DMV1o
    from vlgae_amd.torch_struct import functional as F
    N, K = 12, 5
    dec, attach, lengths, ref = case(N, True)
    ln = torch.tensor(lengths, device=dev)
    dist = DMV1o([to_dev(dec, dev, True), to_dev(attach, dev, True)], ln)
    heads, scores, count = dist.kbest_heads(K, return_scores=True)
    assert heads.shape == (K, 3, N) and heads.dtype == torch.int64 and scores.shape == (K, 3) and scores.dtype == torch.float32
    assert count.shape == (3,) and count.dtype == torch.int32 and torch.equal(dist.kbest_heads(K), heads)
    assert heads.device == scores.device == count.device == ln.device
    R.check_dmv_kbest(dec, attach, lengths, K, heads.cpu().numpy(), scores.cpu().numpy(), count.cpu().numpy(), ref)
    ks = dist.kbest_scores(K)
    assert ks.shape == (K, 3) and torch.equal(ks, scores) and not ks.requires_grad
    live = (torch.arange(K, device=dev).unsqueeze(-1) < count.unsqueeze(0))
    # The sampler's scorer agrees on the trees the k-best kernel found: score and log-partition both come from log2-unit float32 DPs
    # over n = 4 len + 1 terms of magnitude <= 2, each within (2 n + 4) 2^-24 sum |terms| (test_rank_zero_is_the_decode).
    lp = dist.log_prob_heads(heads)
    want = scores - dist.partition.reshape(1, -1)
    n = 4.0 * ln + 1
    tol = (2 * (2 * n + 4) * U * 2 * n).to(torch.float32).view(1, -1).expand(K, -1)
    assert torch.all((lp - want).abs()[live] <= tol[live])
    cd, ca = F.dmv1o_tree_counts(heads, ln, count)
    assert cd.shape == (3, N, 2, 2, 2) and ca.shape == (3, N, N, 2) and cd.dtype == ca.dtype == torch.float32
    assert float(cd.sum() + ca.sum()) == sum(int(c) * (4 * L + 1) for c, L in zip(count.cpu(), lengths))
    for k in (0, 17):
        with pytest.raises(RuntimeError):
            dist.kbest_heads(k)
    with pytest.raises(NotImplementedError, match="kbest_heads"):
        dist.kmax(2)
    with pytest.raises(NotImplementedError):
        dist.topk(2)


def test_capture_replays_on_new_potentials(dev):
    from vlgae_amd.torch_struct import functional as F
    N, K = 41, 8
    dec, attach, lengths, ref = case(N, False)
    dec2, attach2, _, ref2 = case(N, True)
    bd, ba = to_dev(dec, dev), to_dev(attach, dev)
    ln = torch.tensor(lengths, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        F.dmv1o_kbest(bd, ba, ln, K)              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        heads, scores, count = F.dmv1o_kbest(bd, ba, ln, K)
    graph.replay()
    torch.cuda.synchronize()
    R.check_dmv_kbest(dec, attach, lengths, K, heads.cpu().numpy(), scores.cpu().numpy(), count.cpu().numpy(), ref)
    bd.copy_(to_dev(dec2, dev))
    ba.copy_(to_dev(attach2, dev))
    graph.replay()
    torch.cuda.synchronize()
    R.check_dmv_kbest(dec2, attach2, lengths, K, heads.cpu().numpy(), scores.cpu().numpy(), count.cpu().numpy(), ref2)
