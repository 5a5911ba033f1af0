"""GPU: DMV1o.sample_heads (vlg_dmv1o_sample) and DMV1o.log_prob_heads on an MI355X -- steered exactness at every chart placement and
dispatch boundary, forbidden arcs and bad lengths, the exact distribution over all trees of short sentences, arc frequencies against the
marginals, the keying of the draws, capture into a HIP graph, and log_prob_heads with its gradient.

Steered exactness (tests/dmv_sample_restatement.py): the float64 restatement writes into the explicit uniform table, at every cell of a
chosen tree, the midpoint of the wanted split's interval; the kernel must return exactly that tree.  Potentials are 0.25 randn, merged
through DMV1o.merge (at the DepTree test's 0.5 the right chain of a 254-word sentence has a split of probability 8e-5); the smallest
conditional probability steered through is asserted >= 0.01 for EVERY target, none excluded.  The chains are steered as they are; the
root-child sweep runs over the positions whose root split reaches the floor, and the random trees (and the rest of a sweep tree) grow
through splits of probability >= 0.02.

Measured on an MI355X: smallest steered probability 0.0101 (N = 100, f32) ... 1.0; |logp - logp64| at most 0.006 of its bound; tree counts at
most 0.63, arc frequencies at most 0.63 of their bounds; log_prob_heads' gradient errors 3.2e-6 / 2.7e-6 against bounds of 3.1e-4 / 2.2e-4.
"""
import functools
import os

import numpy as np
import pytest
import torch

import dmv_sample_restatement as D
from conftest import GOLDEN, load

pytestmark = pytest.mark.gpu

FLOOR = 0.01


@pytest.fixture(scope="module")
def dev():
    from vlgae_amd.build import build_library
    build_library()
    return torch.device("cuda")


def _ws_threshold():
    "the smallest N whose charts the launcher keeps in the workspace"
    from vlgae_amd import _C
    return next(N for N in range(2, 256) if _C.lib().vlg_dmv1o_sample_workspace(1, N, 1) > 0)


def sample(dec, attach, lengths, n, **kw):
    from vlgae_amd.torch_struct import functional as F
    heads, logp, logZ = F.dmv1o_sample(dec, attach, lengths, n, **kw)
    torch.cuda.synchronize()
    return heads.cpu().numpy(), logp.cpu().numpy(), logZ.cpu().numpy()


def device_merged(dev, dec, attach, root, bf16=False):
    """(dec, attach on the device, the same values as float32 numpy): DMV1o.merge of unmerged numpy potentials, in bf16 if asked.  The
    merge only copies, so it must equal the restatement's."""
    from vlgae_amd.torch_struct import DMV1o
    md, ma = DMV1o.merge(*(torch.from_numpy(x).to(dev) for x in (dec, attach, root)))
    rd, ra = D.merge64(dec, attach, root)
    assert np.array_equal(md.cpu().numpy(), rd) and np.array_equal(ma.cpu().numpy(), ra)
    if bf16:
        md, ma = md.to(torch.bfloat16), ma.to(torch.bfloat16)
    return md, ma, md.float().cpu().numpy(), ma.float().cpu().numpy()


def fixture_merged(dev, name):
    g = load(os.path.join(GOLDEN, name + ".npz"))
    md, ma, nd, na = device_merged(dev, g["dec"], g["attach"], g["root"])
    return g, md, ma, nd.astype(np.float64), na.astype(np.float64), torch.from_numpy(g["lengths"]).to(dev)


def logp_bound(logZ64, length, mag):
    "the DepTree test's form with the DMV term count: at most 4 len + 1 potentials enter a tree's score"
    return 2e-5 * np.maximum(1.0, np.abs(logZ64)) + (4 * length + 1) * 2.0 ** -23 * mag


# ---- 1. steered exactness -----------------------------------------------------------------------------------------------------------------
S_MAX = 9
STEER_NS = (2, 3, 6, 41, 42, 65, 66, "last_lds", "first_ws", 255)


def _bf16_round(a):
    return torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()


@functools.lru_cache(maxsize=None)
def steered_batch(N, bf16):
    """B = 3 ragged sentences (full length, 1, in between), S_MAX targets each (D.steered_rows).  One float64 reference per (N, dtype),
    shared by the S cases, computed from the values the kernel reads (the merged potentials, rounded to bf16 if that is what it gets)."""
    rng = np.random.default_rng(2000 + N + (7 if bf16 else 0))
    lengths = [N - 1, 1, max(1, (N - 1) // 2)]
    raw = D.random_unmerged(rng, 3, N - 1)
    dec, attach = D.merge64(*raw)
    if bf16:
        dec, attach = _bf16_round(dec), _bf16_round(attach)
    u = np.full((S_MAX, 3, 3, N, N), np.nan, np.float32)
    want = np.zeros((S_MAX, 3, N), np.int64)
    ref_logp, mag = np.zeros((S_MAX, 3)), np.zeros((S_MAX, 3))
    logZ, pmin = np.zeros(3), 1.0
    for b, L in enumerate(lengths):
        charts = D.inside64(dec[b], attach[b], L)
        logZ[b] = D.log_partition(charts, L)
        for s, row in enumerate(D.steered_rows(dec[b], attach[b], L, S_MAX, rng, FLOOR, charts)):
            u[s, b], want[s, b] = row[0], D.pad_heads(row[2], N)
            pmin = min(pmin, row[1])
            score, mag[s, b], _, _ = D.tree_score(dec[b], attach[b], row[2], L)
            ref_logp[s, b] = score - logZ[b]
    return raw, dec, attach, lengths, u, want, ref_logp, mag, logZ, pmin


@pytest.mark.parametrize("S", (1, 8, 9))
@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("N", STEER_NS)
def test_steered_trees_come_back_exactly(dev, N, bf16, S):
    if isinstance(N, str):
        N = _ws_threshold() - (1 if N == "last_lds" else 0)
    raw, dec, attach, lengths, u, want, ref_logp, mag, logZ64, pmin = steered_batch(N, bf16)
    print(f"N={N} {'bf16' if bf16 else 'f32'}: smallest steered conditional probability {pmin:.4f}")
    assert pmin >= FLOOR
    md, ma, nd, na = device_merged(dev, *raw, bf16=bf16)
    assert np.array_equal(nd, dec) and np.array_equal(na, attach)        # the reference was computed from what the kernel reads
    heads, logp, logZ = sample(md, ma, torch.tensor(lengths, device=dev), S, u=torch.from_numpy(u[:S]).to(dev))
    assert np.array_equal(heads, want[:S])
    bound = logp_bound(logZ64[None, :], np.array(lengths)[None, :], mag[:S])
    err = np.abs(logp - ref_logp[:S])
    print(f"  max |logp - logp64| / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    assert np.all(np.abs(logZ - logZ64) <= 2e-5 * np.maximum(1.0, np.abs(logZ64)))


# ---- 2., 3. forbidden arcs, bad lengths ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
def test_no_sample_contains_a_forbidden_arc(dev, bf16):
    rng = np.random.default_rng(3)
    B, N, S = 4, 24, 64
    lengths = [23, 7, 1, 16]
    dec, attach = D.merge64(*D.random_unmerged(rng, B, N - 1))
    attach[rng.random(attach.shape) < 0.3] = -np.inf
    for b, L in enumerate(lengths):   # one tree per sentence is guaranteed to be finite, whatever valence its arcs take
        t = D.random_tree(L, rng)
        c = np.arange(1, L + 1)
        arcs = attach[b, t[c], c]
        attach[b, t[c], c] = np.where(np.isinf(arcs), np.float32(0.25), arcs)
    md, ma = torch.from_numpy(dec).to(dev), torch.from_numpy(attach).to(dev)
    if bf16:
        md, ma = md.to(torch.bfloat16), ma.to(torch.bfloat16)
    from vlgae_amd.encoders import DeviceRng
    heads, logp, logZ = sample(md, ma, torch.tensor(lengths, device=dev), S, rng=DeviceRng(11, dev))
    assert np.isfinite(logZ).all() and np.isfinite(logp).all()
    for s in range(S):
        for b, L in enumerate(lengths):
            h = heads[s, b]
            assert D.is_tree(h, L), (s, b, h)
            _, _, _, ca = D.tree_score(dec[b], attach[b], h, L)
            assert np.all(attach[b][ca > 0] > -1e11), (s, b, h)        # every attachment, at the valence the tree gives it, is a finite arc


def test_invalid_length_gives_zero_heads_and_nan(dev):
    rng = np.random.default_rng(4)
    N = 9
    md, ma, _, _ = device_merged(dev, *D.random_unmerged(rng, 3, N - 1))
    from vlgae_amd.encoders import DeviceRng
    heads, logp, logZ = sample(md, ma, torch.tensor([0, N, 5], device=dev), 10, rng=DeviceRng(1, dev))
    assert not heads[:, :2].any() and np.isnan(logp[:, :2]).all() and np.isnan(logZ[:2]).all()
    assert np.isfinite(logp[:, 2]).all() and np.isfinite(logZ[2]) and all(D.is_tree(h, 5) for h in heads[:, 2])


# ---- 4. the exact distribution over every tree of a short sentence ---------------------------------------------------------------------------
def test_tree_counts_match_the_enumerated_distribution(dev):
    g, md, ma, nd, na, ln = fixture_merged(dev, "dmv_B5_L7_s2")
    B, N = nd.shape[:2]
    S = 32768
    from vlgae_amd.encoders import DeviceRng
    heads, logp, logZ = sample(md, ma, ln, S, rng=DeviceRng(2024, dev))
    worst = 0.0
    for b in range(B):
        L, lz = int(g["lengths"][b]), float(g["logZ64"][b, 0])
        rows, first, count = np.unique(heads[:, b], axis=0, return_index=True, return_counts=True)
        if L > 6:   # 7 words: valid trees, and logp against the tree's own score
            for h, k in zip(rows, first):
                assert D.is_tree(h, L), h
                score, mag, _, _ = D.tree_score(nd[b], na[b], h, L)
                assert abs(logp[k, b] - (score - lz)) <= logp_bound(lz, L, mag)
            continue
        trees = D.all_trees(L)
        assert len(trees) == {1: 1, 3: 7, 5: 143, 6: 728}[L]
        scores, mags = np.array([D.tree_score(nd[b], na[b], t, L)[:2] for t in trees]).T
        p = np.exp(scores - lz)
        assert abs(p.sum() - 1.0) <= 1e-9
        index = {tuple(D.pad_heads(t, N)): k for k, t in enumerate(trees)}
        got = np.zeros(len(trees))
        for h, k, n in zip(rows, first, count):
            j = index[tuple(h)]                      # KeyError: not a projective single-root tree of this sentence
            got[j] = n
            assert abs(logp[k, b] - np.log(p[j])) <= logp_bound(lz, L, mags[j])
        dev_ = np.abs(got - S * p)
        bound = 6 * np.sqrt(S * p * (1 - p)) + 4
        worst = max(worst, float(np.max(dev_ / bound)))
        assert np.all(dev_ <= bound), (b, got, S * p)
    print(f"dmv_B5_L7_s2: worst |count - S p| / bound = {worst:.3f}")


# ---- 5. arc frequencies against the marginals -------------------------------------------------------------------------------------------------
def test_arc_frequencies_match_the_marginals(dev):
    g, md, ma, _, _, ln = fixture_merged(dev, "dmv_B8_L40_s0")
    mu = g["grad_attach64"].sum(-1)
    B, N = mu.shape[:2]
    S = 4096
    from vlgae_amd.encoders import DeviceRng
    from vlgae_amd.torch_struct import DMV1o, DependencyCRF
    heads = DMV1o([md, ma], ln).sample_heads(S, rng=DeviceRng(7, dev))
    freq = torch.zeros(B, N, N, dtype=torch.float64, device=dev)
    for s0 in range(0, S, 512):
        freq += DependencyCRF.heads_to_parts(heads[s0:s0 + 512], ln).sum(0, dtype=torch.float64)
    freq = (freq / S).cpu().numpy()
    bound = 6 * np.sqrt(mu * (1 - mu).clip(0) / S) + 4 / S
    print(f"worst |freq - mu| / bound = {np.max(np.abs(freq - mu) / bound):.3f}")
    assert np.all(np.abs(freq - mu) <= bound)


# ---- 6. keying ------------------------------------------------------------------------------------------------------------------------------
def _philox_uniforms(seed, step, site, S, B, N):
    "u [S,B,3,N,N] as the kernel's counter-based source draws them: Philox4x32-10, key site_key(seed, site), counter (kind<<16|hi<<8|lo, s, b, step)"
    M = np.uint64(0xFFFFFFFF)
    s_, b_, k_, lo_, hi_ = np.meshgrid(np.arange(S), np.arange(B), np.arange(3), np.arange(N), np.arange(N), indexing="ij")
    c = [(k_ << 16 | hi_ << 8 | lo_).astype(np.uint64), s_.astype(np.uint64), b_.astype(np.uint64), np.full(s_.shape, step & 0xFFFFFFFF, np.uint64)]
    k0 = np.uint64(seed & 0xFFFFFFFF)
    k1 = np.uint64(((seed >> 32) & 0xFFFFFFFF) ^ ((site * 0x9E3779B9) & 0xFFFFFFFF))
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return ((c[0] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def test_draws_are_keyed_by_state_sentence_sample_and_cell(dev):
    from vlgae_amd.encoders import DeviceRng
    rng_np = np.random.default_rng(9)
    B, N = 3, 24
    dec, attach, root = D.random_unmerged(rng_np, B, N - 1)
    dec[1], attach[1], root[1] = dec[0], attach[0], root[0]                # two sentences with identical potentials
    md, ma, _, _ = device_merged(dev, dec, attach, root)
    ln = torch.tensor([23, 23, 11], device=dev)
    rng = DeviceRng(123 + (5 << 32), dev)
    h1, p1, _ = sample(md, ma, ln, 64, rng=rng)
    h2, p2, _ = sample(md, ma, ln, 64, rng=rng)
    assert np.array_equal(h1, h2) and np.array_equal(p1, p2)               # the same (seed, step): identical output
    from vlgae_amd import _C
    assert _C.lib().vlg_dmv1o_sample_blocks(B, N, 9) != _C.lib().vlg_dmv1o_sample_blocks(B, N, 64)
    h9, p9, _ = sample(md, ma, ln, 9, rng=rng)                             # another grid (fewer blocks per sentence), same samples
    assert np.array_equal(h9, h1[:9]) and np.array_equal(p9, p1[:9])
    assert not np.array_equal(h1[:, 0], h1[:, 1])                          # the sentence index is part of the key
    hs, _, _ = sample(md, ma, ln, 64, rng=rng, site=1)
    assert not np.array_equal(hs, h1)
    # the explicit table filled with the counter-based source's values draws the same trees, at either site
    for site, want in ((0, (h9, p9)), (1, (hs[:9], None))):
        u = torch.from_numpy(_philox_uniforms(123 + (5 << 32), 0, site, 9, B, N)).to(dev)
        hu, pu, _ = sample(md, ma, ln, 9, u=u)
        assert np.array_equal(hu, want[0]) and (want[1] is None or np.array_equal(pu, want[1]))
    rng.advance()
    h3, _, _ = sample(md, ma, ln, 64, rng=rng)
    assert not np.array_equal(h3, h1)
    assert np.array_equal(sample(md, ma, ln, 9, u=torch.from_numpy(_philox_uniforms(123 + (5 << 32), 1, 0, 9, B, N)).to(dev))[0], h3[:9])


# ---- 7. capture -----------------------------------------------------------------------------------------------------------------------------
def test_capture_replays_draw_fresh_samples(dev):
    from vlgae_amd import _C
    from vlgae_amd.encoders import DeviceRng
    from vlgae_amd.torch_struct import DMV1o
    md, ma, _, _ = device_merged(dev, *D.random_unmerged(np.random.default_rng(5), 4, 40))
    ln = torch.tensor([40, 12, 33, 1], device=dev)
    assert _C.lib().vlg_dmv1o_sample_workspace(4, 41, 8) == 0            # charts in LDS: the captured region allocates the outputs only
    dist = DMV1o([md, ma], ln)
    rng = DeviceRng(77, dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dist.sample_heads(8, rng=rng, return_log_prob=True)              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        heads, logp = dist.sample_heads(8, rng=rng, return_log_prob=True)
        rng.advance()
    states, got = [], []
    for _ in range(2):
        states.append(rng.state.clone())
        graph.replay()
        got.append((heads.clone(), logp.clone()))
    torch.cuda.synchronize()
    assert not torch.equal(got[0][0], got[1][0])
    assert rng.state[1].item() == states[0][1].item() + 2
    for state, (h, p) in zip(states, got):
        eager = DeviceRng(0, dev)
        eager.state.copy_(state)
        he, pe = dist.sample_heads(8, rng=eager, return_log_prob=True)
        assert torch.equal(he, h) and torch.equal(pe, p)


# ---- 8. log_prob_heads -----------------------------------------------------------------------------------------------------------------------
def test_log_prob_heads_values_and_gradient(dev):
    g, md, ma, nd, na, ln = fixture_merged(dev, "dmv_B5_L7_s2")
    B, N = nd.shape[:2]
    S = 4
    from vlgae_amd.encoders import DeviceRng
    from vlgae_amd.torch_struct import DMV1o
    md, ma = md.requires_grad_(True), ma.requires_grad_(True)
    dist = DMV1o([md, ma], ln)
    heads, logp = dist.sample_heads(S, rng=DeviceRng(31, dev), return_log_prob=True)
    lp = dist.log_prob_heads(heads)
    assert lp.shape == (S, B)
    lp0 = dist.log_prob_heads(heads[0])                                 # no leading dimension: [B]
    assert lp0.shape == (B,) and torch.allclose(lp0, lp[0], rtol=0, atol=1e-5)
    lp.sum().backward()
    hn, lpn, kn = heads.cpu().numpy(), lp.detach().cpu().numpy(), logp.cpu().numpy()
    want_d, want_a = np.zeros((B, N, 2, 2, 2)), np.zeros((B, N, N, 2))
    for b in range(B):
        L, lz = int(g["lengths"][b]), float(g["logZ64"][b, 0])
        for s in range(S):
            score, mag, cd, ca = D.tree_score(nd[b], na[b], hn[s, b], L)
            bound = logp_bound(lz, L, mag)
            assert abs(lpn[s, b] - (score - lz)) <= bound and abs(kn[s, b] - (score - lz)) <= bound
            assert abs(lpn[s, b] - kn[s, b]) <= bound
            want_d[b] += cd
            want_a[b] += ca
    want_d -= S * g["grad_dec64"]
    want_a -= S * g["grad_attach64"]
    for got, want in ((md.grad, want_d), (ma.grad, want_a)):
        err = np.abs(got.double().cpu().numpy() - want).max()
        print(f"gradient: max error {err:.2e}, bound {1e-4 * np.abs(want).max():.2e}")
        assert err <= 1e-4 * np.abs(want).max()
