"""GPU: DependencyCRF.sample_heads (vlg_deptree_sample) on an MI355X -- steered exactness at every chart placement and dispatch
boundary, forbidden arcs and bad lengths, the exact distribution over all trees of short sentences, arc frequencies against the
marginals, the keying of the draws, and capture into a HIP graph.

Steered exactness (tests/sample_restatement.py): the float64 restatement writes into the explicit uniform table, at every cell of a
chosen tree, the midpoint of the wanted split's interval; the kernel must return exactly that tree.  Potentials are 0.5 randn; the
smallest conditional probability steered through is asserted >= 0.01 for EVERY target, none excluded.  The two extreme trees (the
all-left and the all-right chain) are steered as they are.  For the other two kinds of target that floor cannot be met by trees chosen
without looking at the potentials -- a cell of a sentence of 254 words has up to 254 splits, their probabilities sum to one, and a
middle position as the root's child has probability 6e-5 at N = 255 -- so the root-child sweep runs over the positions whose root split
reaches the floor, and the random trees (and the rest of a sweep tree) grow through splits of probability >= 0.02, drawn uniformly
among those.

Measured on an MI355X: smallest steered probability 0.0104 (N = 65, f32) ... 1.0; |logp - logp64| at most 0.006 of its bound; tree counts at
most 0.50, arc frequencies at most 0.63 of their bounds.
"""
import functools

import numpy as np
import pytest
import torch

import sample_restatement as R
from conftest import GOLDEN, load

pytestmark = pytest.mark.gpu

FLOOR = 0.01


@pytest.fixture(scope="module")
def dev():
    from vlgae_amd.build import build_library
    build_library()
    return torch.device("cuda")


def _ws_threshold():
    "the smallest N whose inside pass keeps its charts in the workspace"
    from vlgae_amd import _C
    return next(N for N in range(2, 256) if _C.lib().vlg_workspace_bytes(_C.OP_DEPTREE_INSIDE, 1, N, 0) > 0)


def sample(arc, lengths, n, **kw):
    from vlgae_amd.torch_struct import functional as F
    heads, logp, logZ = F.deptree_sample(arc, lengths, n, **kw)
    torch.cuda.synchronize()
    return heads.cpu().numpy(), logp.cpu().numpy(), logZ.cpu().numpy()


def _bf16_round(a):
    return torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()


# ---- steered exactness ------------------------------------------------------------------------------------------------------------------
S_MAX = 9
STEER_NS = (2, 3, 6, 41, 42, 65, 66, "ws", 255)


@functools.lru_cache(maxsize=None)
def steered_batch(N, bf16):
    """B = 3 ragged sentences (full length, 1, in between), S_MAX targets each: sample s aims at the left chain, the right chain, a tree
    of the root-child sweep, a random tree, in turn.  One float64 reference per (N, dtype), shared by the S cases."""
    rng = np.random.default_rng(1000 + N + (7 if bf16 else 0))
    lengths = [N - 1, 1, max(1, (N - 1) // 2)]
    arc = (0.5 * rng.standard_normal((3, N, N))).astype(np.float32)
    if bf16:
        arc = _bf16_round(arc)
    u = np.full((S_MAX, 3, 3, N, N), np.nan, np.float32)
    want = np.zeros((S_MAX, 3, N), np.int64)
    ref_logp = np.zeros((S_MAX, 3))
    mag = np.zeros((S_MAX, 3))
    logZ, pmin = np.zeros(3), 1.0
    for b, L in enumerate(lengths):
        charts = R.inside64(arc[b], L)
        logZ[b] = charts[1][0, L]
        t, r = R.terms(*charts, 2, 0, L)
        root_ok = r[R.weights(t) / R.weights(t).sum() >= FLOOR]      # the sweep's positions: the root split itself reaches the floor
        assert root_ok.size >= 1
        for s in range(S_MAX):
            if s % 4 == 0:
                row = R.steer(arc[b], L, R.left_chain(L), charts=charts)
            elif s % 4 == 1:
                row = R.steer(arc[b], L, R.right_chain(L), charts=charts)
            elif s % 4 == 2:
                p = int(root_ok[(s // 4) * max(1, root_ok.size // 2) % root_ok.size])
                row = R.steer(arc[b], L, pick=R.floor_pick(rng, 2 * FLOOR, root_child=p, length=L), charts=charts)
                assert row[2][p] == 0
            else:
                row = R.steer(arc[b], L, pick=R.floor_pick(rng, 2 * FLOOR), charts=charts)
            u[s, b], want[s, b] = row[0], R.pad_heads(row[2], N)
            pmin = min(pmin, row[1])
            score, mag[s, b] = R.tree_score(arc[b], row[2], L)
            ref_logp[s, b] = score - logZ[b]
    return arc, lengths, u, want, ref_logp, mag, logZ, pmin


@pytest.mark.parametrize("S", (1, 8, 9))
@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("N", STEER_NS)
def test_steered_trees_come_back_exactly(dev, N, bf16, S):
    N = _ws_threshold() if N == "ws" else N
    arc, lengths, u, want, ref_logp, mag, logZ64, pmin = steered_batch(N, bf16)
    print(f"N={N} {'bf16' if bf16 else 'f32'}: smallest steered conditional probability {pmin:.4f}")
    assert pmin >= FLOOR
    a = torch.from_numpy(arc).to(dev)
    a = a.to(torch.bfloat16) if bf16 else a
    heads, logp, logZ = sample(a, torch.tensor(lengths, device=dev), S, u=torch.from_numpy(u[:S]).to(dev))
    assert np.array_equal(heads, want[:S])
    bound = 2e-5 * np.maximum(1.0, np.abs(logZ64))[None, :] + np.array(lengths)[None, :] * 2.0 ** -23 * mag[:S]
    err = np.abs(logp - ref_logp[:S])
    print(f"  max |logp - logp64| / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    assert np.all(np.abs(logZ - logZ64) <= 2e-5 * np.maximum(1.0, np.abs(logZ64)))


# ---- forbidden arcs, bad lengths -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
def test_no_sample_contains_a_forbidden_arc(dev, bf16):
    rng = np.random.default_rng(3)
    B, N, S = 4, 24, 64
    lengths = [23, 7, 1, 16]
    arc = (0.5 * rng.standard_normal((B, N, N))).astype(np.float32)
    arc[rng.random((B, N, N)) < 0.3] = -np.inf
    for b, L in enumerate(lengths):   # one tree per sentence is guaranteed to be finite
        t = R.random_tree(L, rng)
        c = np.arange(1, L + 1)
        arc[b, t[c], c] = np.where(np.isinf(arc[b, t[c], c]), 0.25, arc[b, t[c], c])
    a = torch.from_numpy(arc).to(dev)
    a = a.to(torch.bfloat16) if bf16 else a
    from vlgae_amd.encoders import DeviceRng
    heads, logp, logZ = sample(a, torch.tensor(lengths, device=dev), S, rng=DeviceRng(11, dev))
    assert np.isfinite(logZ).all() and np.isfinite(logp).all()
    for s in range(S):
        for b, L in enumerate(lengths):
            h = heads[s, b]
            assert R.is_tree(h, L), (s, b, h)
            assert np.isfinite(arc[b, h[1:L + 1], np.arange(1, L + 1)]).all(), (s, b, h)


def test_invalid_length_gives_zero_heads_and_nan(dev):
    rng = np.random.default_rng(4)
    N = 9
    a = torch.from_numpy((0.5 * rng.standard_normal((3, N, N))).astype(np.float32)).to(dev)
    from vlgae_amd.encoders import DeviceRng
    heads, logp, logZ = sample(a, torch.tensor([0, N, 5], device=dev), 10, rng=DeviceRng(1, dev))
    assert not heads[:, :2].any() and np.isnan(logp[:, :2]).all() and np.isnan(logZ[:2]).all()
    assert np.isfinite(logp[:, 2]).all() and all(R.is_tree(h, 5) for h in heads[:, 2])


# ---- the exact distribution over every tree of a short sentence ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("deptree_B3_N5_s1_enum", "deptree_B4_N6_s0_enum"))
def test_tree_counts_match_the_enumerated_distribution(dev, name):
    import os
    g = load(os.path.join(GOLDEN, name + ".npz"))
    arc, lengths = g["arc"], g["lengths"]
    B, N = arc.shape[:2]
    S = 32768
    from vlgae_amd.encoders import DeviceRng
    heads, logp, logZ = sample(torch.from_numpy(arc).to(dev), torch.from_numpy(lengths).to(dev), S, rng=DeviceRng(2024, dev))
    worst = 0.0
    for b in range(B):
        L = int(lengths[b])
        trees = R.all_trees(L)
        assert len(trees) == {4: 30, 5: 143}[L]
        scores, mags = np.array([R.tree_score(arc[b], t, L) for t in trees]).T
        assert abs(np.logaddexp.reduce(scores) - g["enum_logZ"][b]) <= 1e-9 * max(1.0, abs(g["enum_logZ"][b]))   # the enumeration is the reference's
        p = np.exp(scores - g["enum_logZ"][b])
        index = {tuple(R.pad_heads(t, N)): k for k, t in enumerate(trees)}
        count = np.zeros(len(trees))
        for h in heads[:, b]:
            count[index[tuple(h)]] += 1            # KeyError: not a projective single-root tree of this sentence
        dev_ = np.abs(count - S * p)
        bound = 6 * np.sqrt(S * p * (1 - p)) + 4
        worst = max(worst, float(np.max(dev_ / bound)))
        assert np.all(dev_ <= bound), (b, count, S * p)
        k = [index[tuple(h)] for h in heads[:16, b]]
        assert np.all(np.abs(logp[:16, b] - np.log(p[k])) <= 2e-5 * max(1.0, abs(g["enum_logZ"][b])) + L * 2.0 ** -23 * mags[k])
    print(f"{name}: worst |count - S p| / bound = {worst:.3f}")


# ---- arc frequencies against the marginals ------------------------------------------------------------------------------------------------
def test_arc_frequencies_match_the_marginals(dev):
    import os
    g = load(os.path.join(GOLDEN, "deptree_B8_N41_s1.npz"))
    arc, lengths, mu = g["arc"], g["lengths"], g["marginals64"]
    B, N = arc.shape[:2]
    S = 4096
    from vlgae_amd.encoders import DeviceRng
    from vlgae_amd.torch_struct import DependencyCRF
    dist = DependencyCRF(torch.from_numpy(arc).to(dev), torch.from_numpy(lengths).to(dev))
    heads = dist.sample_heads(S, rng=DeviceRng(7, dev))
    freq = torch.zeros(B, N, N, dtype=torch.float64, device=dev)
    for s0 in range(0, S, 512):
        freq += DependencyCRF.heads_to_parts(heads[s0:s0 + 512], dist.lengths).sum(0, dtype=torch.float64)
    freq = (freq / S).cpu().numpy()
    bound = 6 * np.sqrt(mu * (1 - mu).clip(0) / S) + 4 / S
    print(f"worst |freq - mu| / bound = {np.max(np.abs(freq - mu) / bound):.3f}")
    assert np.all(np.abs(freq - mu) <= bound)


# ---- keying ------------------------------------------------------------------------------------------------------------------------------
def test_draws_are_keyed_by_state_sentence_sample_and_cell(dev):
    from vlgae_amd.encoders import DeviceRng
    rng_np = np.random.default_rng(9)
    B, N = 3, 41
    arc = (0.5 * rng_np.standard_normal((B, N, N))).astype(np.float32)
    arc[1] = arc[0]                                        # two sentences with identical potentials
    a, ln = torch.from_numpy(arc).to(dev), torch.tensor([40, 40, 17], device=dev)
    rng = DeviceRng(123, dev)
    h1, p1, _ = sample(a, ln, 64, rng=rng)
    h2, p2, _ = sample(a, ln, 64, rng=rng)
    assert np.array_equal(h1, h2) and np.array_equal(p1, p2)               # the same (seed, step): identical output
    h16, p16, _ = sample(a, ln, 16, rng=rng)                               # another grid (fewer blocks per sentence), same samples
    assert np.array_equal(h16, h1[:16]) and np.array_equal(p16, p1[:16])
    assert not np.array_equal(h1[:, 0], h1[:, 1])                          # the sentence index is part of the key
    hs, _, _ = sample(a, ln, 64, rng=rng, site=1)
    assert not np.array_equal(hs, h1)
    rng.advance()
    h3, _, _ = sample(a, ln, 64, rng=rng)
    assert not np.array_equal(h3, h1)
    # explicit uniforms: one call with S = 64 equals eight calls with the eight slices of the table
    u = torch.from_numpy(rng_np.random((64, B, 3, N, N)).astype(np.float32)).to(dev)
    hu, pu, _ = sample(a, ln, 64, u=u)
    for k in range(8):
        hk, pk, _ = sample(a, ln, 8, u=u[8 * k:8 * k + 8].contiguous())
        assert np.array_equal(hk, hu[8 * k:8 * k + 8]) and np.array_equal(pk, pu[8 * k:8 * k + 8])
    for b, L in enumerate((40, 40, 17)):                                   # and it is the tree the rule draws, in float64, from that table
        same = sum(np.array_equal(hu[s, b, :L + 1], R.walk(arc[b], L, u[s, b].cpu().numpy())) for s in range(4))
        assert same >= 3   # (a uniform within float32 rounding of an interval's end may fall either way)


# ---- capture -----------------------------------------------------------------------------------------------------------------------------
def test_capture_replays_draw_fresh_samples(dev):
    from vlgae_amd.encoders import DeviceRng
    from vlgae_amd.torch_struct import DependencyCRF
    g = torch.Generator().manual_seed(5)
    arc = (0.5 * torch.randn(4, 41, 41, generator=g)).to(dev)
    ln = torch.tensor([40, 12, 33, 1], device=dev)
    dist = DependencyCRF(arc, ln)
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
