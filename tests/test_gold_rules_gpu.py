"""GPU: the parser's rule-supervised initialisation loss and its marginal loss in the training step.

  * rules1o.gold_rules against the reference's padded rule fields (goldrules_*: bit-equal), invalid sentences;
  * rules1o.gold_rule_score against a float64 sum, its adjoint = g * counts exactly (f32 and bf16);
  * the pair launch's grad_dec = vlg_dmv1o_inside_outside's, bit for bit, and the remembered pass behind `.partition`;
  * train_step.build(dep_loss="gold_rules") on initstep_* (the reference's own init-epoch step), dep_loss="partition" on margstep_*;
  * the init step at B = 256, L = 40 (both layouts) against the same step with a test-local float64 count . potential term;
  * four batches fed in place with parameter updates = a fresh build each time; one HIP graph replayed = the eager step."""
import numpy as np
import pytest
import torch

from conftest import golden_files, golden_ids, load
from test_gold_rules import NOCHILD, np_batch_rules
from test_gpu_parity import trainstep_from_fixture

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def merged_counts(arc, lengths, N):
    """The restatement's counts in the root-merged layout: (cd [B,N,2,2,2], ca [B,N,N,2]) float64."""
    dec, att, root = np_batch_rules(arc, lengths, N - 1)
    B = len(lengths)
    cd, ca = np.zeros((B, N, 2, 2, 2)), np.zeros((B, N, N, 2))
    cd[:, 1:], ca[:, 1:, 1:], ca[:, 0, 1:, NOCHILD] = dec, att, root
    return cd, ca


@pytest.mark.parametrize("path", golden_files("goldrules_"), ids=golden_ids("goldrules_"))
def test_gold_rules_bit_equal_to_the_reference(path):
    from vlgae_amd import rules1o
    g = load(path)
    L = g["dec_rule"].shape[1]
    for dt in (torch.float64, torch.float32):
        dec, att, root = rules1o.gold_rules(t(g["arc"]), t(g["lengths"]), L, dt)
        assert dec.dtype == dt
        assert np.array_equal(dec.cpu().double().numpy(), g["dec_rule"])
        assert np.array_equal(att.cpu().double().numpy(), g["attach_rule"])
        assert np.array_equal(root.cpu().double().numpy(), g["root_rule"])
    # a wider table and a wider arc array: zero past n, the same counts
    arc = np.concatenate([g["arc"], np.full((len(g["lengths"]), 3), 77)], 1)
    dec, att, root = rules1o.gold_rules(t(arc), t(g["lengths"]), L + 2)
    assert np.array_equal(dec.cpu().numpy()[:, :L], g["dec_rule"]) and not dec[:, L:].any()
    assert np.array_equal(att.cpu().numpy()[:, :L, :L], g["attach_rule"]) and not att[:, L:].any() and not att[:, :, L:].any()
    assert np.array_equal(root.cpu().numpy()[:, :L], g["root_rule"])


def _potentials(B, N, seed, dtype=torch.float32):
    import vlgae_amd.torch_struct as ts
    gen = torch.Generator().manual_seed(seed)
    L = N - 1
    dec = torch.randn(B, L, 2, 2, 2, generator=gen).log_softmax(-1)
    attach = torch.randn(B, L, L, 2, generator=gen)
    root = torch.randn(B, L, generator=gen).log_softmax(-1)
    md, ma = ts.DMV1o.merge(dec.to(dev()), attach.to(dev()), root.to(dev()))   # -inf fills in the root row and column 0
    return md.to(dtype).contiguous(), ma.to(dtype).contiguous()


def random_tree(rng, n):
    """One root; every other word attaches to a word placed before it in a random order (non-projective trees included)."""
    order = rng.permutation(n)
    arc = np.zeros(n, dtype=np.int64)
    for i in range(1, n):
        arc[order[i]] = order[rng.integers(0, i)] + 1
    return arc


def _random_arcs(rng, lengths, L):
    arc = np.zeros((len(lengths), L), np.int64)
    for b, n in enumerate(lengths):
        arc[b, :n] = random_tree(rng, int(n))
    return arc


def test_invalid_sentences_give_nan_and_zero_counts():
    from vlgae_amd import rules1o
    L = 6
    arcs = np.array([[2, 0, 2, 3, 0, 0],      # valid (n = 4)
                     [2, 0, 7, 3, 1, 0],      # 7 > n = 6
                     [2, 0, -1, 3, 0, 0],     # negative
                     [2, 3, 1, 0, 0, 0],      # n = 3: no 0 among the first three
                     [0, 1, 1, 1, 1, 1],      # length 0
                     [0, 1, 1, 1, 1, 1]], np.int64)   # length 9 > L
    lengths = np.array([4, 6, 5, 3, 0, 9])
    dec, att, root = rules1o.gold_rules(t(arcs), t(lengths), L)
    assert dec[0].any() and not dec[1:].any() and not att[1:].any() and not root[1:].any()
    md, ma = _potentials(6, L + 1, 0)
    md, ma = md.requires_grad_(), ma.requires_grad_()
    s = rules1o.gold_rule_score(md, ma, t(arcs), t(lengths))
    assert torch.isfinite(s[0]).all() and torch.isnan(s[1:]).all()
    gd, ga = torch.autograd.grad(s[:, 0], [md, ma], torch.full((6,), 0.5, device=dev()))
    assert gd[0].any() and not gd[1:].any() and not ga[1:].any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,L", [(7, 9), (33, 40), (5, 80), (3, 254)])
def test_gold_rule_score_and_adjoint(B, L, dtype):
    from vlgae_amd import rules1o
    rng = np.random.default_rng(L)
    lengths = rng.integers(1, L + 1, B)
    lengths[0] = L
    arc = _random_arcs(rng, lengths, L)
    arc[1, 0] = 0                                                   # several roots
    N = L + 1
    md, ma = _potentials(B, N, L, dtype)
    md, ma = md.requires_grad_(), ma.requires_grad_()
    s = rules1o.gold_rule_score(md, ma, t(arc), t(lengths))
    assert s.shape == (B, 1) and s.dtype == torch.float32
    cd, ca = merged_counts(arc, lengths, N)
    md64, ma64 = md.detach().double().cpu().numpy(), ma.detach().double().cpu().numpy()
    want = (np.where(cd != 0, cd * md64, 0).reshape(B, -1).sum(1) + np.where(ca != 0, ca * ma64, 0).reshape(B, -1).sum(1))
    assert np.isfinite(want).all()
    assert np.abs(s[:, 0].detach().cpu().numpy() - want).max() <= 1e-6 * max(1.0, np.abs(want).max())
    # the adjoint: g[b] * counts, every element written, in the potentials' dtype -- per-sentence g and the expanded scalar of .sum()
    gvec = torch.randn(B, generator=torch.Generator().manual_seed(1)).to(dev())
    for seed_grad, gcol in ((gvec.view(B, 1), gvec.view(B, 1)), (None, torch.ones(B, 1, device=dev()))):
        if seed_grad is None:
            gd, ga = torch.autograd.grad(s.sum(), [md, ma], retain_graph=True)
        else:
            gd, ga = torch.autograd.grad(s, [md, ma], seed_grad, retain_graph=True)
        assert gd.dtype == dtype and ga.dtype == dtype
        wd = (torch.from_numpy(cd).float().to(dev()) * gcol.view(B, 1, 1, 1, 1)).to(dtype)
        wa = (torch.from_numpy(ca).float().to(dev()) * gcol.view(B, 1, 1, 1)).to(dtype)
        assert torch.equal(gd, wd) and torch.equal(ga, wa)


@pytest.mark.parametrize("L", [9, 40, 60])
def test_partition_pass_is_remembered_bit_equal(L):
    """marginals_and_heads(keep_partition=True): the pair launch (N <= 44) or the two-stream form writes grad_dec, and `.partition` +
    autograd.grad of the same potentials then launch nothing and equal a fresh vlg_dmv1o_inside_outside, bit for bit."""
    import vlgae_amd.torch_struct as ts
    from vlgae_amd.torch_struct import functional as F
    from vlgae_amd import _C
    B = 16
    md, ma = _potentials(B, L + 1, 3)
    lengths = torch.randint(1, L + 1, (B,), generator=torch.Generator().manual_seed(L)).to(dev())
    F.viterbi_forget()
    lz0, gd0, ga0 = F.dmv1o_run(md, ma, lengths, _C.SEMIRING_LOG, True)                # vlg_dmv1o_inside_outside
    marg, heads = ts.DMV1o([md, ma], lengths).marginals_and_heads(keep_partition=True)
    assert torch.equal(marg, ga0)
    lz, gd, ga = F._partition_lookup(md, ma, lengths)
    assert torch.equal(lz, lz0) and torch.equal(gd, gd0) and torch.equal(ga, ga0)
    d, a = md.detach().requires_grad_(), ma.detach().requires_grad_()
    part = ts.DMV1o([d, a], lengths).partition
    g = torch.randn(B, 1, generator=torch.Generator().manual_seed(2)).to(dev())
    gd1, ga1 = torch.autograd.grad(part, [d, a], g)
    F.viterbi_forget()
    assert F._partition_lookup(md, ma, lengths) is None
    d2, a2 = md.detach().requires_grad_(), ma.detach().requires_grad_()
    part2 = ts.DMV1o([d2, a2], lengths).partition
    gd2, ga2 = torch.autograd.grad(part2, [d2, a2], g)
    assert torch.equal(part, part2) and torch.equal(gd1, gd2) and torch.equal(ga1, ga2)
    ma.add_(0.0)                                                     # an in-place update invalidates the entry
    ts.DMV1o([md, ma], lengths).marginals_and_heads(keep_partition=True)
    ma.add_(0.0)
    assert F._partition_lookup(md, ma, lengths) is None
    F.viterbi_forget()


def _fixture_step(g, dtype, monkeypatch, dep_loss):
    from vlgae_amd import train_step
    real = train_step.build
    extra = dict(arc=torch.from_numpy(g["arc"])) if dep_loss == "gold_rules" else {}
    monkeypatch.setattr(train_step, "build", lambda *a, given, **k: real(*a, given=dict(given, **extra), dep_loss=dep_loss, **k))
    try:
        return trainstep_from_fixture(g, dtype)
    finally:
        monkeypatch.setattr(train_step, "build", real)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16_forced"])
@pytest.mark.parametrize("path", golden_files("initstep_") + golden_files("margstep_"),
                         ids=golden_ids("initstep_") + golden_ids("margstep_"))
def test_step_matches_the_reference(path, dtype, monkeypatch):
    """initstep_*: the reference's init-epoch step (enll of random gold trees); margstep_*: its marginal-loss step.  f32: the bounds of
    test_training_step_reference_wiring (values 1e-4, loss 1e-5 relative, gradients 3e-4 * max|g| with the 1e-6 * max floor).  bf16:
    teacher-forced on the reference's Viterbi tree (the dep term no longer depends on the tree in these modes, only
    lang_feat_max_tree's input does): loss to 1e-2 relative, every gradient 0.12 relative L2 on the hot path and 0.3 for the parser's
    feed-forwards (bounds of ..._teacher_forced, observed here: see the printed worst errors)."""
    g = load(path)
    init = "initstep_" in path
    f32 = dtype == torch.float32
    with torch.autograd.set_multithreading_enabled(False):
        step, ref = _fixture_step(g, dtype, monkeypatch, "gold_rules" if init else "partition")
        if not f32:
            step.forced_heads = t(g["predicted"]).long()
        loss, grads, _ = step()
    last = step.last
    npf = lambda x: x.detach().float().cpu().numpy()
    assert last["viterbi_max"] is None and last["dep_score"].shape == (len(g["lengths"]), 1)
    heads = last["heads"].cpu().numpy()
    if f32:
        assert np.array_equal(heads, g["predicted"])
    ltol = 1e-5 if f32 else 1e-2
    dep = -float(last["dep_score"].double().sum())
    want_dep = float(g["enll"] if init else g["dep_loss"])
    assert abs(dep - want_dep) <= ltol * abs(want_dep), (dep, want_dep)
    assert abs(float(loss) - float(g["loss"])) <= ltol * abs(float(g["loss"])), (float(loss), float(g["loss"]))
    vtol = 1e-4 if f32 else 3e-2
    for name in ("txt", "txt_marginal", "vis_feat", "x_fused"):
        assert np.abs(npf(last[name]) - g[name]).max() <= (2e-2 if name == "txt_marginal" and not f32 else vtol) * max(1.0, np.abs(g[name]).max()), name
    gmax = max(float(np.abs(v).max()) for v in list(ref.values()) + [g["g_w1_sample"] if ref["w1"] is None else ref["w1"]] if v is not None)
    worst = {}
    for k in step.names:
        got = npf(grads[k])
        got, want = (got[::5, ::7, ::3], g["g_w1_sample"]) if k == "w1" and ref[k] is None else (got, ref[k])
        assert got.shape == want.shape, k
        if f32:
            err = max(np.abs(got - want).max() - 1e-6 * gmax, 0.0) / max(np.abs(want).max(), 1e-12)
            assert err <= 3e-4, (k, err)
        else:
            floor = 2e-3 * gmax * np.sqrt(want.size)
            err = max(np.linalg.norm((got - want).ravel()) - floor, 0.0) / max(np.linalg.norm(want.ravel()), 1e-12)
            assert err <= (0.3 if k.startswith("ff.") or k.endswith("_emb") else 0.12), (k, err)
        worst[k] = err
    print("worst gradient errors:", {k: float(f"{v:.2e}") for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:6]})


def _count_formulation(md, ma, arc, lengths):
    """Test-local: the gold score as float64 torch ops, count . potential over the positions with a nonzero count."""
    N = md.shape[1]
    cd, ca = merged_counts(arc.cpu().numpy(), lengths.cpu().numpy(), N)
    cd, ca = torch.from_numpy(cd).to(md.device), torch.from_numpy(ca).to(md.device)
    sd = torch.where(cd != 0, cd * md.double(), torch.zeros((), dtype=torch.float64, device=md.device))
    sa = torch.where(ca != 0, ca * ma.double(), torch.zeros((), dtype=torch.float64, device=md.device))
    return (sd.flatten(1).sum(1) + sa.flatten(1).sum(1)).float().view(-1, 1)


@pytest.mark.parametrize("factors", [(), ("rel", "attr", "img")], ids=["objects", "shipped"])
def test_init_step_config_size(factors, monkeypatch):
    """B = 256, L = 40, R = 36 in float32: the init step against the SAME step whose dep term is the float64 torch count . potential
    formulation above (everything else identical: same seed, same dropout draws).  Loss to 1e-6 relative, per-sentence scores to 1e-6,
    gradients to 1e-5 * max|g| (the dep term's adjoint is g * counts on both sides; the rest of the chain is the same code)."""
    from vlgae_amd import rules1o, train_step
    B, L, R = 256, 40, 36
    gen = torch.Generator().manual_seed(4)
    lengths = torch.randint(L // 2, L + 1, (B,), generator=gen)
    lengths[0] = L
    arc = torch.from_numpy(_random_arcs(np.random.default_rng(4), lengths.numpy(), L))
    runs = []
    with torch.autograd.set_multithreading_enabled(False):
        for formulation in ("kernel", "float64"):
            if formulation == "float64":
                monkeypatch.setattr(rules1o, "gold_rule_score", lambda md, ma, a, n: _count_formulation(md, ma, a, n))
            step = train_step.build(B, L, R, dev(), dtype=torch.float32, factors=factors, seed=9, dep_loss="gold_rules",
                                    given=dict(lengths=lengths.clone(), arc=arc.clone()))
            loss, grads, _ = step()
            runs.append((float(loss), step.last["dep_score"].clone(), {k: v.clone() for k, v in grads.items()}, step.names))
    (l0, s0, g0, names), (l1, s1, g1, _) = runs
    assert abs(l0 - l1) <= 1e-6 * abs(l1)
    assert torch.allclose(s0, s1, rtol=1e-6, atol=1e-6 * float(s1.abs().max()))
    gmax = max(float(v.abs().max()) for v in g1.values())
    for k in names:
        assert torch.isfinite(g0[k]).all(), k
        assert float((g0[k] - g1[k]).abs().max()) <= 1e-5 * gmax, k


def _batch(gen, B, L, R, T=45):
    lengths = torch.randint(L // 2, L + 1, (B,), generator=gen)
    lengths[0] = L
    n_box = torch.randint((3 * R) // 5, R + 1, (B,), generator=gen)
    return dict(lengths=lengths, token=torch.randint(0, T, (B, L), generator=gen), tag=torch.randint(0, 7, (B, L), generator=gen),
                box_mask=torch.arange(R)[None] < n_box[:, None],
                arc=torch.from_numpy(_random_arcs(np.random.default_rng(int(torch.randint(0, 1000, (1,), generator=gen))), lengths.numpy(), L)))


_NODROP = dict(p_drop=0.0, p_enc=0.0, p_ff_drop=0.0, p_mid_drop=0.0)


def test_init_step_in_place_batches_equal_fresh_builds():
    """batch_on_device=True with dep_loss="gold_rules": four batches copied into the step's own tensors (arc included) with SGD updates of
    the parameters in place between them; each step equals a fresh build on that batch and those parameters (eager; no dropout so
    that the two draw nothing).  Loss and per-sentence scores bit for bit, gradients to one float32 ulp of their largest entry
    (torch's gather backward is an order-dependent scatter-add)."""
    from vlgae_amd import train_step
    B, L, R = 24, 12, 8
    kw = dict(dtype=torch.float32, E=64, H=64, nb=16, n_vis=64, h=64, d=32, **_NODROP)
    gen = torch.Generator().manual_seed(8)
    with torch.autograd.set_multithreading_enabled(False):
        first = {k: v.to(dev()) for k, v in _batch(gen, B, L, R).items()}
        proto = train_step.build(B, L, R, dev(), dep_loss="gold_rules", given=dict(first), **kw)
        P = {k: v.detach() for k, v in proto.P.items()}
        step = train_step.build(B, L, R, dev(), dep_loss="gold_rules", batch_on_device=True, given=dict(P, **first), **kw)
        for it in range(4):
            nxt = {k: v.to(dev()) for k, v in _batch(gen, B, L, R).items()}
            for k, dst in (("lengths", step.lengths), ("token", step.batch["token"]), ("tag", step.batch["tag"]),
                           ("box_mask", step.batch["box_mask"]), ("arc", step.arc)):
                dst.copy_(nxt[k])
            loss, grads, _ = step()
            fresh = train_step.build(B, L, R, dev(), dep_loss="gold_rules", given=dict({k: v.clone() for k, v in P.items()}, **nxt), **kw)
            loss_f, grads_f, _ = fresh()
            assert torch.equal(loss, loss_f), it
            assert torch.equal(step.last["dep_score"], fresh.last["dep_score"]), it
            for k in step.names:
                assert torch.allclose(grads[k], grads_f[k], rtol=0, atol=2.0 ** -23 * 4 * float(grads_f[k].abs().max())), (it, k)
            with torch.no_grad():
                for k in step.trainable:
                    P[k].sub_(1e-2 * grads[k].to(P[k].dtype))


def test_init_step_as_one_hip_graph():
    """The init step captured as ONE HIP graph (gold_rule_score and its adjoint are capturable: no host synchronisation, no
    allocation) and replayed on unchanged inputs: the eager step's loss and per-sentence scores bit for bit, gradients to one bf16 ulp
    (the tolerance of test_training_step_chain_as_one_hip_graph: torch's gather backward is an order-dependent scatter-add)."""
    from vlgae_amd import train_step
    B, L, R = 64, 24, 20
    gen = torch.Generator().manual_seed(5)
    batch = _batch(gen, B, L, R)
    with torch.autograd.set_multithreading_enabled(False):
        step = train_step.build(B, L, R, dev(), dtype=torch.bfloat16, E=96, H=64, nb=24, n_vis=256, dep_loss="gold_rules", given=batch,
                                **_NODROP)
        for _ in range(2):
            total, grads, _ = step()
        want = [total.detach().clone(), step.last["dep_score"].clone()] + [grads[k].clone() for k in step.names]
        del total, grads
        gr = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(device=dev())
        side.wait_stream(torch.cuda.current_stream(dev()))
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream(dev()).wait_stream(side)
        with torch.cuda.graph(gr):
            total_g, grads_g, _ = step()
            score_g = step.last["dep_score"]
        for _ in range(2):
            gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(total_g.detach(), want[0]) and torch.equal(score_g, want[1])
        for k, b in zip(step.names, want[2:]):
            a = grads_g[k]
            assert torch.allclose(a.float(), b.float(), rtol=2.0 ** -7, atol=2.0 ** -7 * float(b.float().abs().max())), k
