"""GPU: the training step's per-batch data on the device -- vlg_step_batch_prepare against the torch formulation it replaces, the grounding
loss with its normaliser in device memory, and `train_step.build(batch_on_device=True)` against the default build on every batch, including
new batches copied into the tensors of a step built once."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHIPPED = ("rel", "attr", "img")
KW = dict(E=96, H=64, nb=24, n_vis=256)      # small feed-forward / feature widths; d = 128, h = 256 and the factor layout as shipped


def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("B", [1, 7, 64])
@pytest.mark.parametrize("L", [1, 10, 50])
@pytest.mark.parametrize("R", [5, 35])
@pytest.mark.parametrize("factors", [(), SHIPPED])
def test_batch_prepare_is_bit_equal_to_the_torch_formulation(B, L, R, factors):
    from vlgae_amd import align, encoders
    g = torch.Generator().manual_seed(B * 1000 + L * 10 + R)
    lengths = torch.randint(1, L + 1, (B,), generator=g).to(dev())
    tag = torch.randint(0, 200, (B, L), generator=g)                                  # ids above 63 and in no set
    tag[:, ::3] = torch.randint(0, 5, tag[:, ::3].shape, generator=g)                # and many inside the sets
    tag = tag.to(dev())
    box = (torch.rand(B, R, generator=g) < 0.7).to(dev())
    pos_for = dict(obj=torch.tensor([0, 1, 2, 70]), rel=torch.tensor([2, 3, 130]), attr=torch.tensor([4, 64]))
    pos_for = {k: t.to(dev()) for k, t in pos_for.items()}
    add = ("rel" in factors, "attr" in factors, "img" in factors)
    _, V, split, names = encoders.factor_layout(R, *add)
    Q = 2 * (L + 1)
    vm = torch.empty((B, V), dtype=torch.bool, device=dev())
    pen = torch.empty((B, Q, len(split)), dtype=torch.float32, device=dev())
    nt, coef, seed = (torch.empty(s, dtype=torch.float32, device=dev()) for s in ((), (2,), (B,)))

    def poison():   # every output element must be written by the launch: start from bytes no correct result has
        vm.view(torch.uint8).fill_(0xFF)
        for t in (pen, nt, coef, seed):
            t.fill_(float("nan"))
    for alpha in (0.5, 0.3):
        poison()
        align.step_batch_prepare(lengths, tag, box, factors, pos_for, Q, alpha, vm, pen, nt, coef, seed)
        want_pen, _ = align.grounding_prior(tag, names, split, pos_for, Q)
        num_token = lengths.sum()
        want_coef = torch.tensor([alpha, -(1.0 - alpha)], dtype=torch.float32, device=dev()) / (num_token.to(torch.float32) + 1e-12)
        assert torch.equal(vm.view(torch.uint8), encoders.factor_mask(box, *add).view(torch.uint8))   # (bytes: 0 / 1, not any non-zero)
        assert torch.equal(pen, want_pen)
        assert torch.equal(nt, num_token.to(torch.float32)) and float(nt) == float(num_token.item())
        assert torch.equal(coef, want_coef) and torch.equal(seed, want_coef[1].repeat(B))
    # no prior: the table is not written, everything else is
    box2 = ~box
    poison()
    align.step_batch_prepare(lengths, tag, box2, factors, pos_for, Q, 0.25, vm, None, nt, coef, seed)
    want_coef = torch.tensor([0.25, -0.75], dtype=torch.float32, device=dev()) / (lengths.sum().to(torch.float32) + 1e-12)
    assert torch.equal(vm.view(torch.uint8), encoders.factor_mask(box2, *add).view(torch.uint8))
    assert torch.equal(coef, want_coef) and torch.equal(seed, want_coef[1].repeat(B)) and float(nt) == float(lengths.sum().item())
    assert torch.isnan(pen).all()


def test_grounding_loss_with_device_num_token_is_bit_equal():
    from vlgae_amd import align, encoders
    g = torch.Generator().manual_seed(3)
    B, L, R = 6, 9, 5
    Q = 2 * (L + 1)
    _, V, split, names = encoders.factor_layout(R)
    pos_for = {k: t.to(dev()) for k, t in dict(obj=torch.tensor([0, 1]), rel=torch.tensor([2]), attr=torch.tensor([4])).items()}
    for dt in (torch.bfloat16, torch.float32):
        txt = torch.randn(B, Q, 128, generator=g).to(dev(), dt).requires_grad_(True)
        vis = torch.randn(B, V, 128, generator=g).to(dev(), dt).requires_grad_(True)
        tmask = (torch.rand(B, Q, generator=g) < 0.8).to(dev())
        vmask = encoders.factor_mask((torch.rand(B, R, generator=g) < 0.7).to(dev()))
        marg = torch.rand(B, Q, generator=g).to(dev())
        pen, seg = align.grounding_prior(torch.randint(0, 6, (B, L), generator=g).to(dev()), names, split, pos_for, Q)
        out = []
        for nt in (37.0, torch.tensor(37.0, device=dev())):
            total, sums = align.grounding_loss_factor_ce(txt, vis, tmask, vmask, marg, nt, 1.0, pen, seg)
            out.append((sums.clone(), *torch.autograd.grad(total, [txt, vis])))
        for a, b in zip(*out):
            assert torch.equal(a, b)


def make_batch(g, lengths, R, dtype=torch.bfloat16, T=45, n_tag=9):
    lengths = torch.as_tensor(lengths, dtype=torch.int64)
    B, L = len(lengths), int(lengths.max())
    n_box = torch.randint(max(1, R // 2), R + 1, (B,), generator=g)
    return dict(emb=(torch.randn(B, L, KW["E"], generator=g) * 0.5).to(dtype).to(dev()),
                vis_box_feat=(torch.randn(B, R, KW["n_vis"], generator=g) * 0.5).to(dtype).to(dev()),
                box_mask=(torch.arange(R)[None] < n_box[:, None]).to(dev()), lengths=lengths.to(dev()),
                token=torch.randint(0, T, (B, L), generator=g).to(dev()), tag=torch.randint(0, n_tag, (B, L), generator=g).to(dev()))


def run(step):
    loss, grads, _ = step()
    return loss.clone(), {k: v.clone() for k, v in grads.items()}, {k: step.last[k].clone() for k in ("merged_dec", "merged_attach", "heads", "sums")}


def same(got, want, tol):
    """loss, merged potentials, heads, grounding sums bit for bit; gradients to `tol` relative (torch's gather backward is an atomic
    scatter-add, order-dependent from run to run: one ulp of the gradient's type)."""
    assert torch.equal(got[0], want[0]), (float(got[0]), float(want[0]))
    for k in want[2]:
        assert torch.equal(got[2][k], want[2][k]), k
    assert set(got[1]) == set(want[1])
    for k, b in want[1].items():
        a, b = got[1][k].float(), b.float()
        assert torch.allclose(a, b, rtol=tol, atol=tol * float(b.abs().max())), k


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_batch_on_device_step_equals_the_default_step_on_every_batch(dtype):
    """ONE step built with batch_on_device=True, fed four batches of its shape by copying them into its tensors (different lengths, tags,
    box masks, features), against a default build on each batch with the dropout generator at the same state: nothing of the first batch
    survives in the step.  Live dropout (every rate as shipped), the shipped factor layout."""
    from vlgae_amd import encoders, train_step
    g = torch.Generator().manual_seed(12)
    R = 6
    batches = [make_batch(g, [9, 3, 7, 9, 1], R, dtype), make_batch(g, [2, 9, 9, 5, 4], R, dtype, n_tag=200),
               make_batch(g, [1, 1, 1, 1, 9], R, dtype), make_batch(g, [9, 3, 7, 9, 1], R, dtype)]
    batches[1]["box_mask"][:, 1::2] = False
    rng = encoders.DeviceRng(5, dev())
    statics = {k: v.clone() for k, v in batches[0].items()}
    step = train_step.build(5, 9, R, dev(), dtype=dtype, factors=SHIPPED, given=dict(statics), rng=rng, batch_on_device=True, **KW)
    params = {k: step.P[k].detach().clone() for k in step.trainable}
    assert all(step.P[k].data_ptr() == statics[k].data_ptr() for k in ("emb", "vis_box_feat"))   # used in place
    for i, batch in enumerate(batches):
        for k, v in batch.items():
            statics[k].copy_(v)
        state = rng.state.clone()
        got = run(step)
        assert int(rng.state[1]) == int(state[1]) + 1
        ref_rng = encoders.DeviceRng(0, dev())
        ref_rng.state.copy_(state)
        ref = train_step.build(5, 9, R, dev(), dtype=dtype, factors=SHIPPED, given=dict(batch, **params), rng=ref_rng, **KW)
        same(got, run(ref), 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -16)
        del ref
        with torch.no_grad():   # an in-place parameter update reaches the next step
            for k in ("w_vis", "b_enc", "ff.head_ff.linear.weight"):
                step.P[k].mul_(0.9)
                params[k].mul_(0.9)


def test_batch_on_device_refuses_tensors_it_would_copy():
    """A given tensor the step would have to convert keeps its build-time values for ever: batch_on_device=True refuses it."""
    from vlgae_amd import train_step
    g = torch.Generator().manual_seed(14)
    batch = make_batch(g, [4, 2, 3], 5)
    ok = train_step.build(3, 4, 5, dev(), factors=SHIPPED, given=dict(batch), batch_on_device=True, **KW)
    w_vis = ok.P["w_vis"].detach()
    for k, v in (("lengths", batch["lengths"].to(torch.int32)), ("box_mask", batch["box_mask"].to(torch.uint8)), ("emb", batch["emb"].float()),
                 ("tag", batch["tag"].cpu()), ("w_vis", w_vis.float()), ("ff.head_ff.linear.weight", ok.P["ff.head_ff.linear.weight"].detach().float())):
        given = dict(batch, **{k: v})
        if k.startswith("ff."):
            given.update({n: ok.P[n].detach() for n in ok.P if n.startswith("ff.") or n in ("token_emb", "root_emb", "dec_emb")}, **{k: v})
        with pytest.raises(ValueError, match="copied"):
            train_step.build(3, 4, 5, dev(), factors=SHIPPED, given=given, batch_on_device=True, **KW)
        train_step.build(3, 4, 5, dev(), factors=SHIPPED, given=given, **KW)   # the default build converts, as before


def test_default_build_takes_a_shared_generator():
    """rng=: the step draws from (and advances) the caller's generator; two steps on one generator follow the step count."""
    from vlgae_amd import encoders, train_step
    g = torch.Generator().manual_seed(13)
    rng = encoders.DeviceRng(9, dev())
    a = train_step.build(4, 6, 5, dev(), factors=SHIPPED, given=make_batch(g, [6, 2, 3, 6], 5), rng=rng, **KW)
    b = train_step.build(3, 4, 5, dev(), factors=SHIPPED, given=make_batch(g, [4, 1, 2], 5), rng=rng, **KW)
    for s in (a, b, a, b):
        s()
    assert int(rng.state[1]) == 4
