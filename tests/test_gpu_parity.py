"""GPU parity tests proper: the HIP path (through the C ABI / the drop-in Python API) against
  (1) golden vectors produced by the reference itself (tests/golden/*.npz),
  (2) the CPU oracle on fresh seeded inputs,
  (3) size-independent properties at BASELINE.json's full sizes.

Tolerances (floating point; stated per check):
  logZ      |err| <= 2e-5 * max(1, |logZ|)   vs fp64 reference   (fp32 charts: 1 ulp at |logZ|~170 is 1.5e-5)
  marginals max-abs-err <= 1e-4 (north-star bound); we assert the tighter 5e-5.  (fp32 charts: at |logZ| ~ 170
            one ulp of a chart value is 1.5e-5 and weights are exp(t - out); the REFERENCE's own fp32 path deviates
            1.7e-5 from its fp64 path on the hardest fixture, dmv_B4_L40_s1_full.)
  Max semiring: best-tree indicators bit-exact, scores to 1e-5 relative
"""
import numpy as np
import pytest
import torch

from conftest import golden_files, golden_ids, load

pytestmark = pytest.mark.gpu

MARG_TOL = 5e-5


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return x if dtype is None else x.to(dtype)


def logz_tol(ref):
    return 2e-5 * np.maximum(1.0, np.abs(ref))


@pytest.fixture(scope="module")
def ts():
    import vlgae_amd.torch_struct as ts
    from vlgae_amd import _C
    _C.lib()   # must load: the product has no fallback
    return ts


def test_xlane_primitives():
    """DPP quad-perm / row mirrors / ds_swizzle must act like an xor-butterfly on block-uniform data."""
    from vlgae_amd import _C
    scratch = torch.full((1,), -1, dtype=torch.int32, device=dev())
    _C.check(_C.lib().vlg_selftest_xlane(_C.ptr(scratch), _C.stream_of(scratch)), "selftest_xlane")
    assert int(scratch.item()) == 0, f"lane-exchange self-test failed, mask {int(scratch.item()):#x}"


# ------------------------------------------------------------------------------------------------ DMV1o
@pytest.mark.parametrize("path", golden_files("dmv_"), ids=golden_ids("dmv_"))
def test_dmv1o_golden(ts, path):
    g = load(path)
    dec, attach, root, lengths = t(g["dec"]), t(g["attach"]), t(g["root"]), t(g["lengths"])
    mdec, mattach = ts.DMV1o.merge(dec, attach, root)
    if "merged_dec" in g:   # merge is fill/copy: bit-exact
        assert torch.equal(mdec.cpu(), torch.from_numpy(g["merged_dec"]))
        assert torch.equal(mattach.cpu(), torch.from_numpy(g["merged_attach"]))
    # the call pattern of joint.py:251-256 / ldndmv.py:289-303
    with torch.enable_grad():
        d = mdec.detach().requires_grad_()
        a = mattach.detach().requires_grad_()
        dist = ts.DMV1o([d, a], lengths)
        logZ = dist.partition
        assert tuple(logZ.shape) == (len(g["lengths"]), 1)
        gd, ga = torch.autograd.grad(logZ.sum(), [d, a])
    assert np.all(np.abs(logZ.detach().cpu().numpy() - g["logZ64"]) <= logz_tol(g["logZ64"]))
    assert np.abs(gd.detach().cpu().numpy() - g["grad_dec64"]).max() <= MARG_TOL
    assert np.abs(ga.detach().cpu().numpy() - g["grad_attach64"]).max() <= MARG_TOL
    assert np.abs(ga.sum(-1).detach().cpu().numpy() - g["arc_marginal"]).max() <= MARG_TOL
    # padded positions: exactly zero
    for b, ln in enumerate(g["lengths"]):
        assert float(ga[b, ln + 1:].abs().max() if ln + 1 < ga.shape[1] else 0) == 0.0
        assert float(ga[b, :, ln + 1:].abs().max() if ln + 1 < ga.shape[1] else 0) == 0.0

    # Max semiring: value, one-hot gradient, argmax property, predicted heads (joint.py:256-258)
    with torch.enable_grad():
        d = mdec.detach().requires_grad_()
        a = mattach.detach().requires_grad_()
        dist = ts.DMV1o([d, a], lengths)
        mx = dist.max
        mgd, mga = torch.autograd.grad(mx.sum(), [d, a])
        am = dist.argmax
    assert np.allclose(mx.detach().cpu().numpy(), g["max"], rtol=1e-5, atol=1e-5)
    assert np.array_equal(mgd.detach().cpu().numpy(), g["maxgrad_dec"])
    assert np.array_equal(mga.detach().cpu().numpy(), g["maxgrad_attach"])
    assert np.array_equal(am.detach().cpu().numpy(), g["argmax"])
    arc = am.sum(-1).nonzero()
    predicted = lengths.new_zeros(len(g["lengths"]), g["dec"].shape[1] + 1)
    predicted[arc[:, 0], arc[:, 2]] = arc[:, 1]
    assert np.array_equal(predicted.detach().cpu().numpy(), g["predicted"])
    # .marginals lazy property == attach gradient
    assert np.abs(dist.marginals.detach().cpu().numpy() - g["marginals"]).max() <= MARG_TOL

    # weighted upstream gradient (grad_logZ scaling) through .backward()
    d = mdec.detach().requires_grad_()
    a = mattach.detach().requires_grad_()
    (ts.DMV1o([d, a], lengths).partition.squeeze(-1) * t(g["wts"])).sum().backward()
    assert np.abs(d.grad.detach().cpu().numpy() - g["wgrad_dec"]).max() <= 2 * MARG_TOL
    assert np.abs(a.grad.detach().cpu().numpy() - g["wgrad_attach"]).max() <= 2 * MARG_TOL

    # MBR chain (ldndmv.py:294-299): DependencyCRF over arc marginals, Max semiring.
    # Fed with the REFERENCE's marginals so that near-ties cannot flip on 1e-6 differences.
    crf = ts.DependencyCRF(t(g["arc_marginal"]), lengths)
    assert np.array_equal(crf.argmax.detach().cpu().numpy(), g["mbr_argmax"])
    mbr_heads = np.zeros(g["predicted"].shape, np.int64)
    bb, hh, cc = np.nonzero(g["mbr_argmax"])
    mbr_heads[bb, cc] = hh
    assert np.array_equal(crf.argmax_heads.cpu().numpy(), mbr_heads)
    assert np.allclose(crf.max.detach().cpu().numpy(), g["mbr_max"], rtol=1e-5, atol=1e-5)


def test_dmv1o_no_grad_and_bf16(ts, oracle_mod):
    g = load(golden_files("dmv_B8_L40_s0")[0])
    md, ma = oracle_mod.dmv1o_merge(g["dec"], g["attach"], g["root"])
    lengths = t(g["lengths"])
    with torch.no_grad():   # inside-only kernel
        lz = ts.DMV1o([t(md), t(ma)], lengths).partition
    assert np.all(np.abs(lz.detach().cpu().numpy() - g["logZ64"]) <= logz_tol(g["logZ64"]))
    # bf16 potentials: parity is defined against the reference algorithm on the SAME bf16-rounded inputs
    md16, ma16 = t(md).bfloat16(), t(ma).bfloat16()
    ref_lz, ref_gd, ref_ga = oracle_mod.dmv1o(md16.float().detach().cpu().numpy(), ma16.float().detach().cpu().numpy(), g["lengths"],
                                              "log", np.float64)
    d = md16.detach().requires_grad_()
    a = ma16.detach().requires_grad_()
    lz = ts.DMV1o([d, a], lengths).partition
    gd, ga = torch.autograd.grad(lz.sum(), [d, a])
    assert lz.dtype == torch.float32   # charts / outputs stay fp32
    assert np.all(np.abs(lz.detach().cpu().numpy() - ref_lz) <= logz_tol(ref_lz))
    assert np.abs(ga.float().detach().cpu().numpy() - ref_ga).max() <= 4e-3   # gradient cast back to bf16 (8 bits)
    from vlgae_amd.torch_struct import functional as F
    _, gd32, ga32 = F.dmv1o_run(md16, ma16, lengths, 0, True)
    assert np.abs(gd32.detach().cpu().numpy() - ref_gd).max() <= MARG_TOL
    assert np.abs(ga32.detach().cpu().numpy() - ref_ga).max() <= MARG_TOL


@pytest.mark.parametrize("B,L,seed", [(64, 40, 11), (16, 63, 12), (8, 80, 13), (4, 120, 14), (33, 5, 15), (2, 254, 16)])
def test_dmv1o_vs_oracle_random(ts, oracle_mod, B, L, seed):
    """Fresh seeded inputs at sizes the oracle finishes in seconds.  The placement follows the padded width N = L + 1
    (vlg_dp_core.h: DmvLayout): N = 6 and 41 run the short image with everything in LDS; N = 64 and 81 the Log overlay
    (mode 1; the Max walk keeps everything in LDS at 64 and moves gI to the workspace at 81); N = 121 and the maximum
    supported size N = 255 Log mode 3 / walk mode 2, and there the inside-only launch keeps C and I in the workspace.
    None of these widths is next to a boundary: tests/test_dmv_placements_gpu.py sits on both sides of each."""
    rng = np.random.default_rng(seed)
    dec = rng.standard_normal((B, L, 2, 2, 2)).astype(np.float32)
    dec = dec - np.log(np.exp(dec).sum(-1, keepdims=True))
    attach = rng.standard_normal((B, L, L, 2)).astype(np.float32)
    root = rng.standard_normal((B, L)).astype(np.float32)
    lengths = rng.integers(1, L + 1, size=B)
    lengths[0] = L
    md, ma = oracle_mod.dmv1o_merge(dec, attach, root)
    for sr, name in ((0, "log"), (1, "max")):
        ref_lz, ref_gd, ref_ga = oracle_mod.dmv1o(md, ma, lengths, name, np.float64)
        from vlgae_amd.torch_struct import functional as F
        lz, gd, ga = F.dmv1o_run(t(md), t(ma), t(lengths), sr, True)
        lz0, _, _ = F.dmv1o_run(t(md), t(ma), t(lengths), sr, False)
        assert np.all(np.abs(lz.detach().cpu().numpy()[:, None] - ref_lz) <= logz_tol(ref_lz)), name
        assert torch.equal(lz, lz0), "inside-only and fused kernels must agree bit for bit"
        if sr == 0:
            assert np.abs(gd.detach().cpu().numpy() - ref_gd).max() <= MARG_TOL
            assert np.abs(ga.detach().cpu().numpy() - ref_ga).max() <= MARG_TOL
        else:   # best tree: compare as trees (ties have measure zero for continuous inputs)
            assert np.array_equal(ga.detach().cpu().numpy(), ref_ga.astype(np.float32))
            assert np.array_equal(gd.detach().cpu().numpy(), ref_gd.astype(np.float32))


@pytest.mark.parametrize("storage", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_dp_short_sentence_image_equals_general_image(ts, storage):
    """Round 5: for N <= 41 the host launches kernels whose span bodies are compiled for <= 3 split points per lane only (half the code
    image: 106 -> 53 KB for the headline kernel, 75.9 -> ~70 us).  Same arithmetic in the same order: the results must be BIT-identical to
    the general image, which the same sentences reach when their potentials are padded to N = 42 (same chart pitch, same lane groups).
    DMV1o Log (logZ, both count tensors), Max (score, tree counts, heads), the marginals + Viterbi pair launch, DepTree Log and Max."""
    from vlgae_amd.torch_struct import functional as Fn
    B, L = 192, 40
    N = L + 1
    gen = torch.Generator().manual_seed(31)
    dec = torch.randn(B, L, 2, 2, 2, generator=gen).log_softmax(-1).to(dev())
    attach = (torch.randn(B, L, L, 2, generator=gen) * 2).to(dev())
    root = torch.randn(B, L, generator=gen).log_softmax(-1).to(dev())
    lengths = torch.randint(1, L + 1, (B,), generator=gen)
    lengths[:3] = torch.tensor([L, 1, 2])
    lengths = lengths.to(dev())
    md, ma = ts.DMV1o.merge(dec, attach, root)
    md, ma = md.to(storage), ma.to(storage)
    md2 = torch.full((B, N + 1, 2, 2, 2), -7.0, device=dev(), dtype=storage)
    ma2 = torch.full((B, N + 1, N + 1, 2), -7.0, device=dev(), dtype=storage)
    md2[:, :N] = md
    ma2[:, :N, :N] = ma
    for sr in (0, 1):
        a = Fn.dmv1o_run(md, ma, lengths, sr, True)                     # (logZ, gdec, gatt): N = 41 -> the short image
        b = Fn.dmv1o_run(md2, ma2, lengths, sr, True)                   # N = 42 -> the general image
        assert torch.equal(a[0], b[0]), sr
        assert torch.equal(a[1], b[1][:, :N]) and torch.equal(a[2], b[2][:, :N, :N]), sr
        assert float(b[1][:, N:].abs().max()) == 0.0 and float(b[2][:, N:].abs().max()) == 0.0 and float(b[2][:, :, N:].abs().max()) == 0.0
        assert torch.equal(Fn.dmv1o_run(md, ma, lengths, sr, False)[0], Fn.dmv1o_run(md2, ma2, lengths, sr, False)[0])   # inside only
    m1, h1 = ts.DMV1o([md, ma], lengths).marginals_and_heads()        # the pair launch
    m2, h2 = ts.DMV1o([md2, ma2], lengths).marginals_and_heads()
    assert torch.equal(m1, m2[:, :N, :N]) and torch.equal(h1, h2[:, :N])
    arc = ma[..., 0].float().contiguous()
    arc2 = ma2[..., 0].float().contiguous()
    for sr in (0, 1):
        a = Fn.deptree_run(arc, lengths, sr, True)
        b = Fn.deptree_run(arc2, lengths, sr, True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1][:, :N, :N]), sr


def test_dmv1o_properties_full_size(ts, oracle_mod):
    """BASELINE.json config 2 (B=256, L=40): size-independent identities, and a 12-sentence fp64-oracle
    slice of the full-size launch for both storage types of the potentials (the headline configuration stores bf16)."""
    B, L = 256, 40
    gen = torch.Generator(device="cpu").manual_seed(0)
    dec = torch.randn(B, L, 2, 2, 2, generator=gen).log_softmax(-1).to(dev())
    attach = torch.randn(B, L, L, 2, generator=gen).to(dev())
    root = torch.randn(B, L, generator=gen).log_softmax(-1).to(dev())
    lengths = torch.randint(1, L + 1, (B,), generator=gen)
    lengths[0] = L
    lengths = lengths.to(dev())
    md, ma = ts.DMV1o.merge(dec, attach, root)
    d, a = md.detach().requires_grad_(), ma.detach().requires_grad_()
    dist = ts.DMV1o([d, a], lengths)
    gd, ga = torch.autograd.grad(dist.partition.sum(), [d, a])
    lf = lengths.float()
    assert torch.allclose(ga.sum((1, 2, 3)), lf, atol=2e-4)                 # (ii) one head per word
    assert torch.allclose(gd.sum((1, 2, 3, 4)), 3 * lf + 1, atol=5e-4)      # (iii) decisions: 2 STOP + 1 GO per word, + root STOP
    col = ga.sum(-1).sum(1)                                                 # (iv) every word has exactly one head
    idx = torch.arange(L + 1, device=dev())[None]
    valid = (idx >= 1) & (idx <= lengths[:, None])
    assert torch.allclose(col[valid], torch.ones_like(col[valid]), atol=2e-4)
    assert float(col[~valid].abs().max()) == 0.0                            # (v) padding: exact zeros
    assert float(ga.min()) >= 0.0 and float(ga.max()) <= 1.0 + 1e-5
    # Max <= Log, and the best tree is a tree
    mx = ts.DMV1o([md, ma], lengths).max
    assert bool((mx <= dist.partition + 1e-4).all())
    am = ts.DMV1o([md, ma], lengths).argmax.sum(-1)
    assert torch.equal(am.sum(1)[valid], torch.ones_like(am.sum(1)[valid]))
    assert torch.equal(am[:, 0].sum(-1), torch.ones(B, device=dev()))       # single root
    # (i) dec == 0 and valence-independent attach  ==>  DMV1o == DependencyCRF on the same arcs
    arc = torch.randn(B, L + 1, L + 1, generator=gen).to(dev())
    z = torch.zeros(B, L + 1, 2, 2, 2, device=dev())
    lz_dmv = ts.DMV1o([z, arc[..., None].expand(-1, -1, -1, 2).contiguous()], lengths).partition.squeeze(-1)
    arc_crf = arc.clone()
    arc_crf[:, :, 0] = -1e12   # DMV never attaches the root as a child; CRF needs the same exclusion
    lz_crf = ts.DependencyCRF(arc_crf, lengths).partition
    # DMV's root has valence NOCHILD only for its single child; with valence-independent scores they coincide
    assert torch.allclose(lz_dmv, lz_crf, rtol=1e-5, atol=1e-3)
    # determinism: same launch twice, bit-identical (no atomics anywhere in the kernels)
    gd2, ga2 = torch.autograd.grad(ts.DMV1o([d, a], lengths).partition.sum(), [d, a])
    assert torch.equal(ga, ga2) and torch.equal(gd, gd2)
    # oracle slice of the B = 256 launch: sentences spread over the batch (first, last, ragged ones in between)
    pick = np.array([0, 1, 2, 3, 37, 64, 100, 127, 128, 200, 254, 255])
    for storage in (torch.float32, torch.bfloat16):
        sd, sa = md.to(storage), ma.to(storage)            # what the kernel reads; the oracle gets the same (rounded) values
        dd, aa = sd.detach().requires_grad_(), sa.detach().requires_grad_()
        lz = ts.DMV1o([dd, aa], lengths).partition
        g_d, g_a = torch.autograd.grad(lz.sum(), [dd, aa])
        rlz, rgd, rga = oracle_mod.dmv1o(sd[pick].float().cpu().numpy(), sa[pick].float().cpu().numpy(), lengths[pick].cpu().numpy(),
                                          "log", np.float64)
        rlz = np.asarray(rlz).reshape(-1)
        assert (np.abs(lz.detach().float().cpu().numpy()[pick, 0] - rlz) <= logz_tol(rlz)).all(), storage
        assert np.abs(g_a.float().cpu().numpy()[pick] - rga).max() <= (MARG_TOL if storage == torch.float32 else 4e-3), storage
        assert np.abs(g_d.float().cpu().numpy()[pick] - rgd).max() <= (MARG_TOL if storage == torch.float32 else 4e-3), storage
        if storage == torch.bfloat16:   # the counts themselves are fp32 inside the kernel; the API hands bf16 leaves bf16 gradients:
            from vlgae_amd.torch_struct import functional as F   # compare the kernel's fp32 counts at the north-star bound
            _, cd, ca = F.dmv1o_run(sd, sa, lengths, 0, True)
            assert np.abs(ca.cpu().numpy()[pick] - rga).max() <= MARG_TOL and np.abs(cd.cpu().numpy()[pick] - rgd).max() <= MARG_TOL


def test_dmv1o_batch_of_2048_equals_its_eight_shards(ts, oracle_mod):
    """BASELINE.json configs[2] on ONE GPU (B = 2048, L = 40, bf16 potentials; eight GPUs are the driver's to launch): the batch is sharded
    along dim 0 with no data-path exchange (`vlgae_amd.dist.shard_batch`), so the launch over all 2048 sentences must equal the eight
    256-sentence launches a node would run -- bit for bit, logZ and every expected count (a workgroup sees one sentence) -- the flat
    gradient buffer summed over the shards must equal the full batch's, and a slice spread over the shards meets the fp64 oracle."""
    from vlgae_amd import dist as vdist
    from vlgae_amd.torch_struct import functional as F
    B, L, W = 2048, 40, 8
    gen = torch.Generator().manual_seed(2048)
    md, ma = ts.DMV1o.merge(torch.randn(B, L, 2, 2, 2, generator=gen).log_softmax(-1).to(dev()), torch.randn(B, L, L, 2, generator=gen).to(dev()),
                            torch.randn(B, L, generator=gen).log_softmax(-1).to(dev()))
    dec, attach = md.bfloat16(), ma.bfloat16()
    lengths = torch.randint(L // 2, L + 1, (B,), generator=gen)
    lengths[::256] = L
    lengths = lengths.to(dev())
    lz, cd, ca = F.dmv1o_run(dec, attach, lengths, 0, True)
    total = torch.zeros_like(cd[0])
    for r in range(W):
        sd, sa, sl = vdist.shard_batch([dec, attach, lengths], r, W)
        s, e = vdist.shard_bounds(B, r, W)
        assert e - s == B // W
        z, gd, ga = F.dmv1o_run(sd.contiguous(), sa.contiguous(), sl.contiguous(), 0, True)
        assert torch.equal(z, lz[s:e]) and torch.equal(gd, cd[s:e]) and torch.equal(ga, ca[s:e]), r
        total += gd.sum(0)
    assert torch.allclose(total, cd.sum(0), rtol=1e-5, atol=1e-3)   # what the all-reduce of the shards' flat buffers adds up to
    pick = np.array([0, 255, 256, 777, 1024, 1500, 2047])
    rlz, rgd, rga = oracle_mod.dmv1o(dec[pick].float().cpu().numpy(), attach[pick].float().cpu().numpy(), lengths[pick].cpu().numpy(), "log", np.float64)
    rlz = np.asarray(rlz).reshape(-1)
    assert (np.abs(lz.float().cpu().numpy().reshape(B, -1)[pick, 0] - rlz) <= logz_tol(rlz)).all()
    assert np.abs(ca.cpu().numpy()[pick] - rga).max() <= MARG_TOL and np.abs(cd.cpu().numpy()[pick] - rgd).max() <= MARG_TOL


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_dmv1o_long_sentences_full_size(ts, oracle_mod, dt):
    """BASELINE.json configs[3] (B=256, L=80): the overlay placement (value charts in LDS for the inside pass, copied to
    the workspace, adjoints laid over them for the outside pass).  Size-independent identities on the whole batch, and
    parity with the fp64 oracle on a slice of it."""
    B, L = 256, 80
    gen = torch.Generator(device="cpu").manual_seed(80)
    dec = torch.randn(B, L, 2, 2, 2, generator=gen).log_softmax(-1)
    attach = torch.randn(B, L, L, 2, generator=gen)
    root = torch.randn(B, L, generator=gen).log_softmax(-1)
    lengths = torch.randint(1, L + 1, (B,), generator=gen)
    lengths[0], lengths[1], lengths[2] = L, 61, 62                       # full length and two long ones.  The placement follows the padded width
    # N = 81, not a sentence's length: every sentence of this batch runs in the overlay (mode 1).  The all-in-LDS boundary (N = 62 / 63)
    # and the others are in tests/test_dmv_placements_gpu.py.
    md, ma = ts.DMV1o.merge(dec.to(dev()), attach.to(dev()), root.to(dev()))
    if dt == "bf16":
        md, ma = md.bfloat16(), ma.bfloat16()
    lengths_d = lengths.to(dev())
    from vlgae_amd.torch_struct import functional as Fn
    # raw launcher: fp32 counts whatever the storage type (autograd would round them to the potentials' dtype)
    lz, gd, ga = Fn.dmv1o_run(md, ma, lengths_d, 0, True)
    lz = lz.reshape(B, 1)
    lf = lengths_d.float()
    assert bool(torch.isfinite(lz).all())
    assert torch.allclose(ga.sum((1, 2, 3)), lf, atol=1e-3)                 # one head per word
    assert torch.allclose(gd.sum((1, 2, 3, 4)), 3 * lf + 1, atol=2e-3)      # 2 STOP + 1 GO per word, + root STOP
    col = ga.sum(-1).sum(1)
    idx = torch.arange(L + 1, device=dev())[None]
    valid = (idx >= 1) & (idx <= lengths_d[:, None])
    assert torch.allclose(col[valid], torch.ones_like(col[valid]), atol=5e-4)
    assert float(col[~valid].abs().max()) == 0.0                            # padding: exact zeros
    assert float(ga.min()) >= 0.0 and float(ga.max()) <= 1.0 + 2e-5
    _, gd2, ga2 = Fn.dmv1o_run(md, ma, lengths_d, 0, True)
    assert torch.equal(ga, ga2) and torch.equal(gd, gd2)                    # bit-reproducible
    # inside-only launch (all charts in LDS at this length) gives the same logZ bits as the fused launch
    with torch.no_grad():
        assert torch.equal(ts.DMV1o([md, ma], lengths_d).partition, lz.detach())
    # oracle slice: the same (possibly bf16-rounded) potentials, fp64
    n = 12
    omd, oma = md[:n].float().cpu().numpy(), ma[:n].float().cpu().numpy()
    rlz, rgd, rga = oracle_mod.dmv1o(omd, oma, lengths[:n].numpy(), "log", np.float64)
    assert np.all(np.abs(lz[:n].detach().cpu().numpy().reshape(rlz.shape) - rlz) <= logz_tol(rlz))
    # fp32 charts at |logZ| ~ 300: one ulp of a chart value is 3e-5 (HISTORY.md section 6: 2e-4 at the peakiest L >= 62 cases)
    assert np.abs(ga[:n].cpu().numpy() - rga).max() <= 1e-4 and np.abs(gd[:n].cpu().numpy() - rgd).max() <= 2e-4
    # Viterbi at full size: a tree per sentence, single root
    heads_am = ts.DMV1o([md, ma], lengths_d).argmax.sum(-1)
    assert torch.equal(heads_am.sum(1)[valid], torch.ones_like(heads_am.sum(1)[valid]))
    assert torch.equal(heads_am[:, 0].sum(-1), torch.ones(B, device=dev()))


@pytest.mark.parametrize("L,scale", [(40, 6.0), (62, 6.0), (63, 6.0), (80, 2.0), (88, 6.0), (89, 6.0), (100, 6.0)],
                         ids=lambda v: str(v))
def test_dmv1o_long_peaky_sentences(ts, oracle_mod, L, scale):
    """tools/stress_dp.py's hardest cases in the suite: ragged batches in every Log placement -- N = L + 1 = 41
    the short image, 63 / 64 and 81 the overlay (mode 1), 89 / 90 and 101 mode 2; these are the first two widths BEYOND the boundaries
    62 / 63 and 88 / 89, the boundaries themselves are in tests/test_dmv_placements_gpu.py -- with arc scores of standard deviation up to 6
    (|score| up to ~25, logZ ~ 550).  fp32 charts carry values of magnitude ~800 (log2 units) there -- one ulp is 6e-5 and the
    adjoint weights exp(t - out) see it -- so the north-star bound (1e-4 at L = 40) is NOT claimed beyond L = 40:
      L <= 40:  expected counts within 1e-4 of the fp64 oracle even at score scale 6 (the bound of BASELINE.json's north_star)
      L  > 40:  within max(1e-4, 6 x the error of the SEQUENTIAL fp32 oracle on the same inputs) and never above 6e-4
                (observed: 1.4e-4 at L = 63, 1.9e-4 at L = 88, 4.9e-4 at L = 89 against 0.2-0.9e-4 for the fp32 oracle: the
                butterfly summation order and the 1-ulp v_exp_f32 / v_log_f32, HISTORY.md section 6)
    logZ to 2e-5 relative, Max-semiring values to 1e-5 relative with a valid projective tree of exactly that score."""
    from vlgae_amd.torch_struct import functional as Fn
    rng = np.random.default_rng(1000 + L)
    B = 4
    lengths = rng.integers(max(1, L // 2), L + 1, B)
    lengths[0] = L
    dec = np.log(rng.dirichlet(np.ones(2), (B, L, 2, 2))).astype(np.float32)
    attach = (rng.standard_normal((B, L, L, 2)) * scale).astype(np.float32)
    root = np.log(rng.dirichlet(np.ones(L), B)).astype(np.float32)
    md, ma = ts.DMV1o.merge(t(dec), t(attach), t(root))
    ln = t(lengths)
    mdn, man = md.cpu().numpy(), ma.cpu().numpy()
    rz, rgd, rga = oracle_mod.dmv1o(mdn, man, lengths, "log", np.float64)
    lz, gd, ga = Fn.dmv1o_run(md, ma, ln, 0, True)
    assert np.all(np.abs(lz.cpu().numpy() - rz[:, 0]) <= logz_tol(rz[:, 0]))
    err = max(np.abs(gd.cpu().numpy() - rgd).max(), np.abs(ga.cpu().numpy() - rga).max())
    if L <= 40:
        bound = 1e-4
    else:
        _, gd32, ga32 = oracle_mod.dmv1o(mdn, man, lengths, "log", np.float32)
        e32 = max(np.abs(gd32 - rgd).max(), np.abs(ga32 - rga).max())
        bound = min(6e-4, max(1e-4, 6 * e32))
    assert err <= bound, (L, scale, err, bound)
    # Max semiring: value, and a projective single-root tree with exactly that score
    mz = Fn.dmv1o_run(md, ma, ln, 1, False)[0]
    qz = oracle_mod.dmv1o(mdn, man, lengths, "max", np.float64)[0][:, 0]
    assert np.all(np.abs(mz.cpu().numpy() - qz) <= 1e-5 * np.maximum(1.0, np.abs(qz)))
    best, heads = Fn.dmv1o_decode(md, ma, ln)
    assert torch.allclose(best, mz)
    h = heads.cpu().numpy()
    for b in range(B):
        assert oracle_mod.is_projective_tree(h[b], int(lengths[b]))
        sc = oracle_mod.dmv1o_tree_score(mdn[b], man[b], h[b], int(lengths[b]))
        assert abs(sc - float(mz[b])) <= 2e-4 * max(1.0, abs(sc))


def test_dmv1o_minus_inf_potentials_and_bad_tokens(ts, oracle_mod):
    """-inf potentials (a caller masking with float('-inf')) act as probability zero, like the reference's logsumexp:
    same logZ / counts as the reference's own finite sentinel in their place, everything finite.  Token ids outside
    [0, T) in the rule-table entry mark the sentence invalid (NaN score, zero counts) instead of indexing out of bounds."""
    from vlgae_amd.torch_struct import functional as Fn
    rng = np.random.default_rng(17)
    B, L = 6, 12
    dec = np.log(rng.dirichlet(np.ones(2), (B, L, 2, 2))).astype(np.float32)
    attach = rng.standard_normal((B, L, L, 2)).astype(np.float32)
    root = np.log(rng.dirichlet(np.ones(L), B)).astype(np.float32)
    lengths = np.array([12, 9, 12, 5, 7, 1])
    kill = rng.random((B, L, L)) < 0.25
    kill[:, np.arange(L), np.arange(L)] = False
    a_inf, a_fin = attach.copy(), attach.copy()
    a_inf[kill] = -np.inf
    a_fin[kill] = -1e12
    outs = []
    for att in (a_inf, a_fin):
        md, ma = ts.DMV1o.merge(t(dec), t(att), t(root))
        outs.append(Fn.dmv1o_run(md, ma, t(lengths), 0, True))
    (lz1, gd1, ga1), (lz2, gd2, ga2) = outs
    assert bool(torch.isfinite(lz1).all() and torch.isfinite(gd1).all() and torch.isfinite(ga1).all())
    assert torch.allclose(lz1, lz2, rtol=1e-6, atol=1e-5) and torch.allclose(ga1, ga2, atol=1e-6) and torch.allclose(gd1, gd2, atol=1e-6)
    omd, oma = oracle_mod.dmv1o_merge(dec, a_fin, root)
    rlz, _, rga = oracle_mod.dmv1o(omd, oma, lengths, "log", np.float64)
    assert np.all(np.abs(lz1.cpu().numpy().reshape(rlz.shape) - rlz) <= logz_tol(rlz))
    assert np.abs(ga1.cpu().numpy() - rga).max() <= MARG_TOL
    assert float(ga1[torch.from_numpy(np.pad(kill, ((0, 0), (1, 0), (1, 0)))).to(dev())].abs().max()) == 0.0   # forbidden arcs: exactly zero
    # Max semiring / decode on the same potentials: a tree that avoids every forbidden arc
    _, heads = Fn.dmv1o_decode(*ts.DMV1o.merge(t(dec), t(a_inf), t(root)), t(lengths))
    hh = heads.cpu().numpy()
    for b in range(B):
        for c in range(1, lengths[b] + 1):
            if hh[b, c] > 0:
                assert not kill[b, hh[b, c] - 1, c - 1]
    # ---- rule tables: an out-of-range token id ----
    T = 7
    rule = rng.standard_normal((B, L, T, 2, 2)).astype(np.float32)
    rroot = rng.standard_normal((T,)).astype(np.float32)
    tok = rng.integers(0, T, (B, L))
    tok_bad = tok.copy()
    tok_bad[1, 3] = T          # inside sentence 1 (length 9)
    tok_bad[3, 8] = -1         # beyond sentence 3's length 5: never read, the sentence stays valid
    good = Fn.dmv1o_rules_run(t(rule), t(dec), t(rroot), t(tok), t(lengths), 0, True)
    bad = Fn.dmv1o_rules_run(t(rule), t(dec), t(rroot), t(tok_bad), t(lengths), 0, True)
    assert bool(torch.isnan(bad["logZ"][1])) and float(bad["grad_rule"][1].abs().max()) == 0.0 and float(bad["grad_root"][1].abs().max()) == 0.0
    keep = [0, 2, 3, 4, 5]
    assert torch.equal(bad["logZ"][keep], good["logZ"][keep]) and torch.equal(bad["grad_rule"][keep], good["grad_rule"][keep])
    with pytest.raises(RuntimeError, match="VLG_SEMIRING_MAX"):
        Fn.dmv1o_rules_run(t(rule), t(dec), t(rroot), t(tok), t(lengths), 0, False, want_heads=True)


def test_dmv1o_edge_cases(ts):
    # B = 0
    lz = ts.DMV1o([torch.zeros(0, 5, 2, 2, 2, device=dev()), torch.zeros(0, 5, 5, 2, device=dev())],
                  torch.zeros(0, dtype=torch.long, device=dev())).partition
    assert tuple(lz.shape) == (0, 1)
    # out-of-range length: NaN score, zero counts, neighbours unaffected
    from vlgae_amd.torch_struct import functional as F
    md = torch.randn(3, 6, 2, 2, 2, device=dev())
    ma = torch.randn(3, 6, 6, 2, device=dev())
    lz, gd, ga = F.dmv1o_run(md, ma, torch.tensor([5, 9, 0], device=dev()), 0, True)
    assert torch.isfinite(lz[0]) and torch.isnan(lz[1]) and torch.isnan(lz[2])
    assert float(ga[1:].abs().max()) == 0.0 and float(gd[1:].abs().max()) == 0.0
    # shape violations raise (mirrors the reference's asserts)
    with pytest.raises(ValueError):
        F.dmv1o_run(md, ma[:, :5], torch.tensor([5, 5, 5], device=dev()), 0, False)
    with pytest.raises(RuntimeError):
        F.dmv1o_run(torch.zeros(2, 300, 2, 2, 2, device=dev()), torch.zeros(2, 300, 300, 2, device=dev()),
                    torch.tensor([5, 5], device=dev()), 0, False)
    # non-contiguous inputs and CPU-resident lengths are accepted
    big = torch.randn(3, 6, 6, 4, device=dev())
    lz2, _, _ = F.dmv1o_run(md, big[..., ::2], torch.tensor([5, 4, 3]), 0, False)
    lz3, _, _ = F.dmv1o_run(md, big[..., ::2].contiguous(), torch.tensor([5, 4, 3], device=dev()), 0, False)
    assert torch.equal(lz2, lz3)


def test_dmv1o_create_graph_is_tolerated(ts):
    """callers may pass create_graph=True (helpers.py:139-152 does); the first derivative is the same and a
    second derivative fails loudly instead of silently dropping the dependence on the potentials."""
    g = torch.Generator().manual_seed(7)
    d = torch.randn(4, 9, 2, 2, 2, generator=g).to(dev()).requires_grad_()
    a = torch.randn(4, 9, 9, 2, generator=g).to(dev()).requires_grad_()
    lengths = torch.tensor([8, 5, 3, 1], device=dev())
    with torch.no_grad():                                   # eval loop of ldndmv.py:289 around enable_grad
        with torch.enable_grad():
            (m0,) = torch.autograd.grad(ts.DMV1o([d, a], lengths).partition.sum(), a)
            (m1,) = torch.autograd.grad(ts.DMV1o([d, a], lengths).partition.sum(), a, create_graph=True)
    assert torch.equal(m0, m1.detach())
    with pytest.raises(RuntimeError):
        m1.sum().backward()
    crf = ts.DependencyCRF(a[..., 0], lengths)
    (c1,) = torch.autograd.grad(crf.partition.sum(), a, create_graph=True)
    assert torch.isfinite(c1).all()


@pytest.mark.parametrize("path", golden_files("rules_"), ids=golden_ids("rules_"))
def test_dmv1o_rules_golden(ts, path):
    """the DP fed from the scorer's rule tables == the reference's gather / mask / merge ops + DMV1o."""
    g = load(path)
    hm = t(g["head_mask"]) if g["head_mask"].any() else None
    ar = t(g["attach_rule"]).requires_grad_()
    dc = t(g["dec"]).requires_grad_()
    root_np = g["root_rule"] if int(g["root_per_sentence"]) else g["root_rule"][0]
    rr = t(root_np).requires_grad_()
    dist = ts.DMV1oRules(ar, dc, rr, t(g["token"]), t(g["lengths"]), head_mask=hm)
    logZ = dist.partition
    assert tuple(logZ.shape) == (ar.shape[0], 1)
    g_ar, g_dc, g_rr = torch.autograd.grad(logZ.sum(), [ar, dc, rr])
    assert np.all(np.abs(logZ.detach().cpu().numpy() - g["logZ64"]) <= logz_tol(g["logZ64"]))
    assert np.abs(g_ar.cpu().numpy() - g["grad_rule64"]).max() <= MARG_TOL
    assert np.abs(g_dc.cpu().numpy() - g["grad_dec64"]).max() <= MARG_TOL
    assert np.abs(g_rr.cpu().numpy().reshape(g["grad_root64"].shape) - g["grad_root64"]).max() <= 4 * MARG_TOL
    # identical to the merged-potential path on the reference's merged tensors
    lz_m = ts.DMV1o([t(g["merged_dec"]), t(g["merged_attach"])], t(g["lengths"])).partition
    assert torch.allclose(lz_m, logZ.detach(), rtol=1e-6, atol=1e-4)
    assert np.allclose(dist.max.detach().cpu().numpy(), g["max"], rtol=1e-5, atol=1e-5)
    import oracle   # repeated tokens make equal-score trees common in rule space: compare Viterbi trees by value
    heads = dist.argmax_heads.cpu().numpy()
    for b, ln in enumerate(g["lengths"]):
        assert oracle.is_projective_tree(heads[b], int(ln)) and np.all(heads[b, ln + 1:] == 0)
        sc = oracle.dmv1o_tree_score(g["merged_dec"][b], g["merged_attach"][b], heads[b], int(ln))
        assert abs(sc - g["max"][b, 0]) <= 1e-4 * max(1.0, abs(g["max"][b, 0]))
    # bf16 rule tables are read as bf16 by the kernel
    d16 = ts.DMV1oRules(ar.detach().bfloat16(), dc.detach().bfloat16(), rr.detach().bfloat16(), t(g["token"]),
                        t(g["lengths"]), head_mask=hm)
    ref16 = ts.DMV1oRules(ar.detach().bfloat16().float(), dc.detach().bfloat16().float(), rr.detach().bfloat16().float(),
                          t(g["token"]), t(g["lengths"]), head_mask=hm)
    assert torch.allclose(d16.partition, ref16.partition, rtol=1e-6, atol=1e-4)


def test_dmv1o_hip_graph_capture(ts):
    """The C ABI only enqueues work on the stream it is given (no allocation, no synchronisation), so a step can
    be captured into a HIP graph and replayed on new data in place."""
    from vlgae_amd.torch_struct import functional as F
    B, L = 32, 24
    gen = torch.Generator().manual_seed(3)
    md = torch.randn(B, L + 1, 2, 2, 2, generator=gen).to(dev())
    ma = torch.randn(B, L + 1, L + 1, 2, generator=gen).to(dev())
    lengths = torch.randint(1, L + 1, (B,), generator=gen).to(dev())
    F.dmv1o_run(md, ma, lengths, 0, True)           # warm-up outside capture (sets kernel attributes once)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lz, gd, ga = F.dmv1o_run(md, ma, lengths, 0, True)
    for seed in (4, 5):
        gen = torch.Generator().manual_seed(seed)
        md.copy_(torch.randn(B, L + 1, 2, 2, 2, generator=gen))
        ma.copy_(torch.randn(B, L + 1, L + 1, 2, generator=gen))
        graph.replay()
        torch.cuda.synchronize()
        lz2, gd2, ga2 = F.dmv1o_run(md, ma, lengths, 0, True)
        assert torch.equal(lz, lz2) and torch.equal(gd, gd2) and torch.equal(ga, ga2)


# ------------------------------------------------------------------------------------------------ DepTree
@pytest.mark.parametrize("path", golden_files("deptree_"), ids=golden_ids("deptree_"))
def test_deptree_golden(ts, path):
    g = load(path)
    arc, lengths = t(g["arc"]), t(g["lengths"])
    dist = ts.DependencyCRF(arc.clone(), lengths)
    lz = dist.partition
    assert tuple(lz.shape) == (arc.shape[0],)
    assert np.all(np.abs(lz.detach().cpu().numpy() - g["logZ64"]) <= logz_tol(g["logZ64"]))
    assert np.abs(dist.marginals.detach().cpu().numpy() - g["marginals64"]).max() <= MARG_TOL
    assert np.allclose(dist.max.detach().cpu().numpy(), g["max"], rtol=1e-5, atol=1e-5)
    assert np.array_equal(dist.argmax.detach().cpu().numpy(), g["argmax"])
    if "enum_logZ" in g:   # brute force over all projective single-root trees (deptree.py:213-228)
        assert np.all(np.abs(lz.detach().cpu().numpy() - g["enum_logZ"]) <= logz_tol(g["enum_logZ"]))
        assert np.allclose(dist.max.detach().cpu().numpy(), g["enum_max"], rtol=1e-5, atol=1e-5)
    a = arc.clone().requires_grad_()
    (ts.DependencyCRF(a, lengths).partition * t(g["wts"])).sum().backward()
    assert np.abs(a.grad.detach().cpu().numpy() - g["wgrad"]).max() <= 2 * MARG_TOL
    # lengths=None means N-1 (deptree.py:151-152)
    if np.all(g["lengths"] == arc.shape[1] - 1):
        assert torch.equal(ts.DependencyCRF(arc.clone()).partition, lz)


@pytest.mark.parametrize("B,N,seed", [(64, 41, 21), (8, 81, 22), (4, 150, 23), (300, 4, 24)])
def test_deptree_vs_oracle_random(ts, oracle_mod, B, N, seed):
    rng = np.random.default_rng(seed)
    arc = rng.standard_normal((B, N, N)).astype(np.float32)
    lengths = rng.integers(1, N, size=B)
    lengths[0] = N - 1
    from vlgae_amd.torch_struct import functional as F
    for sr, name in ((0, "log"), (1, "max")):
        ref_lz, ref_g = oracle_mod.deptree(arc, lengths, name, np.float64)
        lz, garc = F.deptree_run(t(arc), t(lengths), sr, True)
        assert np.all(np.abs(lz.detach().cpu().numpy() - ref_lz) <= logz_tol(ref_lz))
        if sr == 0:
            assert np.abs(garc.detach().cpu().numpy() - ref_g).max() <= MARG_TOL
            col = garc.sum(1).detach().cpu().numpy()   # column sums are 1 inside the sentence, 0 outside
            for b in range(B):
                assert np.allclose(col[b, 1:lengths[b] + 1], 1.0, atol=1e-4)
                assert np.all(col[b, lengths[b] + 1:] == 0) and col[b, 0] == 0
        else:
            assert np.array_equal(garc.detach().cpu().numpy(), ref_g.astype(np.float32))


@pytest.mark.parametrize("B,N", [(256, 41), (24, 81)])
def test_deptree_full_size_properties_and_reproducibility(ts, B, N):
    """DepTree at the headline batch (and at the long-sentence width): arc marginals sum to one per word, the best tree's
    score equals the Max-semiring value, and 20 launches give identical bits (the two directions of a span run on separate
    wave halves and share T(i,j); a race between them would show up here)."""
    from vlgae_amd.torch_struct import functional as F
    g = torch.Generator().manual_seed(B + N)
    arc = torch.randn(B, N, N, generator=g).to(dev())
    lengths = torch.randint(1, N, (B,), generator=g)
    lengths[0] = N - 1
    lengths = lengths.to(dev())
    lz, garc = F.deptree_run(arc, lengths, 0, True)
    col = garc.sum(1)
    inside = torch.arange(N, device=dev())[None] <= lengths[:, None]
    inside[:, 0] = False
    assert float((col[inside] - 1).abs().max()) <= 1e-4 and float(col[~inside].abs().max()) == 0.0
    mz, marc = F.deptree_run(arc, lengths, 1, True)
    best, heads = F.deptree_decode(arc, lengths)
    assert torch.equal(best, mz)
    score = (arc * marc).sum((1, 2))
    assert float((score - mz).abs().max()) <= 1e-3
    picked = torch.zeros_like(marc).scatter_(1, heads.unsqueeze(1), 1.0) * inside[:, None, :]    # marc[b, head[c], c] = 1
    assert torch.equal(picked, marc)
    for _ in range(20):
        lz2, garc2 = F.deptree_run(arc, lengths, 0, True)
        assert torch.equal(lz2, lz) and torch.equal(garc2, garc)
        _, heads2 = F.deptree_decode(arc, lengths)
        assert torch.equal(heads2, heads)


# ------------------------------------------------------------------------------------------------ alignment
@pytest.mark.parametrize("path", golden_files("align_"), ids=golden_ids("align_"))
def test_bilinear_align_golden(path):
    from vlgae_amd import align
    g = load(path)
    txt, vis, tm, vm = t(g["txt"]), t(g["vis"]), t(g["tmask"]), t(g["vmask"])
    out = align.gather_logit(None, (vis.refine_names("A", "V", "Y"), vm.refine_names("A", "V"), None),
                             (txt.refine_names("B", "Q", "X"), tm.refine_names("B", "Q"), None), None)
    assert out.names == ("B", "A", "Q", "V")
    got = out.rename(None).detach().cpu().numpy()
    ref = g["attmap"]
    masked = ref <= -1e19
    assert np.array_equal(got[masked], ref[masked])                     # exactly -INF (1e20) where masked
    assert np.abs(got[~masked] - ref[~masked]).max() <= 2e-4           # fp32 dot of length d, |x| ~ sqrt(d)
    if "bf16" in path:   # bf16 kernel input path on the same (bf16-representable) values
        o16 = align.bilinear_align(txt.bfloat16(), vis.bfloat16(), tm, vm)["full"].detach().cpu().numpy()
        assert np.abs(o16[~masked] - ref[~masked]).max() <= 2e-4
    # fused epilogues against the materialised tensor
    B, A = txt.shape[0], vis.shape[0]
    r = align.bilinear_align(txt, vis, tm, vm, full=True, max_v=True, max_q=True, diag=(A == B))
    full = r["full"]
    assert torch.equal(r["max_v"], full.max(-1).values)
    assert torch.equal(r["max_q"], full.max(-2).values)
    if A == B:
        assert torch.equal(r["diag"], full[torch.arange(B), torch.arange(B)])
    r2 = align.bilinear_align(txt, vis, tm, vm, full=False, max_v=True, max_q=True)
    assert torch.equal(r2["max_v"], r["max_v"]) and torch.equal(r2["max_q"], r["max_q"]) and "full" not in r2


def test_bilinear_align_backward_and_sizes(oracle_mod):
    from vlgae_amd import align
    rng = np.random.default_rng(5)
    for (B, A, Q, V, d) in [(3, 2, 5, 70, 16), (2, 9, 130, 3, 40), (5, 5, 82, 36, 128)]:
        txt = rng.standard_normal((B, Q, d)).astype(np.float32)
        vis = rng.standard_normal((A, V, d)).astype(np.float32)
        tm = rng.random((B, Q)) > 0.2
        vm = rng.random((A, V)) > 0.2
        ref = oracle_mod.bilinear_align(txt, vis, tm, vm, np.float64, -1e20, full=True, maxV=True, maxQ=True)
        r = align.bilinear_align(t(txt), t(vis), t(tm), t(vm), max_v=True, max_q=True)
        keep = ref["full"] > -1e19
        assert np.abs(r["full"].detach().cpu().numpy()[keep] - ref["full"][keep]).max() <= 1e-4
        assert np.all(r["full"].detach().cpu().numpy()[~keep] == np.float32(-1e20))
        # fully masked rows / columns reduce to the float32 fill value; compare in float32
        assert np.allclose(r["max_v"].detach().cpu().numpy(), ref["maxV"].astype(np.float32), atol=1e-4, rtol=1e-6)
        assert np.allclose(r["max_q"].detach().cpu().numpy(), ref["maxQ"].astype(np.float32), atol=1e-4, rtol=1e-6)
    # gradients of the contraction (masked entries carry none)
    tx = t(txt).requires_grad_()
    vi = t(vis).requires_grad_()
    w = torch.randn(B, A, Q, V, device=dev())
    out = align.gather_logit(None, (vi, t(vm), None), (tx, t(tm), None), None).rename(None)
    (out * w).sum().backward()
    keepm = (t(tm)[:, None, :, None] & t(vm)[None, :, None, :]).float()
    tx2 = t(txt).requires_grad_()
    vi2 = t(vis).requires_grad_()
    (torch.einsum("avd,bqd->baqv", vi2, tx2) * w * keepm).sum().backward()
    assert torch.allclose(tx.grad, tx2.grad, atol=1e-3, rtol=1e-4)
    assert torch.allclose(vi.grad, vi2.grad, atol=1e-3, rtol=1e-4)


@pytest.mark.parametrize("B,A,Q,V,d,dt", [(5, 5, 82, 36, 128, "f32"), (5, 5, 82, 36, 128, "bf16"), (3, 4, 7, 130, 64, "f32"),
                                          (2, 3, 100, 5, 32, "bf16"), (1, 1, 1, 1, 128, "f32"), (4, 2, 33, 201, 128, "f32"),
                                          # bf16, d = 128: the split-term kernels -- odd contraction lengths (word loads), the
                                          # concatenated two-pairs-per-step caption side at its limits (V = 4, 40, 44, 48) with odd
                                          # and even outer counts, one / six row tiles, and shapes that fall back per side
                                          (3, 4, 50, 37, 128, "bf16"), (2, 3, 96, 48, 128, "bf16"), (3, 2, 97, 20, 128, "bf16"),
                                          (4, 5, 30, 40, 128, "bf16"), (2, 2, 20, 44, 128, "bf16"), (3, 3, 33, 4, 128, "bf16"),
                                          (33, 34, 17, 36, 128, "bf16"), (2, 40, 82, 64, 128, "bf16")])
def test_bilinear_align_backward_vs_oracle(oracle_mod, B, A, Q, V, d, dt):
    """vlg_bilinear_align_backward (the hand-written adjoint of the materialised tensor, joint.py:413-418 under autograd)
    against the fp64 oracle: both masks, contraction lengths across the 96-element chunk boundary, one- and several-tile
    row counts, all three feature widths, bf16 storage; through autograd (gather_logit) and directly."""
    from vlgae_amd import align
    rng = np.random.default_rng(B * 1000 + Q * 7 + V)
    txt = rng.standard_normal((B, Q, d)).astype(np.float32)
    vis = rng.standard_normal((A, V, d)).astype(np.float32)
    tm, vm = rng.random((B, Q)) > 0.2, rng.random((A, V)) > 0.2
    g = rng.standard_normal((B, A, Q, V)).astype(np.float32)
    tdt = torch.bfloat16 if dt == "bf16" else torch.float32
    tt, tv = t(txt).to(tdt), t(vis).to(tdt)
    txt, vis = tt.float().cpu().numpy(), tv.float().cpu().numpy()
    for masks in ((tm, vm), (None, None)):
        ref_t, ref_v = oracle_mod.bilinear_align_backward(g, txt, vis, masks[0], masks[1], np.float64)
        mt = None if masks[0] is None else t(masks[0])
        mvv = None if masks[1] is None else t(masks[1])
        gt, gv = align.bilinear_align_backward(t(g), tt, tv, mt, mvv)
        for got, want in ((gt, ref_t), (gv, ref_v)):     # exact fp32 products, fp32 accumulation over A*V / B*Q terms
            assert np.abs(got.cpu().numpy() - want).max() <= 2e-5 * max(1.0, np.abs(want).max())
        only_t, none_v = align.bilinear_align_backward(t(g), tt, tv, mt, mvv, want_vis=False)
        assert none_v is None and torch.equal(only_t, gt)
        gt2, gv2 = align.bilinear_align_backward(t(g), tt, tv, mt, mvv)
        assert torch.equal(gt2, gt) and torch.equal(gv2, gv)                # reproducible (two-addend atomics are order-free)
    # through autograd, as the reference's loss would reach it
    a_, b_ = tt.clone().requires_grad_(True), tv.clone().requires_grad_(True)
    out = align.gather_logit(None, (b_, t(vm), None), (a_, t(tm), None), None).rename(None)
    ga, gb = torch.autograd.grad(out, [a_, b_], t(g))
    ref_t, ref_v = oracle_mod.bilinear_align_backward(g, txt, vis, tm, vm, np.float64)
    tol = 2e-5 if dt == "f32" else 8e-3        # bf16 leaves get bf16 gradients
    assert np.abs(ga.float().cpu().numpy() - ref_t).max() <= tol * max(1.0, np.abs(ref_t).max())
    assert np.abs(gb.float().cpu().numpy() - ref_v).max() <= tol * max(1.0, np.abs(ref_v).max())


def test_bilinear_align_backward_config_size():
    """The a9 backward at BASELINE configs[1] widths (B = A = 256, Q = 82, V = 36, d = 128, bf16 features: the split-term
    kernels, caption side two pairs per step, outer ranges split over two blocks): against fp32 torch contractions of the same
    masked cotangent (the oracle is too slow at this size; it pins the same kernels on small batches above), masked rows exactly
    zero, and identical bits on a second run."""
    from vlgae_amd import align
    B, Q, V, d = 256, 82, 36, 128
    g = torch.Generator(device=dev()).manual_seed(17)
    txt = (torch.randn(B, Q, d, generator=g, device=dev()) * 0.5).bfloat16()
    vis = (torch.randn(B, V, d, generator=g, device=dev()) * 0.5).bfloat16()
    tm = torch.rand(B, Q, generator=g, device=dev()) > 0.15
    vm = torch.rand(B, V, generator=g, device=dev()) > 0.15
    cot = torch.randn(B, B, Q, V, generator=g, device=dev())
    gt, gv = align.bilinear_align_backward(cot, txt, vis, tm, vm)
    gm = cot * tm[:, None, :, None] * vm[None, :, None, :]
    want_t = torch.einsum("baqv,avd->bqd", gm, vis.float())
    want_v = torch.einsum("baqv,bqd->avd", gm, txt.float())
    for got, want in ((gt, want_t), (gv, want_v)):
        assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max())   # two-term split: < 2^-17 per product; fp32 sums of 9 k / 21 k terms
    assert not bool(gt[~tm].any()) and not bool(gv[~vm].any())
    gt2, gv2 = align.bilinear_align_backward(cot, txt, vis, tm, vm)
    assert torch.equal(gt, gt2) and torch.equal(gv, gv2)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_bilinear_align_config_size(oracle_mod, dt):
    """BASELINE.json configs[1] shapes (B = A = 256, Q = 82, V = 36, d = 128): the fused maxima / diagonal block are
    bit-equal to reductions of the materialised tensor, masked entries are exactly -1e20, and a 40-pair slice of the
    tensor matches the fp64 oracle."""
    from vlgae_amd import align
    B, Q, V, d = 256, 82, 36, 128
    g = torch.Generator().manual_seed(256)
    tdt = torch.bfloat16 if dt == "bf16" else torch.float32
    txt = (torch.randn(B, Q, d, generator=g) * 0.3).to(dev(), tdt)
    vis = (torch.randn(B, V, d, generator=g) * 0.3).to(dev(), tdt)
    tm = torch.rand(B, Q, generator=g).to(dev()) > 0.05
    tm[:, 0] = tm[:, 41] = False                                   # the two root slots (joint.py:204,248-249)
    vm = torch.rand(B, V, generator=g).to(dev()) > 0.1
    vm[:, 0] = True
    for masks in ((None, None), (tm, vm)):
        full = align.bilinear_align(txt, vis, masks[0], masks[1], full=True)["full"]
        r = align.bilinear_align(txt, vis, masks[0], masks[1], full=False, max_v=True, max_q=True, diag=True)
        assert torch.equal(r["max_v"], full.max(3).values)
        assert torch.equal(r["max_q"], full.max(2).values)
        assert torch.equal(r["diag"], full[torch.arange(B), torch.arange(B)])
        r1 = align.bilinear_align(txt, vis, masks[0], masks[1], full=False, max_q=True)
        r2 = align.bilinear_align(txt, vis, masks[0], masks[1], full=False, max_v=True)
        assert torch.equal(r1["max_q"], r["max_q"]) and torch.equal(r2["max_v"], r["max_v"])
        if masks[0] is not None:
            dead = ~(tm[:, None, :, None] & vm[None, :, None, :])
            assert bool((full[dead] == -1e20).all()) and bool((full[~dead] > -1e19).all())
        # oracle slice: captions 0..7 x images 0..4 (40 pairs), the same (possibly bf16-rounded) features
        nb, na = 8, 5
        tn, vn = txt[:nb].float().cpu().numpy(), vis[:na].float().cpu().numpy()
        ref = oracle_mod.bilinear_align(tn, vn, None if masks[0] is None else tm[:nb].cpu().numpy(),
                                        None if masks[1] is None else vm[:na].cpu().numpy(), np.float64)["full"]
        got = full[:nb, :na].cpu().numpy()
        live = ref > -1e19
        assert np.array_equal(got[~live], ref[~live].astype(np.float32))
        assert np.abs(got[live] - ref[live]).max() <= 2e-5 * max(1.0, np.abs(ref[live]).max())   # fp32 accumulation over d = 128
        del full, r


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_grounding_loss_and_decoder_config_shapes_vs_oracle(oracle_mod, dt):
    """Config-2 widths (Q = 82, V = 36, d = 128) on a 32-caption batch (the loss couples every pair of the batch through
    its soft-max, so the oracle is run on the whole of a smaller batch rather than on a slice of 256): loss sums and
    gradients against the fp64 oracle."""
    from vlgae_amd import align
    B, L, V, d = 32, 40, 36, 128
    N, Q = L + 1, 2 * (L + 1)
    rng = np.random.default_rng(3232)
    txt = (rng.standard_normal((B, Q, d)) * 0.3).astype(np.float32)
    vis = (rng.standard_normal((B, V, d)) * 0.3).astype(np.float32)
    tdt = torch.bfloat16 if dt == "bf16" else torch.float32
    txt_t, vis_t = t(txt).to(tdt), t(vis).to(tdt)
    txt, vis = txt_t.float().cpu().numpy(), vis_t.float().cpu().numpy()      # the oracle sees the rounded features
    lengths = rng.integers(L // 2, L + 1, size=B)
    m1 = np.concatenate([np.zeros((B, 1), bool), np.arange(L)[None] < lengths[:, None]], 1)
    tmask = np.concatenate([m1, m1], 1)
    vmask = rng.random((B, V)) > 0.1
    vmask[:, 0] = True
    marg = (rng.random((B, Q)) * tmask).astype(np.float32)
    num_token = float(lengths.sum())
    ref = oracle_mod.grounding_loss(txt, vis, tmask, vmask, marg, num_token, 1.0, dtype=np.float64)
    a, b = txt_t.clone().requires_grad_(True), vis_t.clone().requires_grad_(True)
    total, sums = align.grounding_loss_factor_ce(a, b, t(tmask), t(vmask), t(marg), num_token, 1.0)
    ga, gb = torch.autograd.grad(total, [a, b])
    s_ = sums.detach().cpu().numpy()
    assert abs(s_[0] - ref["txt2vis"]) <= 1e-4 * max(1.0, abs(ref["txt2vis"]))
    assert abs(s_[1] - ref["vis2txt"]) <= 1e-4 * max(1.0, abs(ref["vis2txt"]))
    for got, want in ((ga, ref["g_txt"]), (gb, ref["g_vis"])):
        tol = (1e-4 if dt == "f32" else 1e-2) * max(1.0, np.abs(want).max())   # bf16: the gradient itself is returned in bf16
        assert np.abs(got.float().cpu().numpy() - want).max() <= tol
    # decoder at the same widths: image choice and top-5 columns of the (prior-free, heuristic-free) decode vs reductions of
    # the oracle's tensor
    dec = align.grounding_decode(txt_t, vis_t, t(tmask), t(vmask))
    full = oracle_mod.bilinear_align(txt, vis, tmask, vmask, np.float64)["full"]
    mv = full.max(3)                                                                # [B,A,Q] (joint.py:519-520)
    f2i, top5, blk = dec["factor2img"].cpu().numpy(), dec["top5"].cpu().numpy(), dec["logit"].cpu().numpy()
    diag = full[np.arange(B), np.arange(B)]                                         # [B,Q,V]
    assert np.abs(blk[diag > -1e19] - diag[diag > -1e19]).max() <= 2e-5 * max(1.0, np.abs(diag[diag > -1e19]).max())
    n_img = n_top = 0
    for b in range(B):
        for q in np.flatnonzero(tmask[b]):
            col = np.sort(mv[b, :, q])[::-1]
            if col[0] - col[1] > 1e-4:                                              # unambiguous at fp32 resolution
                assert f2i[b, q] == int(np.argmax(mv[b, :, q]))
                n_img += 1
            row = np.sort(diag[b, q])[::-1]
            if row[0] - row[1] > 1e-4 and row[0] > -1e19:
                assert top5[b, q, 0] == int(np.argmax(diag[b, q]))
                n_top += 1
    assert n_img > B * 10 and n_top > B * 10


@pytest.mark.parametrize("path", golden_files("attnfuse_"), ids=golden_ids("attnfuse_"))
def test_attn_fuse_golden(path):
    from vlgae_amd import align
    g = load(path)
    out, att = align.attention_fuse(t(g["vis"]), t(g["txt"]), t(g["vis_mid"]), t(g["enc_x"]), t(g["ln_weight"]),
                                    t(g["ln_bias"]), float(g["ln_eps"]), return_attmap=True)
    assert np.abs(att.detach().cpu().numpy() - g["attmap"]).max() <= 2e-5       # softmax probabilities
    assert np.abs(out.detach().cpu().numpy() - g["out"]).max() <= 1e-4          # LayerNorm output, O(1) values
    # without the attention map the matrix-core kernel runs (h <= 256, d and h multiples of 16)
    out2 = align.attention_fuse(t(g["vis"]), t(g["txt"]), t(g["vis_mid"]), t(g["enc_x"]), t(g["ln_weight"]),
                                t(g["ln_bias"]), float(g["ln_eps"]))
    assert np.abs(out2.cpu().numpy() - g["out"]).max() <= 1e-4
    out3 = align.attention_fuse(t(g["vis"]).bfloat16(), t(g["txt"]).bfloat16(), t(g["vis_mid"]).bfloat16(),
                                t(g["enc_x"]).bfloat16(), t(g["ln_weight"]), t(g["ln_bias"]), float(g["ln_eps"]))
    assert np.abs(out3.cpu().numpy() - g["out"]).max() <= 0.15                   # bf16-rounded inputs (8 bits), O(1) outputs


def test_attn_fuse_large_v(oracle_mod):
    """V = 1296 factors (the shipped config's 35 + 35^2 + 35 + 1) exercises the word-chunked launch."""
    from vlgae_amd import align
    rng = np.random.default_rng(9)
    B, L, V, d, h = 2, 13, 1296, 128, 256
    vis, txt = rng.standard_normal((B, V, d)).astype(np.float32) * 0.3, rng.standard_normal((B, L + 1, d)).astype(np.float32) * 0.3
    mid, enc = rng.standard_normal((B, V, h)).astype(np.float32), rng.standard_normal((B, L, h)).astype(np.float32)
    gm, bt = (rng.random(h) + 0.5).astype(np.float32), rng.standard_normal(h).astype(np.float32)
    ref_att, ref_out = oracle_mod.attn_fuse(vis, txt, mid, enc, gm, bt, 1e-5, np.float64)
    out, att = align.attention_fuse(t(vis), t(txt), t(mid), t(enc), t(gm), t(bt), 1e-5, return_attmap=True)
    assert np.abs(att.detach().cpu().numpy() - ref_att).max() <= 2e-5
    assert np.abs(out.detach().cpu().numpy() - ref_out).max() <= 1e-4
    out2 = align.attention_fuse(t(vis), t(txt), t(mid), t(enc), t(gm), t(bt), 1e-5)
    assert np.abs(out2.cpu().numpy() - ref_out).max() <= 1e-4
    # round 6: above 256 keys the differentiable call runs the key-split kernels (chunks of keys per wavefront, chunk records merged in
    # chunk order); value and all six gradients against the fp64 oracle DIRECTLY, and against the one-pass kernels on the same inputs
    # (forced with key_chunk >= V)
    leaves = [t(a).requires_grad_(True) for a in (vis, txt, mid, enc, gm, bt)]
    dout = rng.standard_normal((B, L, h)).astype(np.float32)
    cot = t(dout)
    ref_g = oracle_mod.attn_fuse_backward(vis, txt, mid, enc, gm, dout, 1e-5, np.float64)
    wide = align.attention_fuse(*leaves, 1e-5)
    assert "AttnFuse" in type(wide.grad_fn).__name__
    g_wide = torch.autograd.grad(wide, leaves, cot)
    one = align.attention_fuse(*leaves, 1e-5, key_chunk=V)
    g_one = torch.autograd.grad(one, leaves, cot)
    assert float((wide.detach().cpu() - torch.from_numpy(ref_out)).abs().max()) <= 1e-4 and float((wide - one).detach().abs().max()) <= 1e-4
    for name, a, b, want in zip(ATTN_GRAD_NAMES, g_wide, g_one, ref_g):
        assert np.abs(a.cpu().numpy() - want).max() <= 1e-4 * max(1.0, np.abs(want).max()), name
        assert float((a - b).abs().max()) <= 2e-4 * max(1.0, float(b.abs().max())), name
    assert not g_wide[1][:, 0].any()   # root slot
    # a mid-sized V: four region chunks in the matrix-core kernel, ragged last chunk, three word tiles
    B, L, V = 3, 47, 203
    vis, txt = rng.standard_normal((B, V, d)).astype(np.float32) * 0.3, rng.standard_normal((B, L + 1, d)).astype(np.float32) * 0.3
    mid, enc = rng.standard_normal((B, V, h)).astype(np.float32), rng.standard_normal((B, L, h)).astype(np.float32)
    _, ref_out = oracle_mod.attn_fuse(vis, txt, mid, enc, gm, bt, 1e-5, np.float64)
    out3 = align.attention_fuse(t(vis), t(txt), t(mid), t(enc), t(gm), t(bt), 1e-5)
    assert np.abs(out3.cpu().numpy() - ref_out).max() <= 1e-4


@pytest.mark.parametrize("B,L,V,d,h", [
    (3, 40, 36, 128, 256),    # the benchmark shape: one chunk of three region tiles
    (2, 1, 1, 16, 16),        # smallest legal case: one word, one region, one channel tile
    (2, 16, 16, 32, 64),      # exact tiles everywhere
    (2, 17, 17, 48, 80),      # one past a tile in words and regions; d and h not powers of two
    (2, 33, 64, 144, 240),    # d = 128 + 16: a short second K chunk; V = 64 is the largest single chunk
    (2, 9, 65, 256, 128),     # V = 65: second streamed chunk holds a single region; two full K chunks
    (1, 50, 130, 64, 256),    # three streamed chunks, ragged last
])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_attn_fuse_mfma_shapes(oracle_mod, B, L, V, d, h, dt):
    """Matrix-core attention-fuse against the fp64 oracle over tile / chunk edge cases (joint.py:670-674)."""
    from vlgae_amd import align
    rng = np.random.default_rng(B * 1000 + L * 31 + V)
    vis, txt = rng.standard_normal((B, V, d)).astype(np.float32) * 0.4, rng.standard_normal((B, L + 1, d)).astype(np.float32) * 0.4
    mid, enc = rng.standard_normal((B, V, h)).astype(np.float32), rng.standard_normal((B, L, h)).astype(np.float32)
    gm, bt = (rng.random(h) + 0.5).astype(np.float32), rng.standard_normal(h).astype(np.float32)
    args = [t(vis), t(txt), t(mid), t(enc)]
    if dt == "bf16":   # the oracle sees the same bf16-rounded values, so the tolerance stays the fp32 one
        args = [a.bfloat16() for a in args]
        vis, txt, mid, enc = (a.float().cpu().numpy() for a in args)
    _, ref_out = oracle_mod.attn_fuse(vis, txt, mid, enc, gm, bt, 1e-5, np.float64)
    out = align.attention_fuse(*args, t(gm), t(bt), 1e-5)
    assert out.shape == (B, L, h) and out.dtype == torch.float32
    assert np.abs(out.cpu().numpy() - ref_out).max() <= 1e-4


ATTN_GRAD_NAMES = ("g_vis", "g_txt", "g_vis_mid", "g_enc_x", "g_ln_weight", "g_ln_bias")


def _attn_grads(arrs, gm, bt, dout, eps, bf16=False):
    """Gradients of attention_fuse through torch.autograd (i.e. through vlg_attn_fuse_backward)."""
    from vlgae_amd import align
    leaves = [t(a) for a in arrs]
    if bf16:
        leaves = [a.bfloat16() for a in leaves]
    leaves += [t(gm), t(bt)]
    for a in leaves:
        a.requires_grad_(True)
    out = align.attention_fuse(*leaves, eps)
    return out, torch.autograd.grad(out, leaves, t(dout))


@pytest.mark.parametrize("path", golden_files("attnfuse_"), ids=golden_ids("attnfuse_"))
def test_attn_fuse_backward_golden(path):
    """Adjoint kernels vs torch autograd through the reference's own ops (fixtures: tests/golden/make_golden.py)."""
    g = load(path)
    out, grads = _attn_grads([g["vis"], g["txt"], g["vis_mid"], g["enc_x"]], g["ln_weight"], g["ln_bias"], g["dout"],
                             float(g["ln_eps"]))
    assert np.abs(out.detach().cpu().numpy() - g["out"]).max() <= 1e-4
    for name, got in zip(ATTN_GRAD_NAMES, grads):
        ref = g[name]
        assert tuple(got.shape) == ref.shape, name
        assert np.abs(got.cpu().numpy() - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max()), name
    assert not grads[1][:, 0].any()   # root slot


@pytest.mark.parametrize("B,L,V,d,h", [
    (3, 40, 36, 128, 256),    # the benchmark shape
    (2, 1, 1, 16, 16),        # one word, one region: softmax is the constant 1, dS = 0
    (6, 63, 1, 144, 80),      # one region, many words: d_vis = d_txt = 0 exactly -- with bf16 features only if D is taken over the same
                              # bf16-rounded cotangent the matrix cores see (tools/stress_attn.py found 0.12 here)
    (2, 16, 16, 32, 64),
    (2, 17, 17, 48, 80),
    (2, 33, 64, 144, 240),    # d > 128: sixteen feature tiles in the adjoint
    (2, 9, 65, 256, 128),     # streamed chunks, second holds one region
    (1, 50, 130, 64, 256),
])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_attn_fuse_backward_shapes(oracle_mod, B, L, V, d, h, dt):
    rng = np.random.default_rng(B * 977 + L * 29 + V)
    vis, txt = rng.standard_normal((B, V, d)).astype(np.float32) * 0.4, rng.standard_normal((B, L + 1, d)).astype(np.float32) * 0.4
    mid, enc = rng.standard_normal((B, V, h)).astype(np.float32), rng.standard_normal((B, L, h)).astype(np.float32)
    gm, bt = (rng.random(h) + 0.5).astype(np.float32), rng.standard_normal(h).astype(np.float32)
    dout = rng.standard_normal((B, L, h)).astype(np.float32)
    arrs = [vis, txt, mid, enc]
    if dt == "bf16":   # the oracle sees the same bf16-rounded values
        arrs = [torch.from_numpy(a).bfloat16().float().numpy() for a in arrs]
    ref = oracle_mod.attn_fuse_backward(*arrs, gm, dout, 1e-5, np.float64)
    out, grads = _attn_grads(arrs, gm, bt, dout, 1e-5, bf16=(dt == "bf16"))
    for i, (name, got, want) in enumerate(zip(ATTN_GRAD_NAMES, grads, ref)):
        assert got.dtype == (torch.bfloat16 if dt == "bf16" and i < 4 else torch.float32), name
        tol = (1e-2 if dt == "bf16" and i < 4 else 1e-4) * max(1.0, np.abs(want).max())   # bf16 grads are rounded on return
        assert np.abs(got.float().cpu().numpy() - want).max() <= tol, name


@pytest.mark.parametrize("B,L,V,d,h,ck", [
    (2, 9, 65, 256, 128, 64),      # two chunks, the second holds a single key; sixteen feature tiles in the adjoint
    (1, 50, 130, 64, 256, 64),     # three chunks, ragged last; four word tiles, ragged last
    (3, 47, 203, 128, 256, 128),   # two chunks of two 64-key steps (second ragged)
    (2, 17, 300, 48, 80, 0),       # automatic: above 256 keys -> 64-key chunks at this batch; d and h not powers of two
    (2, 40, 1369, 128, 256, 0),    # the shipped factor layout (config/model/vlgae.yaml:40-42): 36 + 36^2 + 36 + 1 keys
])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_attn_fuse_key_split_vs_oracle(oracle_mod, B, L, V, d, h, ck, dt):
    """The key-split form of the attention-fuse (joint.py:670-674 at many keys), forward and all six gradients, against the fp64 oracle
    directly.  bf16: the oracle sees the same bf16-rounded inputs; the four feature gradients come back as bf16 (rounded once from the
    fp32 accumulators inside the kernels), so they are held to a bf16 rounding (1e-2 of the tensor's largest magnitude)."""
    from vlgae_amd import _C, align
    rng = np.random.default_rng(B * 811 + L * 23 + V)
    vis, txt = rng.standard_normal((B, V, d)).astype(np.float32) * 0.4, rng.standard_normal((B, L + 1, d)).astype(np.float32) * 0.4
    mid, enc = rng.standard_normal((B, V, h)).astype(np.float32), rng.standard_normal((B, L, h)).astype(np.float32)
    gm, bt = (rng.random(h) + 0.5).astype(np.float32), rng.standard_normal(h).astype(np.float32)
    dout = rng.standard_normal((B, L, h)).astype(np.float32)
    arrs = [vis, txt, mid, enc]
    if dt == "bf16":
        arrs = [torch.from_numpy(a).bfloat16().float().numpy() for a in arrs]
    assert _C.lib().vlg_attn_fuse_workspace(B, L, V, h, ck) > 0          # the split path is what runs
    _, ref_out = oracle_mod.attn_fuse(*arrs, gm, bt, 1e-5, np.float64)
    ref = oracle_mod.attn_fuse_backward(*arrs, gm, dout, 1e-5, np.float64)
    leaves = [t(a) for a in arrs]
    if dt == "bf16":
        leaves = [a.bfloat16() for a in leaves]
    leaves += [t(gm), t(bt)]
    for a in leaves:
        a.requires_grad_(True)
    out = align.attention_fuse(*leaves, 1e-5, key_chunk=ck)
    grads = torch.autograd.grad(out, leaves, t(dout))
    with torch.no_grad():
        out_ng = align.attention_fuse(*leaves, 1e-5, key_chunk=ck)
    assert torch.equal(out, out_ng)
    assert np.abs(out.detach().cpu().numpy() - ref_out).max() <= 1e-4
    for i, (name, got, want) in enumerate(zip(ATTN_GRAD_NAMES, grads, ref)):
        assert got.dtype == (torch.bfloat16 if dt == "bf16" and i < 4 else torch.float32) and tuple(got.shape) == want.shape, name
        tol = (1e-2 if dt == "bf16" and i < 4 else 1e-4) * max(1.0, np.abs(want).max())
        assert np.abs(got.float().cpu().numpy() - want).max() <= tol, name
    assert not grads[1][:, 0].any()   # root slot
    # bit-reproducible: no atomics, chunk records merged in chunk order
    grads2 = torch.autograd.grad(align.attention_fuse(*leaves, 1e-5, key_chunk=ck), leaves, t(dout))
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2))


def test_attn_fuse_bf16_gradients_equal_fp32_then_cast():
    """grad_dtype = bf16 rounds the fp32 accumulators once inside the kernels: the same bits as the fp32 gradients cast afterwards
    (one-pass kernels at V = 36, key-split kernels at V = 300)."""
    from vlgae_amd import _C, align
    lib = _C.lib()
    rng = np.random.default_rng(17)
    for B, L, V, d, h in ((5, 40, 36, 128, 256), (2, 21, 300, 64, 96)):
        vis, txt, mid, enc = (t(rng.standard_normal(s).astype(np.float32) * 0.5).bfloat16().contiguous()
                              for s in ((B, V, d), (B, L + 1, d), (B, V, h), (B, L, h)))
        gm, dout = t((rng.random(h) + 0.5).astype(np.float32)), t(rng.standard_normal((B, L, h)).astype(np.float32))
        res = []
        for gdt, tdt in ((_C.F32, torch.float32), (_C.BF16, torch.bfloat16)):
            nbytes = lib.vlg_attn_fuse_backward_workspace(B, L, V, d, h, gdt, 0)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
            outs = [torch.empty(s, dtype=tdt, device=dev()) for s in ((B, V, d), (B, L + 1, d), (B, V, h), (B, L, h))]
            outs += [torch.empty(h, dtype=torch.float32, device=dev()) for _ in range(2)]
            # (saved = NULL: the adjoint recomputes the forward's records -- the path torch.autograd does not take, it hands them over)
            _C.check(lib.vlg_attn_fuse_backward(_C.ptr(vis), _C.ptr(txt), _C.ptr(mid), _C.ptr(enc), _C.ptr(gm), _C.ptr(dout), L * h, h, B, L,
                                                V, d, h, _C.BF16, 1e-5, 0, gdt, None, _C.ptr(ws), nbytes, *(_C.ptr(o) for o in outs),
                                                _C.stream_of(vis)), "attn_fuse_backward")
            res.append(outs)
        for a, b in zip(res[0][:4], res[1][:4]):
            assert torch.equal(a.bfloat16(), b)
        for a, b in zip(res[0][4:], res[1][4:]):
            assert torch.equal(a, b)
        # through torch.autograd the adjoint receives the forward's merged records instead of recomputing them: the same bits
        leaves = [x.clone().requires_grad_(True) for x in (vis, txt, mid, enc)] + [gm.clone().requires_grad_(True), torch.zeros(h, device=dev(), requires_grad=True)]
        auto = torch.autograd.grad(align.attention_fuse(*leaves, 1e-5), leaves, dout)
        for a, b in zip(auto, res[1]):
            assert torch.equal(a, b)
    # fp32 inputs with bf16 gradients is not a combination the library builds
    f = [x.float() for x in (vis, txt, mid, enc)]
    rc = lib.vlg_attn_fuse_backward(*(_C.ptr(x) for x in f), _C.ptr(gm), _C.ptr(dout), L * h, h, B, L, V, d, h, _C.F32, 1e-5, 0, _C.BF16,
                                    None, _C.ptr(ws), nbytes, *(_C.ptr(o) for o in res[1]), _C.stream_of(vis))
    assert rc != 0 and b"grad_dtype" in lib.vlg_last_error()


def test_attn_fuse_backward_reproducible():
    """No atomics, fixed summation orders: two runs give identical bits."""
    rng = np.random.default_rng(5)
    B, L, V, d, h = 16, 40, 36, 128, 256
    arrs = [rng.standard_normal(s).astype(np.float32) for s in ((B, V, d), (B, L + 1, d), (B, V, h), (B, L, h))]
    gm, bt, dout = np.ones(h, np.float32), np.zeros(h, np.float32), rng.standard_normal((B, L, h)).astype(np.float32)
    _, g1 = _attn_grads(arrs, gm, bt, dout, 1e-5)
    _, g2 = _attn_grads(arrs, gm, bt, dout, 1e-5)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))


# ---- grounding loss on the fused alignment maxima (joint.py:439-491) ----
def _ground_inputs(g, bf16=False):
    from vlgae_amd import align
    txt, vis = t(g["txt"]), t(g["vis"])
    if bf16:
        txt, vis = txt.bfloat16(), vis.bfloat16()
    txt.requires_grad_(True)
    vis.requires_grad_(True)
    pen = seg = None
    if bool(g["use_pos_prior"]):
        pos_for = {k: t(g["pos_for_" + k]) for k in ("obj", "rel", "attr")}
        pen, seg = align.grounding_prior(t(g["tag"]), [str(n) for n in g["factor_names"]], [int(w) for w in g["vis_split"]],
                                         pos_for, txt.shape[1])
    return txt, vis, pen, seg


@pytest.mark.parametrize("B,L,V", [(1, 1, 1), (2, 5, 3), (3, 16, 16), (9, 24, 40), (10, 24, 41), (17, 40, 36), (31, 47, 64),
                                   (32, 7, 48), (33, 40, 5), (70, 33, 37)])
def test_grounding_dense_backward_shapes(oracle_mod, B, L, V):
    """The matrix-core backward (bf16, d = 128, Q <= 96, V <= 64) against the fp64 oracle over the corners of its launch logic:
    one pair, outer ranges that are not multiples of the staged chunk, split / unsplit outer loops (B < 32 runs unsplit), odd
    halves, 5 vs 8 staged segments per feature row (V <= 40 / > 40), every row-tile count, rows whose positions collide
    (argV[q] = v and argQ[v] = q happens for the best pair of every block)."""
    from vlgae_amd import align
    rng = np.random.default_rng(B * 977 + L * 31 + V)
    Q, d = 2 * (L + 1), 128
    lengths = rng.integers(max(1, L // 2), L + 1, B)
    m1 = np.concatenate([np.zeros((B, 1), bool), np.arange(L)[None] < lengths[:, None]], 1)
    tmask = np.concatenate([m1, m1], 1)
    vmask = rng.random((B, V)) > 0.15
    vmask[:, 0] = True
    txt = torch.from_numpy((rng.standard_normal((B, Q, d)) * 0.4).astype(np.float32)).bfloat16()
    vis = torch.from_numpy((rng.standard_normal((B, V, d)) * 0.4).astype(np.float32)).bfloat16()
    marg = (rng.random((B, Q)) * tmask).astype(np.float32)
    num = int(lengths.sum())
    ref = oracle_mod.grounding_loss(txt.float().numpy(), vis.float().numpy(), tmask, vmask, marg, num, 1.0, dtype=np.float64)
    tt, tv = txt.to(dev()).requires_grad_(True), vis.to(dev()).requires_grad_(True)
    total, sums = align.grounding_loss_factor_ce(tt, tv, t(tmask), t(vmask), t(marg), num, 1.0)
    s_ = sums.cpu().numpy()
    assert abs(s_[0] - ref["txt2vis"]) <= 1e-4 * max(1.0, abs(ref["txt2vis"]))
    assert abs(s_[1] - ref["vis2txt"]) <= 1e-4 * max(1.0, abs(ref["vis2txt"]))
    g_txt, g_vis = torch.autograd.grad(total, [tt, tv])
    for got, want in ((g_txt, ref["g_txt"]), (g_vis, ref["g_vis"])):
        assert np.abs(got.float().cpu().numpy() - want).max() <= 1e-2 * max(1.0, np.abs(want).max())
    # rows / regions that are masked out receive exactly zero
    assert not g_txt.float().cpu().numpy()[~tmask].any() and not g_vis.float().cpu().numpy()[~vmask].any()


@pytest.mark.parametrize("path", golden_files("ground_"), ids=golden_ids("ground_"))
def test_grounding_loss_golden(oracle_mod, path):
    """vlg_grounding_loss vs the reference's own gather_logit_simple -> loss_grounding_factor_ce + autograd."""
    from vlgae_amd import align
    g = load(path)
    txt, vis, pen, seg = _ground_inputs(g)
    if pen is not None:   # the host-side prior table against the oracle's restatement of joint.py:446-470
        pos_for = dict(obj=g["pos_for_obj"], rel=g["pos_for_rel"], attr=g["pos_for_attr"])
        open_, oseg = oracle_mod.grounding_prior(g["tag"], g["factor_names"], g["vis_split"], pos_for, txt.shape[1])
        assert np.array_equal(pen.cpu().numpy(), open_.astype(np.float32)) and np.array_equal(seg.cpu().numpy(), oseg)
    total, sums = align.grounding_loss_factor_ce(txt, vis, t(g["tmask"]), t(g["vmask"]), t(g["marginal"]), int(g["num_token"]),
                                                 float(g["vis2txt_weight"]), pen, seg)
    s = sums.cpu().numpy()
    assert abs(s[0] - float(g["txt2vis_raw"])) <= 1e-4 * abs(float(g["txt2vis_raw"]))
    assert abs(s[1] - float(g["vis2txt_raw"])) <= 1e-4 * abs(float(g["vis2txt_raw"]))
    assert abs(float(total) - float(g["total"])) <= 1e-4 * abs(float(g["total"]))
    g_txt, g_vis = torch.autograd.grad(total, [txt, vis])
    for name, got in (("g_txt", g_txt), ("g_vis", g_vis)):
        assert np.abs(got.cpu().numpy() - g[name]).max() <= 1e-4 * max(1.0, np.abs(g[name]).max()), name


@pytest.mark.parametrize("B,L,V,d,dt", [(5, 7, 9, 32, "f32"), (6, 40, 36, 128, "f32"), (6, 40, 36, 128, "bf16"),
                                        (3, 50, 70, 64, "f32"), (4, 47, 100, 128, "bf16"), (1, 3, 1, 32, "f32"),
                                        (3, 12, 1369, 128, "f32"), (2, 9, 520, 128, "bf16"),
                                        (6, 40, 1369, 128, "bf16"), (7, 30, 1200, 64, "f32"),
                                        (5, 60, 44, 128, "bf16"), (3, 20, 17, 128, "bf16"), (9, 47, 48, 128, "bf16"),
                                        (3, 3, 4100, 64, "f32")])
def test_grounding_loss_shapes(oracle_mod, B, L, V, d, dt):
    """Against the fp64 oracle: several row groups (Q > 96 / 48), several region groups (V > 48), one pair, bf16 storage
    (V <= 48: align_argmax_kernel, two passes at Q = 122, odd and full region counts, a batch that is no multiple of eight),
    the shipped factor layout's 1369 columns (image-side gradient rows split over several workgroups; caption side with
    one row per wave and the block-level scan of the scattered terms), and 4100 columns: eight strips of 513, one more than a block
    of the LDS-tile cross-entropy has threads, so the streaming cross-entropy kernel (ground_ce_kernel) runs."""
    from vlgae_amd import align
    rng = np.random.default_rng(B * 131 + L * 7 + V)
    Q = 2 * (L + 1)
    lengths = rng.integers(max(1, L // 2), L + 1, B)
    m1 = np.concatenate([np.zeros((B, 1), bool), np.arange(L)[None] < lengths[:, None]], 1)
    tmask = np.concatenate([m1, m1], 1)
    vmask = rng.random((B, V)) > 0.2
    vmask[:, 0] = True
    txt = (rng.standard_normal((B, Q, d)) * 0.5).astype(np.float32)
    vis = (rng.standard_normal((B, V, d)) * 0.5).astype(np.float32)
    marg = (rng.random((B, Q)) * tmask).astype(np.float32)
    split = [V] if V < 4 else [V // 2, V - V // 2 - 1, 1]
    names = ["obj"] if V < 4 else ["obj", "rel", "img"]
    tag = rng.integers(0, 6, (B, L))
    pos_for = dict(obj=np.array([0, 1]), rel=np.array([1, 2]), attr=np.array([5]))
    pen, seg = oracle_mod.grounding_prior(tag, names, split, pos_for, Q)
    if dt == "bf16":
        txt, vis = (torch.from_numpy(a).bfloat16().float().numpy() for a in (txt, vis))
    ref = oracle_mod.grounding_loss(txt, vis, tmask, vmask, marg, int(lengths.sum()), 1.0, pen, seg, -1e20, np.float64)
    tt, tv = t(txt), t(vis)
    if dt == "bf16":
        tt, tv = tt.bfloat16(), tv.bfloat16()
    tt.requires_grad_(True)
    tv.requires_grad_(True)
    total, sums = align.grounding_loss_factor_ce(tt, tv, t(tmask), t(vmask), t(marg), int(lengths.sum()), 1.0,
                                                 t(pen.astype(np.float32)), t(seg))
    s = sums.cpu().numpy()
    assert abs(s[0] - ref["txt2vis"]) <= 1e-4 * max(1.0, abs(ref["txt2vis"]))
    assert abs(s[1] - ref["vis2txt"]) <= 1e-4 * max(1.0, abs(ref["vis2txt"]))
    g_txt, g_vis = torch.autograd.grad(total, [tt, tv])
    tol = 1e-2 if dt == "bf16" else 1e-4   # bf16 gradients are rounded on return
    assert np.abs(g_txt.float().cpu().numpy() - ref["g_txt"]).max() <= tol * max(1.0, np.abs(ref["g_txt"]).max())
    assert np.abs(g_vis.float().cpu().numpy() - ref["g_vis"]).max() <= tol * max(1.0, np.abs(ref["g_vis"]).max())
    # bit-reproducible: no atomics
    total2, _ = align.grounding_loss_factor_ce(tt, tv, t(tmask), t(vmask), t(marg), int(lengths.sum()), 1.0,
                                               t(pen.astype(np.float32)), t(seg))
    g2 = torch.autograd.grad(total2, [tt, tv])
    assert torch.equal(g2[0], g_txt) and torch.equal(g2[1], g_vis)


# ---- gather_logit_reduced (joint.py:421-432) + the caption-image cross-entropy (:493-499) ----
@pytest.mark.parametrize("path", golden_files("reduced_"), ids=golden_ids("reduced_"))
def test_gather_logit_reduced_golden(path):
    from vlgae_amd import align
    g = load(path)
    txt, vis = t(g["txt"]).requires_grad_(), t(g["vis"]).requires_grad_()
    logit = align.gather_logit_reduced(None, None, (vis, t(g["vmask"]), None), (txt, t(g["tmask"]), t(g["marginal"])), None)
    assert np.allclose(logit.detach().cpu().numpy(), g["logit"], rtol=1e-4, atol=1e-4)
    loss = torch.nn.functional.cross_entropy(logit, torch.arange(len(logit), device=dev()))      # joint.py:498
    assert abs(float(loss) - float(g["loss"])) <= 1e-4 * max(1.0, abs(float(g["loss"])))
    g_txt, g_vis = torch.autograd.grad(loss, [txt, vis])
    for name, got in (("g_txt", g_txt), ("g_vis", g_vis)):
        assert np.abs(got.cpu().numpy() - g[name]).max() <= 1e-4 * max(1.0, np.abs(g[name]).max()), name


@pytest.mark.parametrize("B,L,V,d,dt", [(5, 7, 9, 32, "f32"), (6, 40, 36, 128, "bf16"), (3, 50, 70, 64, "f32"), (1, 3, 1, 32, "f32")])
def test_gather_logit_reduced_shapes(oracle_mod, B, L, V, d, dt):
    from vlgae_amd import align
    rng = np.random.default_rng(B * 31 + L + V)
    Q = 2 * (L + 1)
    lengths = rng.integers(max(1, L // 2), L + 1, B)
    m1 = np.concatenate([np.zeros((B, 1), bool), np.arange(L)[None] < lengths[:, None]], 1)
    tmask = np.concatenate([m1, m1], 1)
    vmask = rng.random((B, V)) > 0.2
    vmask[:, 0] = True
    txt = (rng.standard_normal((B, Q, d)) * 0.5).astype(np.float32)
    vis = (rng.standard_normal((B, V, d)) * 0.5).astype(np.float32)
    marg = (rng.random((B, Q)) * tmask).astype(np.float32)
    g_logit = rng.standard_normal((B, B)).astype(np.float32)
    if dt == "bf16":
        txt, vis = (torch.from_numpy(a).bfloat16().float().numpy() for a in (txt, vis))
    ref = oracle_mod.gather_logit_reduced(txt, vis, tmask, vmask, marg, g_logit)
    tt, tv = t(txt), t(vis)
    if dt == "bf16":
        tt, tv = tt.bfloat16(), tv.bfloat16()
    tt.requires_grad_(True)
    tv.requires_grad_(True)
    logit = align.gather_logit_reduced(None, None, (tv, t(vmask), None), (tt, t(tmask), t(marg)), None)
    assert np.allclose(logit.detach().cpu().numpy(), ref["logit"], rtol=1e-4, atol=1e-4)
    g_txt, g_vis = torch.autograd.grad(logit, [tt, tv], t(g_logit), retain_graph=True)
    tol = 1e-2 if dt == "bf16" else 1e-4   # bf16 gradients are rounded on return
    assert np.abs(g_txt.float().cpu().numpy() - ref["g_txt"]).max() <= tol * max(1.0, np.abs(ref["g_txt"]).max())
    assert np.abs(g_vis.float().cpu().numpy() - ref["g_vis"]).max() <= tol * max(1.0, np.abs(ref["g_vis"]).max())
    g2 = torch.autograd.grad(logit, [tt, tv], t(g_logit))       # the backward may run again on the same forward state
    assert torch.equal(g2[0], g_txt) and torch.equal(g2[1], g_vis)


# ---- grounding decoder (joint.py:512-629) on the fused alignment outputs ----
class _VP(dict):
    __getattr__ = dict.__getitem__


def _decode_stub(g):
    from types import SimpleNamespace as NS
    me = NS(cfg=NS(decode_grounding_args=NS(use_pos_prior=bool(g["use_pos_prior"]), use_heuristic=bool(g["use_heuristic"]))),
            vis_factor_names=[str(n) for n in g["factor_names"]], pos_for_obj=t(g["pos_for_obj"]),
            pos_for_rel=t(g["pos_for_rel"]), pos_for_attr=t(g["pos_for_attr"]))
    L = g["tag"].shape[1]
    vp = _VP(tag=t(g["tag"]), mask=torch.zeros(len(g["tag"]), L, dtype=torch.bool))
    if g["vis_box_index"].size:
        vp["vis_box_index"] = torch.from_numpy(g["vis_box_index"])
    return me, vp


@pytest.mark.parametrize("path", golden_files("gdecode_"), ids=golden_ids("gdecode_"))
def test_grounding_decode_golden(path):
    """decode_grounding_on_factor registered from vlgae_amd.align vs the reference's own method (lists and edited block)."""
    from conftest import gdecode_check_lists
    from vlgae_amd import align
    g = load(path)
    me, vp = _decode_stub(g)
    split = [int(w) for w in g["vis_split"]]
    inputs = {"txt_packed": (t(g["txt"]), t(g["tmask"]), None), "vis_packed": (t(g["vis"]), t(g["vmask"]), split)}
    out = align.decode_grounding_on_factor(me, inputs, vp)
    gdecode_check_lists(out["txt_to_factor"], out["txt_to_img"], g, g["diag_after"])
    # the edited block itself: same fp32 edits on alignment values that agree to rounding
    names = me.vis_factor_names
    start = np.concatenate([[0], np.cumsum(split)])
    pen = seg = None
    if bool(g["use_pos_prior"]):
        pos_for = {k: t(g["pos_for_" + k]) for k in ("obj", "rel", "attr")}
        pen, seg = align.grounding_prior(t(g["tag"]), names, split, pos_for, g["txt"].shape[1], scale=1e10)
    r = align.grounding_decode(t(g["txt"]), t(g["vis"]), t(g["tmask"]), t(g["vmask"]), pen, seg, bool(g["use_heuristic"]),
                               split[0], int(start[names.index("rel")]) if "rel" in names else -1,
                               int(start[names.index("attr")]) if "attr" in names else -1, g["tag"].shape[1] + 1)
    got = r["logit"].cpu().numpy()
    assert np.allclose(got, g["diag_after"], rtol=1e-5, atol=1e-4)
    top = r["top5"].cpu().numpy().astype(np.int64)
    assert np.allclose(np.take_along_axis(got, top[..., :g["top_vals"].shape[-1]], -1), g["top_vals"], rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("B,L,n_box,with_rel,with_attr,d,dt", [(6, 40, 36, True, True, 128, "f32"), (3, 12, 10, True, False, 64, "bf16"),
                                                               (4, 9, 70, False, True, 32, "f32"), (2, 5, 3, False, False, 32, "f32")])
def test_grounding_decode_shapes(oracle_mod, B, L, n_box, with_rel, with_attr, d, dt):
    """Edits, top five and image arg-max against the oracle on the kernel's own alignment block (bit-exact: the same fp32
    operations per element); the shipped factor layout obj + rel (n_box^2 columns) + attr + img at V = 1369."""
    from vlgae_amd import align
    rng = np.random.default_rng(B * 17 + L + n_box)
    names, split = ["obj"], [n_box]
    if with_rel:
        names.append("rel"); split.append(n_box * n_box)
    if with_attr:
        names.append("attr"); split.append(n_box)
    names.append("img"); split.append(1)
    V, Q = sum(split), 2 * (L + 1)
    lengths = rng.integers(max(1, L // 2), L + 1, B)
    m1 = np.concatenate([np.zeros((B, 1), bool), np.arange(L)[None] < lengths[:, None]], 1)
    tmask = np.concatenate([m1, m1], 1)
    vmask = rng.random((B, V)) > 0.1
    vmask[:, 0] = True
    txt = t((rng.standard_normal((B, Q, d)) * 0.5).astype(np.float32))
    vis = t((rng.standard_normal((B, V, d)) * 0.5).astype(np.float32))
    if dt == "bf16":
        txt, vis = txt.bfloat16(), vis.bfloat16()
    tag = rng.integers(0, 6, (B, L))
    pos_for = dict(obj=np.array([0, 1]), rel=np.array([1, 2]), attr=np.array([5]))
    start = np.concatenate([[0], np.cumsum(split)])
    pen, seg = align.grounding_prior(t(tag), names, split, {k: t(v) for k, v in pos_for.items()}, Q, scale=1e10)
    before = align.bilinear_align(txt, vis, t(tmask), t(vmask), full=False, max_v=True, diag=True)
    r = align.grounding_decode(txt, vis, t(tmask), t(vmask), pen, seg, True, n_box,
                               int(start[names.index("rel")]) if with_rel else -1,
                               int(start[names.index("attr")]) if with_attr else -1, L + 1)
    ref = oracle_mod.grounding_decode(before["diag"].cpu().numpy(), before["max_v"].cpu().numpy(), tag, names, split, pos_for,
                                      True, True)
    got = r["logit"].cpu().numpy()
    assert np.array_equal(got, ref["logit"])
    assert np.array_equal(r["top5"].cpu().numpy()[..., :min(5, V)], ref["top5"])
    assert np.array_equal(r["factor2img"].cpu().numpy(), ref["factor2img"])
    # one workgroup per sentence (no row split): same bits
    r1 = align.grounding_decode(txt, vis, t(tmask), t(vmask), pen, seg, True, n_box,
                                int(start[names.index("rel")]) if with_rel else -1,
                                int(start[names.index("attr")]) if with_attr else -1, L + 1, split_rows=False)
    assert torch.equal(r1["logit"], r["logit"]) and torch.equal(r1["top5"], r["top5"]) and torch.equal(r1["factor2img"], r["factor2img"])
    # no prior, no heuristic: the block is untouched and only sorted
    r0 = align.grounding_decode(txt, vis, t(tmask), t(vmask))
    assert torch.equal(r0["logit"], before["diag"])
    assert np.array_equal(r0["top5"].cpu().numpy()[..., :min(5, V)],
                          np.argsort(-before["diag"].cpu().numpy().astype(np.float64), axis=-1, kind="stable")[..., :5])


# ---- arc encoder (joint.py:281-287): trilinear term on the matrix cores ----
@pytest.mark.parametrize("path", golden_files("arcenc_"), ids=golden_ids("arcenc_"))
def test_arc_encoder_golden(path):
    from conftest import arcenc_check_w1_grad, arcenc_w1
    from vlgae_amd import align
    g = load(path)
    leaves = [t(g["child"]), t(g["parent"]), t(arcenc_w1(g)), t(g["w2"]), t(g["b"])]
    for a in leaves:
        a.requires_grad_(True)
    arc = align.arc_encoder(*leaves)
    assert np.abs(arc.detach().cpu().numpy() - g["arc"]).max() <= 1e-4 * max(1.0, np.abs(g["arc"]).max())
    grads = torch.autograd.grad(arc, leaves, t(g["dout"]))
    for name, got in (("g_child", grads[0]), ("g_parent", grads[1]), ("g_w2", grads[3]), ("g_b", grads[4])):
        assert np.abs(got.cpu().numpy() - g[name]).max() <= 1e-4 * max(1.0, np.abs(g[name]).max()), name
    arcenc_check_w1_grad(grads[2].cpu().numpy(), g, 1e-4)


@pytest.mark.parametrize("M,X,H,Y,dt", [(100, 32, 32, 32, "f32"), (333, 64, 128, 32, "f32"), (77, 128, 64, 128, "f32"),
                                        (1050, 128, 128, 128, "bf16"), (2501, 128, 128, 128, "bf16"), (65, 48, 32, 64, "bf16"),
                                        (1, 16, 32, 32, "f32")])
def test_arc_trilinear_shapes(oracle_mod, M, X, H, Y, dt):
    """Ragged row counts (M % 64, M % 32 != 0), unequal X / H / Y, against the fp64 oracle."""
    from vlgae_amd import align
    rng = np.random.default_rng(M * 7 + X)
    child, parent = (rng.standard_normal((M, X)) * 0.5).astype(np.float32), (rng.standard_normal((M, Y)) * 0.5).astype(np.float32)
    w1 = (rng.standard_normal((X, H, Y)) / np.sqrt(X * Y)).astype(np.float32)
    g = rng.standard_normal((M, H)).astype(np.float32)
    if dt == "bf16":
        child, parent, w1 = (torch.from_numpy(a).bfloat16().float().numpy() for a in (child, parent, w1))
    ref = oracle_mod.arc_encoder(child, parent, w1, None, None, np.float64)
    d_child, d_parent, d_w1, _, _ = oracle_mod.arc_encoder_backward(child, parent, w1, None, g, np.float64)
    leaves = [t(child), t(w1), t(parent)]
    if dt == "bf16":
        leaves = [a.bfloat16() for a in leaves]
    for a in leaves:
        a.requires_grad_(True)
    out = align.arc_trilinear(*leaves)
    assert out.dtype == torch.float32 and tuple(out.shape) == (M, H)
    assert np.abs(out.detach().cpu().numpy() - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())
    grads = torch.autograd.grad(out, leaves, t(g))
    tol = 2e-2 if dt == "bf16" else 1e-4   # bf16: the cotangent and the returned gradients are rounded to 8 bits
    for name, got, want in (("d_child", grads[0], d_child), ("d_w1", grads[1], d_w1), ("d_parent", grads[2], d_parent)):
        assert np.abs(got.float().cpu().numpy() - want).max() <= tol * max(1.0, np.abs(want).max()), name
    if M >= 1024:   # the LDS-staged kernels (tri2_kernel, tri_dw2_kernel): fixed-order partial slabs -> run-to-run bit equality
        out2 = align.arc_trilinear(*leaves)
        grads2 = torch.autograd.grad(out2, leaves, t(g))
        assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))


@pytest.mark.parametrize("M", [1050, 10496])
def test_arc_trilinear_float32_on_fp16_parts(M):
    """float32 operands at X = H = Y = 128 (the reference's `precision: 32`): every MFMA operand row as two fp16 parts under a power-of-two row
    scale, three products per pair (tri3_kernel, tri_dw3_kernel).  Against float64 torch: the error must stay at float32's own level -- 2e-6 of the
    largest entry (the exact-fp32 kernels measured 6e-6 at M = 10 496; two bf16 parts, round 4: 2e-5) -- with rows / cotangents whose magnitudes
    span 2^24 (every ROW of the row-wise results is held to 1e-5 of its own largest entry: the row scales), and bit-reproducible."""
    from vlgae_amd import align
    gen = torch.Generator().manual_seed(M)
    rows = torch.exp2(torch.randint(-12, 13, (M, 1), generator=gen).float())             # per-row magnitudes 2^-12 .. 2^12
    child = (torch.randn(M, 128, generator=gen) * 0.5 * rows).to(dev()).requires_grad_(True)
    parent = (torch.randn(M, 128, generator=gen) * 0.5 * rows.flip(0)).to(dev()).requires_grad_(True)
    w1 = (torch.randn(128, 128, 128, generator=gen) / 128 * torch.exp2(torch.randint(-6, 7, (128, 128, 1), generator=gen).float())).to(dev()).requires_grad_(True)
    g = (torch.randn(M, 128, generator=gen) * 1e-4 * torch.exp2(torch.randint(-10, 11, (M, 1), generator=gen).float())).to(dev())
    out = align.arc_trilinear(child, w1, parent)
    grads = torch.autograd.grad(out, [child, w1, parent], g)
    out2 = align.arc_trilinear(child, w1, parent)
    grads2 = torch.autograd.grad(out2, [child, w1, parent], g)
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    c64, w64, p64 = (a.detach().double().requires_grad_(True) for a in (child, w1, parent))
    t = torch.einsum("mhy,my->mh", torch.einsum("mx,xhy->mhy", c64, w64), p64)
    r_c, r_w, r_p = torch.autograd.grad(t, [c64, w64, p64], g.double())
    for name, got, want, rowwise in (("out", out, t.detach(), True), ("d_child", grads[0], r_c, True), ("d_w", grads[1], r_w, False), ("d_parent", grads[2], r_p, True)):
        err = (got.double() - want).abs()
        assert float(err.max()) <= 2e-6 * float(want.abs().max()), (name, float(err.max()) / float(want.abs().max()))
        if rowwise:
            rel = err.amax(1) / want.abs().amax(1).clamp_min(1e-300)
            assert float(rel.max()) <= 1e-5, (name, float(rel.max()))


def test_training_step_chain_as_one_hip_graph():
    """The chained training-step hot path (vlgae_amd/train_step.py: attention-fuse -> library GEMMs -> DMV marginals + heads on two
    streams -> arc encoder -> grounding loss -> -DMV.max -> every gradient) captured as ONE HIP graph: capture succeeds (no
    entry point synchronises, allocates through the driver or reads a device value on the host), and a replay gives the eager
    step's loss bit for bit and its gradients to one bf16 ulp."""
    from vlgae_amd import train_step
    with torch.autograd.set_multithreading_enabled(False):
        # fixed SharedDropout masks: a replay must reproduce the eager step (masks drawn inside the step differ per replay by design)
        gen = torch.Generator().manual_seed(5)
        drop = (torch.rand(4, 64, 128, generator=gen) >= 0.33).float() / 0.67
        enc_drop = (torch.rand(64, 24, 96, generator=gen) >= 0.33).float() / 0.67
        step = train_step.build(64, 24, 20, dev(), dtype=torch.bfloat16, E=96, H=64, nb=24, n_vis=256, given=dict(drop=drop, enc_drop=enc_drop),
                                p_ff_drop=0.0, p_mid_drop=0.0)
        for _ in range(3):
            total, grads, pot_grads = step()
        want = [total.detach().clone()] + [grads[k].clone() for k in step.names] + [g.clone() for g in pot_grads]
        # nothing of an earlier step's autograd graph may be alive across the capture: torch 2.10 / ROCm 7 segfaults in
        # capture_end when a loss tensor of a previous eager step is still referenced (a plain x @ w -> relu -> sum step does
        # it too; nothing to do with these kernels)
        del total, grads, pot_grads
        gr = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(device=dev())
        side.wait_stream(torch.cuda.current_stream(dev()))
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream(dev()).wait_stream(side)
        with torch.cuda.graph(gr):
            total_g, grads_g, pot_g = step()
        for _ in range(2):
            gr.replay()
        torch.cuda.synchronize()
        got = [total_g] + [grads_g[k] for k in step.names] + list(pot_g)
        assert torch.equal(total_g.detach(), want[0])
        for a, b in zip(got, want):
            # (the loss is bit-equal; gradients that pass through torch's gather backward -- an atomic scatter-add over repeated
            #  parents -- are order-dependent from run to run, eager or not: one bf16 ulp is allowed there)
            assert torch.allclose(a.float(), b.float(), rtol=2.0 ** -7, atol=2.0 ** -7 * float(b.float().abs().max()))


def _tools_path():
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)


def _bf16_grid(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(torch.float32).numpy()


def trainstep_from_fixture(g, dtype, ff_dtype=None):
    """vlgae_amd.train_step.build (the function bench.py times) on a trainstep_* fixture's tensors: the raw embeddings and region
    features, every parameter (the two encoders' included), the recorded dropout masks.  Everything -- the parser's feed-forwards
    too -- runs in `dtype`, exactly as `bench.py` runs it, unless ff_dtype says otherwise.  Returns (step, reference gradients keyed
    like the step's leaves)."""
    from vlgae_amd import train_step
    B, L, E = g["emb"].shape
    R, n_vis = g["vis_box_feat"].shape[1:]
    h, d = g["w_text"].shape[0], g["w2"].shape[0]
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    if "w1" in g:
        w1, g_w1 = g["w1"], g["g_w1"]
    else:   # rank factors; the reference ran on the bf16-rounded product (make_golden.trainstep_cases)
        w1 = _bf16_grid(np.einsum("xr,hr,yr->xhy", g["w1_u"], g["w1_v"], g["w1_z"]).astype(np.float32))
        g_w1 = None
    factors = [str(n) for n in g["factor_names"]][1:]
    fcs = ["box_fc"] + [f + "_fc" for f in ("rel", "attr") if f in factors]          # the encoders whose outputs the model reads, stacked
    cat = lambda pre, suf: np.concatenate([g[f"{pre}vis.{m}.{suf}"] for m in fcs], 0)
    given = dict(emb=tt(g["emb"]), vis_box_feat=tt(g["vis_box_feat"]), w_text=tt(g["w_text"]), w_venc=tt(cat("", "weight")), b_venc=tt(cat("", "bias")),
                 w_vis=tt(g["w_vis"]),
                 w_enc=tt(np.concatenate([g["w_word"], g["w_child"], g["w_parent"]], 0)),
                 b_enc=tt(np.concatenate([g["b_word"], g["b_child"], g["b_parent"]], 0)), ln_w=tt(g["ln_w"]), ln_b=tt(g["ln_b"]),
                 w1=tt(w1), w2=tt(g["w2"]), b=tt(g["b_arc"]), token_emb=tt(g["token_emb"]), root_emb=tt(g["root_emb"]),
                 dec_emb=tt(g["dec_emb"]), lengths=tt(g["lengths"]), token=tt(g["token"]), tag=tt(g["tag"]), box_mask=tt(g["box_mask"]),
                 drop=tt(g["drop_masks"]) if g["drop_masks"].shape[0] else None,
                 enc_drop=tt(g["enc_drop_mask"]) if g["enc_drop_mask"].shape[0] else None)
    given.update({k: tt(v) for k, v in g.items() if k.startswith("ff.")})
    pos_for = {k: tt(g["pos_for_" + k]) for k in ("obj", "rel", "attr")}
    step = train_step.build(B, L, R, dev(), dtype=dtype, ff_dtype=ff_dtype, d=d, h=h, E=E, n_vis=int(n_vis), given=given, alpha=float(g["alpha"]), use_pos_prior=True,
                            p_ff_drop=0.0, p_mid_drop=0.0,   # (the fixtures ran the parser's feed-forwards without their dropout)
                            p_enc=float(g["p_enc"]), vis2txt=float(g["vis2txt_weight"]), factors=factors, pos_for=pos_for, ln_eps=float(g["ln_eps"]),
                            feature_grads=True)
    assert step.batch["vis_split"] == [int(w) for w in g["vis_split"]] and np.array_equal(step.batch["vis_mask"].cpu().numpy(), g["vis_mask"])
    ref = {k: g["g_" + k] for k in ("emb", "vis_box_feat", "w_text", "w_vis", "ln_w", "ln_b", "w2", "token_emb", "root_emb", "dec_emb")}
    ref.update({k: g["g_" + k] for k in g if k.startswith("ff.")})
    ref["w_venc"], ref["b_venc"] = cat("g_", "weight"), cat("g_", "bias")
    ref["w_enc"] = np.concatenate([g["g_w_word"], g["g_w_child"], g["g_w_parent"]], 0)
    ref["b_enc"] = np.concatenate([g["g_b_word"], g["g_b_child"], g["g_b_parent"]], 0)
    ref["b"] = g["g_b_arc"]
    ref["w1"] = g_w1
    return step, ref


@pytest.mark.parametrize("dtype,ff_dtype", [(torch.float32, None), (torch.bfloat16, None), (torch.bfloat16, torch.float32)], ids=["f32", "bf16", "bf16_ff32"])
@pytest.mark.parametrize("path", golden_files("trainstep_"), ids=golden_ids("trainstep_"))
def test_training_step_reference_wiring(path, dtype, ff_dtype):
    """THE function `bench.py` times as configs[4] (vlgae_amd.train_step.build, wiring="reference") against one whole training step
    executed by the reference's own modules and methods (make_golden.trainstep_cases: VisBoxRelSimpleEncoder.forward + MLPEncoder.forward
    on the frozen features -> DependencyBoxRel._forward -> DiscriminativeNDMV._forward -> _vis_forward -> loss with alpha = 0.5, POS
    prior, ragged vis_mask, live nn.Dropout / SharedDropout masks -> reduce_loss('token') -> autograd): every intermediate the fixture
    holds and the gradient of the reduced loss w.r.t. every input feature (raw embeddings, raw region features) and parameter.

    f32 (the reference's `precision: 32`): values to 1e-4 * max|.|, heads and masks exact, loss to 1e-5 relative, gradients to
    3e-4 * max|g| (fp32 summation order in the split reductions; the alignment's arg-max positions are exact at this precision).
    bf16 (BASELINE.json configs[4], EXACTLY what bench.py times: every feature, parameter and activation between kernels stored in bf16,
    fp32 accumulation, the parser's six-layer feed-forwards included): inputs sit on the bf16 grid, so both sides start from identical
    numbers: values to 3e-2 * max|.| (potentials 5e-2 absolute), loss and the Viterbi score -max to 1e-2 relative.  The potentials of
    these small fixtures are scorer outputs amplified 36-100x to give the trees a spread of ~1.5 nats (make_golden: sc_gain), so a
    bf16 potential carries ~2e-2 nats of rounding and attachments whose best alternatives lie within that flip: heads equal on >= 45 %
    of the words here (observed 50 / 86 / 90 %; 96.7 % at B = 256 with unamplified scorers, ..._config_size[bf16]) -- what stays pinned
    is that the tree chosen is a near-tie (the -max score bound).  Gradients: 8e-2 relative L2 per tensor when every tree agrees, a
    sanity bound (0.5) when >= 85 % of the words do, finiteness below that (the -max term's gradient IS the tree).
    bf16_ff32: the same with the parser's feed-forwards kept in float32 -- the potentials then differ from the reference's only through
    the hot path's own rounding: heads equal on >= 95 % of the words; the other bounds as for bf16."""
    g = load(path)
    f32 = dtype == torch.float32
    with torch.autograd.set_multithreading_enabled(False):
        step, ref = trainstep_from_fixture(g, dtype, ff_dtype)
        loss, grads, _ = step()
        last = step.last
    npf = lambda x: x.detach().float().cpu().numpy()
    vtol = 1e-4 if f32 else 3e-2

    def close(name, got, want, tol=vtol):
        err = np.abs(got - want).max()
        assert err <= tol * max(1.0, np.abs(want).max()), (name, err, np.abs(want).max())

    close("enc_x", npf(last["enc_x"]), g["enc_x"])
    close("vis_mid", npf(last["vis_mid"]), g["vis_mid"])
    close("x_fused", npf(last["x_fused"]), g["x_fused"])
    fin = g["merged_attach"] > -1e11
    close("merged_attach", npf(last["merged_attach"])[fin], g["merged_attach"][fin], 2e-5 if f32 else 5e-2)
    assert np.array_equal(npf(last["merged_attach"])[~fin], g["merged_attach"][~fin])
    find = g["merged_dec"] > -1e11
    close("merged_dec", npf(last["merged_dec"])[find], g["merged_dec"][find], 2e-5 if f32 else 5e-2)
    heads = last["heads"].cpu().numpy()
    valid = np.concatenate([np.zeros((len(g["lengths"]), 1), bool), np.arange(g["token"].shape[1])[None] < g["lengths"][:, None]], 1)
    agree = (heads == g["predicted"])[valid].mean()
    assert agree == 1.0 if f32 else agree >= (0.95 if ff_dtype == torch.float32 else 0.45), agree
    assert np.array_equal(last["txt_mask"].cpu().numpy(), g["txt_mask"])
    if f32 or agree == 1.0:
        close("txt", npf(last["txt"]), g["txt"])
        close("txt_marginal", npf(last["txt_marginal"]), g["txt_marginal"], 1e-4 if f32 else 2e-2)
    close("vis_feat", npf(last["vis_feat"]), g["vis_feat"])
    ltol = 1e-5 if f32 else 1e-2
    dep = -float(last["viterbi_max"].double().sum())
    assert abs(dep - float(g["dep_loss"])) <= ltol * abs(float(g["dep_loss"]))
    total = step.batch["alpha"] * float(last["mt_loss"]) + (1 - step.batch["alpha"]) * dep
    assert abs(total - float(g["total"])) <= ltol * abs(float(g["total"]))
    assert abs(float(loss) - float(g["loss"])) <= ltol * abs(float(g["loss"]))
    worst = {}
    gmax = max(float(np.abs(v).max()) for v in list(ref.values()) + [g["g_w1_sample"] if ref["w1"] is None else ref["w1"]] if v is not None)
    same_tree = agree == 1.0
    for k in step.names:
        got = npf(grads[k])
        if k == "w1" and ref[k] is None:
            got, want = got[::5, ::7, ::3], g["g_w1_sample"]
        else:
            want = ref[k]
        assert got.shape == want.shape, k
        # absolute floors relative to the largest gradient of the step (1e-6 of it in float32, 2e-3 per element in bf16): a softmax is invariant to a bias shared by its arguments
        # (attach_scorer.project2.bias), so some reference gradients are pure rounding noise (~1e-8 here)
        if f32:
            err = max(np.abs(got - want).max() - 1e-6 * gmax, 0.0) / max(np.abs(want).max(), 1e-12)
            worst[k] = np.abs(got - want).max() / max(np.abs(want).max(), 1e-6 * gmax)
            assert err <= 3e-4, (k, err)
        else:
            err = max(np.linalg.norm((got - want).ravel()) - 2e-3 * gmax * np.sqrt(want.size), 0.0) / max(np.linalg.norm(want.ravel()), 1e-12)
            worst[k] = np.linalg.norm((got - want).ravel()) / max(np.linalg.norm(want.ravel()), 2e-3 * gmax * np.sqrt(want.size))
            # where bf16 rounding flipped a near-tied arc of the Viterbi tree (<= 5 % of the words) the rows of that sentence feed
            # different parents into the arc encoder: only a sanity bound then
            # ... and where more than 15 % of the words changed heads (the smallest all-bf16 fixture) the -max term's gradient is that of
            # another derivation altogether: finiteness only
            assert np.isfinite(got).all(), k
            assert agree < 0.85 or err <= (8e-2 if same_tree else 0.5), (k, err, agree)
    print(f"heads agree {agree:.3f}, largest |gradient| {gmax:.3g}, loss {float(loss):.6f} vs {float(g['loss']):.6f}; worst gradient errors:",
          {k: float(f"{v:.2e}") for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:6]})


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("path", golden_files("trainstep_"), ids=golden_ids("trainstep_"))
def test_training_step_reference_wiring_teacher_forced(path, dtype):
    """The same function on the same fixtures with the TREE TAKEN OUT of the comparison: `step.forced_heads` = the fixture's `predicted`
    (the reference's own Viterbi heads, joint.py:256-258), so lang_feat_max_tree reads the reference's parents and marginals and the
    parser's loss is -score(that tree) -- the function of the parameters the reference differentiated (it treats its tree as a constant,
    joint.py:256-273, ldndmv.py:277-281).  What is left between the two sides in bf16 is rounding alone: EVERY gradient tensor is bounded
    on ALL fixtures (0.12 relative L2 on the hot path, 0.3 for the parser's feed-forwards: see the end of the test; the free-running
    variant above can only assert finiteness where bf16 flipped near-tied attachments), txt and its marginals to the bf16 value tolerance.  f32: the bounds of the free-running case (the trees agree there)."""
    g = load(path)
    f32 = dtype == torch.float32
    with torch.autograd.set_multithreading_enabled(False):
        step, ref = trainstep_from_fixture(g, dtype)
        step.forced_heads = t(g["predicted"]).long()
        loss, grads, _ = step()
        last = step.last
    npf = lambda x: x.detach().float().cpu().numpy()
    assert np.array_equal(last["heads"].cpu().numpy(), g["predicted"])
    vtol = 1e-4 if f32 else 3e-2
    for name, tol in (("txt", vtol), ("txt_marginal", 1e-4 if f32 else 2e-2), ("vis_feat", vtol), ("x_fused", vtol)):
        got, want = npf(last[name]), g[name]
        assert np.abs(got - want).max() <= tol * max(1.0, np.abs(want).max()), name
    ltol = 1e-5 if f32 else 1e-2
    assert abs(float(loss) - float(g["loss"])) <= ltol * abs(float(g["loss"])), (float(loss), float(g["loss"]))
    gmax = max(float(np.abs(v).max()) for v in list(ref.values()) + [g["g_w1_sample"] if ref["w1"] is None else ref["w1"]] if v is not None)
    worst, bad = {}, {}
    for k in step.names:
        got = npf(grads[k])
        got, want = (got[::5, ::7, ::3], g["g_w1_sample"]) if k == "w1" and ref[k] is None else (got, ref[k])
        assert got.shape == want.shape, k
        if f32:
            err = max(np.abs(got - want).max() - 1e-6 * gmax, 0.0) / max(np.abs(want).max(), 1e-12)
            worst[k] = err
            assert err <= 3e-4, (k, err)
        else:   # absolute floor 2e-3 * max|g| per element, as in the free-running case (softmax-invariant biases are rounding noise)
            floor = 2e-3 * gmax * np.sqrt(want.size)
            err = max(np.linalg.norm((got - want).ravel()) - floor, 0.0) / max(np.linalg.norm(want.ravel()), 1e-12)
            worst[k] = np.linalg.norm((got - want).ravel()) / max(np.linalg.norm(want.ravel()), floor)
            bad[k] = err
    print("teacher-forced", "f32" if f32 else "bf16", "worst gradient errors:", {k: float(f"{v:.2e}") for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:8]})
    # bf16, same tree on both sides: 0.12 relative L2 for every tensor of the hot path (observed over the three fixtures: <= 0.104 -- the raw
    # region features' gradient on the B = 8 fixture; w_venc / b_venc / b 0.08; everything else <= 0.07), 0.3 for the parser's six-layer
    # LeakyReLU feed-forwards and their embeddings (observed <= 0.27 on the 3-sentence fixture, <= 0.10 on the 8-sentence one: a
    # pre-activation within bf16 rounding of zero takes the other branch and its term changes by 1 / slope = 100x, and a 24-to-150-element
    # bias gradient of a 3-sentence batch is a handful of such terms; these fixtures also amplify the scorer outputs 36-100x).  The
    # free-running variant could only assert finiteness here.
    for k, err in bad.items():
        assert err <= (0.3 if k.startswith("ff.") or k.endswith("_emb") else 0.12), (k, err)


@pytest.mark.parametrize("dtype,nb", [(torch.float32, 24), (torch.float32, 0), (torch.bfloat16, 40)], ids=["f32_nb24", "f32_nb0", "bf16_nb40"])
def test_parser_feed_forward_vs_module_by_module(dtype, nb):
    """vlgae_amd.parser_ff.parser_feed_forward (ONE pass of mid_ff over all rows, folded bottlenecks and linear2, fused GEMMs,
    hand-written adjoint) against the reference's module-by-module formulation (vlgae_amd.train_step.scorer_feed_forward: the restatement
    of MLP / DMVSkipConnectEncoder / DMVFactorizedBilinear.project* that the trainstep fixtures pin on the reference's own modules) in
    float64: the five outputs and the gradient w.r.t. every input and parameter.  float32: 2e-5 * max (folding W1 W0 and P W2 re-associates
    fp32 products); bf16: 3e-2 * max values, 0.2 relative L2 gradients.  The cases with a bottleneck also run with training-mode dropout
    (SharedDropout masks of the MLPs, nn.Dropout mask of mid_ff) given explicitly to both formulations."""
    from vlgae_amd import train_step
    from vlgae_amd import parser_ff
    B, L, E, h, Et, T, H, r = 24, 11, 40, 64, 16, 9, 64, 8
    gen = torch.Generator().manual_seed(3)
    P = train_step.init_feed_forward(gen, dev(), dtype, E, h, Et, T, H, nb, r)
    for k in list(P):
        if k.endswith(".bias"):      # (init_feed_forward's small biases; make them matter)
            P[k] = (torch.randn(P[k].shape, generator=gen) * 0.3).to(dev(), dtype).requires_grad_(True)
    emb = (torch.randn(B, L, E, generator=gen) * 0.5).to(dev(), dtype).requires_grad_(True)
    x = torch.randn(B, L, h, generator=gen).to(dev(), dtype).requires_grad_(True)
    names = sorted(P)
    leaves = [emb, x] + [P[k] for k in names]
    # training-mode dropout as explicit masks, the same ones on both sides (every second case; rates of the shipped config)
    # a fixed draw: the bf16 bound below is statistical (see there), and in float32 about one draw in 40 puts a pre-activation within
    # rounding of zero -- float32 and the float64 reference then take different LeakyReLU branches (seed 7 does: one element, 100x)
    dgen = torch.Generator(device=dev()).manual_seed(11)
    masks = parser_ff.dropout_masks(B, L, T, H, 0.33, 0.3, device=dev(), dtype=torch.float32, generator=dgen) if nb else (None, None, None)
    outs = parser_ff.parser_feed_forward(P, emb, x, None, None, None, *masks)
    cot = [torch.randn(o.shape, generator=gen).to(dev()) for o in outs]
    got = torch.autograd.grad([o.float() for o in outs], leaves, cot)
    P64 = {k: v.detach().double().requires_grad_(True) for k, v in P.items()}
    e64, x64 = emb.detach().double().requires_grad_(True), x.detach().double().requires_grad_(True)
    ref = train_step.scorer_feed_forward(P64, e64, x64, *(None if m is None else m.double() for m in masks))
    want = torch.autograd.grad(list(ref), [e64, x64] + [P64[k] for k in names], [c.double() for c in cot])
    f32 = dtype == torch.float32
    for name, a, b in zip(("x1", "x2", "y1", "y2", "root_rule"), outs, ref):
        assert a.shape == b.shape, name
        assert float((a.double() - b).abs().max()) <= (2e-5 if f32 else 3e-2) * max(1.0, float(b.abs().max())), name
    gmax = max(float(w.abs().max()) for w in want)
    for name, a, b in zip(["emb", "x"] + names, got, want):
        assert a.shape == b.shape, name
        if name == "ff.root_scorer.project2.bias":   # shared by every argument of root_rule's softmax: exactly zero in exact arithmetic
            assert float(a.double().abs().max()) <= (1e-5 if f32 else 2e-3) * gmax and float(b.abs().max()) <= 1e-5 * gmax
            continue
        if f32:
            assert float((a.double() - b).abs().max()) <= 2e-5 * max(float(b.abs().max()), 1e-3 * gmax), name
        else:
            # (bf16: six LeakyReLUs deep, a pre-activation within bf16 rounding of zero takes the other branch than in float64 and its
            #  term changes by 1 / slope = 100x; the float32 cases above are the check of the mathematics.  Over 40 mask draws the
            #  worst tensor -- a 40-element bias gradient -- reaches 0.13 relative: 0.2 here, on one fixed draw)
            assert float((a.double() - b).norm()) <= 0.2 * float(b.norm()) + 2e-3 * gmax * b.numel() ** 0.5, name


def test_parser_feed_forward_counter_based_mid_dropout():
    """mid_ff's nn.Dropout (nn/dmv_spec.py:52) drawn INSIDE the activation kernel from the step's DeviceRng (no mask tensor): the result
    and every gradient are BIT-identical to the same call with the explicit mask that the same generator state writes out through
    encoders.dropout (same site, same element indexing), forward and adjoint regenerate the same bits, and advancing the state changes
    them.  Also: encoders.dropout_mask (the small SharedDropout rows) has the right support and rate."""
    from vlgae_amd import encoders, parser_ff, train_step
    B, L, E, h, Et, T, H, r, nb, p = 24, 11, 40, 64, 16, 9, 64, 8, 24, 0.3
    gen = torch.Generator().manual_seed(9)
    P = train_step.init_feed_forward(gen, dev(), torch.bfloat16, E, h, Et, T, H, nb, r)
    emb = (torch.randn(B, L, E, generator=gen) * 0.5).to(dev(), torch.bfloat16).requires_grad_(True)
    x = torch.randn(B, L, h, generator=gen).to(dev(), torch.bfloat16).requires_grad_(True)
    names = sorted(P)
    leaves = [emb, x] + [P[k] for k in names]
    rng = encoders.DeviceRng(77, dev())
    rows = 4 * (B * L + T + 3)

    def run(**kw):
        outs = parser_ff.parser_feed_forward(P, emb, x, **kw)
        cot = [torch.ones_like(o) * 0.5 for o in outs]
        return outs, torch.autograd.grad([o.float() for o in outs], leaves, [c.float() for c in cot])
    got = run(mid_rng=rng, p_mid=p)
    mask = encoders.dropout(torch.ones(rows, H, device=dev()), p, rng=rng, site=encoders.SITE_MID_FF)      # the same state written out
    keep = float((mask != 0).double().mean())
    assert abs(keep - (1 - p)) < 4 * (p * (1 - p) / mask.numel()) ** 0.5 + 1e-4
    want = run(drop_mid=(mask != 0).to(torch.bfloat16), mid_scale=float(mask.max()))
    for a, b in zip(got[0] + got[1], want[0] + want[1]):
        assert torch.equal(a, b)
    rng.advance()
    again = run(mid_rng=rng, p_mid=p)
    assert not torch.equal(again[0][0], got[0][0])
    small = encoders.dropout_mask(rng, encoders.SITE_SHARED, 0.33, 100003)
    vals = torch.unique(small)
    assert vals.numel() == 2 and float(vals[0]) == 0.0 and abs(float(vals[1]) - 1.0 / (1.0 - round(0.33 * 65536) / 65536.0)) < 1e-6
    assert abs(float((small != 0).double().mean()) - 0.67) < 4 * (0.33 * 0.67 / 100003) ** 0.5 + 1e-4


def test_parser_feed_forward_fp32_master_weights_with_bf16_activations():
    """float32 parameters (master weights) with bf16 embeddings: every operand the grouped small products read is then a TEMPORARY cast made
    inside the forward (`w.to(bf16)`, `.t()` of one), alive only because SmallMatmulGroup keeps its operands referenced until launch()
    (without that the caching allocator hands a freed cast to the next one before the kernel runs).  Outputs must be
    BIT-identical to the same call with the parameters cast to bf16 beforehand; gradients equal after the same cast (1 bf16 ulp)."""
    from vlgae_amd import parser_ff, train_step
    B, L, E, h, Et, T, H, r, nb = 24, 11, 40, 64, 16, 9, 64, 8, 24
    gen = torch.Generator().manual_seed(21)
    P32 = train_step.init_feed_forward(gen, dev(), torch.float32, E, h, Et, T, H, nb, r)
    for k in list(P32):
        if k.endswith(".bias"):
            P32[k] = (torch.randn(P32[k].shape, generator=gen) * 0.3).to(dev()).requires_grad_(True)
    P16 = {k: v.detach().to(torch.bfloat16).requires_grad_(True) for k, v in P32.items()}
    emb = (torch.randn(B, L, E, generator=gen) * 0.5).to(dev(), torch.bfloat16).requires_grad_(True)
    x = torch.randn(B, L, h, generator=gen).to(dev(), torch.bfloat16).requires_grad_(True)
    names = sorted(P32)
    cot = None
    res = []
    for P in (P32, P16, P32):            # (the fp32 case twice: allocator state differs between the first and a later call)
        outs = parser_ff.parser_feed_forward(P, emb, x)
        if cot is None:
            cot = [torch.randn(o.shape, generator=gen).to(dev()) for o in outs]
        grads = torch.autograd.grad([o.float() for o in outs], [emb, x] + [P[k] for k in names], cot)
        res.append((outs, grads))
    for other in (res[1], res[2]):
        for name, a, b in zip(("x1", "x2", "y1", "y2", "root_rule"), res[0][0], other[0]):
            assert a.dtype == b.dtype and torch.equal(a, b), name
    for name, a, b in zip(["emb", "x"] + names, res[0][1], res[1][1]):
        assert a.dtype == (torch.bfloat16 if name in ("emb", "x") else torch.float32) and b.dtype == torch.bfloat16, name
        scale = max(float(b.float().abs().max()), 1e-6)
        assert float((a.float() - b.float()).abs().max()) <= 2.0 ** -7 * scale, name
    for name, a, b in zip(["emb", "x"] + names, res[0][1], res[2][1]):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_ff_elementwise_kernels(dtype):
    """csrc/vlg_ff.hip through the C ABI against the torch chains they replace (nn/common.py:47-51, nn/dmv_spec.py:41-52), computed in
    float64 from the same stored inputs: fp32 to 1e-6, bf16 to one rounding of the result (2^-8 relative)."""
    from vlgae_amd import _C
    lib, adt = _C.lib(), (_C.BF16 if dtype == torch.bfloat16 else _C.F32)
    gen = torch.Generator().manual_seed(5)
    B, L, Ms, H, slope = 5, 7, 6, 40, 0.01
    M0, M = B * L, B * L + Ms
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev(), dtype)
    st = _C.stream_of(rnd(1))
    tol = 1e-6 if dtype == torch.float32 else 2.0 ** -8
    lrelu = lambda t: torch.where(t > 0, t, t * slope)

    def close(name, got, want):
        err = (got.double() - want).abs()
        assert bool((err <= tol * want.abs() + 1e-30).all()), (name, float(err.max()))

    # MLP epilogue, in place
    X, cterm = rnd(M, H), rnd(B, H)
    dh = (torch.rand(B, H, generator=gen) < 0.6).float().to(dev()) / 0.6
    ds = (torch.rand(Ms, generator=gen) < 0.6).float().to(dev()) / 0.6
    want = X.double().clone()
    want[:M0] = (lrelu(want[:M0].view(B, L, H) + cterm.double().unsqueeze(1)) * dh.double().unsqueeze(1)).view(M0, H)
    want[M0:] = lrelu(want[M0:]) * ds.double().unsqueeze(1)
    X0 = X.clone()
    _C.check(lib.vlg_ff_mlp_act(_C.ptr(X), _C.ptr(cterm), _C.ptr(dh), _C.ptr(ds), B, L, Ms, H, adt, slope, st), "ff_mlp_act")
    close("mlp_act", X, want)
    X2 = X0.clone()
    _C.check(lib.vlg_ff_mlp_act(_C.ptr(X2), _C.ptr(cterm), None, None, B, L, Ms, H, adt, slope, st), "ff_mlp_act")
    want2 = X0.double().clone()
    want2[:M0] = lrelu(want2[:M0].view(B, L, H) + cterm.double().unsqueeze(1)).view(M0, H)
    want2[M0:] = lrelu(want2[M0:])
    close("mlp_act_nomask", X2, want2)
    # residual + activation (+ mask), plain and with the (val, dir) -> (dir, val) store permutation
    for J, swap, with_res, with_mask in ((2, False, True, False), (4, True, True, False), (1, False, False, True), (4, True, False, True), (3, False, True, True)):
        inp, res = rnd(M, J, H), (rnd(M, H) if with_res else None)
        mask = ((torch.rand(M, J, H, generator=gen) < 0.7).to(dev(), dtype) / 0.7) if with_mask else None
        w = inp.double() + (res.double().unsqueeze(1) if with_res else 0.0)
        w = lrelu(w)
        if swap:
            w = w.view(M, 2, 2, H).permute(0, 2, 1, 3).reshape(M, J, H)
        if with_mask:
            w = w * mask.double()
        if with_mask and J == 3:        # a 0 / 1 keep-mask with the scale as an argument (nn.Dropout without the division pass)
            keep = (mask != 0).to(dtype)
            out2 = inp.clone()
            _C.check(lib.vlg_ff_act(_C.ptr(out2), _C.ptr(res), _C.ptr(keep), 1.0 / 0.7, None, 0, 0.0, _C.ptr(out2), M, J, H, 0, adt, slope, st), "ff_act")
            close("act, keep-mask x scale", out2, lrelu(inp.double() + res.double().unsqueeze(1)) * keep.double() * float(np.float32(1.0 / 0.7)))
        out = torch.empty_like(inp) if swap else inp.clone()
        _C.check(lib.vlg_ff_act(_C.ptr(inp if swap else out), _C.ptr(res), _C.ptr(mask), 1.0, None, 0, 0.0, _C.ptr(out), M, J, H, int(swap), adt, slope, st), "ff_act")
        close(f"act J={J} swap={swap}", out, w)
    # adjoint: LeakyReLU' from the stored activation, mask, group sum (= / +=), permutation
    for J, swap, with_mask, acc in ((1, False, True, False), (4, True, False, False), (2, False, False, True), (4, True, True, True)):
        g, act = rnd(M, J, H), rnd(M, J, H)
        act[0, 0, :8] = 0.0                       # LeakyReLU'(0) = slope (torch's `self > 0`)
        mask = ((torch.rand(M, J, H, generator=gen) < 0.7).to(dev(), dtype) / 0.7) if with_mask else None
        t = g.double() * (mask.double() if with_mask else 1.0)
        t = torch.where(act.double() > 0, t, t * slope)
        total0 = torch.randn(M, H, generator=gen).to(dev())
        total = total0.clone()
        out = torch.empty_like(g)
        _C.check(lib.vlg_ff_act_backward(_C.ptr(g), _C.ptr(act), _C.ptr(mask), 1.0, None, 0, 0.0, _C.ptr(out), _C.ptr(total), M, J, H, int(swap), int(acc), adt,
                                         slope, st), "ff_act_backward")
        close(f"act_bwd J={J} swap={swap}", out, t.view(M, 2, 2, H).permute(0, 2, 1, 3).reshape(M, J, H) if swap else t)
        want_total = out.double().sum(1) + (total0.double() if acc else 0.0)      # the sum is of the STORED values (what the next GEMM reads)
        assert float((total.double() - want_total).abs().max()) <= 1e-5 * max(1.0, float(want_total.abs().max()))
        if not swap:                              # in place, without the sum
            g2 = g.clone()
            _C.check(lib.vlg_ff_act_backward(_C.ptr(g2), _C.ptr(act), _C.ptr(mask), 1.0, None, 0, 0.0, _C.ptr(g2), None, M, J, H, 0, 0, adt, slope, st), "ff_act_backward")
            assert torch.equal(g2, out)
    # MLP adjoint
    gX, T_, Xs = torch.randn(M, H, generator=gen).to(dev()), rnd(M, H), rnd(M, H)
    w = gX.double() + T_.double()
    w[:M0] = (w[:M0].view(B, L, H) * dh.double().unsqueeze(1)).view(M0, H)
    w[M0:] = w[M0:] * ds.double().unsqueeze(1)
    w = torch.where(Xs.double() > 0, w, w * slope)
    gpre = torch.empty_like(Xs)
    _C.check(lib.vlg_ff_mlp_act_backward(_C.ptr(gX), _C.ptr(T_), _C.ptr(Xs), _C.ptr(dh), _C.ptr(ds), _C.ptr(gpre), B, L, Ms, H, adt, slope, st),
             "ff_mlp_act_backward")
    close("mlp_act_bwd", gpre, w)
    # the sentence's context vector (ldndmv.py:226): mean over the positions of float32 encodings, in the activations' dtype
    xs = torch.randn(B, L, 72, generator=gen).to(dev())
    cm = torch.empty((B, 72), dtype=dtype, device=dev())
    _C.check(lib.vlg_ff_context_mean(_C.ptr(xs), _C.F32, B, L, 72, _C.ptr(cm), adt, st), "ff_context_mean")
    assert float((cm.double() - xs.to(dtype).double().mean(1)).abs().max()) <= (1e-6 if dtype == torch.float32 else 2.0 ** -8)   # (a mean near zero: absolute)
    # argument checks (host side)
    assert lib.vlg_ff_act(_C.ptr(Xs), None, None, 1.0, None, 0, 0.0, _C.ptr(Xs), M, 1, 12, 0, adt, slope, st) == 0x1001          # H not a multiple of 8
    assert lib.vlg_ff_act(_C.ptr(Xs), None, None, 1.0, None, 0, 0.0, _C.ptr(Xs), M, 2, H, 1, adt, slope, st) == 0x1001           # the permutation is of J = 4
    assert lib.vlg_ff_act(_C.ptr(Xs), None, None, 1.0, None, 0, 0.0, _C.ptr(Xs), M // 4, 4, H, 1, adt, slope, st) == 0x1003      # ... and not in place
    assert lib.vlg_ff_act(_C.ptr(Xs), None, None, 1.0, None, 0, 0.0, _C.ptr(Xs), M, 1, H, 0, 7, slope, st) == 0x1002


def test_linear_wgrad_partial_tiles():
    """vlg_linear_wgrad on output / input widths that are not multiples of its 64 x 64 tile (round 4: multiples of 8 suffice; the
    edge tiles are staged with zeros and stored masked), strided operands, against float64; run-to-run bit equality.
    The row count is FIXED here (K = 10496: every stage full, and only (512, 8) has an odd number of stages per split);
    tests/test_wgrad_plans_gpu.py varies it over every split plan from K = 1."""
    from vlgae_amd import align
    gen = torch.Generator().manual_seed(11)
    K = 10496
    for M, N, ldy, ldx in ((384, 256, 384, 256), (256, 800, 256, 800), (32, 256, 32, 256), (24, 72, 40, 88), (512, 8, 512, 8), (8, 8, 8, 8)):
        dy_full = torch.randn(K, ldy, generator=gen).to(dev(), torch.bfloat16)
        x_full = torch.randn(K, ldx, generator=gen).to(dev(), torch.bfloat16)
        dy, x = dy_full[:, :M], x_full[:, :N]
        dw, db = align.linear_wgrad(dy, x)
        dw2, db2 = align.linear_wgrad(dy, x)
        assert torch.equal(dw, dw2) and torch.equal(db, db2)
        rw, rb = dy.double().t() @ x.double(), dy.double().sum(0)
        assert float((dw.double() - rw).abs().max()) <= 1e-5 * float(rw.abs().max()) + 1e-3, (M, N)
        assert float((db.double() - rb).abs().max()) <= 1e-5 * float(rb.abs().max()) + 1e-3, (M, N)
        _, xs = align.linear_wgrad(dy, x, want_x_colsum=True)
        assert float((xs.double() - x.double().sum(0)).abs().max()) <= 1e-3, (M, N)
        # a column block of a wider gradient tensor written in place (ld_dw > N), bf16 output
        wide = torch.zeros(M, N + 40, device=dev(), dtype=torch.bfloat16)
        align.linear_wgrad(dy, x, want_bias=False, out=(wide[:, 16:16 + N], None))
        assert torch.equal(wide[:, 16:16 + N], dw.to(torch.bfloat16)) and float(wide[:, :16].abs().max()) == 0 and float(wide[:, 16 + N:].abs().max()) == 0


def test_linear_wgrad_lazy_group_equals_single_launches():
    """A lazy WgradGroup (the split-K launches of several products as one grid per kernel image, vlg_linear_wgrad_partial_group) gives the bits of
    the products launched one by one: every image class (64-tile, 128-tile with bias sum / x column sum / none), more items than one launch
    holds, a float32 item among them, operands that are column slices."""
    from vlgae_amd import align
    g = torch.Generator().manual_seed(21)
    bf = torch.bfloat16
    cases = [(4100, 32, 256, True, False), (4099, 256, 256, True, False), (2400, 512, 256, True, False), (2400, 256, 800, False, True),
             (2200, 384, 384, False, False), (2304, 768, 256, True, False)] + [(2048 + 8 * i, 64, 72, True, False) for i in range(9)]
    ops = []
    for K, M, N, bias, colsum in cases:
        wide = torch.randn(K, M + 8, generator=g).to(dev(), bf)
        ops.append((wide[:, 8:], torch.randn(K, N, generator=g).to(dev(), bf), bias, colsum))
    ops.append((torch.randn(2100, 64, generator=g).to(dev()), torch.randn(2100, 40, generator=g).to(dev()), True, False))     # float32 operands
    def run(lazy):
        wg = align.WgradGroup(lazy=lazy)
        outs = [align.linear_wgrad(dy, x, want_bias=b, want_x_colsum=c, defer=wg) for dy, x, b, c in ops]
        wg.flush()
        return outs
    single = [align.linear_wgrad(dy, x, want_bias=b, want_x_colsum=c) for dy, x, b, c in ops]
    for outs in (run(False), run(True), run(True)):
        for (dw, db), (sw, sb), (dy, x, b, c) in zip(outs, single, ops):
            assert torch.equal(dw, sw)
            assert (db is None and sb is None) or torch.equal(db, sb)
    dy, x = ops[1][0], ops[1][1]
    want = dy.double().t() @ x.double()
    assert float((run(True)[1][0].double() - want).abs().max()) <= 1e-5 * float(want.abs().max()) + 1e-3


def test_linear_wgrad_float32_operands():
    """vlg_linear_wgrad with float32 operands (the reference's `precision: 32`): three bf16 products per pair on hi / lo parts split on the way
    into LDS.  Against float64: the error is that of the dropped lo x lo term and the split residues (~2^-16 relative per PRODUCT, random in
    sign over the K rows), i.e. a few 1e-6 of the largest entry -- the bound here is 2e-5 of it; bias / column sums (hi + lo against ones)
    likewise; bit-reproducible; both tile shapes, partial tiles, strided operands, in-place column blocks."""
    from vlgae_amd import align
    gen = torch.Generator().manual_seed(12)
    for K, M, N, ldy, ldx in ((10496, 384, 256, 384, 256), (9216, 256, 2048, 256, 2048), (10240, 256, 800, 256, 800), (4100, 24, 72, 40, 88), (2048, 8, 8, 8, 8),
                              (256, 256, 512, 256, 512)):
        dy_full = (torch.randn(K, ldy, generator=gen) * torch.rand(K, 1, generator=gen) * 1e-3).to(dev())     # cotangent-sized values
        x_full = torch.randn(K, ldx, generator=gen).to(dev())
        dy, x = dy_full[:, :M], x_full[:, :N]
        dw, db = align.linear_wgrad(dy, x)
        dw2, db2 = align.linear_wgrad(dy, x)
        assert dw.dtype == torch.float32 and torch.equal(dw, dw2) and torch.equal(db, db2)
        rw, rb = dy.double().t() @ x.double(), dy.double().sum(0)
        assert float((dw.double() - rw).abs().max()) <= 2e-5 * float(rw.abs().max()), (K, M, N, float((dw.double() - rw).abs().max()) / float(rw.abs().max()))
        assert float((db.double() - rb).abs().max()) <= 2e-5 * float(rb.abs().max()) + 1e-9, (K, M, N)
        _, xs = align.linear_wgrad(dy, x, want_x_colsum=True)
        assert float((xs.double() - x.double().sum(0)).abs().max()) <= 2e-5 * float(x.double().sum(0).abs().max()) + 1e-6, (K, M, N)
        wide = torch.zeros(M, N + 40, device=dev())
        wg = align.WgradGroup()
        align.linear_wgrad(dy, x, want_bias=False, out=(wide[:, 16:16 + N], None), defer=wg)
        wg.flush()
        assert torch.equal(wide[:, 16:16 + N], dw) and float(wide[:, :16].abs().max()) == 0 and float(wide[:, 16 + N:].abs().max()) == 0
    with pytest.raises(ValueError):
        align.linear_wgrad(dy, x.bfloat16())


def _reference_step_in_torch(step, P64, token, tag, vmask, drop, alpha, pen_args, forced_heads=None):
    """The reference's lines for one training step (the order and the formulas of make_golden.trainstep_cases' calls: joint.py:658-711,
    ldndmv.py:171-216,277-281, fn.py:50-56) as float64 torch ops on the step's own leaves -- an independent formulation of everything
    except the structured DP itself (DMV1o marginals / heads / max come from this package's DP kernels on the torch-made potentials;
    those kernels are parity-tested on their own at this size) and the parser's feed-forwards (vlgae_amd.train_step.scorer_feed_forward:
    plain torch ops, pinned by the trainstep fixtures).  Returns (loss, heads)."""
    from vlgae_amd import train_step
    import vlgae_amd.torch_struct as ts
    from vlgae_amd import align
    F = torch.nn.functional
    lengths = step.lengths
    B, L, E = P64["emb"].shape
    h, d = P64["w_text"].shape[0], P64["w2"].shape[0]
    N = L + 1
    # ---- the two encoders, base.py:229 / :68: VisBoxRelSimpleEncoder.forward (box_rel.py:29-52) as written there -- the concatenated
    # [box ; mean box] input and, for `rel`, the pairwise-mean tensor -- and MLPEncoder.forward (mlp_encoder.py:36-40) ----
    feat = P64["vis_box_feat"]
    R, n = feat.shape[1:]
    inputs = torch.cat([feat, feat.mean(1, keepdim=True).expand(-1, R, -1)], -1)                   # box_rel.py:33-38
    factors = step.batch["factors"]
    Wv, bv = P64["w_venc"], P64["b_venc"]
    fc = lambda k, inp: F.leaky_relu(inp @ Wv[k * h:(k + 1) * h].T + bv[k * h:(k + 1) * h], 0.01)    # MLP: Linear -> LeakyReLU (dropout 0)
    box = fc(0, inputs)                                                                            # :47
    parts, k = [box], 1
    if "rel" in factors:
        parts.append(fc(k, (inputs.unsqueeze(1) + inputs.unsqueeze(2)) / 2).view(B, R * R, h))      # :41-45
        k += 1
    if "attr" in factors:
        parts.append(fc(k, inputs))                                                                # :48-49
    if "img" in factors:
        parts.append(box.mean(1, keepdim=True))                                                    # joint.py:163
    vis_mid = torch.cat(parts, 1)                                                                  # joint.py:171
    enc_drop = step.batch["enc_drop"]
    emb_d = P64["emb"] if enc_drop is None else P64["emb"] * enc_drop.double()                     # nn.Dropout with the step's own mask
    x = emb_d @ P64["w_text"].T                                                                    # mlp_encoder.py:39
    wmask = torch.arange(L, device=lengths.device)[None] < lengths[:, None]
    mask1 = torch.cat([wmask.new_zeros(B, 1), wmask], 1)
    D = None if drop is None else drop.double()                                                    # [B,4,d]
    We, be = P64["w_enc"], P64["b_enc"]
    lin = lambda k, inp: inp @ We[k * d:(k + 1) * d].T + be[k * d:(k + 1) * d]
    x1 = torch.cat([(x.masked_fill(~wmask.unsqueeze(2), 0).sum(1) / lengths.unsqueeze(1)).unsqueeze(1), x], 1)   # joint.py:204-208
    vis = vis_mid @ P64["w_vis"].T                                                                # :175
    word0 = lin(0, x1) * (1.0 if D is None else D[:, 0:1])                                        # :209 (+ SharedDropout)
    att = torch.einsum("bvd,bqd->bqv", vis, word0[:, 1:]).softmax(2)                              # :670-672
    x_f = F.layer_norm(x + torch.einsum("bqv,bvh->bqh", att, vis_mid), (h,), P64["ln_w"], P64["ln_b"], 1e-5)   # :673-674
    sx1, sx2, sy1, sy2, root_rule = train_step.scorer_feed_forward(P64, P64["emb"], x_f)          # ldndmv.py:174-205
    attach_rule = torch.einsum("bhdve,cdve->bhcdv", sx1, sx2).log_softmax(2)                      # :184
    ap = attach_rule.gather(2, token.reshape(B, 1, L, 1, 1).expand(B, L, L, 2, 2))                # :188
    tri = lambda k: torch.ones(L, L, device=x.device, dtype=torch.float64).tril(-1) if k == 0 else torch.ones(L, L, device=x.device, dtype=torch.float64).triu(1)
    ap = ap[..., 0, :] * tri(0)[None, :, :, None] + ap[..., 1, :] * tri(1)[None, :, :, None]      # :189-192
    dc = torch.einsum("bhdve,kdve->bhkdv", sy1, sy2).permute(0, 1, 3, 4, 2).log_softmax(-1)       # :201
    rt = torch.gather(root_rule.unsqueeze(0).expand(B, -1), 1, token)                             # :205-206
    md = torch.full((B, N, 2, 2, 2), -1e12, dtype=torch.float64, device=x.device)                 # DMV1o.merge, distributions.py:253-265
    ma = torch.full((B, N, N, 2), -1e12, dtype=torch.float64, device=x.device)
    md = torch.cat([torch.cat([md[:, :1, :1], torch.zeros_like(md[:, :1, 1:])], 2), dc], 1)
    ma = torch.cat([torch.cat([ma[:, :1, :1], torch.stack([ma[:, 0, 1:, 0], rt], -1).unsqueeze(1)], 2),
                    torch.cat([ma[:, 1:, :1], ap], 2)], 1)
    with torch.no_grad():                                                                          # joint.py:251-258
        marg, heads = ts.DMV1o([md.float(), ma.float()], lengths).marginals_and_heads()
        if forced_heads is not None:
            heads = forced_heads
        arc_margin = marg.sum(-1).double().gather(-1, heads.unsqueeze(-1)).squeeze(-1)
        tmarg = torch.cat([mask1.double(), arc_margin], 1)
    tmask = torch.cat([mask1, mask1], 1)
    word = lin(0, x1) * (1.0 if D is None else D[:, 1:2])                                         # :267
    child = F.leaky_relu(lin(1, x1), 0.01) * (1.0 if D is None else D[:, 2:3])                    # :269
    parent = F.leaky_relu(lin(2, x1.gather(1, heads.unsqueeze(-1).expand(-1, -1, h))), 0.01) * (1.0 if D is None else D[:, 3:4])   # :270-273
    arc = torch.einsum("bcx,xhy,bcy->bch", child, P64["w1"], parent) + (child + parent) @ P64["w2"] + P64["b"]   # :278-287
    txt = torch.cat([word, arc], 1)
    att4 = torch.einsum("avd,bqd->baqv", vis, txt)                                                # :413-415
    att4 = att4.masked_fill(~vmask[None, :, None, :], -1e20).masked_fill(~tmask[:, None, :, None], -1e20)
    pen, seg = align.grounding_prior(tag, *pen_args, 2 * N)                                       # :446-470 as a table
    ar = torch.arange(B, device=x.device)
    diag = att4[ar, ar] - pen.double()[:, :, seg.long()]
    att4 = att4.clone()
    att4[ar, ar] = diag
    num = lengths.sum().double()
    t2v = -(att4.max(3).values.log_softmax(1).diagonal().T * tmarg).sum()                         # :473-478
    v2t = -(att4.max(2).values.log_softmax(0).diagonal().T * vmask).sum()                         # :480-489
    mt = t2v / (t2v.detach() + 1e-6) * num + v2t / (v2t.detach() + 1e-6) * num
    if forced_heads is None:
        dep = -ts.DMV1o([md, ma], lengths).max.sum()                                              # ldndmv.py:277-281
    else:   # the same tree on both sides: -score(tree) (vlgae_amd.train_step.forced_tree_score on this side's float64 potentials)
        dep = -train_step.forced_tree_score(md, ma, forced_heads, lengths).double().sum()
    return (alpha * mt + (1 - alpha) * dep) / (num + 1e-12), heads                                # joint.py:709, fn.py:56


@pytest.mark.parametrize("case", ["f32", "bf16", "bf16_forced", "f32_shipped", "bf16_shipped_forced"])
def test_training_step_reference_wiring_config_size(case):
    """vlgae_amd.train_step.build at BASELINE.json configs[4]'s size (B = 256, L = 40, R = 36, d = 128, h = 256), from the frozen
    features, against the reference's formulation restated in float64 torch ops on the same leaves (`_reference_step_in_torch`).

    f32 (the reference's `precision: 32`; narrower feed-forwards so that the float64 side stays small): loss to 1e-5 relative, Viterbi
    heads identical, and every gradient with >= 99.99 % of its elements within 3e-4 * max|g| and none beyond 5e-3 * max|g| -- at this
    size a handful of the 7.7 M arg-max decisions of the alignment and of the 2.7 M LeakyReLU branches sit within fp32 rounding of a
    tie and move one term of a row's sum.
    bf16 (what `bench.py` times: bf16 storage of every feature, parameter and activation between kernels, fp32 accumulation, the
    SHIPPED widths E = 800, n_vis = 2048, H = 256, n_bottleneck = 150): loss to 2e-2 relative; Viterbi heads equal on >= 90 % of the
    words (a bf16 potential is ~3 significant digits: near-tied attachments flip); every gradient tensor within 0.35 relative L2 of
    the float64 one (plus an absolute floor of 2e-3 * max|g| per element) -- the sentences whose tree flipped feed other parents into
    the arc encoder and another derivation into -max, so this is a bound on the tensor, not on elements; the float32 case above is the
    check of the mathematics.
    bf16_forced (round 6): the same bf16 step with the float64 side's Viterbi heads handed to it (`step.forced_heads`): the same tree on both
    sides, so the bound is on rounding alone -- every gradient tensor within 0.12 relative L2 (observed <= 0.105; 0.25 free-running).
    *_shipped (round 6): the SHIPPED factor layout (config/model/vlgae.yaml:40-42: add_rel / add_attr / add_image -> V = 36 + 36^2 + 36
    + 1 = 1369 columns; rel_fc / attr_fc on the path, joint.py:143-171, box_rel.py:41-45; the attention fuse over 1369 keys = the
    key-split kernels) at B = 64: f32 as above; bf16 teacher-forced as above."""
    from vlgae_amd import train_step
    f32, forced, shipped = case.startswith("f32"), case.endswith("forced"), "shipped" in case
    dtype = torch.float32 if f32 else torch.bfloat16
    B, L, R, d = (64 if shipped else 256), 40, 36, 128
    factors = ("rel", "attr", "img") if shipped else ()
    widths = dict(E=96, Et=16, H=64, nb=24, n_vis=128) if f32 else {}
    E = widths.get("E", 800)
    gen = torch.Generator().manual_seed(5)
    drop = (torch.rand(4, B, d, generator=gen) >= 0.33).float() / 0.67
    enc_drop = (torch.rand(B, L, E, generator=gen) >= 0.33).float() / 0.67
    with torch.autograd.set_multithreading_enabled(False):
        step = train_step.build(B, L, R, dev(), dtype=dtype, given=dict(drop=drop, enc_drop=enc_drop), seed=21, p_ff_drop=0.0, p_mid_drop=0.0,
                                factors=factors, **widths)
        assert step.shape["V"] == (1369 if shipped else 36)
        P64 = {k: v.detach().double().requires_grad_(v.requires_grad) for k, v in step.P.items()}
        bt = step.batch
        ref_loss, ref_heads = _reference_step_in_torch(step, P64, bt["token"], bt["tag"], bt["vis_mask"], drop.permute(1, 0, 2).to(dev()),
                                                       bt["alpha"], (bt["factor_names"], bt["vis_split"], bt["pos_for"]))
        ref = torch.autograd.grad(ref_loss, [P64[k] for k in step.names])
        if forced:
            step.forced_heads = ref_heads
        loss, grads, _ = step()
        heads = step.last["heads"]
    valid = torch.cat([torch.zeros(B, 1, dtype=torch.bool, device=heads.device), torch.arange(L, device=heads.device)[None] < step.lengths[:, None]], 1)
    agree = float((heads == ref_heads)[valid].double().mean())
    assert torch.equal(heads, ref_heads) if (f32 or forced) else (agree >= 0.90), agree
    assert abs(float(loss) - float(ref_loss)) <= (1e-5 if f32 else 2e-2) * abs(float(ref_loss)), (float(loss), float(ref_loss))
    gmax = max(float(r.abs().max()) for r in ref)
    report = {}
    for k, want in zip(step.names, ref):
        got = grads[k].double()
        if k.endswith("project2.bias"):   # a bias shared by all arguments of a (log-)softmax: its gradient is exactly zero in exact
            assert float(got.abs().max()) <= (1e-5 if f32 else 2e-3) * gmax and float(want.abs().max()) <= 1e-5 * gmax, k   # arithmetic, rounding noise in both
            continue
        if f32:
            scale = max(float(want.abs().max()), 1e-6 * gmax)
            err = (got - want).abs() / scale
            report[k] = (float(err.max()), float((err > 3e-4).double().mean()))
            # (shipped layout: 38x the columns, so 38x the alignment's arg-max decisions near a tie: 5e-4 of the elements)
            assert float((err > 3e-4).double().mean()) <= (5e-4 if shipped else 1e-4) and float(err.max()) <= 5e-3, (k, report[k])
        else:
            floor = 2e-3 * gmax * want.numel() ** 0.5
            rel = max(float((got - want).norm()) - floor, 0.0) / max(float(want.norm()), 1e-30)
            report[k] = (float((got - want).norm()) / max(float(want.norm()), floor), 0.0)
            assert rel <= (0.12 if forced else 0.35), (k, rel, agree)   # forced, observed: <= 0.105 (ff.child_ff.linear.bias: 45 token rows), hot path <= 0.065
    print(f"config-size training step ({case}) vs float64 torch formulation: loss", float(loss), float(ref_loss), f"heads agree {agree:.4f};",
          "worst:", sorted(report.items(), key=lambda kv: -kv[1][0])[:6])


@pytest.mark.parametrize("B,L,V,d", [(6, 9, 12, 32), (256, 40, 36, 128)], ids=["toy", "config2"])
def test_training_step_chain(oracle_mod, B, L, V, d):
    """One pass over the whole path as the model wires it (joint.py:245-287 lang_feat_max_tree, :406-491 grounding):
    DMV marginals + best heads -> txt_marginal and parent gather -> arc encoder -> alignment -> grounding loss -> gradients
    to the feature tensors and the arc-encoder weights.  Ours end to end vs the same wiring in plain torch ops; the DP
    results (parity-tested on their own above) feed both sides as the constants they are in the reference (joint.py:251-264)."""
    import vlgae_amd.torch_struct as ts
    from vlgae_amd import align
    rng = np.random.default_rng(77)
    N, Q = L + 1, 2 * (L + 1)
    lengths = np.array([9, 7, 9, 4, 8, 5]) if B == 6 else rng.integers(L // 2, L + 1, size=B)
    lengths[0] = L
    dec = np.log(rng.dirichlet(np.ones(2), (B, L, 2, 2))).astype(np.float32)
    attach = rng.standard_normal((B, L, L, 2)).astype(np.float32)
    root = np.log(rng.dirichlet(np.ones(L), B)).astype(np.float32)
    # ---- DP: ours on the GPU, oracle on the CPU; both give arc marginals and the best heads ----
    md, ma = ts.DMV1o.merge(t(dec), t(attach), t(root))
    ma_ = ma.detach().requires_grad_(True)
    dist = ts.DMV1o([md, ma_], t(lengths))
    arc_margin = torch.autograd.grad(dist.partition.sum(), ma_)[0].sum(-1)          # joint.py:255
    heads = ts.DMV1o([md, ma], t(lengths)).argmax_heads                              # replaces joint.py:256-258
    wmask = np.arange(L)[None] < lengths[:, None]
    mask1 = np.concatenate([np.zeros((B, 1), bool), wmask], 1)
    margin = arc_margin.gather(-1, heads.unsqueeze(-1)).squeeze(-1) * t(mask1)      # joint.py:262-264 (add_marginal)
    txt_marginal = torch.cat([t(mask1).float(), margin], 1)                          # joint.py:266
    tmask = t(np.concatenate([mask1, mask1], 1))
    assert np.allclose(arc_margin.sum((1, 2)).cpu().numpy(), lengths, atol=1e-3)     # one head per word
    # ---- features: the two sides of the chain share the leaves ----
    def leaves():
        g = torch.Generator().manual_seed(3)
        mk = lambda *s, sc=0.5: (torch.randn(*s, generator=g) * sc).to(dev()).requires_grad_(True)
        return dict(child=mk(B, N, d), parent_src=mk(B, N, d), word=mk(B, N, d), w1=mk(d, d, d, sc=1.0 / d), w2=mk(d, d, sc=0.2),
                    b=mk(d, sc=0.1), vis=mk(B, V, d))
    vmask = t(rng.random((B, V)) > 0.15)
    vmask[:, 0] = True
    num_token = int(lengths.sum())
    idx = heads.unsqueeze(-1).expand(-1, -1, d)

    def run(ours):
        p = leaves()
        if not ours:   # the plain-torch side in float64 (round 5): its arg-max positions are then the exact ones -- torch's float32 einsum and this
            # package's kernels each round a near-tie their own way (at config size ~1 of 5.9 M positions), and one moved position is 1e-3 of a gradient row
            p = {k: v.detach().double().requires_grad_(True) for k, v in p.items()}
        parent = p["parent_src"].gather(1, idx)                                      # joint.py:278-280
        if ours:
            arc = align.arc_encoder(p["child"], parent, p["w1"], p["w2"], p["b"])
            txt = torch.cat([p["word"], arc], 1)
            total, _ = align.grounding_loss_factor_ce(txt, p["vis"], tmask, vmask, txt_marginal, num_token, 1.0)
        else:
            arc = torch.einsum("bcx,xhy,bcy->bch", p["child"], p["w1"], parent) + torch.matmul(p["child"] + parent, p["w2"]) + p["b"]
            txt = torch.cat([p["word"], arc], 1)
            att = torch.einsum("avd,bqd->baqv", p["vis"], txt)
            att = att.masked_fill(~vmask[None, :, None, :], -1e20).masked_fill(~tmask[:, None, :, None], -1e20)
            t2v = -(att.max(3).values.log_softmax(1).diagonal().T * txt_marginal.double()).sum()
            v2t = -(att.max(2).values.log_softmax(0).diagonal().T * vmask).sum()
            total = t2v / (t2v.detach() + 1e-6) * num_token + v2t / (v2t.detach() + 1e-6) * num_token
        names = sorted(p)
        return total, dict(zip(names, torch.autograd.grad(total, [p[k] for k in names])))

    (t1, g1), (t2, g2) = run(True), run(False)
    assert abs(float(t1) - float(t2)) <= 1e-4 * abs(float(t2))
    # config size: 65 536 pairs x 118 arg-max terms feed each gradient row -- fp32 summation order differs between the
    # sparse row updates here and autograd's dense GEMMs there
    rel = 2e-4 if B <= 8 else 1e-3
    for k in g2:
        scale = max(1e-3, float(g2[k].abs().max()))
        assert float((g1[k].double() - g2[k]).abs().max()) <= rel * scale, (k, float((g1[k].double() - g2[k]).abs().max()) / scale)


def test_grounding_argmax_float32_positions_against_float64():
    """float32 features at config-2 widths (B = A = 256, Q = 82, V = 36, d = 128; the reference's `precision: 32`): the arg-max positions the
    grounding loss leaves in its workspace (align_argmax_kernel on two fp16 parts per feature, three MFMAs per product) against float64 scores --
    every position must be the float64 one unless the two best scores of its row are within 1e-6 of each other (at this seed: none differs of
    5.9 M; the exact-fp32 MFMA kernel it replaces differs in one), and the position stored must be the FIRST of equal maxima."""
    from vlgae_amd import _C
    B, L, V, d = 256, 40, 36, 128
    Q = 2 * (L + 1)
    g = torch.Generator().manual_seed(3)
    txt, vis = (torch.randn(B, Q, d, generator=g) * 0.5).to(dev()), (torch.randn(B, V, d, generator=g) * 0.5).to(dev())
    vis[5, 7] = vis[5, 3]                                     # two equal regions: the first must win every row of image 5
    lengths = torch.randint(L // 2, L + 1, (B,), generator=g)
    m1 = torch.cat([torch.zeros(B, 1, dtype=torch.bool), torch.arange(L)[None] < lengths[:, None]], 1)
    tmask, vmask = torch.cat([m1, m1], 1).to(dev()), (torch.rand(B, V, generator=g) > 0.2).to(dev())
    vmask[:, 0] = True
    vmask[5, 3] = vmask[5, 7] = True
    marg = torch.rand(B, Q, generator=g).to(dev()) * tmask
    lib = _C.lib()
    nbytes = lib.vlg_grounding_loss_workspace(B, Q, V)
    ws, sums = torch.zeros(nbytes // 4, device=dev()), torch.zeros(3, device=dev())
    tm, vm = tmask.to(torch.uint8), vmask.to(torch.uint8)
    _C.check(lib.vlg_grounding_loss(_C.ptr(txt), _C.ptr(vis), _C.ptr(tm), _C.ptr(vm), _C.ptr(marg), None, None, 0, B, Q, V, d, _C.F32, -1e20,
                                    float(lengths.sum()), 1.0, _C.ptr(ws), nbytes, _C.ptr(sums), None, None, None), "grounding_loss")
    up = lambda x: (x + 63) & ~63
    nV, nQ = B * B * Q, B * B * V
    off_argV = up(nV) + up(nQ) + up(2 * B * 8) + 64           # GroundPlan (csrc/vlg_ground.hip): maxV | maxQ | partial losses | coefficients | argV | argQ
    off_argQ = off_argV + up((nV + 1) // 2)
    argV = ws[off_argV:off_argV + (nV + 1) // 2].view(torch.int16)[:nV].view(B, B, Q).to(torch.int64) & 0xffff
    argQ = ws[off_argQ:off_argQ + (nQ + 1) // 2].view(torch.int16)[:nQ].view(B, B, V).to(torch.int64) & 0xffff
    S = torch.einsum("bqd,avd->baqv", txt.double(), vis.double())
    S = S.masked_fill(~vmask[None, :, None, :], -1e20).masked_fill(~tmask[:, None, :, None], -1e20)
    for arg, dim in ((argV, 3), (argQ, 2)):
        top2 = S.topk(2, dim=dim).values
        best, second = top2.select(dim, 0), top2.select(dim, 1)
        live = best > -1e19
        differ = (arg != S.argmax(dim)) & live
        assert int(differ.sum()) <= 2, int(differ.sum())
        assert bool((((best - second) <= 1e-6 * best.abs())[differ]).all())
    live5 = tmask[:, None].expand(B, 1, Q)[:, 0] & True
    assert not bool(((argV[:, 5] == 7) & live5).any())       # region 3 == region 7: never the later one


def test_marginals_and_heads_two_streams(ts):
    """The overlapped pair equals the two separate calls bit for bit (same kernels, different streams)."""
    g = torch.Generator().manual_seed(11)
    B, L = 64, 23
    dec = torch.randn(B, L, 2, 2, 2, generator=g).log_softmax(-1).to(dev())
    attach = torch.randn(B, L, L, 2, generator=g).to(dev())
    root = torch.randn(B, L, generator=g).log_softmax(-1).to(dev())
    lengths = torch.randint(3, L + 1, (B,), generator=g).to(dev())
    md, ma = ts.DMV1o.merge(dec, attach, root)
    for _ in range(3):   # repeated: the side stream is reused and must stay ordered with the current one
        marg, heads = ts.DMV1o([md, ma], lengths).marginals_and_heads()
        d2 = ts.DMV1o([md, ma], lengths)
        assert torch.equal(marg, d2.marginals) and torch.equal(heads, d2.argmax_heads)


@pytest.mark.parametrize("B,N", [(256, 41), (7, 5), (1, 2), (300, 81)])
def test_count_sum_matches_batch_sum(B, N):
    """vlg_dmv1o_count_sum: the batch-summed expected counts the data-parallel all-reduce carries (bench.py's multi-GPU
    step).  Against a float64 sum: the kernel's fixed-order fp32 sum of B terms is within B * 2^-24 relative."""
    from vlgae_amd import _C
    g = torch.Generator().manual_seed(B * 131 + N)
    gdec = torch.rand(B, N, 2, 2, 2, generator=g).to(dev())
    gatt = torch.rand(B, N, N, 2, generator=g).to(dev())
    out = torch.full((N * 8 + N * N * 2 + 5,), -7.0, device=dev())
    _C.check(_C.lib().vlg_dmv1o_count_sum(_C.ptr(gdec), _C.ptr(gatt), B, N, _C.ptr(out), _C.stream_of(out)), "count_sum")
    want = torch.cat([gdec.double().view(B, -1).sum(0), gatt.double().view(B, -1).sum(0)])
    got = out[:-5].double()
    assert float((got - want).abs().max()) <= B * 2.0 ** -22
    assert bool((out[-5:] == -7.0).all())          # nothing written past the end
    out2 = torch.empty_like(out)
    _C.check(_C.lib().vlg_dmv1o_count_sum(_C.ptr(gdec), _C.ptr(gatt), B, N, _C.ptr(out2), _C.stream_of(out)), "count_sum")
    assert torch.equal(out2[:-5], out[:-5])        # fixed order: identical bits run to run


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_api_backward_scales_and_casts_in_one_launch(dtype):
    """autograd through `.partition` / DepTree: counts * upstream gradient, cast to the potentials' dtype (vlg_scale_counts),
    bit-equal to the torch expression it replaces -- per-sentence weights, the expanded scalar of `.sum()`, and a
    non-contiguous upstream gradient."""
    import vlgae_amd.torch_struct as ts
    from vlgae_amd.torch_struct import functional as Fn
    B, N = 9, 12
    g = torch.Generator().manual_seed(3)
    dec = torch.randn(B, N, 2, 2, 2, generator=g).to(dev()).to(dtype).requires_grad_(True)
    att = torch.randn(B, N, N, 2, generator=g).to(dev()).to(dtype).requires_grad_(True)
    lengths = torch.tensor([11, 5, 11, 1, 7, 3, 11, 2, 9], device=dev())
    _, cd, ca = Fn.dmv1o_run(dec, att, lengths, 0, True)
    w = torch.randn(B, 2, generator=g).to(dev())[:, :1]                      # [B,1], non-contiguous
    for up in (w, None):
        z = ts.DMV1o([dec, att], lengths).partition
        loss = (z * up).sum() * 0.37 if up is not None else z.sum() * 0.37
        gd, ga = torch.autograd.grad(loss, [dec, att])
        scale = (up.reshape(-1) * 0.37) if up is not None else torch.full((B,), 0.37, device=dev())
        assert gd.dtype == dtype and ga.dtype == dtype
        assert torch.equal(gd, (cd * scale.view(-1, 1, 1, 1, 1)).to(dtype)) and torch.equal(ga, (ca * scale.view(-1, 1, 1, 1)).to(dtype))
    arc = torch.randn(B, N, N, generator=g).to(dev()).to(dtype).requires_grad_(True)
    _, cr = Fn.deptree_run(arc, lengths, 0, True)
    (gr,) = torch.autograd.grad((ts.DependencyCRF(arc, lengths).partition * w.reshape(-1)).sum(), [arc])
    assert gr.dtype == dtype and torch.equal(gr, (cr * w.reshape(-1, 1, 1)).to(dtype))
    # only one of the two potentials wants a gradient
    att2 = att.detach()
    (gd2,) = torch.autograd.grad(ts.DMV1o([dec, att2], lengths).partition.sum(), [dec])
    assert torch.equal(gd2, cd.to(dtype))


# ------------------------------------------------------------------------------------------------ visual encoder: rel features
@pytest.mark.parametrize("path", golden_files("boxrel_"), ids=golden_ids("boxrel_"))
def test_box_rel_golden(path):
    """rel_features (one library GEMM + the pairwise HIP epilogue) against the reference's own VisBoxRelSimpleEncoder."""
    from vlgae_amd import vis_encoder
    g = load(path)
    feat, w, b = t(g["feat"]).requires_grad_(True), t(g["weight"]).requires_grad_(True), t(g["bias"]).requires_grad_(True)
    rel = vis_encoder.rel_features(feat, w, b, True, float(g["slope"]))
    assert rel.shape == g["rel"].shape
    assert np.abs(rel.detach().cpu().numpy() - g["rel"]).max() <= 2e-5 * max(1.0, np.abs(g["rel"]).max())
    gf, gw, gb = torch.autograd.grad(rel, [feat, w, b], t(g["dout"]))
    for got, name in ((gf, "g_feat"), (gw, "g_weight"), (gb, "g_bias")):
        assert np.abs(got.cpu().numpy() - g[name]).max() <= 5e-5 * max(1.0, np.abs(g[name]).max()), name


@pytest.mark.parametrize("B,R,n,H,dt", [(4, 35, 96, 256, "f32"), (3, 7, 40, 64, "f32"), (1, 1, 8, 4, "f32"), (5, 36, 64, 256, "bf16"),
                                        (2, 33, 32, 128, "bf16")])
def test_box_rel_vs_oracle(oracle_mod, B, R, n, H, dt):
    from vlgae_amd import vis_encoder
    rng = np.random.default_rng(B * 100 + R)
    feat = rng.standard_normal((B, R, n)).astype(np.float32)
    w = (rng.standard_normal((H, 2 * n)) / np.sqrt(2 * n)).astype(np.float32)
    b = (rng.standard_normal(H) * 0.1).astype(np.float32)
    dout = rng.standard_normal((B, R * R, H)).astype(np.float32)
    tdt = torch.bfloat16 if dt == "bf16" else torch.float32
    tf, tw, tb = (t(x).to(tdt).requires_grad_(True) for x in (feat, w, b))
    ref = oracle_mod.box_rel(tf.detach().float().cpu().numpy(), tw.detach().float().cpu().numpy(), tb.detach().float().cpu().numpy(),
                             0.01, True, dout)
    rel = vis_encoder.rel_features(tf, tw, tb)
    grads = torch.autograd.grad(rel, [tf, tw, tb], t(dout).to(tdt))
    if dt == "f32":
        for got, want in zip((rel.detach(), *grads), ref):
            assert np.abs(got.float().cpu().numpy() - want).max() <= 2e-5 * max(1.0, np.abs(want).max())
    else:
        # bf16 storage: the library GEMMs around the kernel round y and every gradient to bf16, and the rounding of y flips
        # LeakyReLU'(pre) where pre ~ 0 -- so the chain is only checked on its forward value here, and the kernel pair itself is
        # checked exactly: pairwise_rel on a given bf16 y against fp64 arithmetic on the same values
        assert np.abs(rel.detach().float().cpu().numpy() - ref[0]).max() <= 2e-2 * max(1.0, np.abs(ref[0]).max())
        y = (torch.randn(B, R, H, generator=torch.Generator().manual_seed(R)) * 2).to(dev(), tdt).requires_grad_(True)
        bias = t(b).requires_grad_(True)
        gout = t(dout).to(tdt).view(B, R, R, H)
        out = vis_encoder.pairwise_rel(y, bias)
        gy, gb = torch.autograd.grad(out, [y, bias], gout)
        y64, g64 = y.detach().double().cpu().numpy(), gout.double().cpu().numpy()
        pre = (y64[:, :, None] + y64[:, None, :]) / 2 + b.astype(np.float64)
        want = np.where(pre > 0, pre, pre * 0.01)
        assert np.abs(out.detach().float().cpu().numpy() - want).max() <= 2.0 ** -8 * max(1.0, np.abs(want).max())   # output rounded to bf16
        gp = g64 * np.where(pre > 0, 1.0, 0.01)
        # the kernel forms pre in fp32 from the bf16 y: identical sign decisions except within 1 fp32 ulp of zero
        want_gy = (gp.sum(2) + gp.sum(1)) / 2
        assert np.abs(gy.float().cpu().numpy() - want_gy).max() <= 2.0 ** -7 * max(1.0, np.abs(want_gy).max())      # returned in bf16
        assert np.abs(gb.cpu().numpy() - gp.sum((0, 1, 2))).max() <= 1e-4 * max(1.0, np.abs(gp.sum((0, 1, 2))).max())
    # reproducible, and nothing past the end
    rel2 = vis_encoder.rel_features(tf, tw, tb)
    assert torch.equal(rel2, rel)


def test_box_rel_config_size():
    """Shipped sizes (36 boxes, n_in = 2 x 2048, H = 256) at B = 64: against the reference formulation in torch ops on the
    GPU (pairwise mean materialised: 1.3 GB), forward and gradients."""
    from vlgae_amd import vis_encoder
    B, R, n, H = 64, 36, 2048, 256
    g = torch.Generator().manual_seed(64)
    feat = (torch.randn(B, R, n, generator=g) * 0.5).to(dev())
    w = (torch.randn(H, 2 * n, generator=g) / (2 * n) ** 0.5).to(dev())
    b = (torch.randn(H, generator=g) * 0.1).to(dev())
    dout = torch.randn(B, R * R, H, generator=g).to(dev())
    outs = []
    for ours in (True, False):
        f_, w_, b_ = (x.clone().requires_grad_(True) for x in (feat, w, b))
        if ours:
            rel = vis_encoder.rel_features(f_, w_, b_)
        else:
            inputs = torch.cat([f_, f_.mean(1, keepdim=True).expand(-1, R, -1)], -1)
            rel = torch.nn.functional.leaky_relu(torch.nn.functional.linear((inputs.unsqueeze(1) + inputs.unsqueeze(2)) / 2, w_, b_))
            rel = rel.view(B, R * R, H)
        outs.append((rel.detach(), *torch.autograd.grad(rel, [f_, w_, b_], dout)))
    # forward: fp32 rounding of two summation orders over n_in = 4096.  Gradients: LeakyReLU' is discontinuous at 0, and the
    # few of the 21 M pre-activations that land within rounding of 0 take the other slope in the other summation order --
    # one such flip moves a gradient entry by ~ |dout| |w| ~ 4e-3
    for k, (a, r) in enumerate(zip(*outs)):
        assert float((a - r).abs().max()) <= (2e-5 if k == 0 else 3e-3) * max(1.0, float(r.abs().max())), k


def _vis_encoder_reference(feat, W, b, factors, slope=0.01):
    """VisBoxRelSimpleEncoder.forward (box_rel.py:29-52) + the cat of vis_feat_unprune (joint.py:143-171) as those lines write them:
    the concatenated [box ; mean box] input, the pairwise-mean tensor, one Linear + LeakyReLU per encoder."""
    B, R, n = feat.shape
    h = W.shape[0] // (1 + ("rel" in factors) + ("attr" in factors))
    F = torch.nn.functional
    inputs = torch.cat([feat, feat.mean(1, keepdim=True).expand(-1, R, -1)], -1)
    fc = lambda k, inp: F.leaky_relu(inp @ W[k * h:(k + 1) * h].T + b[k * h:(k + 1) * h], slope)
    box = fc(0, inputs)
    parts, k = [box], 1
    if "rel" in factors:
        parts.append(fc(k, (inputs.unsqueeze(1) + inputs.unsqueeze(2)) / 2).view(B, R * R, h))
        k += 1
    if "attr" in factors:
        parts.append(fc(k, inputs))
    if "img" in factors:
        parts.append(box.mean(1, keepdim=True))
    return torch.cat(parts, 1)


@pytest.mark.parametrize("B,R,n,H,factors,dt", [(3, 5, 24, 32, ("rel", "attr", "img"), "f32"), (4, 36, 64, 256, (), "f32"), (2, 7, 40, 64, ("rel",), "f32"),
                                                (5, 9, 16, 128, ("attr", "img"), "f32"), (6, 36, 96, 256, ("rel", "attr", "img"), "bf16"),
                                                (64, 36, 2048, 256, (), "bf16")])
def test_vis_box_rel_encoder(B, R, n, H, factors, dt):
    """encoders.vis_box_rel_encoder (one GEMM for the F encoders + one per-image GEMM + the HIP epilogue; adjoint + two split-K weight
    gradients written into the two column halves of one tensor) against the reference's formulation in float64 torch ops: the factor
    tensor, and the gradients w.r.t. the region features, the stacked weights and biases.  float32: 2e-5 / 5e-5 of max; bf16 storage:
    the forward value to 2e-2 of max, gradients to 5e-2 relative L2 (LeakyReLU' flips where a bf16 pre-activation rounds across 0)."""
    from vlgae_amd import encoders
    tdt = torch.bfloat16 if dt == "bf16" else torch.float32
    g = torch.Generator().manual_seed(B * 100 + R)
    F_ = 1 + ("rel" in factors) + ("attr" in factors)
    feat = (torch.randn(B, R, n, generator=g) * 0.5).to(dev(), tdt).requires_grad_(True)
    W = (torch.randn(F_ * H, 2 * n, generator=g) * (2 * n) ** -0.5).to(dev(), tdt).requires_grad_(True)
    b = (torch.randn(F_ * H, generator=g) * 0.1).to(dev(), tdt).requires_grad_(True)
    mid, split, names = encoders.vis_box_rel_encoder(feat, W, b, "rel" in factors, "attr" in factors, "img" in factors)
    V = R + ("rel" in factors) * R * R + ("attr" in factors) * R + ("img" in factors)
    assert tuple(mid.shape) == (B, V, H) and sum(split) == V and names[0] == "obj" and mid.dtype == tdt
    cot = torch.randn(B, V, H, generator=g).to(dev(), tdt)
    got = torch.autograd.grad(mid, [feat, W, b], cot)
    f64, W64, b64 = (x.detach().double().requires_grad_(True) for x in (feat, W, b))
    ref = _vis_encoder_reference(f64, W64, b64, factors)
    want = torch.autograd.grad(ref, [f64, W64, b64], cot.double())
    if dt == "f32":
        assert float((mid.double() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))
        for name, a, w in zip(("feat", "W", "b"), got, want):
            assert float((a.double() - w).abs().max()) <= 5e-5 * max(1.0, float(w.abs().max())), name
    else:
        assert float((mid.double() - ref).abs().max()) <= 2e-2 * max(1.0, float(ref.abs().max()))
        for name, a, w in zip(("feat", "W", "b"), got, want):
            assert float((a.double() - w).norm()) <= 5e-2 * float(w.norm()), (name, float((a.double() - w).norm()) / float(w.norm()))
    mid2, _, _ = encoders.vis_box_rel_encoder(feat, W, b, "rel" in factors, "attr" in factors, "img" in factors)
    got2 = torch.autograd.grad(mid2, [feat, W, b], cot)
    assert torch.equal(mid, mid2) and all(torch.equal(a, c) for a, c in zip(got, got2))       # fixed summation orders: bit-reproducible
    # the mask vis_feat_unprune builds for this layout (joint.py:140-170)
    box_mask = (torch.rand(B, R, generator=g) > 0.3).to(dev())
    vm = encoders.factor_mask(box_mask, "rel" in factors, "attr" in factors, "img" in factors)
    assert tuple(vm.shape) == (B, V) and torch.equal(vm[:, :R], box_mask)
    if "rel" in factors:
        rel = (box_mask.unsqueeze(1) * box_mask.unsqueeze(2)).triu(1).view(B, -1)
        assert torch.equal(vm[:, R:R + R * R], rel)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_mlp_encoder_and_counter_based_dropout(dt):
    """encoders.mlp_encoder = MLPEncoder.forward (mlp_encoder.py:36-40).  (i) With an explicit nn.Dropout mask: value and gradients
    against float64 torch ops on the same mask.  (ii) With the counter-based draw (DeviceRng): the result is x * m @ W^T for SOME mask m
    with entries in {0, 1/(1-p)} (recovered by running the same draw on a tensor of ones), the backward pass regenerates the SAME mask
    (d_emb = (g W) * m exactly as recomputed from m), the keep rate is 1 - p within 4 sigma, `advance()` changes the mask, two sites
    draw different masks from one state, and a re-created generator with the same seed reproduces the bits."""
    from vlgae_amd import encoders
    tdt = torch.bfloat16 if dt == "bf16" else torch.float32
    B, L, E, h, p = 16, 40, 800, 256, 0.33
    g = torch.Generator().manual_seed(4)
    emb = (torch.randn(B, L, E, generator=g) * 0.5).to(dev(), tdt).requires_grad_(True)
    W = (torch.randn(h, E, generator=g) * E ** -0.5).to(dev(), tdt).requires_grad_(True)
    cot = torch.randn(B, L, h, generator=g).to(dev(), tdt)
    mask = ((torch.rand(B, L, E, generator=g) >= p).float() / (1 - p)).to(dev())
    tol = 1e-5 if dt == "f32" else 2e-2
    # (i) explicit mask
    x = encoders.mlp_encoder(emb, W, p, mask=mask)
    ge, gw = torch.autograd.grad(x, [emb, W], cot)
    e64, W64 = emb.detach().double().requires_grad_(True), W.detach().double().requires_grad_(True)
    ref = (e64 * mask.double()) @ W64.T
    re, rw = torch.autograd.grad(ref, [e64, W64], cot.double())
    for name, a, w in (("x", x, ref), ("d_emb", ge, re), ("d_W", gw, rw)):
        assert float((a.double() - w).abs().max()) <= tol * max(1.0, float(w.abs().max())), name
    # eval mode: the Linear alone
    assert float((encoders.mlp_encoder(emb, W, p, training=False).double() - e64 @ W64.T).abs().max()) <= tol * max(1.0, float(ref.abs().max()))
    # (ii) counter-based draw
    rng = encoders.DeviceRng(1234, dev())
    ones = torch.ones(B, L, E, device=dev(), dtype=torch.float32)
    m0 = encoders.dropout(ones, p, rng=rng, site=encoders.SITE_TEXT_ENCODER)
    vals = torch.unique(m0)
    thr = round(p * 65536)
    scale = 1.0 / (1.0 - thr / 65536.0)
    assert vals.numel() == 2 and float(vals[0]) == 0.0 and abs(float(vals[1]) - scale) < 1e-6
    keep = float((m0 != 0).double().mean())
    n_el = B * L * E
    assert abs(keep - (1 - p)) <= 4 * (p * (1 - p) / n_el) ** 0.5 + 2.0 ** -16, keep
    x = encoders.mlp_encoder(emb, W, p, rng=rng)
    ge, gw = torch.autograd.grad(x, [emb, W], cot)
    ref = (e64 * m0.double()) @ W64.T
    re, rw = torch.autograd.grad(ref, [e64, W64], cot.double())
    for name, a, w in (("x", x, ref), ("d_emb", ge, re), ("d_W", gw, rw)):
        assert float((a.double() - w).abs().max()) <= tol * max(1.0, float(w.abs().max())), "rng " + name
    assert torch.equal(ge == 0, (m0 == 0) | (ge == 0))                      # dropped elements get exactly zero gradient
    m_other_site = encoders.dropout(ones, p, rng=rng, site=encoders.SITE_MID_FF)
    assert not torch.equal(m_other_site, m0) and abs(float(((m_other_site != 0) & (m0 != 0)).double().mean()) - (1 - p) ** 2) < 5e-3   # independent
    rng.advance()
    m1 = encoders.dropout(ones, p, rng=rng, site=encoders.SITE_TEXT_ENCODER)
    assert not torch.equal(m1, m0)
    rng2 = encoders.DeviceRng(1234, dev())
    assert torch.equal(encoders.dropout(ones, p, rng=rng2, site=encoders.SITE_TEXT_ENCODER), m0)
    rng2.advance()
    assert torch.equal(encoders.dropout(ones, p, rng=rng2, site=encoders.SITE_TEXT_ENCODER), m1)
    # SharedDropout ([B,1,E] masks, nn/dropout.py:52-53) through the same kernel
    sm = ((torch.rand(B, E, generator=g) >= 0.2).float() / 0.8).to(dev())
    xs = encoders.dropout(emb, 0.0, mask=sm, shared_rows=L)
    assert float((xs.double() - emb.detach().double() * sm.double().unsqueeze(1)).abs().max()) <= (1e-6 if dt == "f32" else 2.0 ** -8 * 4)
    # argument checks
    with pytest.raises(ValueError):
        encoders.dropout(emb, p)
    with pytest.raises(RuntimeError, match="no CPU path"):
        encoders.mlp_encoder(emb.detach().cpu(), W.detach().cpu(), p, training=False)


# ------------------------------------------------------------------------------------------------ multi-GPU (RCCL)
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs >= 2 GPUs: the RCCL (nccl backend) path of bench.py")
@pytest.mark.parametrize("workload", ["dp", "train_step"])
def test_bench_two_gpus_over_rccl(workload):
    """First box with two GPUs exercises RCCL without anyone asking: `bench.py --gpus 2` self-launches two rank
    processes on the nccl backend; the line must report both ranks in the collective, and bench.py itself asserts that
    the all-reduced buffer is the sum over ranks (expected counts / word counts)."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "VLGAE_BENCH_DRYRUN", "VLGAE_BENCH_SHARE_GPU", "VLGAE_DIST_BACKEND"):
        env.pop(k, None)
    cmd = [sys.executable, "bench.py", "--gpus", "2", "--steps", "5", "--warmup", "2", "--cpu-seconds", "0",
           "--workload", workload]
    proc = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.lstrip().startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, proc.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["data"] == "synthetic" and out["value"] > 0
    assert out["comm"]["backend"] == "nccl" and out["comm"]["rccl_ranks_seen"] == 2
    assert out["comm"]["allreduce_ms"] > 0
    if workload == "train_step":
        chk = out["comm"]["mean_over_ranks_check"]
        assert abs(chk["slot"] - chk["expected"]) <= 1e-3 * chk["expected"]
    else:
        assert out["train_step_sharded"]["comm"]["rccl_ranks_seen"] == 2


@pytest.mark.timeout(900)
@pytest.mark.parametrize("workload", ["dp", "train_step"])
def test_bench_two_ranks_sharing_one_gpu(workload):
    """The multi-rank path with REAL kernels on the 1-GPU box: `bench.py --gpus 2` self-launches two fresh rank processes, both on
    cuda:0, collectives over gloo (VLGAE_BENCH_SHARE_GPU=1 -- labelled DEBUG in the line, never a measurement).  What it executes
    that no CPU dry-run can: HIP-graph capture of the sharded step while a process group is alive, the buckets' collectives
    enqueued behind a graph replay, bench.py's own mean-over-ranks / word-count assertions on device results, and the line's
    `step_mode` saying what actually ran (graph, unless the capture failed and the in-process eager fallback took over)."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", VLGAE_BENCH_SHARE_GPU="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "VLGAE_BENCH_DRYRUN", "VLGAE_DIST_BACKEND"):
        env.pop(k, None)
    cmd = [sys.executable, "bench.py", "--gpus", "2", "--steps", "5", "--warmup", "2", "--cpu-seconds", "0",
           "--workload", workload, "--step-mode", "graph", "--batch", "64"]
    proc = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=800)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.lstrip().startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, proc.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["value"] > 0 and "DEBUG: ranks share one GPU" in out["config"]["parallelism"]
    assert out["comm"]["backend"] == "gloo" and out["comm"]["rccl_ranks_seen"] == 2 and out["comm"]["allreduce_ms"] > 0
    ts_line = out if workload == "train_step" else out["train_step_sharded"]
    assert "error" not in ts_line, ts_line
    chk = ts_line["comm"]["mean_over_ranks_check"]
    assert abs(chk["slot"] - chk["expected"]) <= 1e-3 * chk["expected"]
    assert ts_line["step_mode"].startswith("graph") and "capture_error" not in ts_line, ts_line


# ------------------------------------------------------------------------------------------------ lang_feat_max_tree
def _langfeat_params(g, device, dtype=torch.float32):
    from conftest import arcenc_w1
    w_enc = np.concatenate([g["w_word"], g["w_child"], g["w_parent"]], 0)
    b_enc = np.concatenate([g["b_word"], g["b_child"], g["b_parent"]], 0)
    return [t(a).to(dtype).requires_grad_(True) for a in (w_enc, b_enc, arcenc_w1(g), g["w2"], g["b_arc"])]


def _langfeat_grad_close(got, ref, name, tol):
    scale = max(1.0, float(np.abs(ref).max()))
    assert float(np.abs(got.astype(np.float64) - ref).max()) <= tol * scale, name


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("path", golden_files("langfeat_"), ids=golden_ids("langfeat_"))
def test_lang_feat_max_tree_golden(ts, oracle_mod, path, dtype):
    """vlgae_amd.langfeat.lang_feat_max_tree against the reference's own method (joint.py:235-292) and torch autograd through
    it.  float32 features (the reference's `precision: 32`) are computed in float32 end to end -- nothing is down-cast: tolerance
    1e-4 of the largest reference magnitude per tensor, values and gradients, against the reference's own numbers.
    bfloat16 features compute in bf16 with fp32 accumulation: tolerance 2e-2 of the largest reference magnitude per tensor
    (bf16 has 8 mantissa bits: 4e-3 per rounding, a handful of roundings per path); masks, heads exact; marginals 5e-5.
    Gradients through LeakyReLU' are discontinuous in the pre-activations: one that is within bf16 rounding of zero takes the
    other branch than in the fp32 reference and its term changes by the factor 1 / slope.  So the gradients are held (a) to
    the tolerance against the oracle's adjoint evaluated on the branches the device took (the oracle itself is pinned on the
    reference's gradients in tests/test_oracle_golden.py), with at most 1 % of the branches differing from the reference's,
    and (b) to 8e-2 in relative L2 norm against the reference's own gradients."""
    from vlgae_amd import langfeat
    from conftest import arcenc_check_w1_grad, arcenc_w1
    g = load(path)
    f32 = dtype == torch.float32
    x = t(g["x"]).to(dtype).requires_grad_(True)
    lengths = t(g["lengths"])
    params = _langfeat_params(g, dev(), dtype)
    aux = {}
    txt, txt_mask, txt_marginal = langfeat.lang_feat_max_tree(x, lengths, t(g["merged_dec"]), t(g["merged_attach"]), *params,
                                                               add_marginal=bool(g["add_marginal"]), slope=float(g["slope"]), aux=aux)
    assert txt.dtype == dtype and tuple(txt.shape) == g["txt"].shape            # the features' own dtype: no silent down-cast
    assert (aux["heads"].cpu().numpy() == g["predicted"]).all()
    assert (txt_mask.cpu().numpy() == g["txt_mask"]).all()
    assert np.abs(txt_marginal.cpu().numpy() - g["txt_marginal"]).max() <= MARG_TOL
    tol = 1e-4 if f32 else 2e-2
    assert np.abs(txt.detach().float().cpu().numpy() - g["txt"]).max() <= tol * max(1.0, np.abs(g["txt"]).max())
    grads = torch.autograd.grad(txt, [x] + params, t(g["dout"]).to(txt.dtype))
    d = g["w2"].shape[0]
    got = {"x": grads[0], "w_word": grads[1][:d], "w_child": grads[1][d:2 * d], "w_parent": grads[1][2 * d:], "b_word": grads[2][:d],
           "b_child": grads[2][d:2 * d], "b_parent": grads[2][2 * d:], "w2": grads[4], "b_arc": grads[5]}
    cb, pb = (aux[k].float().cpu().numpy() > 0 for k in ("child", "parent"))
    w1 = arcenc_w1(g)
    _, og = oracle_mod.lang_feat(g["x"], g["lengths"], g["predicted"], g["w_word"], g["b_word"], g["w_child"], g["b_child"],
                                 g["w_parent"], g["b_parent"], w1, g["w2"], g["b_arc"], float(g["slope"]), g["dout"], cb, pb)
    _, og_ref = oracle_mod.lang_feat(g["x"], g["lengths"], g["predicted"], g["w_word"], g["b_word"], g["w_child"], g["b_child"],
                                     g["w_parent"], g["b_parent"], w1, g["w2"], g["b_arc"], float(g["slope"]), g["dout"])
    for k, v in got.items():
        v = v.float().cpu().numpy()
        _langfeat_grad_close(v, og[k], k, tol)
        ref = g["g_" + k]
        assert np.linalg.norm(v - ref) <= (1e-4 if f32 else 8e-2) * np.linalg.norm(ref), k
        if f32:   # fp32 pre-activations take the reference's branches: the reference's own gradients, element-wise
            _langfeat_grad_close(v, ref, k + " (reference)", tol)
    _langfeat_grad_close(grads[3].float().cpu().numpy(), og["w1"], "w1", tol)
    arcenc_check_w1_grad(grads[3].float().cpu().numpy(), g, tol)
    # the branches differ from the fp32 reference's on a handful of near-zero pre-activations only
    x1 = np.concatenate([(g["x"] * (np.arange(g["x"].shape[1])[None] < g["lengths"][:, None])[..., None]).sum(1, keepdims=True)
                         / g["lengths"][:, None, None], g["x"]], 1).astype(np.float64)
    ref_cb = x1 @ g["w_child"].T.astype(np.float64) + g["b_child"] > 0
    assert (ref_cb != cb).mean() <= (0.0 if f32 else 0.01)


def test_lang_feat_dropout_and_word_only(ts):
    """SharedDropout (nn/dropout.py:42-63: one mask [B,1,d] per encoder, after the activation, nn/common.py:47-51) inside
    lang_feat_max_tree and lang_feat_word_only (joint.py:193-211), both storage types, against the same lines in torch ops
    (float32: 1e-5 * max; bf16: 2e-2 * max), plus: masks given as views of one wider draw are taken in place, and a
    Viterbi result remembered by the asynchronous form is ordered for a `.max` taken BEFORE `handle.wait()`."""
    from vlgae_amd import langfeat
    from vlgae_amd.torch_struct import functional as Fn
    B, L, h, d, p = 5, 11, 64, 32, 0.33
    N = L + 1
    gen = torch.Generator().manual_seed(9)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=gen) * sc).to(dev())
    lengths = torch.tensor([11, 7, 3, 11, 1], device=dev())
    dec, attach, root = rnd(B, L, 2, 2, 2).log_softmax(-1), rnd(B, L, L, 2), rnd(B, L).log_softmax(-1)
    md, ma = ts.DMV1o.merge(dec, attach, root)
    heads = ts.DMV1o([md, ma], lengths).argmax_heads
    drop4 = langfeat.shared_dropout_masks(B, d, p, n=4, device=dev())
    assert all(min(abs(float(v)), abs(float(v) - 1 / (1 - p))) < 1e-6 for v in np.unique(drop4.cpu().numpy()))
    for dtype, tol in ((torch.float32, 1e-5), (torch.bfloat16, 2e-2)):
        mk = lambda *s, sc=1.0: rnd(*s, sc=sc).to(dtype).requires_grad_(True)
        x, w_enc, b_enc = mk(B, L, h, sc=0.5), mk(3 * d, h, sc=h ** -0.5), mk(3 * d, sc=0.1)
        w1, w2, b_arc = mk(d, d, d, sc=1.0 / d), mk(d, d, sc=d ** -0.5), mk(d, sc=0.1)
        leaves = [x, w_enc, b_enc, w1, w2, b_arc]
        txt, tmask, _ = langfeat.lang_feat_max_tree(x, lengths, md, ma, w_enc, b_enc, w1, w2, b_arc, drop=drop4[:, 1:4])
        word, wmask, wmarg = langfeat.lang_feat_word_only(x, lengths, w_enc[:d], b_enc[:d], drop=drop4[:, 0:1])
        assert txt.dtype == dtype and word.dtype == dtype
        dout, dword = rnd(B, 2 * N, d), rnd(B, N, d)
        got = torch.autograd.grad([txt, word], leaves, [dout.to(dtype), dword.to(dtype)])
        # the reference's lines (joint.py:193-211, 262-288; MLP.forward nn/common.py:47-51) in float64 torch ops
        f = [a.detach().double().requires_grad_(True) for a in leaves]
        X, We, be, W1, W2, ba = f
        m = (torch.arange(L, device=dev())[None] < lengths[:, None])
        rootrow = (X.masked_fill(~m.unsqueeze(2), 0).sum(1) / lengths.unsqueeze(1)).unsqueeze(1)
        X1 = torch.cat([rootrow, X], 1)
        D = drop4.double()
        lin = lambda k, inp: inp @ We[k * d:(k + 1) * d].T + be[k * d:(k + 1) * d]
        rword = lin(0, X1) * D[:, 1:2]
        rchild = torch.nn.functional.leaky_relu(lin(1, X1), 0.01) * D[:, 2:3]
        rparent = torch.nn.functional.leaky_relu(lin(2, X1.gather(1, heads.unsqueeze(-1).expand(-1, -1, h))), 0.01) * D[:, 3:4]
        rarc = torch.einsum("bcx,xhy,bcy->bch", rchild, W1, rparent) + (rchild + rparent) @ W2 + ba
        rtxt = torch.cat([rword, rarc], 1)
        rword0 = lin(0, X1) * D[:, 0:1]
        want = torch.autograd.grad([rtxt, rword0], f, [dout.double(), dword.double()])
        cl = lambda a, b, name: np.testing.assert_array_less(float((a.double() - b).abs().max()), tol * max(1.0, float(b.abs().max())) + 1e-30, name)
        cl(txt, rtxt, "txt")
        cl(word, rword0, "word_only")
        assert torch.equal(wmask, torch.cat([torch.zeros(B, 1, dtype=torch.bool, device=dev()), m], 1)) and torch.equal(wmarg, wmask.float())
        if dtype == torch.float32:
            for name, a, b in zip(("x", "w_enc", "b_enc", "w1", "w2", "b_arc"), got, want):
                cl(a, b, "grad " + name)
        else:
            for name, a, b in zip(("x", "w_enc", "b_enc", "w1", "w2", "b_arc"), got, want):
                assert float((a.double() - b).norm()) <= 8e-2 * float(b.norm()), name
        # a dropped channel carries no gradient into its encoder's bias column... and a kept one does
        dead = (drop4[:, 2] == 0).all(0).cpu().numpy()
        assert np.all(got[2].float().cpu().numpy()[d:2 * d][dead] == 0)
    # ---- the remembered Viterbi result of the asynchronous form: `.max` before `handle.wait()` ----
    Fn.viterbi_forget()
    big = 256
    gen2 = torch.Generator().manual_seed(3)
    dec2 = torch.randn(big, 40, 2, 2, 2, generator=gen2).log_softmax(-1).to(dev())
    att2, root2 = torch.randn(big, 40, 40, 2, generator=gen2).to(dev()), torch.randn(big, 40, generator=gen2).log_softmax(-1).to(dev())
    md2, ma2 = ts.DMV1o.merge(dec2, att2, root2)
    len2 = torch.full((big,), 40, device=dev())
    fresh = ts.DMV1o([md2.clone(), ma2.clone()], len2).max.clone()
    for _ in range(5):
        Fn.viterbi_forget()
        handle = ts.DMV1o([md2, ma2], len2).marginals_and_heads_async(keep_viterbi=True)
        early = ts.DMV1o([md2, ma2], len2).max.clone()          # cache hit while the side stream may still be writing: must be ordered
        handle.wait()
        assert torch.equal(early, fresh)
    Fn.viterbi_forget()


def test_lang_feat_max_tree_config_size(ts, oracle_mod):
    """B = 256, L = 40, h = 256, d = 128 (BASELINE.json configs[4] widths): against the fp64 oracle on the bf16-rounded inputs
    for a slice of the batch, run-to-run bit equality (fixed summation orders: split-K partials, scatter-add by head), and the
    one-Viterbi-pass-per-step contract (`keep_viterbi` -> a later `DMV1o(same potentials).max` launches nothing)."""
    from vlgae_amd import langfeat
    from vlgae_amd.torch_struct import functional as F
    B, L, h, d = 256, 40, 256, 128
    g = torch.Generator().manual_seed(5)
    bf = torch.bfloat16
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dev())
    x = rnd(B, L, h, sc=0.5).to(bf).requires_grad_(True)
    w_enc, b_enc = rnd(3 * d, h, sc=h ** -0.5).to(bf).requires_grad_(True), rnd(3 * d, sc=0.1).to(bf).requires_grad_(True)
    w1, w2, b_arc = rnd(d, d, d, sc=1.0 / d).to(bf).requires_grad_(True), rnd(d, d, sc=d ** -0.5).to(bf).requires_grad_(True), rnd(d, sc=0.1).to(bf).requires_grad_(True)
    dec = torch.randn(B, L, 2, 2, 2, generator=g).log_softmax(-1).to(dev())
    attach, root = torch.randn(B, L, L, 2, generator=g).to(dev()), torch.randn(B, L, generator=g).log_softmax(-1).to(dev())
    md, ma = ts.DMV1o.merge(dec, attach, root)
    md, ma = md.to(bf), ma.to(bf)
    lengths = torch.randint(L // 2, L + 1, (B,), generator=g)
    lengths[0] = L
    lengths = lengths.to(dev())
    params = [w_enc, b_enc, w1, w2, b_arc]
    F.viterbi_forget()
    aux = {}
    txt, txt_mask, txt_marginal = langfeat.lang_feat_max_tree(x, lengths, md, ma, *params, keep_viterbi=True, aux=aux)
    dout = (torch.randn(B, 2 * (L + 1), d, generator=g).to(dev()) * txt_mask.unsqueeze(-1)).to(bf)
    grads = torch.autograd.grad(txt, [x] + params, dout)
    # the Viterbi pass is remembered: .max of a detached alias of the same potentials reuses it and matches a fresh launch
    pot = [md.detach().requires_grad_(True), ma.detach().requires_grad_(True)]
    hit = F._viterbi_lookup(pot[0], pot[1], lengths)
    assert hit is not None
    best = ts.DMV1o(pot, lengths).max
    gd, ga = torch.autograd.grad(-best.sum(), pot)
    F.viterbi_forget()
    best2 = ts.DMV1o(pot, lengths).max
    gd2, ga2 = torch.autograd.grad(-best2.sum(), pot)
    assert torch.equal(best, best2) and torch.equal(gd, gd2) and torch.equal(ga, ga2)
    heads = ts.DMV1o([md, ma], lengths).argmax_heads
    assert torch.equal(heads, hit[3])
    md[0, 1, 0, 0, 0] += 1.0                                            # an in-place update through any alias invalidates the entry
    F._viterbi_remember(md, ma, lengths, hit)
    md[0, 1, 0, 0, 0] -= 1.0
    assert F._viterbi_lookup(pot[0], pot[1], lengths) is None
    F.viterbi_forget()
    # run-to-run bit equality
    txt_b, _, _ = langfeat.lang_feat_max_tree(x, lengths, md, ma, *params)
    grads_b = torch.autograd.grad(txt_b, [x] + params, dout)
    assert torch.equal(txt, txt_b) and all(torch.equal(a, b) for a, b in zip(grads, grads_b))
    # oracle on a slice (rows of the first 6 sentences; weight gradients need the whole batch and are checked by linearity below)
    S = 6
    f64 = lambda a: a.detach().float().cpu().numpy().astype(np.float64)
    wn, bn = f64(w_enc), f64(b_enc)
    cb, pb = (aux[k][:S].float().cpu().numpy() > 0 for k in ("child", "parent"))      # the LeakyReLU branches the device took
    otxt, og = oracle_mod.lang_feat(f64(x)[:S], lengths[:S].cpu().numpy(), heads[:S].cpu().numpy(), wn[:d], bn[:d], wn[d:2 * d], bn[d:2 * d],
                                    wn[2 * d:], bn[2 * d:], f64(w1), f64(w2), f64(b_arc), 0.01, f64(dout)[:S], cb, pb)
    tol = 2e-2
    assert np.abs(f64(txt)[:S] - otxt).max() <= tol * np.abs(otxt).max()
    _langfeat_grad_close(f64(grads[0])[:S], og["x"], "x", tol)
    # parameter gradients are sums over sentences: the batch run on the first S sentences alone must match the oracle's
    xs = x[:S].detach().requires_grad_(True)
    aux_s = {}
    txt_s, _, _ = langfeat.lang_feat_max_tree(xs, lengths[:S].contiguous(), md[:S].contiguous(), ma[:S].contiguous(), *params, aux=aux_s)
    cb, pb = (aux_s[k].float().cpu().numpy() > 0 for k in ("child", "parent"))      # (a smaller GEMM may round differently)
    _, og = oracle_mod.lang_feat(f64(x)[:S], lengths[:S].cpu().numpy(), heads[:S].cpu().numpy(), wn[:d], bn[:d], wn[d:2 * d], bn[d:2 * d],
                                 wn[2 * d:], bn[2 * d:], f64(w1), f64(w2), f64(b_arc), 0.01, f64(dout)[:S], cb, pb)
    gs = torch.autograd.grad(txt_s, [xs] + params, dout[:S])
    for name, got, ref in (("w_enc", gs[1], np.concatenate([og["w_word"], og["w_child"], og["w_parent"]])),
                           ("b_enc", gs[2], np.concatenate([og["b_word"], og["b_child"], og["b_parent"]])), ("w1", gs[3], og["w1"]),
                           ("w2", gs[4], og["w2"]), ("b_arc", gs[5], og["b_arc"])):
        _langfeat_grad_close(f64(got), ref, name, tol)


# ------------------------------------------------------------------------------------------------ scorer -> merged potentials (f1)
@pytest.mark.parametrize("path", golden_files("scorer_"), ids=golden_ids("scorer_"))
def test_ndmv_potentials_golden(ts, path):
    """vlgae_amd.scorer.ndmv_potentials against the reference's own `DiscriminativeNDMV._forward` (ldndmv.py:171-216) and torch
    autograd through it: fp32 in, fp32 out.  Fills (-1e12, -1e20) bit-exact; scores 2e-5 (fp32 dots and log-sum-exp in a
    different summation order); gradients 1e-4 of the largest reference magnitude."""
    from vlgae_amd import scorer
    g = load(path)
    ins = [t(g[k]).requires_grad_(True) for k in ("x1", "x2", "y1", "y2", "root_rule")]
    md, ma = scorer.ndmv_potentials(*ins, t(g["token"]), t(g["head_mask"]), float(g["mask_fill"]))
    for got, ref in ((md, g["merged_dec"]), (ma, g["merged_attach"])):
        got = got.detach().cpu().numpy()
        big = np.abs(ref) > 1e11
        assert (got[big] == ref[big]).all()
        assert np.abs(got[~big] - ref[~big]).max() <= 2e-5
    grads = torch.autograd.grad([md, ma], ins, [t(g["g_merged_dec"]), t(g["g_merged_attach"])])
    for k, v in zip(("x1", "x2", "y1", "y2", "root_rule"), grads):
        ref = g["g_" + k]
        assert np.abs(v.cpu().numpy() - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max()), k


def test_ndmv_potentials_config_size_feeds_the_dp(ts, oracle_mod):
    """B = 256, L = 40, T = 45, r = 16 (config/model/vlgae.yaml): the fused score construction feeding the fused DP --
    expected counts back to the scorers' inputs in three launches -- against the fp64 oracle chain (oracle.ndmv_potentials ->
    oracle.dmv1o -> adjoint) on a slice, run-to-run bit equality, bf16 storage of the potentials."""
    from vlgae_amd import scorer
    B, L, T, r = 256, 40, 45, 16
    g = torch.Generator().manual_seed(9)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dev())
    ins = [rnd(B, L, 2, 2, r, sc=0.5).requires_grad_(True), rnd(T, 2, 2, r, sc=0.5).requires_grad_(True),
           rnd(B, L, 2, 2, r, sc=0.5).requires_grad_(True), rnd(2, 2, 2, r, sc=0.5).requires_grad_(True),
           torch.randn(T, generator=g).log_softmax(-1).to(dev()).requires_grad_(True)]
    token = torch.randint(0, T, (B, L), generator=g).to(dev())
    head_mask = (torch.rand(B, L, generator=g) < 0.1).to(dev())
    lengths = torch.randint(L // 2, L + 1, (B,), generator=g)
    lengths[0] = L
    lengths = lengths.to(dev())

    def run(out_dtype):
        md, ma = scorer.ndmv_potentials(*ins, token, head_mask, out_dtype=out_dtype)
        logZ = ts.DMV1o([md, ma], lengths).partition
        return md, ma, logZ, torch.autograd.grad(logZ.sum(), ins)
    md, ma, logZ, grads = run(torch.float32)
    md2, ma2, logZ2, grads2 = run(torch.float32)
    assert torch.equal(ma, ma2) and torch.equal(logZ, logZ2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    S = 5
    f64 = lambda a: a.detach().cpu().numpy().astype(np.float64)
    omd, oma = oracle_mod.ndmv_potentials(f64(ins[0])[:S], f64(ins[1]), f64(ins[2])[:S], f64(ins[3]), f64(ins[4]), token[:S].cpu().numpy(),
                                          head_mask[:S].cpu().numpy())
    big = np.abs(oma) > 1e11
    assert (ma[:S].detach().cpu().numpy()[big] == oma[big].astype(np.float32)).all() and np.abs(f64(ma)[:S][~big] - oma[~big]).max() <= 2e-5
    olz, ogd, oga = oracle_mod.dmv1o(omd, oma, lengths[:S].cpu().numpy(), "log", np.float64)
    olz = np.asarray(olz).reshape(-1)
    assert (np.abs(f64(logZ)[:S, 0] - olz) <= logz_tol(olz)).all()
    _, _, og = oracle_mod.ndmv_potentials(f64(ins[0])[:S], f64(ins[1]), f64(ins[2])[:S], f64(ins[3]), f64(ins[4]), token[:S].cpu().numpy(),
                                          head_mask[:S].cpu().numpy(), -1e20, ogd, oga)
    for k, idx in (("x1", 0), ("y1", 2)):                                  # per-sentence gradients: the slice's rows
        assert np.abs(f64(grads[idx])[:S] - og[k]).max() <= 2e-4 * max(1.0, np.abs(og[k]).max()), k
    # batch-shared tables: gradients are sums over sentences -- the first S sentences alone must match the oracle's
    ins_s = [ins[0][:S].detach().requires_grad_(True), ins[1], ins[2][:S].detach().requires_grad_(True), ins[3], ins[4]]
    md_s, ma_s = scorer.ndmv_potentials(*ins_s, token[:S].contiguous(), head_mask[:S].contiguous())
    gs = torch.autograd.grad(ts.DMV1o([md_s, ma_s], lengths[:S].contiguous()).partition.sum(), ins_s)
    for k, idx in (("x2", 1), ("y2", 3), ("root_rule", 4)):
        assert np.abs(f64(gs[idx]) - og[k]).max() <= 2e-4 * max(1.0, np.abs(og[k]).max()), k
    # bf16 storage of the potentials (what the DP benchmark reads): the rounding of the stored potentials is the only difference
    md_b, ma_b, logZ_b, _ = run(torch.bfloat16)
    assert ma_b.dtype == torch.bfloat16 and torch.equal(ma_b, ma.to(torch.bfloat16)) and torch.equal(md_b, md.to(torch.bfloat16))


def test_bilinear_align_backward_generic_path_is_reproducible():
    """the generic a9-backward kernel (d = 32 / 64, or > 96 rows / positions per pair) used to split its outer range
    up to 8 ways with atomicAdd partial sums -- order-dependent for more than two addends.  The split now stops at 2: two runs
    give the same bits (shape from the finding: B=8, A=256, Q=100, V=36), and d outside {32, 64, 128} is refused in forward."""
    from vlgae_amd import align
    g = torch.Generator().manual_seed(3)
    B, A, Q, V, d = 8, 256, 100, 36, 64
    txt = torch.randn(B, Q, d, generator=g).to(dev())
    vis = torch.randn(A, V, d, generator=g).to(dev())
    cot = torch.randn(B, A, Q, V, generator=g).to(dev())
    runs = [align.bilinear_align_backward(cot, txt, vis) for _ in range(3)]
    for gt, gv in runs[1:]:
        assert torch.equal(gt, runs[0][0]) and torch.equal(gv, runs[0][1])
    ref_t = torch.einsum("baqv,avd->bqd", cot.double(), vis.double())
    assert float((runs[0][0].double() - ref_t).abs().max()) <= 1e-4 * float(ref_t.abs().max())
    bad = torch.randn(2, 5, 48, generator=g).to(dev()).requires_grad_(True)
    with pytest.raises(ValueError, match="matching width"):
        align.gather_logit(None, (torch.randn(3, 4, 48).to(dev()), None, None), (bad, None, None))


@pytest.mark.parametrize("B,A,Q,V", [(9, 7, 82, 36), (3, 20, 97, 44), (2, 3, 200, 40), (17, 5, 5, 4)])
def test_bilinear_align_full_tensor_direct_kernel(oracle_mod, B, A, Q, V):
    """align_full_kernel (round 3: the materialised tensor alone, bf16, d = 128, V <= 44, V % 4 == 0 -- swapped MFMA operands, the
    wave's output block assembled in LDS in the output's own layout, linear copy-out) against the fp64 oracle and, bit for bit,
    against the LDS-tile kernel (taken when a maximum is requested as well), with and without masks; several query passes
    (Q > 96), captions past a multiple of the eight waves, a single region tile."""
    from vlgae_amd import align
    rng = np.random.default_rng(B * 1000 + Q)
    txt = t(rng.standard_normal((B, Q, 128)).astype(np.float32)).bfloat16()
    vis = t(rng.standard_normal((A, V, 128)).astype(np.float32)).bfloat16()
    tm, vm = rng.random((B, Q)) > 0.2, rng.random((A, V)) > 0.2
    for masks in (False, True):
        kw = dict(txt_mask=t(tm), vis_mask=t(vm)) if masks else {}
        got = align.bilinear_align(txt, vis, **kw)["full"]
        other = align.bilinear_align(txt, vis, max_v=True, **kw)["full"]
        assert torch.equal(got, other)
        ref = oracle_mod.bilinear_align(txt.float().cpu().numpy(), vis.float().cpu().numpy(), tm if masks else None, vm if masks else None,
                                        np.float64)["full"]
        big = np.abs(ref) > 1e19
        g = got.cpu().numpy()
        assert (g[big] == np.float32(-1e20)).all() and np.abs(g[~big] - ref[~big]).max() <= 1e-3


@pytest.mark.parametrize("B,L,T,r,dt", [(5, 11, 100, 12, "f32"), (3, 40, 45, 32, "bf16"), (2, 80, 30, 16, "f32"), (4, 6, 3, 5, "f32"),
                                        (2, 80, 45, 32, "f32"), (3, 63, 100, 16, "bf16")])   # the adjoint's coefficient table in several passes
def test_ndmv_potentials_shapes(oracle_mod, B, L, T, r, dt):
    """Ranks without a compile-time instantiation (run-time loop), long sentences, more tokens than positions, bf16 inputs;
    and the shape the workgroup's LDS cannot hold is refused, not mis-computed."""
    from vlgae_amd import scorer
    rng = np.random.default_rng(B * 100 + r)
    mk = lambda *s: (rng.standard_normal(s) * 0.5).astype(np.float32)
    arrs = [mk(B, L, 2, 2, r), mk(T, 2, 2, r), mk(B, L, 2, 2, r), mk(2, 2, 2, r)]
    root = np.log(rng.dirichlet(np.ones(T))).astype(np.float32)
    token = rng.integers(0, T, size=(B, L))
    hm = rng.random((B, L)) < 0.2
    if dt == "bf16":
        arrs = [torch.from_numpy(a).bfloat16().float().numpy() for a in arrs]
    g_md, g_ma = rng.random((B, L + 1, 2, 2, 2)).astype(np.float32), rng.random((B, L + 1, L + 1, 2)).astype(np.float32)
    omd, oma, og = oracle_mod.ndmv_potentials(*arrs, root, token, hm, -1e20, g_md, g_ma)
    ins = [t(a).bfloat16() if dt == "bf16" else t(a) for a in arrs] + [t(root)]
    for a in ins:
        a.requires_grad_(True)
    md, ma = scorer.ndmv_potentials(*ins, t(token), t(hm))
    for got, ref in ((md, omd), (ma, oma)):
        got = got.detach().cpu().numpy()
        big = np.abs(ref) > 1e11
        assert (got[big] == ref[big].astype(np.float32)).all() and np.abs(got[~big] - ref[~big]).max() <= 5e-5
    grads = torch.autograd.grad([md, ma], ins, [t(g_md), t(g_ma)])
    tol = 1e-2 if dt == "bf16" else 1e-4   # bf16 leaves get bf16 gradients
    for k, v in zip(("x1", "x2", "y1", "y2", "root_rule"), grads):
        assert np.abs(v.float().cpu().numpy() - og[k]).max() <= tol * max(1.0, np.abs(og[k]).max()), k
    if B == 5:
        with pytest.raises(RuntimeError, match="LDS"):
            scorer.ndmv_potentials(t(mk(1, 40, 2, 2, 64)), t(mk(5000, 2, 2, 64)), t(mk(1, 40, 2, 2, 64)), t(mk(2, 2, 2, 64)),
                                   t(np.zeros(5000, np.float32)), t(np.zeros((1, 40), np.int64)))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_ndmv_potentials_strided_side_by_side(oracle_mod, dt):
    """The scorers' inputs as column slices of wider GEMM outputs (rows a constant stride apart, read in place): attach.project1 |
    dec.project1 side by side in one [4 B L, 2r] buffer and x2 / y2 inside a [4 (T + 3), 4r] one, as vlgae_amd.parser_ff hands them.
    Values equal the contiguous call's bit for bit; the adjoint returns d_x1 | d_y1 side by side again, in the inputs' dtype."""
    from vlgae_amd import scorer
    B, L, T, r = 4, 9, 7, 16
    rng = np.random.default_rng(77)
    dtype = torch.bfloat16 if dt == "bf16" else torch.float32
    big = t((rng.standard_normal((B * L * 4, 2 * r)) * 0.5).astype(np.float32)).to(dtype)
    small = t((rng.standard_normal((4 * (T + 3), 4 * r)) * 0.5).astype(np.float32)).to(dtype)
    root = t(np.log(rng.dirichlet(np.ones(T))).astype(np.float32))
    token, hm = t(rng.integers(0, T, size=(B, L))), t(rng.random((B, L)) < 0.2)
    views = [big[:, :r].view(B, L, 2, 2, r), small[:4 * T, :r].view(T, 2, 2, r), big[:, r:].view(B, L, 2, 2, r),
             small[4 * T + 4:, 3 * r:].view(2, 2, 2, r)]
    assert not any(v.is_contiguous() for v in views)
    g_md, g_ma = t(rng.random((B, L + 1, 2, 2, 2)).astype(np.float32)), t(rng.random((B, L + 1, L + 1, 2)).astype(np.float32))
    res = []
    for ins in (views, [v.contiguous() for v in views]):
        ins = [v.detach().requires_grad_(True) for v in ins] + [root.clone().requires_grad_(True)]
        md, ma = scorer.ndmv_potentials(*ins, token, hm)
        res.append((md, ma, torch.autograd.grad([md, ma], ins, [g_md, g_ma])))
    (md_s, ma_s, g_s), (md_c, ma_c, g_c) = res
    assert torch.equal(md_s, md_c) and torch.equal(ma_s, ma_c)
    for a, b in zip(g_s, g_c):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    assert g_s[0].dtype == dtype and g_s[4].dtype == torch.float32
    assert g_s[2].data_ptr() == g_s[0].data_ptr() + r * g_s[0].element_size() and g_s[0].stride() == (L * 8 * r, 8 * r, 4 * r, 2 * r, 1)
    arrs = [v.float().cpu().numpy() for v in views]
    omd, oma, og = oracle_mod.ndmv_potentials(*arrs, root.cpu().numpy(), token.cpu().numpy(), hm.cpu().numpy(), -1e20, g_md.cpu().numpy(),
                                              g_ma.cpu().numpy())
    fin = np.abs(oma) < 1e11
    assert np.abs(ma_s.detach().cpu().numpy()[fin] - oma[fin]).max() <= 5e-5
    for k, v in zip(("x1", "x2", "y1", "y2", "root_rule"), g_s):
        assert np.abs(v.float().cpu().numpy() - og[k]).max() <= (1e-2 if dt == "bf16" else 1e-4) * max(1.0, np.abs(og[k]).max()), k


def test_linear_wgrad_bf16_outputs():
    """vlg_linear_wgrad writing the parameter's storage type: the bf16 results are the fp32 results rounded once (same reduction)."""
    from vlgae_amd import align
    gen = torch.Generator().manual_seed(4)
    K, M, N = 4200, 96, 136
    dy, x = torch.randn(K, M, generator=gen).to(dev(), torch.bfloat16), torch.randn(K, N, generator=gen).to(dev(), torch.bfloat16)
    dw32, db32 = align.linear_wgrad(dy, x)
    dw16, db16 = align.linear_wgrad(dy, x, out_dtype=torch.bfloat16)
    assert dw16.dtype == db16.dtype == torch.bfloat16 and torch.equal(dw16, dw32.bfloat16()) and torch.equal(db16, db32.bfloat16())
    _, xs16 = align.linear_wgrad(dy, x, want_x_colsum=True, out_dtype=torch.bfloat16)
    assert torch.equal(xs16, align.linear_wgrad(dy, x, want_x_colsum=True)[1].bfloat16())
    out = (torch.empty(M, N, dtype=torch.bfloat16, device=dev()), torch.empty(M, dtype=torch.bfloat16, device=dev()))
    align.linear_wgrad(dy, x, out=out)
    assert torch.equal(out[0], dw16) and torch.equal(out[1], db16)


def test_attn_fuse_backward_broadcast_cotangent():
    """The cotangent of the fused encodings as the parser's context_mode 'mean' produces it -- one row per sentence broadcast over the
    positions (a stride-0 view) -- is read in place and gives the gradients of the materialised tensor, bit for bit."""
    from vlgae_amd import align
    gen = torch.Generator().manual_seed(8)
    B, L, V, d, h = 5, 13, 9, 32, 64
    mk = lambda *s: torch.randn(*s, generator=gen).to(dev())
    leaves = [mk(B, V, d), mk(B, L + 1, d), mk(B, V, h), mk(B, L, h), mk(h), mk(h)]
    for a in leaves:
        a.requires_grad_(True)
    row = mk(B, h)
    out = align.attention_fuse(*leaves, 1e-5)
    g_view = torch.autograd.grad(out, leaves, row.unsqueeze(1).expand(B, L, h), retain_graph=True)
    g_full = torch.autograd.grad(out, leaves, row.unsqueeze(1).expand(B, L, h).contiguous())
    for a, b in zip(g_view, g_full):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_dmv1o_marginals_viterbi_one_launch(ts, dt):
    """vlg_dmv1o_marginals_viterbi (both DPs of lang_feat_max_tree as one grid (B, 2) launch) against the two separate launches it
    replaces, bit for bit: logZ / marginals of the Log semiring, best score / heads / tree counts of the Max semiring; ragged lengths,
    a sentence of length 1, an invalid length (NaN score, zero counts).  Longer sentences take the two-stream form, same results."""
    from vlgae_amd import _C
    from vlgae_amd.torch_struct import functional as F
    gen = torch.Generator().manual_seed(21)
    for B, L in ((37, 40), (5, 7), (3, 43), (3, 44), (4, 60)):
        N = L + 1
        dec = torch.randn(B, L, 2, 2, 2, generator=gen).log_softmax(-1).to(dev())
        attach = (torch.randn(B, L, L, 2, generator=gen) * 2).to(dev())
        root = torch.randn(B, L, generator=gen).log_softmax(-1).to(dev())
        md, ma = ts.DMV1o.merge(dec, attach, root)
        if dt == "bf16":
            md, ma = md.bfloat16(), ma.bfloat16()
        lengths = torch.randint(1, L + 1, (B,), generator=gen)
        lengths[0], lengths[1] = L, 1
        lengths = lengths.to(dev())
        assert bool(_C.lib().vlg_dmv1o_marginals_viterbi_supported(N)) == (N <= 44)
        F.viterbi_forget()
        logZ, gatt, heads = F.dmv1o_marginals_and_heads(md, ma, lengths, keep_viterbi=True)
        best, vdec, vatt, vheads = F._viterbi_lookup(md, ma, lengths)
        lz2, _, ga2 = F.dmv1o_run(md, ma, lengths, _C.SEMIRING_LOG, True, want_dec=False)
        b2, vd2, va2, h2 = F.dmv1o_viterbi(md, ma, lengths)
        assert torch.equal(logZ, lz2) and torch.equal(gatt, ga2)
        assert torch.equal(best, b2) and torch.equal(vdec, vd2) and torch.equal(vatt, va2) and torch.equal(heads, h2) and vheads is heads
        _, _, heads3 = F.dmv1o_marginals_and_heads(md, ma, lengths)          # heads only: the tree counts are not written
        assert torch.equal(heads3, h2)
        # one attachment per word; STOP decisions: two per word and the root's RIGHT one; one GO decision per attachment
        assert float(vatt.sum()) == float(lengths.sum()) and float(vdec[..., 1].sum()) == float((2 * lengths + 1).sum())
        assert float(vdec[..., 0].sum()) == float(lengths.sum())
    F.viterbi_forget()
    bad = torch.tensor([3, 0, 9], device=dev())
    md, ma = ts.DMV1o.merge(torch.zeros(3, 6, 2, 2, 2, device=dev()), torch.zeros(3, 6, 6, 2, device=dev()), torch.zeros(3, 6, device=dev()))
    logZ, gatt, heads = F.dmv1o_marginals_and_heads(md, ma, bad, keep_viterbi=True)
    assert torch.isnan(logZ[1:]).all() and not gatt[1:].any() and not heads[1:].any() and torch.isfinite(logZ[0])
    F.viterbi_forget()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_small_matmul(dtype):
    """vlg_small_gemm (one wavefront per 32 x 32 output tile, operands through element strides) against float64: plain / batched / broadcast
    operands, transposed and column-sliced views read in place, ragged M / N / K, bias, rank-one term, alpha, accumulate, both output types.
    float32 operands: exact products (v_mfma_f32_16x16x4_f32), 2e-6 relative to the magnitude sum; bf16: the products of bf16 inputs are
    exact in fp32, so the same bound on the fp32 output and one bf16 rounding on a bf16 output."""
    from vlgae_amd import align
    gen = torch.Generator().manual_seed(17)
    mk = lambda *s: torch.randn(*s, generator=gen).to(dev(), dtype)

    def check(name, got, a, b, alpha=1.0, bias=None, rank1=None, base=None):
        a64, b64 = a.double(), b.double()
        ref = alpha * (a64 @ b64)
        mag = abs(alpha) * (a64.abs() @ b64.abs())
        if bias is not None:
            ref = ref + bias.double().unsqueeze(-2)
        if rank1 is not None:
            ref = ref + rank1[0].double().unsqueeze(-1) * rank1[1].double().unsqueeze(-2)
        if base is not None:
            ref = ref + base.double()
        tol = 2e-6 * (mag + ref.abs()) + (2.0 ** -8 * ref.abs() if got.dtype == torch.bfloat16 else 0.0) + 1e-30
        err = (got.double() - ref).abs()
        assert got.shape == ref.shape and bool((err <= tol).all()), (name, float((err / tol).max()))

    a, b = mk(256, 150), mk(150, 256)
    check("plain", align.small_matmul(a, b), a, b)
    a3, b3 = mk(4, 256, 150), mk(4, 150, 256)
    check("batched", align.small_matmul(a3, b3), a3, b3)
    check("batched, fp32 out", align.small_matmul(a3, b3, out_dtype=torch.float32), a3, b3)
    check("transposed views", align.small_matmul(a3.transpose(1, 2), b3.transpose(1, 2)), a3.transpose(1, 2), b3.transpose(1, 2))
    wide = mk(70, 300)
    sl, bt = wide[:, 40:141], mk(33, 101).t()                      # column slice [70,101] x transposed [101,33]: ragged everything
    check("sliced x transposed", align.small_matmul(sl, bt), sl, bt)
    bias, u, v = mk(33), mk(70), mk(33)
    check("bias + rank one + alpha", align.small_matmul(sl, bt, alpha=0.25, bias=bias, rank1=(u, v)), sl, bt, 0.25, bias, (u, v))
    ub, vb, biasb = mk(4, 256), mk(4, 256), mk(4, 256)
    check("batched bias + rank one", align.small_matmul(a3, b3, bias=biasb, rank1=(ub, vb)), a3, b3, 1.0, biasb, (ub, vb))
    check("broadcast b", align.small_matmul(a3, b), a3, b.unsqueeze(0).expand(4, -1, -1))
    base = torch.randn(4, 256, 256, generator=gen).to(dev())
    out = base.clone()
    align.small_matmul(a3, b3, out=out, accumulate=True)
    check("accumulate into fp32", out, a3, b3, base=base)
    one = mk(1, 7), mk(7, 1)
    check("1 x 1", align.small_matmul(*one), *one)
    # both contraction indices unit-stride and 16-byte aligned rows: the one-load-per-fragment path; K = 264 has a ragged last chunk in bf16
    av, bv = mk(96, 264), mk(72, 264).t()
    check("16-byte fragments", align.small_matmul(av, bv), av, bv)
    av2 = mk(3, 40, 272)[:, :, 8:264]                                  # K = 256 inside a wider row: aligned, full chunks only
    bv2 = mk(3, 50, 256).transpose(1, 2)
    check("16-byte fragments, batched", align.small_matmul(av2, bv2, out_dtype=torch.float32), av2, bv2)
    odd, bo = mk(20, 131)[:, 1:], mk(130, 24)                          # rows an odd number of elements apart, start misaligned: element loads
    check("element loads", align.small_matmul(odd, bo), odd, bo)
    with pytest.raises(ValueError):
        align.small_matmul(a, b.float() if dtype == torch.bfloat16 else b.bfloat16())
    with pytest.raises(ValueError):
        align.small_matmul(a, mk(151, 256))
    # ---- several independent problems as ONE launch (vlg_small_gemm_group): bit-identical to the single launches, mixed shapes / dtypes / strides;
    # 14 problems span two launches of up to 12 ----
    other = torch.float32 if dtype == torch.bfloat16 else torch.bfloat16
    mo = lambda *s: torch.randn(*s, generator=gen).to(dev(), other)
    ao, bo2 = mo(40, 72), mo(72, 24)
    specs = [dict(a=a, b=b), dict(a=a3, b=b3, out_dtype=torch.float32), dict(a=sl, b=bt, alpha=0.25, bias=bias, rank1=(u, v)),
             dict(a=a3, b=b3, bias=biasb, rank1=(ub, vb)), dict(a=a3, b=b), dict(a=one[0], b=one[1]), dict(a=av, b=bv), dict(a=av2, b=bv2, out_dtype=torch.float32),
             dict(a=odd, b=bo), dict(a=ao, b=bo2), dict(a=ao, b=bo2, out_dtype=dtype), dict(a=a3.transpose(1, 2), b=b3.transpose(1, 2)),
             dict(a=bt.t(), b=sl.t()), dict(a=b, b=a)]
    grp = align.SmallMatmulGroup()
    outs = [grp.add(**sp) for sp in specs]
    acc_out = base.clone()
    grp.add(a3, b3, out=acc_out, accumulate=True)
    grp.launch()
    for k, (sp, got) in enumerate(zip(specs, outs)):
        assert torch.equal(got, align.small_matmul(**sp)), k
    assert torch.equal(acc_out, out)
    grp.launch()                                                       # an empty group is a no-op


# ------------------------------------------------------------------------------------------------ fused Linear + element-wise pass (round 6)
def _leaky(v, slope=0.01):
    return torch.where(v > 0, v, v * slope)


@pytest.mark.parametrize("rows,nb,rs,om,oy,with_res,keep", [
    (41, 1, 0, 1, 0, False, None),         # plain layer, ragged last tile
    (96, 2, 0, 2, 1, True, None),          # (no | has) bottlenecks + skip connection: out [m,2,H], residual = the input row
    (130, 2, 1, 4, 2, True, None),         # (left | right) bottlenecks on rows (m,val): out [m,dir,val,H]
    (4096 + 64 + 7, 1, 0, 1, 0, False, "mask"),
    (1000, 1, 0, 1, 0, False, "rng"),
    (1, 1, 0, 1, 0, False, None),
])
def test_ff_linear_act_forward(rows, nb, rs, om, oy, with_res, keep):
    """vlg_ff_linear_act (row-streaming Linear fused with bias, skip connection, LeakyReLU, dropout and the store permutation) against the pair
    it replaces -- library GEMM with a bf16 result, then vlg_ff_act -- computed in float64 on the same bf16 inputs: equal up to the product's
    summation order (one bf16 rounding of the Linear's output, one of the result)."""
    from vlgae_amd import _C, encoders
    from vlgae_amd import parser_ff
    H = 256
    g = torch.Generator().manual_seed(rows * 7 + nb)
    bf = torch.bfloat16
    x = (torch.randn(rows, H, generator=g) * 0.5).to(dev(), bf)
    w = (torch.randn(nb * H, H, generator=g) / 16).to(dev(), bf)
    bias = (torch.randn(nb * H, generator=g) * 0.2).to(dev(), bf)
    res = (torch.randn(rows >> rs, H, generator=g) * 0.5).to(dev(), bf) if with_res else None
    if with_res and rs == 0:
        res = x
    n_out = (rows >> rs) * om if nb == 2 else rows
    out = torch.full((n_out, H), float("nan"), dtype=bf, device=dev())
    mask, rng, p, scale = None, None, 0.0, 1.0
    if keep == "mask":
        mask = (torch.rand(n_out, H, generator=g) > 0.3).to(dev(), bf)
        scale = 1.0 / 0.7
    elif keep == "rng":
        rng, p = encoders.DeviceRng(123, dev()), 0.3
    parser_ff._linear_act(x, w, bias, out, nb=nb, residual=res, rs=rs, om=om, oy=oy, mask=mask, mask_scale=scale, rng=rng, p=p)
    lin = (x.double() @ w.double().t() + bias.double()).to(bf).double()                 # the library GEMM's bf16 output
    rowi = torch.arange(rows, device=dev())
    ref = torch.empty(n_out, H, dtype=torch.float64, device=dev())
    for y in range(nb):
        v = lin[:, y * H:(y + 1) * H]
        if res is not None:
            v = v + res.double()[rowi >> rs]
        orow = (rowi >> rs) * om + y * oy + (rowi & ((1 << rs) - 1))
        ref[orow] = _leaky(v)
    if keep == "mask":
        ref = ref * mask.double() * scale
    if keep == "rng":   # the kernel's own draw, as vlg_ff_act makes it over the same element indices
        ones = torch.ones(n_out, H, dtype=bf, device=dev())
        drawn = parser_ff._act(ones, torch.empty_like(ones), n_out, 1, H, rng=rng, p=p)
        assert 0.6 < float((drawn > 0).float().mean()) < 0.8
        ref = ref * drawn.double()
    assert not torch.isnan(out.float()).any()
    err = (out.double() - ref).abs()
    # one bf16 ulp where the two summation orders round the Linear's output differently (then LeakyReLU' <= 1 and one more rounding)
    assert float((err / ref.abs().clamp_min(1.0)).max()) <= 2.0 ** -6 and float(err.mean()) <= 2e-3
    assert float((err > 2.0 ** -7 * ref.abs().clamp_min(0.5)).float().mean()) <= 0.02       # (beyond the result's own bf16 rounding: rare)
    out2 = torch.empty_like(out)
    parser_ff._linear_act(x, w, bias, out2, nb=nb, residual=res, rs=rs, om=om, oy=oy, mask=mask, mask_scale=scale, rng=rng, p=p)
    assert torch.equal(out, out2)


@pytest.mark.parametrize("rows,J,swap,acc,keep", [(4 * 35, 4, True, False, None), (2 * 77, 2, False, True, None), (333, 1, False, False, "mask"),
                                                  (4096 + 8, 1, False, False, "rng"), (4, 4, True, False, None)])
def test_ff_linear_act_backward(rows, J, swap, acc, keep):
    """vlg_ff_linear_act_backward against library GEMM (bf16 result) + vlg_ff_act_backward in float64 on the same bf16 inputs."""
    from vlgae_amd import encoders, parser_ff
    H = 256
    g = torch.Generator().manual_seed(rows + J)
    bf = torch.bfloat16
    gin = torch.randn(rows, H, generator=g).to(dev(), bf)
    W = (torch.randn(H, H, generator=g) / 16).to(dev(), bf)                              # the layer's weight [out, in]: d x = g @ W
    act = torch.randn(rows, H, generator=g).to(dev(), bf)
    wT = torch.empty(1, H, H, dtype=bf, device=dev())
    parser_ff._transpose256([W], wT)
    assert torch.equal(wT[0], W.t().contiguous())
    mask, rng, p, scale = None, None, 0.0, 1.0
    if keep == "mask":
        mask, scale = (torch.rand(rows, H, generator=g) > 0.3).to(dev(), bf), 1.0 / 0.7
    elif keep == "rng":
        rng, p = encoders.DeviceRng(5, dev()), 0.3
    total0 = torch.randn(rows // J, H, generator=g).to(dev()) if acc else None
    total = total0.clone() if acc else torch.full((rows // J, H), float("nan"), device=dev())
    out = torch.full((rows, H), float("nan"), dtype=bf, device=dev())
    parser_ff._linear_act_bwd(gin, wT[0], act, out, J=J, mask=mask, mask_scale=scale, rng=rng, p=p, total=total, accumulate=acc, swap=swap)
    lin = (gin.double() @ W.double()).to(bf)                                             # the library product's bf16 output
    want_out, want_total = torch.empty_like(out), (total0.clone() if acc else torch.empty_like(total))
    parser_ff._act_bwd(lin, act, want_out, rows // J, J, H, mask=mask, total=want_total, accumulate=acc, swap=swap, mask_scale=scale, rng=rng, p=p)
    err = (out.double() - want_out.double()).abs()
    assert float((err / want_out.double().abs().clamp_min(1.0)).max()) <= 2.0 ** -6 and float(err.mean()) <= 2e-3
    assert float((err > 2.0 ** -7 * want_out.double().abs().clamp_min(0.5)).float().mean()) <= 0.02
    assert float((total - want_total).abs().max()) <= 0.05 * J and float((total - want_total).abs().mean()) <= 4e-3
    # the group sums are sums of the STORED values (what the next product reads)
    o = out.float().view(rows // J, J, H)
    if swap:
        o = o   # (the permutation moves rows inside a group: the sum is the same)
    assert float((total - ((total0 if acc else 0) + o.sum(1))).abs().max()) <= 1e-5 * max(1.0, float(total.abs().max()))


@pytest.mark.parametrize("rows,k", [(333, 512), (4096 + 40, 512), (32 * 300, 32), (77, 32), (1, 512)])
def test_ff_linear_act_backward_other_contractions(rows, k):
    """vlg_ff_linear_act_backward at k = 512 (the cotangent of a two-block stage, the weight as two transposed [256,256] blocks) and k = 32 (the
    folded projections' cotangent, the weight rows as they lie) against the library product (bf16 result) + vlg_ff_act_backward."""
    from vlgae_amd import parser_ff
    H = 256
    g = torch.Generator().manual_seed(rows + k)
    bf = torch.bfloat16
    gin = torch.randn(rows, k, generator=g).to(dev(), bf)
    W = (torch.randn(k, H, generator=g) / k ** 0.5).to(dev(), bf)                         # d x = g @ W, W [k, 256]
    act = torch.randn(rows, H, generator=g).to(dev(), bf)
    out = torch.full((rows, H), float("nan"), dtype=bf, device=dev())
    if k == 512:
        wT = parser_ff._transpose256([W[:H].contiguous(), W[H:].contiguous()], torch.empty(2, H, H, dtype=bf, device=dev()))
        assert torch.equal(wT[1], W[H:].t().contiguous())
        parser_ff._linear_act_bwd(gin, wT, act, out)
    else:
        parser_ff._linear_act_bwd(gin, W, act, out, w_kn=True)
    lin = (gin.double() @ W.double()).to(bf)
    want = torch.empty_like(out)
    parser_ff._act_bwd(lin, act, want, rows, 1, H)
    err = (out.double() - want.double()).abs()
    assert not torch.isnan(out.float()).any()
    assert float((err / want.double().abs().clamp_min(1.0)).max()) <= 2.0 ** -6 and float(err.mean()) <= 2e-3
    assert float((err > 2.0 ** -7 * want.double().abs().clamp_min(0.5)).float().mean()) <= 0.02
    from vlgae_amd import _C
    with pytest.raises(RuntimeError):      # the [k][256] layout belongs to k = 32, the blocked one to the others
        parser_ff._linear_act_bwd(gin, W, act, out, w_kn=(k != 32))
    if k == 512:
        with pytest.raises(RuntimeError):  # a plain layer's adjoint only
            parser_ff._linear_act_bwd(gin, wT, act, out, total=torch.zeros(rows, H, device=dev()))


@pytest.mark.parametrize("rows,k", [(77, 32), (333, 512)])
def test_ff_linear_act_backward_generic_images(rows, k):
    """Option words outside the compiled set take the generic image of their contraction length (options read at run time): k = 32 with a
    dropout mask, k = 512 with the accumulate flag (which has nothing to act on without group sums).  Same reference and bounds as the
    compiled images above."""
    from vlgae_amd import parser_ff
    H = 256
    g = torch.Generator().manual_seed(rows + k)
    bf = torch.bfloat16
    gin = torch.randn(rows, k, generator=g).to(dev(), bf)
    W = (torch.randn(k, H, generator=g) / k ** 0.5).to(dev(), bf)
    act = torch.randn(rows, H, generator=g).to(dev(), bf)
    out = torch.full((rows, H), float("nan"), dtype=bf, device=dev())
    mask, scale = None, 1.0
    if k == 512:
        wT = parser_ff._transpose256([W[:H].contiguous(), W[H:].contiguous()], torch.empty(2, H, H, dtype=bf, device=dev()))
        parser_ff._linear_act_bwd(gin, wT, act, out, accumulate=True)
    else:
        mask, scale = (torch.rand(rows, H, generator=g) > 0.3).to(dev(), bf), 1.0 / 0.7
        parser_ff._linear_act_bwd(gin, W, act, out, w_kn=True, mask=mask, mask_scale=scale)
    lin = (gin.double() @ W.double()).to(bf)
    want = torch.empty_like(out)
    parser_ff._act_bwd(lin, act, want, rows, 1, H, mask=mask, mask_scale=scale)
    err = (out.double() - want.double()).abs()
    assert not torch.isnan(out.float()).any()
    assert float((err / want.double().abs().clamp_min(1.0)).max()) <= 2.0 ** -6 and float(err.mean()) <= 2e-3
    assert float((err > 2.0 ** -7 * want.double().abs().clamp_min(0.5)).float().mean()) <= 0.02


@pytest.mark.parametrize("rows,n,ldw,ldo", [(2048, 800, 864, 800), (10240, 800, 800, 800), (2055, 256, 256, 320), (4100, 40, 48, 40), (3000, 1032, 1032, 1036)])
def test_ff_linear_kn(rows, n, ldw, ldo):
    """vlg_ff_linear_kn (a 256-output Linear's input gradient g @ weight as one row-streaming launch, the weight read where it lies) against
    the float64 product of the same bf16 operands; column slices of wider weights, padded outputs, ragged last column block and row tile."""
    from vlgae_amd import align
    g = torch.Generator().manual_seed(rows + n)
    bf = torch.bfloat16
    x = torch.randn(rows, 256, generator=g).to(dev(), bf)
    wide = (torch.randn(256, ldw, generator=g) / 16).to(dev(), bf)
    w = wide[:, ldw - n:]                                                                # a column slice (2-byte aligned only)
    out_wide = torch.full((rows, ldo), float("nan"), dtype=bf, device=dev())
    out = out_wide[:, :n]
    assert align.linear_kn_ok(x, w)
    align.linear_kn(x, w, out=out)
    want = x.double() @ w.double()
    assert not torch.isnan(out.float()).any()
    err = (out.double() - want).abs()
    assert float((err / want.abs().clamp_min(1.0)).max()) <= 2.0 ** -7, float((err / want.abs().clamp_min(1.0)).max())
    if ldo > n:
        assert bool(torch.isnan(out_wide[:, n:].float()).all())                            # nothing written past the valid columns
    assert torch.equal(out, align.linear_kn(x, w))                                        # reproducible
    # with the counter-based draw in the epilogue: the same bits as the product followed by encoders.dropout at the same (state, site, p)
    from vlgae_amd import encoders
    rng = encoders.DeviceRng(11, dev())
    drawn = align.linear_kn(x, w, rng=rng, site=encoders.SITE_TEXT_ENCODER, p=0.33)
    ref = encoders.dropout(align.linear_kn(x, w), 0.33, rng=rng, site=encoders.SITE_TEXT_ENCODER)
    assert 0.6 < float((drawn != 0).float().mean()) < 0.75
    assert torch.equal(drawn, ref)
    # through autograd: the input gradient of align.linear with 256 outputs is this launch
    xin = torch.randn(rows, n, generator=g).to(dev(), bf).requires_grad_(True)
    weight = w.detach().contiguous().requires_grad_(True)                                # [256, n]
    y = align.linear(xin, weight)
    cot = x
    gx, gw = torch.autograd.grad(y, [xin, weight], cot)
    assert torch.equal(gx, align.linear_kn(cot, weight.detach()))
    assert float((gw.double() - cot.double().t() @ xin.detach().double()).abs().max()) <= 2e-2 * float(gw.abs().max())


@pytest.mark.parametrize("rows,keep", [(4 * 300, "rng"), (4 * 9, "mask"), (4 * 1031, None)])
def test_ff_linear_act_chain2_equals_two_launches(rows, keep):
    """vlg_ff_linear_act_chain2 (two consecutive 256 -> 256 stages in one launch, the second on the first's rows through LDS) gives the bits of the
    two single launches, forward (a plain layer with dropout, then a plain layer) and backward (a plain layer's adjoint with the regenerated
    mask, then an adjoint with the (dir,val) permutation and the group sums)."""
    from vlgae_amd import encoders, parser_ff
    H = 256
    g = torch.Generator().manual_seed(rows)
    bf = torch.bfloat16
    x = torch.randn(rows, H, generator=g).to(dev(), bf)
    W1, W2 = ((torch.randn(H, H, generator=g) / 16).to(dev(), bf) for _ in range(2))
    b1, b2 = ((torch.randn(H, generator=g) / 4).to(dev(), bf) for _ in range(2))
    act1, act2 = (torch.randn(rows, H, generator=g).to(dev(), bf) for _ in range(2))
    mask, rng, p, scale = None, None, 0.0, 1.0
    if keep == "mask":
        mask, scale = (torch.rand(rows, H, generator=g) > 0.3).to(dev(), bf), 1.0 / 0.7
    elif keep == "rng":
        rng, p = encoders.DeviceRng(5, dev()), 0.3
    new = lambda *sh, dt=bf: torch.full(sh, float("nan"), dtype=dt, device=dev())
    # forward
    o1, o2, c1, c2 = new(rows, H), new(rows, H), new(rows, H), new(rows, H)
    parser_ff._linear_act(x, W1, b1, o1, mask=mask, mask_scale=scale, rng=rng, p=p)
    parser_ff._linear_act(o1, W2, b2, o2)
    parser_ff._linear_act_chain2(x, parser_ff._stage(W1, c1, bias=b1, mask=mask, mask_scale=scale, rng=rng, p=p), parser_ff._stage(W2, c2, bias=b2))
    assert not torch.isnan(c2.float()).any()
    assert torch.equal(o1, c1) and torch.equal(o2, c2)
    # backward
    wT = parser_ff._transpose256([W1, W2], torch.empty(2, H, H, dtype=bf, device=dev()))
    o1, o2, c1, c2 = new(rows, H), new(rows, H), new(rows, H), new(rows, H)
    t1, t2 = new(rows // 4, H, dt=torch.float32), new(rows // 4, H, dt=torch.float32)
    parser_ff._linear_act_bwd(x, wT[0], act1, o1, mask=mask, mask_scale=scale, rng=rng, p=p)
    parser_ff._linear_act_bwd(o1, wT[1], act2, o2, J=4, total=t1, swap=True)
    parser_ff._linear_act_chain2(x, parser_ff._stage(wT[0], c1, act=act1, mask=mask, mask_scale=scale, rng=rng, p=p),
                                 parser_ff._stage(wT[1], c2, act=act2, J=4, total=t2, swap=True), backward=True)
    assert not torch.isnan(c2.float()).any() and not torch.isnan(t2).any()
    assert torch.equal(o1, c1) and torch.equal(o2, c2) and torch.equal(t1, t2)
    from vlgae_amd import _C
    with pytest.raises(RuntimeError):       # the first stage keeps its rows
        parser_ff._linear_act_chain2(x, parser_ff._stage(wT[0], c1, act=act1, J=4, swap=True), parser_ff._stage(wT[1], c2, act=act2), backward=True)


def test_mlp_encoder_fused_adjoint_equals_unfused(monkeypatch):
    """encoders.mlp_encoder with the counter-based draw at a row count that takes the fused adjoint (_DropoutLinear: (g @ W) * keep in one launch)
    against the same call on the dropout + linear Functions: identical output, identical d_emb bits, d_W equal (same split-K product)."""
    from vlgae_amd import align, encoders
    B, L, E, h, p = 64, 40, 800, 256, 0.33
    g = torch.Generator().manual_seed(9)
    bf = torch.bfloat16
    emb = (torch.randn(B, L, E, generator=g) * 0.5).to(dev(), bf).requires_grad_(True)
    W = (torch.randn(h, E, generator=g) * E ** -0.5).to(dev(), bf).requires_grad_(True)
    cot = torch.randn(B, L, h, generator=g).to(dev(), bf)
    runs = []
    for library in (False, True):
        monkeypatch.setattr(align, "_KN_LIBRARY", library)
        rng = encoders.DeviceRng(77, dev())
        x = encoders.mlp_encoder(emb, W, p, rng=rng)
        assert (type(x.grad_fn).__name__.startswith("_DropoutLinear")) == (not library)
        runs.append((x.detach(), *torch.autograd.grad(x, [emb, W], cot)))
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][2], runs[1][2])
    # d_emb: the fused launch rounds the product to bf16 once and multiplies by the keep value; the unfused path does the same in two launches
    a, b = runs[0][1].double(), runs[1][1].double()
    assert torch.equal(a == 0, b == 0)
    assert float((a - b).abs().max()) <= 2.0 ** -7 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("B,L,Ms,masks", [(7, 13, 14, True), (3, 40, 5, False), (64, 40, 35, True)])
def test_ff_linear_mlp_act_backward(B, L, Ms, masks):
    """vlg_ff_linear_mlp_act_backward (the head of the skip-connect encoder's adjoint in one launch) against the library product (bf16 result) +
    vlg_ff_mlp_act_backward on the same inputs."""
    from vlgae_amd import _C, parser_ff
    H, M0 = 256, B * L
    M = M0 + Ms
    g = torch.Generator().manual_seed(B + L)
    bf = torch.bfloat16
    gY = torch.randn(M, 2 * H, generator=g).to(dev(), bf)
    W = (torch.randn(2 * H, H, generator=g) / 22).to(dev(), bf)
    X = torch.randn(M, H, generator=g).to(dev(), bf)
    gX = torch.randn(M, H, generator=g).to(dev())
    dh = ((torch.rand(B, H, generator=g) > 0.33).float() / 0.67).to(dev()) if masks else None
    ds = ((torch.rand(Ms, generator=g) > 0.33).float() / 0.67).to(dev()) if masks else None
    wT = parser_ff._transpose256([W[:H].contiguous(), W[H:].contiguous()], torch.empty(2, H, H, dtype=bf, device=dev()))
    out = torch.full((M, H), float("nan"), dtype=bf, device=dev())
    _C.check(_C.lib().vlg_ff_linear_mlp_act_backward(_C.ptr(gY), gY.stride(0), _C.ptr(wT), M, _C.ptr(gX), _C.ptr(X), _C.ptr(dh), _C.ptr(ds), M0, L,
                                                     _C.ptr(out), parser_ff.SLOPE, _C.stream_of(out)), "ff_linear_mlp_act_backward")
    gT = (gY.double() @ W.double()).to(bf)
    want = torch.empty_like(out)
    _C.check(_C.lib().vlg_ff_mlp_act_backward(_C.ptr(gX), _C.ptr(gT), _C.ptr(X), _C.ptr(dh), _C.ptr(ds), _C.ptr(want), B, L, Ms, H, _C.BF16,
                                              parser_ff.SLOPE, _C.stream_of(want)), "ff_mlp_act_backward")
    assert not torch.isnan(out.float()).any()
    err = (out.double() - want.double()).abs()
    assert float((err / want.double().abs().clamp_min(1.0)).max()) <= 2.0 ** -6 and float(err.mean()) <= 3e-3
    assert float((err > 2.0 ** -7 * want.double().abs().clamp_min(0.5)).float().mean()) <= 0.02
    if masks:      # masked rows / channels are exact zeros
        assert float(out[:M0].view(B, L, H)[(dh == 0).unsqueeze(1).expand(B, L, H)].abs().max()) == 0.0


def test_parser_feed_forward_fused_layers_equal_library_path(monkeypatch):
    """parser_feed_forward at the shipped width (H = 256, bf16) with its skip-connect encoder as fused row-streaming launches against the same call with
    library GEMMs + element-wise passes (VLGAE_FF_LIBRARY): outputs and every gradient agree to bf16 rounding; the fused path is what runs by default."""
    from vlgae_amd import parser_ff, train_step
    B, L, E, h, Et, T, H, r, nb = 9, 13, 104, 64, 16, 11, 256, 16, 40
    gen = torch.Generator().manual_seed(4)
    bf = torch.bfloat16
    P = train_step.init_feed_forward(gen, dev(), bf, E, h, Et, T, H, nb, r)
    emb = (torch.randn(B, L, E, generator=gen) * 0.5).to(dev(), bf).requires_grad_(True)
    x = torch.randn(B, L, h, generator=gen).to(dev(), bf).requires_grad_(True)
    names = sorted(P)
    leaves = [emb, x] + [P[k] for k in names]
    dgen = torch.Generator(device=dev()).manual_seed(11)
    masks = parser_ff.dropout_masks(B, L, T, H, 0.33, 0.3, device=dev(), dtype=torch.float32, generator=dgen)
    assert parser_ff._fused(bf, H)
    runs = []
    for library in (False, True):
        monkeypatch.setattr(parser_ff, "_FF_LIBRARY", library)
        outs = parser_ff.parser_feed_forward(P, emb, x, None, None, None, *masks)
        cot = [torch.randn(o.shape, generator=torch.Generator().manual_seed(3)).to(dev()) for o in outs]
        runs.append(([o.detach().float() for o in outs], [g_.float() for g_ in torch.autograd.grad([o.float() for o in outs], leaves, cot)]))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert float((a - b).abs().max()) <= 3e-2 * max(1.0, float(b.abs().max()))
    gmax = max(float(w.abs().max()) for w in runs[1][1])
    for name, a, b in zip(["emb", "x"] + names, runs[0][1], runs[1][1]):
        # (both paths in bf16: a pre-activation within rounding of zero may take different LeakyReLU branches -- relative L2, as the float64 comparison above)
        assert float((a - b).norm()) <= 0.1 * float(b.norm()) + 2e-3 * gmax * b.numel() ** 0.5, name
