"""GPU: the evaluation step (vlgae_amd/eval_step.py), its metric kernels (vlg_eval_metrics) and the MBR decode entry
(vlg_deptree_mbr_decode) against
  (1) fixtures the reference's own methods and metric classes produced (tests/golden/evalmetric_*, evalstep_*: make_golden_eval.py),
  (2) the numpy restatement of the counters (tests/eval_restatement.py, pinned on those fixtures by test_eval_metrics.py) on inputs no
      fixture covers (B = 256, sentences shorter than the prediction count, empty masks, no gold alignment),
  (3) the training step's forward (same parameters, dropout off: bit-equal) and its own eager run (one HIP graph, replayed)."""
import json

import numpy as np
import pytest
import torch

from conftest import golden_files, golden_ids, load
from eval_restatement import COUNTS, eval_counts
from test_eval_metrics import batch_of
from test_gpu_parity import dev, trainstep_from_fixture

pytestmark = pytest.mark.gpu

SMALL = dict(E=96, H=64, nb=24, n_vis=256)        # widths of the frozen features / the parser's feed-forwards (as the training step's graph test)
LAYOUTS = {"obj": (), "shipped": ("rel", "attr", "img")}


def tt(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return x if dtype is None else x.to(dtype)


def counts_of(counters):
    c = counters.counts()
    return {k: c[k] for k in COUNTS}


def random_gold(rng, B, L, R, lengths, short=True):
    """A synthetic gold side: arcs, a punctuation mask with holes (sentences with fewer scored tokens than predictions, empty masks),
    region boxes, scene-graph boxes near proposals, sentences without any gold alignment."""
    wmask = np.arange(L)[None] < lengths[:, None]
    mask = wmask & (rng.random((B, L)) > 0.15)
    if short:
        mask[1] = False                                  # an empty mask
        mask[2, 3:] = False                              # m <= 3 < K
        mask[3] = False
        mask[3, 0] = True                                # m = 1
    arc = rng.integers(0, L + 1, size=(B, L)) * wmask
    xy, wh = rng.uniform(0, 0.6, size=(B, R, 2)), rng.uniform(0.2, 0.4, size=(B, R, 2))
    vis_box = np.concatenate([xy, xy + wh], -1).astype(np.float32)
    pick = rng.integers(0, R, size=(B, L, 2))
    sg_box = (vis_box[np.arange(B)[:, None, None], pick] + rng.uniform(-0.03, 0.03, size=(B, L, 2, 4))).astype(np.float32).reshape(B, L, 8)
    sg_type = rng.integers(0, 4, size=(B, L)) * wmask
    sg_type[4] = 0                                       # a sentence with no gold alignment at all
    return dict(arc=arc.astype(np.int64), mask=mask, vis_box=vis_box, sg_box=sg_box, sg_type=sg_type.astype(np.int64), sg_mask=sg_type != 0)


# ------------------------------------------------------------------------------------------------ the metric kernels
@pytest.mark.parametrize("path", golden_files("evalmetric_"), ids=golden_ids("evalmetric_"))
def test_eval_metrics_kernel_reproduces_the_reference_counters(path):
    """Every counter equals the reference's metric state after each of the two consecutive batches, and compute() its dict."""
    from vlgae_amd import metrics
    z = np.load(path)
    ec = metrics.EvalCounters(dev())
    for i in range(2):
        kw = batch_of(z, i)
        box = {k: tt(kw[k]) for k in ("vis_box", "sg_box", "sg_type", "sg_mask") if k in kw}
        ec.update(tt(kw["pred"]), tt(kw["gold"]), tt(kw["mask"]), tt(kw["lengths"]), tt(kw["factor2img"]), tt(kw["top5"]),
                  loss=tt(z[f"loss_{i}"]).reshape(()), factors=kw["factors"], **box)
        got = counts_of(ec)
        assert [got[k] for k in COUNTS] == z[f"counters_{i}"].tolist(), (i, got)
    assert ec.counts()["n_batches"] == 2
    want = json.loads(str(z["compute"]))
    got = ec.compute()
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-6, abs=1e-30), k
    assert got["loss"] == want["loss"]                   # float64 adds of the float32 losses in batch order: the same bits
    ec.reset()
    assert all(v == 0 for v in ec.counts().values())


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_eval_metrics_kernel_equals_the_restatement_at_config_size(layout):
    """B = 256, L = 40, R = 36 on random inputs through the C entry itself: against the numpy restatement, including sentences with fewer
    scored tokens than predictions, empty masks and sentences without gold; counters and workspace poisoned first; without the box
    arguments the box counters stay untouched; two runs bit-identical."""
    from vlgae_amd import _C
    B, L, R = 256, 40, 36
    factors = LAYOUTS[layout]
    V = R + ("rel" in factors) * R * R + ("attr" in factors) * R + ("img" in factors)
    Q = 2 * (L + 1)
    rng = np.random.default_rng(3)
    lengths = rng.integers(1, L + 1, size=B)
    lengths[0] = L
    gold = random_gold(rng, B, L, R, lengths)
    pred = np.where(rng.random((B, L)) < 0.5, gold["arc"], rng.integers(0, L + 1, size=(B, L))).astype(np.int64)
    top5 = rng.integers(0, V, size=(B, Q, 5)).astype(np.int32)
    top5[:, 1:L + 1, 0] = np.where(rng.random((B, L)) < 0.5, rng.integers(0, R, size=(B, L)), top5[:, 1:L + 1, 0])
    f2i = np.where(rng.random((B, Q)) < 0.5, np.arange(B)[:, None], rng.integers(0, B, size=(B, Q))).astype(np.int32)
    heads = np.concatenate([np.zeros((B, 1), np.int64), pred], 1)      # the decoder's [B, L + 1] layout: pred is its view [:, 1:]
    d = {k: tt(v) for k, v in dict(gold, heads=heads, top5=top5, f2i=f2i, lengths=lengths.astype(np.int64)).items()}
    lib = _C.lib()
    nbytes = lib.vlg_eval_metrics_workspace(B)
    loss = torch.tensor(1.25, device=dev())

    def run(with_box, with_mask=True):
        counters = torch.full((16,), 1000, dtype=torch.int64, device=dev())
        counters[15:].view(torch.float64)[0] = 0.5
        ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=dev())
        pr = d["heads"][:, 1:]
        box = [d["vis_box"], d["sg_box"], d["sg_type"], d["sg_mask"].view(torch.uint8)] if with_box else [None] * 4
        _C.check(lib.vlg_eval_metrics(_C.ptr(pr), pr.stride(0), _C.ptr(d["arc"]), _C.ptr(d["mask"].view(torch.uint8)) if with_mask else None, _C.ptr(d["lengths"]), _C.ptr(d["f2i"]),
                                      _C.ptr(d["top5"]), *[_C.ptr(t) for t in box], _C.ptr(loss), B, L, Q, R, int("rel" in factors),
                                      int("attr" in factors), int("img" in factors), _C.ptr(ws), nbytes, _C.ptr(counters), _C.stream_of(counters)),
                 "eval_metrics")
        torch.cuda.synchronize()
        return counters.cpu()

    got = run(True)
    want = eval_counts(pred, gold["arc"], gold["mask"], lengths, f2i, top5, gold["vis_box"], gold["sg_box"], gold["sg_type"], gold["sg_mask"], factors)
    assert [int(v) - 1000 for v in got[:14]] == [want[k] for k in COUNTS], (dict(zip(COUNTS, (got[:14] - 1000).tolist())), want)
    assert int(got[14]) == 1001 and got[15:].view(torch.float64).item() == 1.75
    assert min(want[k] for k in ("correct_obj", "correct_rel" if "rel" in factors else "correct_obj", "n_ucm", "f2i_correct")) > 0
    assert torch.equal(run(True), got)
    # no mask given = vp.mask, the length mask, derived in the kernel
    wmask = np.arange(L)[None] < lengths[:, None]
    want = eval_counts(pred, gold["arc"], wmask, lengths, f2i, top5, gold["vis_box"], gold["sg_box"], gold["sg_type"], gold["sg_mask"], factors)
    assert [int(v) - 1000 for v in run(True, with_mask=False)[:14]] == [want[k] for k in COUNTS]
    nobox = run(False)
    assert torch.equal(nobox[:6], got[:6]) and [int(v) for v in nobox[6:14]] == [1000] * 8


# ------------------------------------------------------------------------------------------------ the MBR decode
MBR_N = [2, 10, 41, 81, 107, 127, 255]            # the short image, all in LDS, and the Max walk's workspace placements (106/107, 126/127)


def mbr_inputs(N):
    B = 9
    g = torch.Generator().manual_seed(N)
    marg = (torch.rand(B, N, N, 2, generator=g) * torch.rand(B, N, N, 1, generator=g)).to(dev())
    lengths = torch.randint(1, N, (B,), generator=g)
    lengths[0] = N - 1
    return marg, lengths.to(dev())


@pytest.mark.parametrize("N", MBR_N)
def test_mbr_decode_equals_deptree_decode_of_the_valence_sum(N):
    """vlg_deptree_mbr_decode on [B,N,N,2] float32 marginals = deptree_decode(marginals.sum(-1)) bit for bit (heads and score), ragged lengths."""
    from vlgae_amd.torch_struct import functional as tsf
    marg, lengths = mbr_inputs(N)
    best, heads = tsf.deptree_mbr_decode(marg, lengths)
    want_best, want_heads = tsf.deptree_decode(marg.sum(-1), lengths)
    assert torch.equal(heads, want_heads) and torch.equal(best, want_best)
    assert int((heads[0, 1:] > 0).sum()) >= N - 2          # a tree: one root child, every other word has a head
    with pytest.raises(ValueError, match="float32"):
        tsf.deptree_mbr_decode(marg.bfloat16(), lengths)


@pytest.mark.parametrize("N", MBR_N)
def test_mbr_decode_is_the_best_tree_of_the_fp64_oracle(oracle_mod, N):
    """The check above compares two launches of one kernel family; this one does not: the heads are a projective single-root tree per
    sentence, nothing outside it, and the tree's score -- the float32 valence sums added up in float64 -- is within 1e-5 relative of the
    fp64 oracle's Max-semiring value on those sums, as is the score the launch returns."""
    from vlgae_amd.torch_struct import functional as tsf
    marg, lengths = mbr_inputs(N)
    best, heads = tsf.deptree_mbr_decode(marg, lengths)
    arc = marg.sum(-1).cpu().numpy()                       # a two-term float32 sum has one order: the values the load stage forms
    ln, h, got = lengths.cpu().numpy(), heads.cpu().numpy(), best.cpu().numpy()
    want = oracle_mod.deptree(arc, ln, "max", np.float64, grad=False)[0]
    for b, n in enumerate(ln):
        assert oracle_mod.is_projective_tree(h[b], int(n)), b
        assert h[b, 0] == 0 and not h[b, n + 1:].any(), b
        score = float(sum(np.float64(arc[b, h[b, c], c]) for c in range(1, n + 1)))
        assert abs(score - want[b]) <= 1e-5 * max(1.0, abs(want[b])), (b, score, want[b])
        assert abs(float(got[b]) - want[b]) <= 1e-5 * max(1.0, abs(want[b])), (b, got[b], want[b])


# ------------------------------------------------------------------------------------------------ the step on reference-made fixtures
def eval_from_fixture(path, dtype=torch.float32, **kw):
    """eval_step.build on the parameters of a training step built from the paired trainstep_* fixture (given=train.P: in place), with the
    evalstep_* fixture's gold side."""
    from vlgae_amd import eval_step
    z = load(path)
    g = load(path.replace("evalstep_", "trainstep_"))
    train, _ = trainstep_from_fixture(g, dtype)
    sh = train.shape
    gold = dict(arc=tt(z["gold_arc"]), mask=tt(z["mask"]))
    if bool(z["with_sg"]):
        gold.update({k: tt(z[k]) for k in ("vis_box", "sg_box", "sg_type", "sg_mask")})
    b = train.batch
    step = eval_step.build(sh["B"], sh["L"], sh["R"], dev(), dtype=dtype, d=sh["d"], h=sh["h"], E=sh["E"], n_vis=sh["n_vis"], factors=b["factors"],
                           pos_for=b["pos_for"], ln_eps=float(g["ln_eps"]), use_pos_prior=bool(z["use_pos_prior"]), use_heuristic=bool(z["use_heuristic"]),
                           given=dict(train.P, lengths=train.lengths, token=b["token"], tag=b["tag"], box_mask=b["box_mask"], **gold), **kw)
    return step, train, z, g


@pytest.mark.parametrize("path", golden_files("evalstep_"), ids=golden_ids("evalstep_"))
def test_eval_step_reference_fixture(path):
    """float32 against the reference's eval-mode step (make_golden_eval.step_cases): potentials within the training step's fixture
    tolerance (2e-5 * max(1, max|.|)), Viterbi and MBR heads, top-5 columns and factor -> image exact, loss to 1e-5 relative, counters
    exact after one and two steps, compute() to float32 rounding.  Top-5 ranks whose value is a dead fill (-1e10: the prior absorbs the
    logit, equal values have no defined order in torch.argsort) are compared by value."""
    step, train, z, g = eval_from_fixture(path)
    out = step()
    last = step.last
    npf = lambda x: x.detach().float().cpu().numpy()
    for name in ("merged_attach", "merged_dec"):
        got, want = npf(last[name]), z[name]
        fin = want > -1e11
        assert np.abs(got[fin] - want[fin]).max() <= 2e-5 * max(1.0, np.abs(want[fin]).max()), name
        assert np.array_equal(got[~fin], want[~fin]), name
    assert np.array_equal(out["arc"].cpu().numpy(), z["arc_viterbi"])
    assert abs(float(out["loss"]) - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    rows = z["txt_mask"]
    assert np.array_equal(last["txt_mask"].cpu().numpy(), rows)
    top5, logit = out["top5"].cpu().numpy(), npf(out["logit"])
    want_vals = np.take_along_axis(z["logit"], z["top5"].astype(np.int64), -1)
    got_vals = np.take_along_axis(logit, top5.astype(np.int64), -1)
    live = want_vals > -1e5
    assert np.array_equal(top5[rows][live[rows]], z["top5"][rows][live[rows]])
    assert np.array_equal(got_vals[rows][~live[rows]], want_vals[rows][~live[rows]])            # dead fills: equal values, bit for bit
    assert np.abs(got_vals[rows][live[rows]] - want_vals[rows][live[rows]]).max() <= 1e-4 * max(1.0, np.abs(want_vals[rows][live[rows]]).max())
    assert np.array_equal(out["factor2img"].cpu().numpy()[rows], z["factor2img"][rows])
    assert [counts_of(step.counters)[k] for k in COUNTS] == z["counters_0"].tolist()
    step()
    assert [counts_of(step.counters)[k] for k in COUNTS] == z["counters_1"].tolist()
    want = json.loads(str(z["compute"]))
    got = step.counters.compute()
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-5 if k == "loss" else 1e-6, abs=1e-30), k
    # the lists write_prediction takes: one host read
    pred = step.predictions()
    assert pred["arc"] == z["arc_viterbi"].tolist()
    assert [[int(v) for v in row] for row in pred["txt_to_img"]] == json.loads(str(z["txt_to_img"]))
    assert [len(s) for s in pred["txt_to_factor"]] == [int(r.sum()) for r in rows]
    # MBR decoding (ldndmv.py:294-299) on the same parameters: the heads change, nothing else does
    mbr, _, _, _ = eval_from_fixture(path, mbr_decoding=True)
    out_m = mbr()
    assert np.array_equal(out_m["arc"].cpu().numpy(), z["arc_mbr"])
    assert torch.equal(out_m["top5"], out["top5"]) and torch.equal(out_m["loss"], out["loss"])
    assert not np.array_equal(z["arc_mbr"], z["arc_viterbi"])


# ------------------------------------------------------------------------------------------------ the step at config size
def build_pair(B, L, R, dtype, factors, **kw):
    """A training step without dropout and an evaluation step on ITS parameters and batch tensors, with a synthetic gold side."""
    from vlgae_amd import eval_step, train_step
    train = train_step.build(B, L, R, dev(), dtype=dtype, factors=factors, p_drop=0.0, p_enc=0.0, p_ff_drop=0.0, p_mid_drop=0.0,
                             given=dict(drop=None), **SMALL)
    rng = np.random.default_rng(B + L)
    gold = random_gold(rng, B, L, R, train.lengths.cpu().numpy())
    b = train.batch
    step = eval_step.build(B, L, R, dev(), dtype=dtype, factors=factors, E=SMALL["E"], n_vis=SMALL["n_vis"],
                           given=dict(train.P, lengths=train.lengths, token=b["token"], tag=b["tag"], box_mask=b["box_mask"],
                                      **{k: tt(v) for k, v in gold.items()}), **kw)
    return train, step, gold


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_eval_forward_is_the_training_forward_without_dropout(dtype, layout):
    """B = 256: the step's potentials, txt and vis_feat are bit-equal to `step.last` of a training step built with every dropout rate 0 on
    the same parameters (the same launches on the same values); in bf16 the counters equal the numpy restatement applied to the step's
    OWN heads / top-5 / factor2img (bf16 trees may flip against float32; the metric kernel may not)."""
    B, L, R = 256, 40, 36
    with torch.autograd.set_multithreading_enabled(False):
        train, step, gold = build_pair(B, L, R, dtype, LAYOUTS[layout])
        train()
        out = step()
    for k in ("merged_dec", "merged_attach", "txt", "vis_feat", "txt_marginal", "x_fused"):
        assert torch.equal(step.last[k], train.last[k]), k
    assert torch.equal(step.last["heads"], train.last["heads"])
    want = eval_counts(out["arc"].cpu().numpy(), gold["arc"], gold["mask"], train.lengths.cpu().numpy(), out["factor2img"].cpu().numpy(),
                       out["top5"].cpu().numpy(), gold["vis_box"], gold["sg_box"], gold["sg_type"], gold["sg_mask"], LAYOUTS[layout])
    assert counts_of(step.counters) == want
    assert want["total"] > 0 and want["f2i_total"] == 2 * int(train.lengths.sum())
    # the eval loss is the parser's alone, reduced by token: -sum(max) / (num_token + 1e-12)
    ref = -float(step.last["dep_score"].double().sum()) / float(train.lengths.sum())
    assert abs(float(out["loss"]) - ref) <= 1e-5 * abs(ref)
    assert step.counters.compute()["loss"] == pytest.approx(float(out["loss"]), rel=1e-8)


def test_eval_step_on_training_parameters_sees_in_place_updates():
    """Built on a training step's P (in place, no copies): after an optimiser-style in-place update of the parameters the evaluation
    outputs change, and equal those of a fresh build on clones of the updated values."""
    from vlgae_amd import eval_step
    B, L, R = 32, 20, 12
    with torch.autograd.set_multithreading_enabled(False):
        train, step, gold = build_pair(B, L, R, torch.float32, ("rel", "attr", "img"))
        for k in train.P:
            assert step.P[k].data_ptr() == train.P[k].data_ptr(), k
        before = {k: v.clone() for k, v in step().items() if torch.is_tensor(v)}
        _, grads, _ = train()
        with torch.no_grad():
            for k in train.trainable:
                train.P[k].sub_(0.5 * grads[k].to(train.P[k].dtype) / (grads[k].abs().max() + 1e-12))
        after = step()
        b = train.batch
        fresh = eval_step.build(B, L, R, dev(), dtype=torch.float32, factors=b["factors"], E=SMALL["E"], n_vis=SMALL["n_vis"],
                                given=dict({k: v.detach().clone() for k, v in train.P.items()}, lengths=train.lengths, token=b["token"], tag=b["tag"],
                                           box_mask=b["box_mask"], **{k: tt(v) for k, v in gold.items()}))
        want = fresh()
    assert not torch.equal(after["loss"], before["loss"]) and not torch.equal(after["logit"], before["logit"])
    for k in ("arc", "loss", "top5", "factor2img", "logit"):
        assert torch.equal(after[k], want[k]), k
    with pytest.raises(ValueError, match="copied"):
        eval_step.build(B, L, R, dev(), dtype=torch.bfloat16, factors=b["factors"], E=SMALL["E"], n_vis=SMALL["n_vis"], given=dict(train.P))


@pytest.mark.parametrize("mbr", [False, True], ids=["viterbi", "mbr"])
def test_eval_step_as_one_hip_graph(mbr):
    """The whole step -- forward, the one DP pass, decode, loss and the metric update -- captures as ONE HIP graph (no entry point
    synchronises, allocates through the driver or reads a device value on the host); k = 3 replays on unchanged inputs add 3 x the eager
    step's counters and leave outputs bit-equal to the eager step's."""
    B, L, R, k = 64, 24, 20, 3
    with torch.autograd.set_multithreading_enabled(False):
        _, step, _ = build_pair(B, L, R, torch.bfloat16, ("rel", "attr", "img"), mbr_decoding=mbr)
        for _ in range(2):
            out = step()
        want = {n: out[n].clone() for n in ("arc", "loss", "top5", "factor2img", "logit")}
        step.counters.reset()
        step()
        one = counts_of(step.counters)
        loss_one = step.counters.counts()["loss_sum"]
        del out
        gr = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(device=dev())
        side.wait_stream(torch.cuda.current_stream(dev()))
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream(dev()).wait_stream(side)
        torch.cuda.synchronize()
        step.counters.reset()
        with torch.cuda.graph(gr):
            got = step()
        torch.cuda.synchronize()
        assert all(v == 0 for v in step.counters.counts().values())          # capturing runs nothing
        for _ in range(k):
            gr.replay()
        torch.cuda.synchronize()
    assert counts_of(step.counters) == {n: k * v for n, v in one.items()}
    c = step.counters.counts()
    assert c["n_batches"] == k and c["loss_sum"] == k * loss_one
    for n, w in want.items():
        assert torch.equal(got[n], w), n
