#!/usr/bin/env python3
"""Golden vectors of the evaluation step, produced by RUNNING THE REFERENCE (like make_golden.py / make_golden_init.py, which this script
imports and does not change).  Run from the repo root:   python tests/golden/make_golden_eval.py

  evalmetric_*.npz   random predictions (heads, top-5 factor columns, factor -> image) against random gold (arc, scene-graph boxes that are
                     jittered region proposals) through the reference's own DependencyParsingMetric, FactorImageMatchingMetric and
                     BoxRelMatchingMetric (src/utility/metric.py) over TWO consecutive batches: the state after each, and compute().  The
                     nested lists the classes take are built from the index arrays by the reference's decode_grounding_on_factor
                     (joint.py:594-629), called unbound on a logit tensor whose row order is the chosen columns.
  evalstep_*.npz     make_golden.trainstep_cases' two small shapes once more in EVAL mode (`training=False` on both namespaces, modules in
                     eval(): every dropout the identity), on the same inputs and parameters (read by the tests from the paired
                     trainstep_* file): potentials, decode with both `mbr_decoding` values, decode_grounding_on_factor, the eval loss,
                     the three metrics.  The B = 3 shape has a sentence of 4 words, on which BoxRelMatchingMetric raises (fewer scored
                     tokens than predictions per token, metric.py:171): it is evaluated without `sg_box`, as a batch without gold boxes is.

`torchmetrics.Metric` gets a real base here (add_state = setattr of a clone) and `torchvision.ops.boxes._upcast` is the identity for float
tensors; with those the three classes import and run on the CPU.  Conditions asserted so that no test has to skip entries (on failure:
another seed): no compared IoU within 1e-4 of 0.5; the live ones of the six largest edited logits of every kept row pairwise distinct (see
eval_pass for the bound and why); the Viterbi and the MBR tree ahead of every single-arc change by a margin (printed); m_b >= K everywhere."""
import json
import os
import sys
import types
from types import SimpleNamespace as NS

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import _ref_import  # noqa: E402
from eval_restatement import COUNTS, iou  # noqa: E402


class _MetricBase:
    def __init__(self, *args, **kwargs):
        pass

    def add_state(self, name, default, dist_reduce_fx=None):
        setattr(self, name, default.clone())


def import_metrics():
    src, joint = _ref_import.import_joint()
    import torchmetrics
    import torchvision.ops
    torchmetrics.Metric = _MetricBase
    torchvision.ops.boxes = types.SimpleNamespace(_upcast=lambda t: t)
    from src.utility import metric
    return src, joint, metric


class VP(dict):
    __getattr__ = dict.__getitem__


STATE = dict(correct_arcs=("dep", "correct_arcs"), total=("dep", "total"), n_ucm=("dep", "n_ucm"), n=("dep", "n"), f2i_correct=("f2i", "correct"),
             f2i_total=("f2i", "total"), correct_obj=("box", "correct_obj"), correct_attr=("box", "correct_attr"), correct_rel=("box", "correct_rel"),
             correct_r_rel=("box", "correct_r_rel"), total_obj=("box", "total_obj"), total_attr=("box", "total_attr"), total_rel=("box", "total_rel"),
             processed_token=("box", "processed_token"))


def new_metrics(metric):
    return dict(dep=metric.DependencyParsingMetric(None), f2i=metric.FactorImageMatchingMetric(None), box=metric.BoxRelMatchingMetric(None))


def state_of(ms):
    return np.array([int(round(float(getattr(ms[m], a)))) for m, a in (STATE[k] for k in COUNTS)], dtype=np.int64)


def compute_of(ms, losses):
    out = {k: float(v) for k, v in ms["dep"].compute().items()}
    out["factor2img/acc"] = float(ms["f2i"].compute()["acc"])
    out.update({f"box/{k}": float(v) for k, v in ms["box"].compute().items()})
    out["loss"] = sum(losses) / (len(losses) + 1e-9)                                   # pipeline.py:149
    return out


def update_all(ms, predict, gold, mask):
    for m in ms.values():
        m.update(predict, gold, mask)


def lists_from_indices(joint, top5, f2i, tmask, names, widths):
    """txt_to_factor / txt_to_img for given index arrays, by the reference's decode_grounding_on_factor: a [B,A,Q,V] logit whose diagonal
    block sorts to `top5` and whose arg-max image is `f2i` (no prior, no heuristic: the method's list-building lines act on it as is)."""
    B, Q, _ = top5.shape
    V = sum(widths)
    g = torch.Generator().manual_seed(1234)
    logit = torch.rand(B, B, Q, V, generator=g)                       # < 1 everywhere
    for b in range(B):
        for q in range(Q):
            for k in range(min(5, V)):
                logit[b, b, q, top5[b, q, k]] = 10.0 - k
            if f2i[b, q] != b:
                logit[b, f2i[b, q], q, 0] = 20.0
    me = NS(cfg=NS(decode_grounding_args=NS(use_pos_prior=False, use_heuristic=False)), vis_factor_names=list(names))
    vp = VP(seq_len_cpu=[0] * B)
    out = joint.DependencyBoxRel.decode_grounding_on_factor(
        me, {"match_logit": logit.refine_names("B", "A", "Q", "V"), "vis_packed": (None, torch.ones(B, V, dtype=torch.bool), list(widths)),
             "txt_packed": (None, tmask, None)}, vp)
    return out


def put_column(row, k, col):
    """row[k] = col, keeping the row's entries distinct."""
    at = np.flatnonzero(row == col)
    if len(at):
        row[at[0]] = row[k]
    row[k] = col


def random_boxes(rng, *shape):
    xy = rng.uniform(0.0, 0.6, size=(*shape, 2))
    wh = rng.uniform(0.2, 0.4, size=(*shape, 2))
    return np.concatenate([xy, xy + wh], -1).astype(np.float32)


def gold_for(rng, top5, vis_box, lengths, R, factors, p_hit=0.7, live=None):
    """Gold scene-graph fields for given predictions: a token's gold box pair is, mostly, the jittered box pair of one of its predicted
    columns (sometimes swapped, for r_rel), so that every correct_* counter moves; otherwise random boxes.  live [B,L] (optional): tokens
    that may carry a gold alignment; the others get sg_type 0 (no alignment: vlparse.py:208 masks them)."""
    from eval_restatement import column_types
    B, Q, _ = top5.shape
    L = Q // 2 - 1
    V = R + ("rel" in factors) * R * R + ("attr" in factors) * R + ("img" in factors)
    K = min(5, V)
    sg_box = random_boxes(rng, B, L, 2).reshape(B, L, 8)
    sg_type = rng.integers(0, 4, size=(B, L)).astype(np.int64)
    for b in range(B):
        for t in range(L):
            if t >= lengths[b] or (live is not None and not live[b, t]):
                sg_type[b, t] = 0
                continue
            if rng.random() < p_hit:
                typ, bi, bj = column_types(top5[b, t + 1, :K], R, factors)
                k = int(rng.integers(0, K))
                if typ[k] == 0:
                    continue
                pair = np.stack([vis_box[b, bi[k]], vis_box[b, bj[k]]])
                if typ[k] == 3 and rng.random() < 0.4:
                    pair = pair[::-1]
                sg_box[b, t] = (pair + rng.uniform(-0.01, 0.01, size=pair.shape).astype(np.float32)).reshape(8)
                sg_type[b, t] = typ[k]
    sg_mask = sg_type != 0                                              # vlparse.py:208
    return sg_box, sg_type, sg_mask


def assert_iou_margin(vis_box, sg_box, what):
    B, L = sg_box.shape[:2]
    g = sg_box.reshape(B, L, 1, 2, 4)
    v = iou(vis_box[:, None, :, None, :], g)                           # every proposal against both gold boxes of every token
    gap = np.abs(v[np.isfinite(v)] - 0.5).min()
    assert gap > 1e-4, (what, gap)
    return gap


def metric_cases():
    src, joint, metric = import_metrics()
    for name, seed, B, L, R, factors, punct, with_sg in (
            ("evalmetric_B4_L8_box6_rel_attr_s0", 0, 4, 8, 6, ("rel", "attr"), False, True),
            ("evalmetric_B3_L9_box5_rel_attr_img_punct_s1", 1, 3, 9, 5, ("rel", "attr", "img"), True, True),
            ("evalmetric_B4_L7_box6_nosg_s2", 2, 4, 7, 6, (), False, False)):
        rng = np.random.default_rng(seed)
        names = ["obj", *factors]
        widths = [R] + [R * R] * ("rel" in factors) + [R] * ("attr" in factors) + [1] * ("img" in factors)
        V, N, Q = sum(widths), L + 1, 2 * (L + 1)
        K = min(5, V)
        ms, store, losses = new_metrics(metric), {}, []
        for i in range(2):
            lengths = rng.integers(7 if punct else 5, L + 1, size=B)
            lengths[0] = L
            wmask = np.arange(L)[None] < lengths[:, None]
            mask = wmask.copy()
            if punct:                                                   # a punctuation mask with holes, away from the sentence end too
                for b in range(B):
                    mask[b, rng.choice(lengths[b], size=2, replace=False)] = False
            assert (mask.sum(1) >= K).all()
            gold_arc = rng.integers(0, L + 1, size=(B, L)) * wmask
            pred_arc = np.where(rng.random((B, L)) < 0.6, gold_arc, rng.integers(0, L + 1, size=(B, L))) * wmask
            pred_arc[1] = gold_arc[1]                                    # a sentence that counts for ucm
            top5 = np.stack([np.stack([rng.permutation(V)[:5] for _ in range(Q)]) for _ in range(B)]).astype(np.int32)
            if "img" in factors:                                        # type 0 as a token's FIRST prediction, and further down a row
                put_column(top5[0, 1], 0, V - 1)
                put_column(top5[1, 2], 3, V - 1)
            f2i = np.where(rng.random((B, Q)) < 0.5, np.arange(B)[:, None], rng.integers(0, B, size=(B, Q))).astype(np.int32)
            vis_box = random_boxes(rng, B, R)
            m1 = np.concatenate([np.zeros((B, 1), bool), wmask], 1)
            tmask = torch.from_numpy(np.concatenate([m1, m1], 1))
            lists = lists_from_indices(joint, top5, f2i, tmask, names, widths)
            predict = {"arc": torch.from_numpy(pred_arc), **lists}
            gold = {"arc": torch.from_numpy(gold_arc)}
            rec = dict(lengths=lengths.astype(np.int64), mask=mask, gold_arc=gold_arc.astype(np.int64), pred_arc=pred_arc.astype(np.int64), top5=top5,
                       factor2img=f2i, vis_box=vis_box)
            if with_sg:
                sg_box, sg_type, sg_mask = gold_for(rng, top5, vis_box, lengths, R, factors)
                gap = assert_iou_margin(vis_box, sg_box, name)
                gold.update(sg_box=torch.from_numpy(sg_box), sg_type=torch.from_numpy(sg_type), sg_mask=torch.from_numpy(sg_mask),
                            vis_box=torch.from_numpy(vis_box))
                rec.update(sg_box=sg_box, sg_type=sg_type, sg_mask=sg_mask)
            update_all(ms, predict, gold, torch.from_numpy(mask))
            loss = np.float32(rng.uniform(1.0, 3.0))
            losses.append(float(loss))
            rec.update(loss=loss, counters=state_of(ms))
            store.update({f"{k}_{i}": v for k, v in rec.items()})
        comp = compute_of(ms, losses)
        final = state_of(ms)
        if with_sg:
            assert all(final[COUNTS.index(k)] > 0 for k in ("correct_obj", "correct_attr", "correct_rel", "correct_r_rel")), dict(zip(COUNTS, final))
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **store, factors=np.array(list(factors), dtype="U4"), counter_names=np.array(COUNTS),
                            compute=np.array(json.dumps(comp)))
        print(name, dict(zip(COUNTS, final.tolist())), {k: round(v, 3) for k, v in comp.items()})


# ----------------------------------------------------------------------------------------------------------------------------
def step_cases():
    src, joint, metric = import_metrics()
    from src.model import ldndmv
    from src.model.text_encoder.mlp_encoder import MLPEncoder
    from src.utility.fn import reduce_loss
    ts = mg.ts
    JB, ND = joint.DependencyBoxRel, ldndmv.DiscriminativeNDMV
    real_vis_forward, real_enc_forward, real_savez = JB._vis_forward, MLPEncoder.forward, np.savez_compressed
    seen, done = {}, {}

    def enc_forward(self, emb, vp):
        seen["text_enc"], seen["emb"] = self, emb
        return real_enc_forward(self, emb, vp)

    def vis_forward(me, inputs, vis_enc, encoded, score, vp):
        out = real_vis_forward(me, inputs, vis_enc, encoded, score, vp)          # the training step's own call, undisturbed
        if seen["emb"].shape[1] >= 40:                                           # (the L = 40 shape is not stored)
            return out
        dep = me.dependency
        mods = [m for holder in (me, dep) for m in vars(holder).values() if isinstance(m, torch.nn.Module)]
        # trainstep_cases' recorder hooks (the `_mid` tensors, the scorers' projected inputs) must not see the eval pass
        subs = [s_ for m in mods for s_ in m.modules()]
        hooks = [(s_, dict(s_._forward_hooks), dict(s_._forward_pre_hooks)) for s_ in subs]
        for s_ in subs:
            s_._forward_hooks.clear()
            s_._forward_pre_hooks.clear()
        for m in mods:
            m.eval()
        me.training = dep.training = False
        try:
            done["rec"] = eval_pass(me, dep, inputs, vis_enc, vp)
        finally:
            for m in mods:
                m.train()
            for s_, fw, pre in hooks:
                s_._forward_hooks.update(fw)
                s_._forward_pre_hooks.update(pre)
            me.training = dep.training = True
        return out

    def eval_pass(me, dep, inputs, vis_enc, vp):
        emb = seen["emb"]
        B, L = emb.shape[:2]
        factors = tuple(me.vis_factor_names[1:])
        R = inputs["vis_box_mask"].shape[1]
        text_eval = NS(dropout=lambda x: x, shared_dropout=torch.nn.Identity(), linear=seen["text_enc"].linear)
        encoded = {f"vis_{k}": t for k, t in vis_enc.items()}
        encoded |= real_enc_forward(text_eval, emb, vp)
        encoded["emb"] = emb
        score = JB._forward(me, inputs, encoded, vp)
        score = {**score, **real_vis_forward(me, inputs, vis_enc, encoded, score, vp)}
        lengths = vp.seq_len
        # ---- decode, both settings (ldndmv.py:289-304) ----
        arcs = {}
        for mbr in (False, True):
            dep.cfg.mbr_decoding = mbr
            arcs[mbr] = ND.decode(dep, score, vp)["arc"]
        # margins: the Viterbi tree against the best tree that differs (every arc of it penalised in turn), the same for the MBR tree
        md, ma = score["merged_dec"].detach(), score["merged_attach"].detach()
        marg = torch.autograd.grad(ts.DMV1o([md.clone().requires_grad_(), (ma_ := ma.clone().requires_grad_())], lengths).partition.sum(), ma_)[0]
        arc_sc = marg.sum(-1)
        best_v = ts.DMV1o([md, ma], lengths).max
        best_m = ts.DependencyCRF(arc_sc, lengths).max
        gap_v, gap_m = np.inf, np.inf
        for b in range(B):
            for c in range(1, int(lengths[b]) + 1):
                pa = ma.clone()
                pa[b, arcs[False][b, c - 1], c] -= 1e4
                gap_v = min(gap_v, float(best_v[b] - ts.DMV1o([md, pa], lengths).max[b]))
                ps = arc_sc.clone()
                ps[b, arcs[True][b, c - 1], c] -= 1e4
                gap_m = min(gap_m, float((best_m[b] - ts.DependencyCRF(ps, lengths).max[b]).detach()))
        # float32 potentials of magnitude ~10 carry ~1e-6 of rounding each and a tree adds ~3 L of them: a runner-up 2e-4 behind cannot
        # overtake (the training-mode trees of trainstep_cases sit at the same kind of distance under its sc_gain)
        assert gap_v > 2e-4 and gap_m > 2e-4, (gap_v, gap_m)
        # ---- the eval loss (joint.py:700) ----
        total, parts = JB.loss(me, score, {}, vp)
        assert set(parts) == {"nll"}
        loss = reduce_loss("token", total, vp.num_token, vp.batch_size)
        # ---- grounding decode (joint.py:512-629); it edits the diagonal of match_logit in place ----
        use_heur = "img" in factors
        me.cfg.decode_grounding_args = NS(use_pos_prior=True, use_heuristic=use_heur)
        vp.seq_len_cpu                                                       # (the lazy `.cpu()` copy the method reads)
        plain = score["match_logit"].rename(None).detach()
        f2i = plain.max(3).values.max(1).indices.to(torch.int32)            # joint.py:520, before the edits
        before = plain.diagonal().permute(2, 0, 1).clone()
        lists = JB.decode_grounding_on_factor(me, {**score, "match_logit": score["match_logit"].detach(), "arc": arcs[False]}, vp)
        diag = plain.diagonal().permute(2, 0, 1).clone()                      # [B,Q,V] after the edits
        tmask = score["txt_packed"][1].rename(None)
        # Order of the top five.  The prior subtracts 1e10, which absorbs every logit in float32: penalised columns TIE at -1e10 / -2e10, and
        # torch.argsort's order among equal values is not defined (the decoder kernel's is: ascending column).  So the condition is on the
        # LIVE values (> -1e5, the decoder's own threshold, joint.py:566): those among a kept row's six largest are pairwise distinct by
        # more than 1e-4 of the spread of the row's alignment scores (before the edits: the heuristic's -100 would inflate it); ranks that
        # hold a dead value are compared by value, and tokens whose five predictions are not all live carry no gold alignment (their order
        # cannot reach a counter).  1e-4 and not the 1e-3 first aimed at: the inputs are trainstep_cases' (its seeds are not this
        # script's to change) and their closest pairs sit at 9e-4 (B = 3) and 7e-4 (B = 4, heuristic on) of the
        # spread -- two summation orders of a 32-term float32 dot product of O(1) terms differ by ~1e-6 of it.  The B = 3 shape runs
        # without the heuristic: with it, its closest pair is about 3e-5 of the spread.
        srt = diag.sort(-1, descending=True)
        top6 = srt.values[..., :6]
        alive = before > -1e5
        spread = (before.masked_fill(~alive, -np.inf).max(-1).values - before.masked_fill(~alive, np.inf).min(-1).values).clamp(min=1e-30)
        gaps = (top6[..., :-1] - top6[..., 1:]) / spread.unsqueeze(-1)
        gaps = gaps.masked_fill(top6[..., :-1] <= -1e5, np.inf)              # a gap below a dead value is a tie by construction
        sep = gaps.min(-1).values[tmask]
        assert sep.min() > 1e-4, float(sep.min())
        live5 = (top6[..., :5] > -1e5).all(-1)[:, 1:L + 1].numpy()            # word rows 1..L
        top5 = srt.indices[..., :5].to(torch.int32)
        # ---- metrics over this batch, twice (two consecutive batches of the same content: counters accumulate) ----
        rng = np.random.default_rng(5 + B)
        wmask = vp.mask.numpy()
        with_sg = bool((lengths >= 5).all())
        mask = wmask.copy()
        if with_sg:                                                          # the B = 4 shape: a punctuation mask with one hole per sentence
            for b in range(B):
                mask[b, rng.integers(0, int(lengths[b]))] = False
            assert (mask.sum(1) >= 5).all()
        pred = arcs[False].numpy()
        gold_arc = (np.where(rng.random((B, L)) < 0.5, pred, rng.integers(0, L + 1, size=(B, L))) * wmask).astype(np.int64)
        rec = dict(gold_arc=gold_arc, mask=mask)
        gold = {"arc": torch.from_numpy(gold_arc)}
        if with_sg:
            vis_box = random_boxes(rng, B, R)
            sg_box, sg_type, sg_mask = gold_for(rng, top5.numpy(), vis_box, lengths.numpy(), R, factors, p_hit=0.9, live=live5)
            assert_iou_margin(vis_box, sg_box, "evalstep")
            gold.update(sg_box=torch.from_numpy(sg_box), sg_type=torch.from_numpy(sg_type), sg_mask=torch.from_numpy(sg_mask), vis_box=torch.from_numpy(vis_box))
            rec.update(vis_box=vis_box, sg_box=sg_box, sg_type=sg_type, sg_mask=sg_mask)
        ms = new_metrics(metric)
        predict = {"arc": arcs[False], **lists}
        states = []
        for _ in range(2):
            update_all(ms, predict, gold, torch.from_numpy(mask))
            states.append(state_of(ms))
        comp = compute_of(ms, [float(loss.item())] * 2)
        to_img = [[int(t) for t in row] for row in lists["txt_to_img"]]
        rec.update(merged_dec=mg._np(score["merged_dec"]), merged_attach=mg._np(score["merged_attach"]), arc_viterbi=arcs[False].numpy(),
                   arc_mbr=arcs[True].numpy(), loss=mg._np(loss), nll=mg._np(total), logit=mg._np(diag), top5=top5.numpy(), factor2img=f2i.numpy(),
                   txt_mask=tmask.numpy(), counters_0=states[0], counters_1=states[1], counter_names=np.array(COUNTS), compute=np.array(json.dumps(comp)),
                   txt_to_factor=np.array(json.dumps(lists["txt_to_factor"])), txt_to_img=np.array(json.dumps(to_img)),
                   use_pos_prior=np.bool_(True), use_heuristic=np.bool_(use_heur), with_sg=np.bool_(with_sg), emb_check=mg._np(emb[0, 0, :4]))
        print(f"  eval: loss {float(loss.detach()):.6f} margins viterbi {gap_v:.4f} mbr {gap_m:.5f} top-6 separation {float(sep.min()):.4f} "
              f"mbr != viterbi on {int((arcs[True] != arcs[False]).sum())} words; {dict(zip(COUNTS, states[1].tolist()))}")
        return rec

    def savez(path, **kw):
        name = os.path.basename(path)
        if "_L40_" in name:
            return
        old = np.load(path)                                                   # the committed trainstep_* file: same inputs, bit for bit
        assert np.array_equal(old["emb"], kw["emb"]) and np.array_equal(old["w_text"], kw["w_text"]) and np.array_equal(old["loss"], kw["loss"]), name
        rec = done.pop("rec")
        rec["top_vals"] = np.sort(rec["logit"], -1)[..., ::-1][..., :5].copy()
        assert np.array_equal(rec.pop("emb_check"), kw["emb"][0, 0, :4])
        real_savez(os.path.join(HERE, name.replace("trainstep_", "evalstep_")), **rec)
        print(name.replace("trainstep_", "evalstep_"), {k: getattr(v, "shape", None) for k, v in rec.items() if k in ("merged_attach", "logit", "top5")})

    JB._vis_forward, MLPEncoder.forward, np.savez_compressed = vis_forward, enc_forward, savez
    try:
        mg.trainstep_cases()
    finally:
        JB._vis_forward, MLPEncoder.forward, np.savez_compressed = real_vis_forward, real_enc_forward, real_savez


if __name__ == "__main__":
    metric_cases()
    step_cases()
