"""One VLGAE evaluation step -- host-side mirror of `Pipeline.validation_step` / `test_step` / `predict_step` (src/pipeline.py:132-174;
paths relative to the reference checkout), the half of the loop `train_step` does not cover:

    score   = model(x, vp)              eval mode: every dropout is the identity            step_model.forward (train_step's), no mask drawn
    predict = model.decode(score, vp)   ldndmv.py:289-304 (Viterbi or MBR heads)            the step's ONE DMV pass (+ one DepTree launch for MBR)
                                        joint.py:512-629 (grounding decode)                 align.grounding_decode
    loss    = model.loss(score, y, vp)  joint.py:700: eval mode returns the parser's loss   -max.sum() or -partition.sum() of the same pass,
              reduce_loss('token')      utility/fn.py:50-56                                 / (num_token + 1e-12)
    metric.update(predict, y, mask)     utility/metric.py                                   metrics.EvalCounters (vlg_eval_metrics)

The reference runs the DMV DP four times per batch on the same potentials (lang_feat_max_tree's marginals and arg-max, decode's arg-max,
the loss's max), each with a `nonzero()` host synchronisation, and walks nested Python lists for the grounding predictions and the box
metric.  Here the marginals + Viterbi pair that lang_feat_max_tree needs also yields the decoded heads, the Viterbi score and logZ; the
MBR decode reads those marginals in one DepTree launch (vlg_deptree_mbr_decode); the metrics are integer counts over device tensors.
`step()` performs no host synchronisation and allocates only through torch's caching allocator: it captures as one HIP graph.
`step.predictions()` is the one call that reads the device (the nested lists `write_prediction` wants)."""
import torch

from . import step_model


class _Structure:
    """What lang_feat_max_tree's `structure=` expects: the DP results of this step, already on the current stream."""

    def __init__(self, out):
        self.out = out

    def wait(self):
        return self.out


def build(B, L, R, dev, dtype=torch.bfloat16, d=128, h=256, seed=11, T=45, r=16, given=None, E=800, Et=32, H=256, nb=150, factors=(),
          n_vis=2048, pos_for=None, ln_eps=1e-5, ff_dtype=None, dep_loss="viterbi", mbr_decoding=False, use_pos_prior=True,
          use_heuristic=True, metrics=True, counters=None):
    """The step function of one evaluation step at B sentences of <= L words and R region boxes per image; the conventions are
    `train_step.build`'s (factors, dtype / ff_dtype, `given` tensors by name, `step.last`, `step.P`).

    given: parameters and features under train_step's names -- pass `given=train.P` to evaluate the parameters a training step
    updates; batch tensors lengths / token / tag [B,L] int64, box_mask [B,R] bool; and the gold side of the batch: arc [B,L] int64 (1-based
    heads, 0 = root), mask [B,L] bool (`punct_mask`; default: the length mask vp.mask of the current `lengths`), vis_box
    [B,R,4], sg_box [B,L,8], sg_type [B,L] int64, sg_mask [B,L] bool (all four or none: without them the box metric is skipped).
    EVERY given tensor is used in place: copy the next batch of the same shape into the batch tensors, let the optimiser update the
    parameters, call step() again.  One that would have to be copied (another dtype or device, not contiguous) raises ValueError.
    Whatever is not given is drawn from `seed` by the builder train_step.build draws with, step_model.build_inputs (a synthetic batch; gold
    trees random).

    dep_loss: "viterbi" (`viterbi_training: true`: nll = -max.sum()) or "partition" (-partition.sum()); mbr_decoding: ldndmv.py:294-299
    instead of the Viterbi tree (config/model/vlgae.yaml:85 ships false); use_pos_prior / use_heuristic: `decode_grounding_args`
    (vlgae.yaml:64-66 ships both true).  metrics=False: no metric launches (loss and predictions only); counters: the
    metrics.EvalCounters to add into (default: a new one, `step.counters`).

    step() -> dict(arc [B,L] int64 (the reference's `predicted`: heads of words 1..L, 0 past the length; a view of the heads [B,L+1]),
    loss (0-d float32), top5 [B,Q,5] / factor2img [B,Q] int32, logit [B,Q,V] (the edited diagonal block), counters)."""
    if dep_loss not in ("viterbi", "partition"):
        raise ValueError(f"eval_step.build: dep_loss {dep_loss!r} ('viterbi' or 'partition': the rule-supervised loss exists in training mode only)")
    from vlgae_amd import align, langfeat, metrics as metrics_mod
    from vlgae_amd.torch_struct import functional as tsf
    N, Q = L + 1, 2 * (L + 1)
    given_as_it_came, given = given or {}, dict(given or {})
    ff_dtype = dtype if ff_dtype is None else ff_dtype
    P, batch, layout, g = step_model.build_inputs("eval_step.build", given, seed, B, L, R, dev, dtype, ff_dtype, d, h, E, Et, T, H, nb, r, n_vis,
                                                  factors, train=False)
    lengths, token, tag, box_mask = batch["lengths"], batch["token"], batch["tag"], batch["box_mask"]
    factors, V, vis_split, factor_names = layout["factors"], layout["V"], layout["vis_split"], layout["factor_names"]
    arc = given.pop("arc").to(dev, torch.int64).contiguous() if "arc" in given else \
        (torch.randint(0, L + 1, (B, L), generator=g) * (torch.arange(L)[None] < lengths.cpu()[:, None])).to(dev)
    punct_mask = given.pop("mask").to(dev, torch.bool).contiguous() if "mask" in given else None
    gold_box = {k: given.pop(k) for k in ("vis_box", "sg_box", "sg_type", "sg_mask") if k in given}
    if gold_box and len(gold_box) != 4:
        raise ValueError(f"eval_step.build: vis_box, sg_box, sg_type and sg_mask go together (got {sorted(gold_box)})")
    if gold_box:
        gold_box = dict(vis_box=gold_box["vis_box"].to(dev, torch.float32).contiguous(),
                        sg_box=gold_box["sg_box"].to(dev, torch.float32).contiguous().view(B, L, 8),
                        sg_type=gold_box["sg_type"].to(dev, torch.int64).contiguous(), sg_mask=gold_box["sg_mask"].to(dev, torch.bool).contiguous())
    if given:
        raise ValueError(f"eval_step.build: unknown given entries {sorted(given)}")
    if tuple(arc.shape) != (B, L) or (punct_mask is not None and tuple(punct_mask.shape) != (B, L)):
        raise ValueError(f"eval_step.build: arc / mask must be [B, L] = {(B, L)}")
    step_model.check_in_place("eval_step.build", given_as_it_came, dict(P, **batch, arc=arc, **gold_box, **({} if punct_mask is None else dict(mask=punct_mask))),
                              dev, dict(int64=("arc", "sg_type"), bool=("mask", "sg_mask"), float32=("vis_box", "sg_box")))
    if metrics and counters is None:
        counters = metrics_mod.EvalCounters(dev)
    # buffers the first launch of every step fills from the batch tensors' current contents (vlg_step_batch_prepare): the factor mask, the
    # decoder's POS prior table (scale 1e10, joint.py:528-552), num_token and -1 / (num_token + 1e-12) per sentence (alpha = 0: the
    # parser's loss alone, reduced by token)
    buf = step_model.batch_buffers(B, Q, layout, step_model.default_pos_for(pos_for, dev), use_pos_prior, dev)
    vmask, pen, seg, num_token, coef, seed_score, pos_for = (buf[k] for k in ("vmask", "pen", "seg", "num_token", "coef", "seed", "pos_for"))
    rel_off = vis_split[0] if layout["add_rel"] else -1
    attr_off = vis_split[0] + (vis_split[1] if layout["add_rel"] else 0) if layout["add_attr"] else -1

    @torch.no_grad()
    def step():
        align.step_batch_prepare(lengths, tag, box_mask, factors, pos_for, Q, 0.0, vmask, pen, num_token, coef, seed_score, scale=1e10)
        # ---- JointModelBase.forward in eval mode: the training step's forward, every dropout the identity ----
        vis_mid, enc_x, vis_feat, pre, x_f, md, ma = step_model.forward(P, batch, layout, dtype, ln_eps)
        # ---- ONE DP pass: marginals (lang_feat_max_tree, MBR), logZ (the marginal loss), Viterbi heads (lang_feat_max_tree, decode) and
        # the Viterbi score (the Viterbi loss) ----
        logZ, marg, heads = tsf.dmv1o_marginals_and_heads(md, ma, lengths, keep_viterbi=dep_loss == "viterbi")
        if dep_loss == "viterbi":
            score = tsf._viterbi_lookup(md, ma, lengths)[0]
        else:
            score = logZ
        txt, tmask, tmarg = langfeat.lang_feat_max_tree(None, lengths, md, ma, None, None, P["w1"], P["w2"], P["b"], pre=pre,
                                                        structure=_Structure((logZ, marg, heads)))
        # ---- decode: ldndmv.py:289-304, joint.py:512-596 ----
        out_heads = tsf.deptree_mbr_decode(marg, lengths)[1] if mbr_decoding else heads
        dec = align.grounding_decode(txt, vis_feat, tmask, vmask, pen, seg, use_heuristic, vis_split[0], rel_off, attr_off, N)
        # ---- loss: joint.py:700 -> ldndmv.py:277-281, reduce_loss('token') ----
        loss = torch.dot(score.view(-1), seed_score)
        pred = out_heads[:, 1:]
        if metrics:
            # mask: the batch's punct_mask, else vp.mask (pipeline.py:139-141), which the kernel derives from the lengths
            counters.update(pred, arc, punct_mask, lengths, dec["factor2img"], dec["top5"], loss=loss, factors=factors, **gold_box)
        step.last = dict(enc_x=enc_x, vis_mid=vis_mid, x_fused=x_f, merged_dec=md, merged_attach=ma, txt=txt, txt_mask=tmask, txt_marginal=tmarg,
                         vis_feat=vis_feat, heads=heads, out_heads=out_heads, marginals=marg, logZ=logZ, dep_score=score)
        step.out = dict(arc=pred, loss=loss, top5=dec["top5"], factor2img=dec["factor2img"], logit=dec["logit"], counters=counters)
        return step.out

    def predictions():
        """The reference's `predict` dict of the last step() for `write_prediction` -- the one call that reads the device: arc as nested
        lists, txt_to_factor / txt_to_img as joint.py:596-629 builds them."""
        lists = align.grounding_lists(step.out["top5"], step.out["factor2img"], step.last["txt_mask"], factor_names, vis_split)
        return dict(arc=step.out["arc"].tolist(), **lists)

    step.out = step.last = None
    step.predictions = predictions
    step.P, step.lengths, step.counters, step.dep_loss, step.mbr_decoding = P, lengths, counters, dep_loss, mbr_decoding
    step.batch = dict(token=token, tag=tag, box_mask=box_mask, arc=arc, mask=punct_mask, vis_mask=vmask, factor_names=factor_names, vis_split=vis_split,
                      factors=factors, pos_for=pos_for, use_pos_prior=use_pos_prior, use_heuristic=use_heuristic, **gold_box)
    step.shape = dict(B=B, L=L, R=R, V=V, d=d, h=h, E=E, n_vis=n_vis)
    return step
