"""One VLGAE evaluation step -- host-side mirror of `Pipeline.validation_step` / `test_step` / `predict_step` (src/pipeline.py:132-174;
paths relative to the reference checkout), the half of the loop `train_step` does not cover:

    score   = model(x, vp)              eval mode: every dropout is the identity            the forward of train_step.build, no mask drawn
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

from .train_step import SLOPE, init_feed_forward


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
    Whatever is not given is drawn from `seed` as train_step.build draws it (a synthetic batch; gold trees random).

    dep_loss: "viterbi" (`viterbi_training: true`: nll = -max.sum()) or "partition" (-partition.sum()); mbr_decoding: ldndmv.py:294-299
    instead of the Viterbi tree (config/model/vlgae.yaml:85 ships false); use_pos_prior / use_heuristic: `decode_grounding_args`
    (vlgae.yaml:64-66 ships both true).  metrics=False: no metric launches (loss and predictions only); counters: the
    metrics.EvalCounters to add into (default: a new one, `step.counters`).

    step() -> dict(arc [B,L] int64 (the reference's `predicted`: heads of words 1..L, 0 past the length; a view of the heads [B,L+1]),
    loss (0-d float32), top5 [B,Q,5] / factor2img [B,Q] int32, logit [B,Q,V] (the edited diagonal block), counters)."""
    if dep_loss not in ("viterbi", "partition"):
        raise ValueError(f"eval_step.build: dep_loss {dep_loss!r} ('viterbi' or 'partition': the rule-supervised loss exists in training mode only)")
    from vlgae_amd import align, encoders, langfeat, metrics as metrics_mod, parser_ff, scorer
    from vlgae_amd.torch_struct import functional as tsf
    N, Q = L + 1, 2 * (L + 1)
    given = dict(given or {})
    given_ptrs = {k: t.data_ptr() for k, t in given.items() if torch.is_tensor(t)}
    factors = tuple(factors)
    if any(f not in ("rel", "attr", "img") for f in factors):
        raise ValueError(f"eval_step.build: factors {factors}")
    add_rel, add_attr, add_image = "rel" in factors, "attr" in factors, "img" in factors
    _, V, vis_split, factor_names = encoders.factor_layout(R, add_rel, add_attr, add_image)
    n_enc = 1 + add_rel + add_attr
    ff_dtype = dtype if ff_dtype is None else ff_dtype
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc

    def leaf(name, make, dt=dtype):
        t = given.pop(name) if name in given else make()
        return t.detach().to(dev, dt).contiguous()

    # ---- features and parameters, in train_step.build's order (the same seed draws the same synthetic values) ----
    P = dict(
        emb=leaf("emb", lambda: rnd(B, L, E, sc=0.5), ff_dtype), vis_box_feat=leaf("vis_box_feat", lambda: rnd(B, R, n_vis, sc=0.5)),
        w_text=leaf("w_text", lambda: rnd(h, E, sc=E ** -0.5), ff_dtype),
        w_venc=leaf("w_venc", lambda: rnd(n_enc * h, 2 * n_vis, sc=(2 * n_vis) ** -0.5)), b_venc=leaf("b_venc", lambda: rnd(n_enc * h, sc=0.1)),
        w_vis=leaf("w_vis", lambda: rnd(d, h, sc=h ** -0.5)),
        w_enc=leaf("w_enc", lambda: rnd(3 * d, h, sc=h ** -0.5)), b_enc=leaf("b_enc", lambda: rnd(3 * d, sc=0.1)),
        ln_w=leaf("ln_w", lambda: torch.ones(h), torch.float32), ln_b=leaf("ln_b", lambda: torch.zeros(h), torch.float32),
        w1=leaf("w1", lambda: rnd(d, d, d, sc=1.0 / d)), w2=leaf("w2", lambda: rnd(d, d, sc=d ** -0.5)), b=leaf("b", lambda: rnd(d, sc=0.1)),
    )
    ff_given = {k: given.pop(k) for k in list(given) if k.startswith("ff.") or k in ("token_emb", "root_emb", "dec_emb")}
    if ff_given:
        P.update({k: t.detach().to(dev, ff_dtype).contiguous() for k, t in ff_given.items()})
    else:
        P.update({k: t.detach() for k, t in init_feed_forward(g, dev, ff_dtype, E, h, Et, T, H, nb, r).items()})
    # ---- the batch ----
    if "lengths" in given:
        lengths = given.pop("lengths").to(dev, torch.int64).contiguous()
    else:
        lengths = torch.randint(max(1, L // 2), L + 1, (B,), generator=g)
        lengths[0] = L
        lengths = lengths.to(dev)
    token = given.pop("token").to(dev).contiguous() if "token" in given else torch.randint(0, P["token_emb"].shape[0], (B, L), generator=g).to(dev)
    tag = given.pop("tag").to(dev).contiguous() if "tag" in given else torch.randint(0, 7, (B, L), generator=g).to(dev)
    if "box_mask" in given:
        box_mask = given.pop("box_mask").to(dev, torch.bool).contiguous()
    else:
        n_box = torch.randint(max(1, (3 * R) // 5), R + 1, (B,), generator=g)
        box_mask = (torch.arange(R)[None] < n_box[:, None]).to(dev)
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
    used = dict(P, lengths=lengths, token=token, tag=tag, box_mask=box_mask, arc=arc, **gold_box, **({} if punct_mask is None else dict(mask=punct_mask)))
    copied = [k for k, p in given_ptrs.items() if k in used and used[k].data_ptr() != p]
    if copied:
        raise ValueError(f"eval_step.build: given {copied} would be copied, not used in place -- pass them on {dev}, contiguous, in the "
                         "step's types (parameters: `dtype`, ln_w / ln_b float32, emb / w_text / token_emb / root_emb / dec_emb / ff.*: `ff_dtype`; "
                         "lengths / token / tag / arc / sg_type int64; box_mask / mask / sg_mask bool; vis_box / sg_box float32)")
    if pos_for is None:
        pos_for = dict(obj=torch.tensor([0, 1, 2]), rel=torch.tensor([2, 3]), attr=torch.tensor([4]))
    pos_for = {k: t.to(dev, torch.int64).contiguous() for k, t in pos_for.items()}
    if metrics and counters is None:
        counters = metrics_mod.EvalCounters(dev)
    # buffers the first launch of every step fills from the batch tensors' current contents (vlg_step_batch_prepare): the factor mask, the
    # decoder's POS prior table (scale 1e10, joint.py:528-552), num_token and -1 / (num_token + 1e-12) per sentence (alpha = 0: the
    # parser's loss alone, reduced by token)
    vmask = torch.empty((B, V), dtype=torch.bool, device=dev)
    pen = torch.empty((B, Q, len(vis_split)), dtype=torch.float32, device=dev) if use_pos_prior else None
    seg = align.segment_map(vis_split, dev) if use_pos_prior else None
    num_token = torch.empty((), dtype=torch.float32, device=dev)
    coef = torch.empty(2, dtype=torch.float32, device=dev)
    seed_score = torch.empty(B, dtype=torch.float32, device=dev)
    rel_off = vis_split[0] if add_rel else -1
    attr_off = vis_split[0] + (vis_split[1] if add_rel else 0) if add_attr else -1

    @torch.no_grad()
    def step():
        align.step_batch_prepare(lengths, tag, box_mask, factors, pos_for, Q, 0.0, vmask, pen, num_token, coef, seed_score, scale=1e10)
        # ---- JointModelBase.forward in eval mode: the training step's forward, every dropout the identity ----
        vis_mid, _, _ = encoders.vis_box_rel_encoder(P["vis_box_feat"], P["w_venc"], P["b_venc"], add_rel, add_attr, add_image, SLOPE)
        enc_x = encoders.mlp_encoder(P["emb"], P["w_text"], training=False)
        if enc_x.dtype != dtype:
            enc_x = enc_x.to(dtype)
        vis_feat = align.linear(vis_mid, P["w_vis"])
        pre = langfeat.encoder_projection(enc_x, lengths, P["w_enc"], P["b_enc"])
        word0, _, _ = langfeat.lang_feat_word_only(None, lengths, pre=pre, masks=False)
        x_f = align.attention_fuse(vis_feat, word0, vis_mid, enc_x, P["ln_w"], P["ln_b"], ln_eps)
        x1, x2, y1, y2, root_rule = parser_ff.parser_feed_forward(P, P["emb"], x_f)
        md, ma = scorer.ndmv_potentials(x1, x2, y1, y2, root_rule, token)
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
