"""What the training step (train_step.build) and the evaluation step (eval_step.build) share, once: the parameter table, the builder of
the parameters `P` and of the batch, the refusal of given tensors that would be copied, the buffers vlg_step_batch_prepare fills, and
the forward from the frozen features to the merged potentials (JointModelBase.forward up to DiscriminativeNDMV._forward; the map to the
reference's lines is train_step's docstring).  `seed` draws the same model and batch in both builders because both draw here."""
import torch

SLOPE = 0.01           # nn.LeakyReLU() default, nn/common.py:31
FF_LEAVES = ("token_emb", "root_emb", "dec_emb")


def is_ff(name):
    """A parameter of the parser's feed-forwards (stored in `ff_dtype`; one readiness group)."""
    return name.startswith("ff.") or name in FF_LEAVES


def ff_table(E, h, Et, T, H, nb, r):
    """The rows of `param_table` behind `b`: the reference modules' shapes (vlgae.yaml: H = 256, n_bottleneck = 150, ranks 16), named by
    the modules' own `named_parameters()` behind "ff.<module>." so that a fixture's tensors drop in."""
    rows = []

    def lin(name, n_in, n_out):
        rows.append((name + ".weight", (n_out, n_in), "ff_dtype", n_in ** -0.5))
        rows.append((name + ".bias", (n_out,), "ff_dtype", 0.1))

    for name, n_in in (("head_ff", E + h), ("child_ff", Et), ("root_ff", 10), ("dec_ff", 10)):
        lin(f"ff.{name}.linear", n_in, H)
    for name in ("HASCHILD_linear", "NOCHILD_linear", "LEFT_linear", "RIGHT_linear"):
        if nb:
            lin(f"ff.mid_ff.{name}.0", H, nb)
            lin(f"ff.mid_ff.{name}.1", nb, H)
        else:
            lin(f"ff.mid_ff.{name}", H, H)
    for name in ("valence_linear", "direction_linear", "linear1", "linear2"):
        lin(f"ff.mid_ff.{name}", H, H)
    for name in ("attach_scorer", "dec_scorer", "root_scorer"):
        lin(f"ff.{name}.project1", H, r)
        lin(f"ff.{name}.project2", H, r)
    return rows + [("token_emb", (T, Et), "ff_dtype", 1.0), ("root_emb", (1, 10), "ff_dtype", 1.0), ("dec_emb", (2, 10), "ff_dtype", 1.0)]


def param_table(d, h, E, Et, T, H, nb, r, n_vis, n_enc, B=1, L=1, R=1):
    """Every leaf of a step, IN THE ORDER ITS SYNTHETIC VALUES ARE DRAWN: [(name, shape, storage class, init)].  Storage class: "dtype",
    "ff_dtype" or "float32"; init: the scale of a standard normal draw, or "ones" / "zeros" (no draw).  n_enc = 1 + add_rel + add_attr
    visual-encoder MLPs; B, L, R only size the two frozen features in front (emb, vis_box_feat)."""
    return [("emb", (B, L, E), "ff_dtype", 0.5), ("vis_box_feat", (B, R, n_vis), "dtype", 0.5),
            ("w_text", (h, E), "ff_dtype", E ** -0.5),
            ("w_venc", (n_enc * h, 2 * n_vis), "dtype", (2 * n_vis) ** -0.5), ("b_venc", (n_enc * h,), "dtype", 0.1),
            ("w_vis", (d, h), "dtype", h ** -0.5),
            ("w_enc", (3 * d, h), "dtype", h ** -0.5), ("b_enc", (3 * d,), "dtype", 0.1),
            ("ln_w", (h,), "float32", "ones"), ("ln_b", (h,), "float32", "zeros"),
            ("w1", (d, d, d), "dtype", 1.0 / d), ("w2", (d, d), "dtype", d ** -0.5), ("b", (d,), "dtype", 0.1)] + ff_table(E, h, Et, T, H, nb, r)


def ready_groups(names):
    """The trainable parameters among `names` in the order their gradients become FINAL during the backward pass (autograd runs the
    later-created node first: -max, grounding loss, lang_feat_max_tree | score construction, the parser's feed-forwards | attention fuse,
    word-only encoder, vis_mlp_pre_matching | the text and visual encoders): what a data-parallel trainer's buckets follow."""
    return (["w1", "w2", "b"], [k for k in names if is_ff(k)], ["ln_w", "ln_b", "w_enc", "b_enc", "w_vis"], ["w_text", "w_venc", "b_venc"])


def _draw(g, shape, init):
    if isinstance(init, str):
        return torch.ones(shape) if init == "ones" else torch.zeros(shape)
    return torch.randn(*shape, generator=g) * init


def init_feed_forward(g, dev, dtype, E, h, Et, T, H, nb, r):
    """Random parameters of the parser's feed-forwards (the `ff_table` rows), drawn from `g`."""
    return {name: _draw(g, shape, init).to(dev, dtype).requires_grad_(True) for name, shape, _, init in ff_table(E, h, Et, T, H, nb, r)}


def build_inputs(who, given, seed, B, L, R, dev, dtype, ff_dtype, d, h, E, Et, T, H, nb, r, n_vis, factors, train, feature_grads=False):
    """The model and the batch of one step: (P, batch, layout, g).  P: every `param_table` leaf by name; batch: lengths [B], token / tag
    [B,L] int64, box_mask [B,R] bool; layout: factors, the three add_* flags, V, vis_split, factor_names (encoders.factor_layout); g: the
    generator behind the last draw, for the caller's own synthetic tensors.
    `given` (the caller's dict) is consumed: whatever it names is popped and used in its place, WITHOUT a draw (the draws behind it
    shift); what is left in it is the caller's.  A given "ff.*" / token_emb / root_emb / dec_emb entry means the feed-forwards come whole
    under their own names: none of them is drawn.  train: the leaves require gradients (vis_box_feat only under feature_grads)."""
    from vlgae_amd import encoders
    factors = tuple(factors)
    if any(f not in ("rel", "attr", "img") for f in factors):
        raise ValueError(f"{who}: factors {factors}")
    add_rel, add_attr, add_image = "rel" in factors, "attr" in factors, "img" in factors
    _, V, vis_split, factor_names = encoders.factor_layout(R, add_rel, add_attr, add_image)
    layout = dict(factors=factors, add_rel=add_rel, add_attr=add_attr, add_image=add_image, V=V, vis_split=vis_split, factor_names=factor_names)
    types = dict(dtype=dtype, ff_dtype=ff_dtype, float32=torch.float32)
    g = torch.Generator().manual_seed(seed)
    # ---- the frozen features (BERT subword + tag embedding; Faster-RCNN region features) and every trainable weight behind them ----
    rows = param_table(d, h, E, Et, T, H, nb, r, n_vis, 1 + add_rel + add_attr, B, L, R)
    ff_given = [k for k in given if is_ff(k)]
    if ff_given:
        rows = [row for row in rows if not is_ff(row[0])] + [(k, None, "ff_dtype", None) for k in ff_given]
    P = {}
    for name, shape, storage, init in rows:
        t = given.pop(name) if name in given else _draw(g, shape, init)
        P[name] = t.detach().to(dev, types[storage]).contiguous().requires_grad_(train and (feature_grads or name != "vis_box_feat"))
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
    else:   # ragged region lists as the reference's collate builds them: image i has n_i <= R boxes, `masks_output[i, :n_i] = True` and
        # padding behind them (src/datamodule/task/vlparse.py:68-83) -- a PREFIX mask per image, n_i drawn from [0.6 R, R]
        n_box = torch.randint(max(1, (3 * R) // 5), R + 1, (B,), generator=g)
        box_mask = (torch.arange(R)[None] < n_box[:, None]).to(dev)
    return P, dict(lengths=lengths, token=token, tag=tag, box_mask=box_mask), layout, g


def check_in_place(who, given, used, dev, extra):
    """A given tensor the step had to copy (another dtype / device, not contiguous) would keep its build-time values for ever: later
    batches copied into it and optimiser updates would be ignored without a word -- refuse it.  given: the caller's dict as it came;
    used: what the step holds under the same names; extra: the caller's own batch tensors by type, {"int64": names, ...}."""
    copied = [k for k, t in given.items() if torch.is_tensor(t) and k in used and used[k].data_ptr() != t.data_ptr()]
    if copied:
        kinds = dict(int64=("lengths", "token", "tag"), bool=("box_mask",), float32=())
        kinds = "; ".join(" / ".join(names + tuple(extra.get(k, ()))) + " " + k for k, names in kinds.items() if names or extra.get(k))
        raise ValueError(f"{who}: given {copied} would be copied, not used in place -- pass them on {dev}, contiguous, in the step's types "
                         f"(parameters: `dtype`, ln_w / ln_b float32, emb / w_text / token_emb / root_emb / dec_emb / ff.*: `ff_dtype`; {kinds})")


def default_pos_for(pos_for, dev):
    """The POS tag ids that may ground on each factor (`self.pos_for_*`), on the device."""
    if pos_for is None:
        pos_for = dict(obj=torch.tensor([0, 1, 2]), rel=torch.tensor([2, 3]), attr=torch.tensor([4]))
    return {k: t.to(dev) for k, t in pos_for.items()}


def batch_buffers(B, Q, layout, pos_for, use_pos_prior, dev):
    """Buffers the first launch of every step fills from the batch tensors' current contents (vlg_step_batch_prepare), and the POS sets in
    the form it reads: dict(vmask [B,V] bool, pen [B,Q,S] / seg [V] (None without the prior), num_token (0-d), coef [2], seed [B] (the
    per-sentence seed of the parser's score), pos_for)."""
    from vlgae_amd import align
    vis_split = layout["vis_split"]
    return dict(vmask=torch.empty((B, layout["V"]), dtype=torch.bool, device=dev),
                pen=torch.empty((B, Q, len(vis_split)), dtype=torch.float32, device=dev) if use_pos_prior else None,
                seg=align.segment_map(vis_split, dev) if use_pos_prior else None,      # a function of the layout alone
                num_token=torch.empty((), dtype=torch.float32, device=dev),           # read by the grounding loss's kernel
                coef=torch.empty(2, dtype=torch.float32, device=dev), seed=torch.empty(B, dtype=torch.float32, device=dev),
                pos_for={k: t.to(torch.int64).contiguous() for k, t in pos_for.items()})


def forward(P, batch, layout, dtype, ln_eps, d0=None, enc_drop=None, p_enc=0.0, rng=None, ff_masks=None, fused_ff=True):
    """From the frozen features to the merged potentials: (vis_mid, enc_x, vis_feat, pre, x_fused, merged_dec, merged_attach).
    Every dropout is off by default (eval mode).  d0: the word-only SharedDropout mask [B,1,d]; enc_drop with p_enc > 0: MLPEncoder's
    nn.Dropout, "draw" (from `rng`) or a mask [B,L,E]; ff_masks: the parser feed-forwards' masks (parser_ff.parser_feed_forward's keywords);
    fused_ff=False: the module-by-module form train_step.scorer_feed_forward instead of vlgae_amd.parser_ff (same values)."""
    from vlgae_amd import align, encoders, langfeat, parser_ff, scorer
    lengths, ff_masks = batch["lengths"], ff_masks or {}
    # ---- JointModelBase.forward, base.py:229 / :68: the two trainable encoders on the frozen features ----
    vis_mid, _, _ = encoders.vis_box_rel_encoder(P["vis_box_feat"], P["w_venc"], P["b_venc"], layout["add_rel"], layout["add_attr"], layout["add_image"], SLOPE)
    if enc_drop is None or p_enc == 0:
        enc_x = encoders.mlp_encoder(P["emb"], P["w_text"], training=False)
    elif isinstance(enc_drop, str):
        enc_x = encoders.mlp_encoder(P["emb"], P["w_text"], p_enc, rng=rng)
    else:
        enc_x = encoders.mlp_encoder(P["emb"], P["w_text"], p_enc, mask=enc_drop)
    if enc_x.dtype != dtype:                                          # (ff_dtype != dtype: the language side runs in `dtype`)
        enc_x = enc_x.to(dtype)
    # ---- DependencyBoxRel._forward, joint.py:658-675 ----
    vis_feat = align.linear(vis_mid, P["w_vis"])                                                         # :175 (and again :688: same values)
    # the word | child | parent encoders' Linear on cat([masked mean, x]) ONCE: joint.py:204-209 (word-only) and :262-273 (max-tree) read the
    # same un-fused encodings through the same word encoder, under two SharedDropout masks
    pre = langfeat.encoder_projection(enc_x, lengths, P["w_enc"], P["b_enc"])
    word0, _, _ = langfeat.lang_feat_word_only(None, lengths, drop=d0, pre=pre, masks=False)             # :667 (the fuse reads the features only)
    x_f = align.attention_fuse(vis_feat, word0, vis_mid, enc_x, P["ln_w"], P["ln_b"], ln_eps)             # :670-674
    # ---- DiscriminativeNDMV._forward on the fused copy, ldndmv.py:171-216 ----
    if fused_ff:   # the same mathematics with folded / fused GEMMs and a hand-written adjoint
        x1, x2, y1, y2, root_rule = parser_ff.parser_feed_forward(P, P["emb"], x_f, **ff_masks)
    else:          # module by module, as the reference runs it (explicit masks: the comparison form of the tests)
        from .train_step import scorer_feed_forward
        n_rows, H = P["emb"].shape[0] * P["emb"].shape[1] + P["token_emb"].shape[0] + 3, P["ff.head_ff.linear.weight"].shape[0]
        mid = None if "mid_rng" not in ff_masks else encoders.dropout(torch.ones(4 * n_rows, H, device=x_f.device), ff_masks["p_mid"],
                                                                       rng=ff_masks["mid_rng"], site=encoders.SITE_MID_FF)
        x1, x2, y1, y2, root_rule = scorer_feed_forward(P, P["emb"], x_f, ff_masks.get("drop_head"), ff_masks.get("drop_small"), mid)
    md, ma = scorer.ndmv_potentials(x1, x2, y1, y2, root_rule, batch["token"])
    return vis_mid, enc_x, vis_feat, pre, x_f, md, ma
