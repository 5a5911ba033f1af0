"""One VLGAE training step (BASELINE.json configs[4]: "frozen BERT + Faster-RCNN feats -> biaffine -> inside-outside marginal loss")
from the FROZEN FEATURES to the gradient of every trainable parameter, wired AS THE REFERENCE WIRES IT -- host-side mirror of
`JointModelBase.forward` + `DependencyBoxRel.loss` + `reduce_loss` + `loss.backward()`.  Paths are relative to /root/reference.

Contract.  `build(...)` returns `step()`; `step()` runs forward + backward of the chain below on the current HIP stream (no host
synchronisation, no allocation through the driver: capturable as one HIP graph) and returns (reduced loss, {leaf name: gradient}, ()).
The SAME function is what
  * `tests/test_gpu_parity.py::test_training_step_reference_wiring[*]` runs on fixtures produced by the reference's own methods
    (tests/golden/trainstep_*.npz, make_golden.py `trainstep_cases`), in float32 and in the bf16 configuration the bench times,
  * `..._config_size[*]` runs at B = 256 against the reference's formulation in float64 torch ops,
  * `bench.py`'s `train_step` entries time (vlgae_amd/bench/secondary.py), and
  * `bench.py --workload train_step [--gpus N]` shards (vlgae_amd/bench/sharded_step.py).

  JointModelBase.forward           src/model/base.py:215-241
    VisBoxRelSimpleEncoder.forward src/model/vis_encoder/box_rel.py:29-52   base.py:229   box_fc / rel_fc / attr_fc on [box ; mean box],
      + the cat of vis_feat_unprune src/model/joint.py:143-171              one [B,V,H] factor tensor (obj | rel | attr | img)        -> encoders.vis_box_rel_encoder
    MLPEncoder.forward             src/model/text_encoder/mlp_encoder.py:36-40   base.py:68   x = Linear(Dropout(emb))               -> encoders.mlp_encoder
    DependencyBoxRel._forward      src/model/joint.py:658-675
      vis_feat_unprune             :137-178   vis_feat = vis_mlp_pre_matching(vis_mid)  (bias-free nn.Linear)          -> align.linear
      lang_feat_word_only          :193-211   root row = masked mean, word encoder (+ SharedDropout)                  -> langfeat.lang_feat_word_only
      attention fuse               :670-674   softmax(vis_feat . word^T) vis_mid, residual, LayerNorm                  -> align.attention_fuse
        the fused x goes into a COPY of `encoded` (feat_fuse_args.replace: false, :376-377): only the parser sees it
    DiscriminativeNDMV._forward    src/model/ldndmv.py:171-216  on that copy
      context_mode 'mean'          :226,:254  h = cat([emb, mean_l(fused x)])
      head_ff / child_ff / root_ff / dec_ff (MLP, nn/common.py:23-51), mid_ff (DMVSkipConnectEncoder, nn/dmv_spec.py:6-54),
      the scorers' project1 / project2 (nn.Linear, nn/dmv_spec.py:63-68)                                               -> parser_ff.parser_feed_forward
                                                                     (module by module in torch: `scorer_feed_forward` below, the tests' comparison)
      scores -> log-softmax over tokens -> gather / direction select / root gather / merge   :184-209                   -> scorer.ndmv_potentials
    DependencyBoxRel._vis_forward  joint.py:677-691
      lang_feat_max_tree           :235-292   on the caller's `encoded`, i.e. the UN-fused x: DMV1o marginals + Viterbi heads of
                                              the detached potentials, word | child | parent encoders (+ SharedDropout), arc encoder -> langfeat.lang_feat_max_tree
      gather_logit_simple          :406-419   } never materialised: alignment maxima + arg-max on the matrix cores,
  DependencyBoxRel.loss            :693-711   }
      loss_grounding_factor_ce     :439-491   } POS prior (use_pos_prior: true), both cross-entropies, vis2txt = 1          -> align.grounding_loss_factor_ce
      DiscriminativeNDMV.loss      ldndmv.py:260-285, by `dep_loss`:
                                     "viterbi"    (viterbi_training, after the init epochs) -DMV1o(potentials).max.sum() (the step's one
                                                  Viterbi pass is reused)
                                     "gold_rules" (the first init_epoch epochs of init_method 'y', :262-275) enll = -(rule counts of the
                                                  batch's gold `arc` . potentials), rules1o.gold_rule_score
                                     "partition"  (viterbi_training: false, :280-281) -DMV1o(potentials).partition.sum() (the
                                                  inside-outside pass of lang_feat_max_tree is reused)
      alpha * mt_loss + (1 - alpha) * dep_loss, alpha = grounding_interpolation = 0.5 (config/model/vlgae.yaml:67)
  reduce_loss('token')             src/utility/fn.py:50-56 (src/pipeline.py:124,249-250): / (num_token + 1e-12)
  loss.backward()                  every adjoint of the above

Leaves: the frozen features `emb` [B,L,E] (= what `self.embedding` emits: [BERT subword ; tag embedding]; its gradient is computed, the
tag embedding is trainable) and `vis_box_feat` [B,R,n] (no gradient unless `feature_grads`), and every trainable tensor: `w_text`
(MLPEncoder.linear), `w_venc` / `b_venc` (the visual encoder's box_fc | rel_fc | attr_fc stacked), `w_vis`, `w_enc` / `b_enc` (word | child |
parent encoders stacked), `ln_w` / `ln_b`, `w1` / `w2` / `b` (arc encoder), `token_emb` / `root_emb` / `dec_emb` and the "ff.*" feed-forwards.
"""
import torch
import torch.nn.functional as F

from . import step_model
from .step_model import SLOPE, init_feed_forward   # noqa: F401 -- (init_feed_forward: re-exported, callers import it from here)

DEP_LOSSES = ("viterbi", "gold_rules", "partition")
FF_MODULES = ("head_ff", "child_ff", "root_ff", "dec_ff", "mid_ff", "attach_scorer", "dec_scorer", "root_scorer")


# ----------------------------------------------------------------------------------------------------------------------------
# The parser's feed-forwards (out of the hot path: plain Linear / LeakyReLU stacks, left to the library).  Parameter names are
# the reference modules' own `named_parameters()` names behind "ff.<module>." so that a fixture's tensors drop in.
# ----------------------------------------------------------------------------------------------------------------------------
def _lin(P, name, x):
    return F.linear(x, P[name + ".weight"], P.get(name + ".bias"))


def _mlp(P, name, x, drop=None):
    """MLP (nn/common.py:23-51): Linear -> LeakyReLU -> SharedDropout (a mask broadcastable to the output, or None)."""
    y = F.leaky_relu(_lin(P, f"ff.{name}.linear", x), SLOPE)
    return y if drop is None else y * drop.to(y.dtype)


def _bottleneck(P, name, x):
    if name + ".weight" in P:                                   # n_bottleneck == 0: one Linear
        return _lin(P, name, x)
    return _lin(P, name + ".1", _lin(P, name + ".0", x))      # nn.Sequential(Linear(H, nb), Linear(nb, H)), no activation between


def _skip_connect(P, x, drop=None):
    """DMVSkipConnectEncoder.forward (nn/dmv_spec.py:38-54): [..., H] -> [..., dir, val, H].  drop: nn.Dropout's mask [..., 2, 2, H] or None."""
    act = lambda t: F.leaky_relu(t, SLOPE)
    m = "ff.mid_ff."
    has_child = _bottleneck(P, m + "HASCHILD_linear", x) + x
    no_child = _bottleneck(P, m + "NOCHILD_linear", x) + x
    h = torch.stack([no_child, has_child], dim=-2)
    h = act(_lin(P, m + "valence_linear", act(h)))
    x4 = x.unsqueeze(-2)
    left = _bottleneck(P, m + "LEFT_linear", h) + x4
    right = _bottleneck(P, m + "RIGHT_linear", h) + x4
    h = torch.stack([left, right], dim=-3)
    h = act(_lin(P, m + "direction_linear", act(h)))
    if drop is not None:
        h = h * drop.to(h.dtype)
    return _lin(P, m + "linear2", act(_lin(P, m + "linear1", h)))


def scorer_feed_forward(P, emb, x_fused, drop_head=None, drop_small=None, drop_mid=None):
    """ldndmv.py:174-205 up to the scorers' projected inputs, MODULE BY MODULE as the reference runs it: (x1 [B,L,2,2,r], x2 [T,2,2,r],
    y1 [B,L,2,2,r], y2 [2,2,2,r], root_rule [T]).  context_mode 'mean' (:226): every token's representation is cat([emb, mean over ALL L
    positions of x]).  Dropout masks as in vlgae_amd.parser_ff.parser_feed_forward (explicit, so that the two formulations can be compared)."""
    B, L, _ = emb.shape
    T = P["token_emb"].shape[0]
    H = P["ff.head_ff.linear.weight"].shape[0]
    M0 = B * L
    ctx = x_fused.mean(1, keepdim=True).expand(-1, L, -1)
    h = torch.cat([emb, ctx.to(emb.dtype)], dim=-1)
    ds = (lambda a, b: None) if drop_small is None else (lambda a, b: drop_small[a:b].unsqueeze(1))
    dm = (lambda a, b, shp: None) if drop_mid is None else (lambda a, b, shp: drop_mid[4 * a:4 * b].reshape(*shp, 2, 2, H))
    h_parent = _skip_connect(P, _mlp(P, "head_ff", h, None if drop_head is None else drop_head.unsqueeze(1)), dm(0, M0, (B, L)))
    h_child = _skip_connect(P, _mlp(P, "child_ff", P["token_emb"], ds(0, T)), dm(M0, M0 + T, (T,)))                  # [T,2,2,H]
    h_root = _skip_connect(P, _mlp(P, "root_ff", P["root_emb"], ds(T, T + 1)), dm(M0 + T, M0 + T + 1, (1,)))        # [1,2,2,H]
    h_dec = _skip_connect(P, _mlp(P, "dec_ff", P["dec_emb"], ds(T + 1, T + 3)), dm(M0 + T + 1, M0 + T + 3, (2,)))   # [2,2,2,H]
    x1, x2 = _lin(P, "ff.attach_scorer.project1", h_parent), _lin(P, "ff.attach_scorer.project2", h_child)
    y1, y2 = _lin(P, "ff.dec_scorer.project1", h_parent), _lin(P, "ff.dec_scorer.project2", h_dec)
    r1, r2 = _lin(P, "ff.root_scorer.project1", h_root), _lin(P, "ff.root_scorer.project2", h_child)
    root_rule = torch.einsum("hdve,cdve->hc", r1.float(), r2.float()).log_softmax(-1)[0]   # :205: sum over (dir, val), softmax over tokens
    return x1, x2, y1, y2, root_rule


def forced_tree_score(md, ma, heads, lengths, big=1e4):
    """Score [B,1] of the dependency tree `heads` [B,N] under root-merged DMV1o potentials, differentiable w.r.t. both: the body lives in
    vlgae_amd.torch_struct.functional.dmv1o_tree_score (DMV1o.log_prob_heads shares it)."""
    from vlgae_amd.torch_struct.functional import dmv1o_tree_score
    return dmv1o_tree_score(md, ma, heads, lengths, big)


# ----------------------------------------------------------------------------------------------------------------------------
def build(B, L, R, dev, dtype=torch.bfloat16, d=128, h=256, seed=11, T=45, r=16, given=None,
          alpha=0.5, use_pos_prior=True, vis2txt=1.0, p_drop=0.33, E=800, Et=32, H=256, nb=150, p_ff_drop=0.33, p_mid_drop=0.3,
          factors=(), n_vis=2048, p_enc=0.33, pos_for=None, ln_eps=1e-5, ff_dtype=None, fused_ff=True, feature_grads=False, rng=None,
          batch_on_device=False, dep_loss="viterbi"):
    """The step function of one training step at B sentences of <= L words and R region boxes per image.

    factors: which of ("rel", "attr", "img") the model adds to the object factor (cfg.add_rel / add_attr / add_image; the shipped
    config/model/vlgae.yaml:39-41 has all three: V = R + R^2 + R + 1 columns, 1369 at R = 36; BASELINE.json configs[1] names R = 36
    region columns: the object factor alone, the default).  n_vis / E: widths of the frozen region features / embeddings (2048 / 800).
    `given` (a dict) replaces any of the synthetic inputs / parameters by name (tests: the fixture's tensors) -- features emb [B,L,E],
    vis_box_feat [B,R,n_vis]; batch lengths / token / tag [B,L], box_mask [B,R], drop [4,B,d] (the SharedDropout masks in the reference's
    call order: word-only, then word | child | parent; or None), enc_drop [B,L,E] (MLPEncoder's nn.Dropout mask; or None), heads [B,L+1] (a tree
    to use INSTEAD of the Viterbi tree of the step's own potentials -- teacher forcing, see `step.forced_heads` below); parameters
    w_text [h,E], w_venc [F h, 2 n_vis] / b_venc [F h], w_vis [d,h], w_enc [3d,h], b_enc [3d], ln_w, ln_b [h], w1 [d,d,d], w2 [d,d], b [d],
    token_emb / root_emb / dec_emb and the "ff.*" feed-forward parameters.  With `given` drop / enc_drop absent, fresh masks are drawn
    every step (p_drop / p_enc; the embedding dropout from a device-resident counter-based generator, encoders.DeviceRng).
    ff_dtype: storage / compute type of the parser's feed-forwards and of `emb` (default = dtype); fused_ff: vlgae_amd.parser_ff (folded /
    fused library GEMMs, hand-written adjoint) instead of the module-by-module torch formulation `scorer_feed_forward` (same values).
    p_ff_drop / p_mid_drop: the parser feed-forwards' dropout (shipped: 0.33 / 0.3; masks drawn per step; 0 = off, as in the fixtures).
    alpha / use_pos_prior / vis2txt: config/model/vlgae.yaml:62-67.  feature_grads: also return the gradient w.r.t. vis_box_feat (the
    reference does not compute it -- the region features are data; the parity tests do).
    rng: the encoders.DeviceRng the step draws its dropout masks from (default: a new one seeded from `seed`; steps built for several
    batch shapes can share one, so that the draws follow the step count).  batch_on_device: derive NOTHING from the batch's contents at
    build time -- the first launch of every step(), vlg_step_batch_prepare, writes the vis mask, the POS prior table, num_token and the
    loss coefficients into buffers the step owns, from the CURRENT contents of lengths / tag / box_mask.  Every given batch tensor and
    parameter is used in place (copy the next batch of the same shape into them, update the parameters in place, call step() again); one
    that would have to be copied -- another dtype or device, not contiguous -- raises ValueError.  Same values, bit for bit.
    Returns step(); step() -> (loss, {name: gradient}, ()).

    dep_loss: the parser's loss (DiscriminativeNDMV.loss, ldndmv.py:260-285).  "viterbi": -max of the step's potentials (viterbi_training,
    after the initialisation epochs; the default).  "gold_rules": the rule-supervised initialisation epochs (init_method 'y', the first
    init_epoch epochs): -score of the gold tree given as the batch tensor `arc` [B,L] int64 (1-based heads, 0 = root; given["arc"],
    required, used in place under batch_on_device), rules1o.gold_rule_score; lang_feat_max_tree then keeps no Viterbi pass and
    `forced_heads` only changes the tree it reads.  "partition": the marginal loss (viterbi_training: false), -logZ of the step's
    potentials, reusing lang_feat_max_tree's inside-outside pass.  Every mode seeds its per-sentence score with the same coefficient
    -(1 - alpha) / num_token; step.last["dep_score"] holds it.
    Returns step(); step() -> (loss, {name: gradient}, ())."""
    if dep_loss not in DEP_LOSSES:
        raise ValueError(f"train_step.build: dep_loss {dep_loss!r} (one of {DEP_LOSSES})")
    has_arc = bool(given) and "arc" in given
    if dep_loss == "gold_rules" and not has_arc:
        raise ValueError("train_step.build(dep_loss='gold_rules') needs the batch's gold trees: given['arc'] [B,L] int64 (1-based heads, 0 = root)")
    if has_arc and dep_loss != "gold_rules":
        raise ValueError(f"train_step.build: given['arc'] is only read with dep_loss='gold_rules' (got dep_loss={dep_loss!r})")
    import vlgae_amd.torch_struct as ts
    from vlgae_amd import align, encoders, langfeat, rules1o
    Q = 2 * (L + 1)
    given_as_it_came, given = given or {}, dict(given or {})
    ff_dtype = dtype if ff_dtype is None else ff_dtype
    P, batch, layout, _ = step_model.build_inputs("train_step.build", given, seed, B, L, R, dev, dtype, ff_dtype, d, h, E, Et, T, H, nb, r, n_vis,
                                                  factors, train=True, feature_grads=feature_grads)
    lengths, token, tag, box_mask = batch["lengths"], batch["token"], batch["tag"], batch["box_mask"]
    factors, V, vis_split, factor_names = layout["factors"], layout["V"], layout["vis_split"], layout["factor_names"]
    fixed_drop = given.pop("drop") if "drop" in given else "draw"
    if fixed_drop is not None and not isinstance(fixed_drop, str):
        fixed_drop = fixed_drop.to(dev, torch.float32).permute(1, 0, 2).contiguous()      # [B,4,d]
    forced_heads = given.pop("heads").to(dev, torch.int64) if "heads" in given else None
    arc = given.pop("arc").to(dev, torch.int64).contiguous() if "arc" in given else None
    if arc is not None and tuple(arc.shape) != (B, L):
        raise ValueError(f"train_step.build: given['arc'] must be [B, L] = {(B, L)}, got {tuple(arc.shape)}")
    enc_drop = given.pop("enc_drop") if "enc_drop" in given else "draw"
    if enc_drop is not None and not isinstance(enc_drop, str):
        enc_drop = enc_drop.to(dev, torch.float32).contiguous()                           # [B,L,E]
    if given:
        raise ValueError(f"train_step.build: unknown given entries {sorted(given)}")
    if batch_on_device:
        step_model.check_in_place("train_step.build(batch_on_device=True)", given_as_it_came, dict(P, **batch, **({} if arc is None else dict(arc=arc))),
                                  dev, dict(int64=("arc",)))
    if rng is None:
        rng = encoders.DeviceRng(seed * 7919 + 17, dev)   # the counter-based dropout draws of the step (advanced on the device once per step)
    pos_for = step_model.default_pos_for(pos_for, dev)
    names = sorted(k for k in P if P[k].requires_grad)
    leaves = [P[k] for k in names]
    aux = {}
    if batch_on_device:
        buf = step_model.batch_buffers(B, Q, layout, pos_for, use_pos_prior, dev)
        vmask, pen, seg, coef, seed_max, pos_for = buf["vmask"], buf["pen"], buf["seg"], buf["coef"], buf["seed"], buf["pos_for"]
        num_token = num_token_f = buf["num_token"]
        c_mt = coef[0]
    else:
        # vis_feat_unprune's mask (joint.py:140-170): data, built once per batch
        vmask = encoders.factor_mask(box_mask, layout["add_rel"], layout["add_attr"], layout["add_image"])
        num_token = lengths.sum()                                     # a 0-d tensor like vp.num_token (var_pool.py:18)
        num_token_f = float(num_token.item())
        # the POS prior table (joint.py:446-470) is a function of the batch's tags only -- data, like the masks: built once per batch
        pen = seg = None
        if use_pos_prior:
            pen, seg = align.grounding_prior(tag, factor_names, vis_split, pos_for, Q)
        # loss = (alpha mt + (1 - alpha) dep) / (num_token + 1e-12), dep = -sum_b max_b: two per-batch coefficients.  They seed the
        # backward pass directly (autograd.grad's grad_outputs), so the scalar arithmetic of the combination has no adjoint launches.
        coef = (torch.tensor([alpha, -(1.0 - alpha)], dtype=torch.float32, device=dev) / (num_token.to(torch.float32) + 1e-12))
        c_mt, c_max = coef[0], coef[1]
        seed_max = c_max.repeat(B)
    T_, H_ = P["token_emb"].shape[0], P["ff.head_ff.linear.weight"].shape[0]

    def draw_masks():
        """(drop [B,4,d] or None, parser_ff masks): the per-sentence SharedDropout masks of one step come out of ONE launch of the
        counter-based generator when the rates agree; mid_ff's nn.Dropout is drawn inside its activation kernel (no tensor)."""
        mid = dict(mid_rng=rng, p_mid=p_mid_drop) if p_mid_drop > 0 else {}
        if isinstance(fixed_drop, str) and p_drop == p_ff_drop and 0 < p_drop < 1:
            n0, n1 = B * 4 * d, B * H_
            buf = encoders.dropout_mask(rng, encoders.SITE_SHARED, p_drop, n0 + n1 + T_ + 3)
            return buf[:n0].view(B, 4, d), dict(drop_head=buf[n0:n0 + n1].view(B, H_), drop_small=buf[n0 + n1:], **mid)
        if isinstance(fixed_drop, str):
            drop = encoders.dropout_mask(rng, encoders.SITE_SHARED, p_drop, B * 4 * d).view(B, 4, d) if 0 < p_drop < 1 else None
        else:
            drop = fixed_drop
        ff = {}
        if 0 < p_ff_drop < 1:
            buf = encoders.dropout_mask(rng, encoders.SITE_SHARED_FF, p_ff_drop, B * H_ + T_ + 3)
            ff = dict(drop_head=buf[:B * H_].view(B, H_), drop_small=buf[B * H_:])
        return drop, dict(**ff, **mid)

    def step(stage_hook=None):
        """forward + backward; returns (reduced loss, gradients by leaf name, ()).  stage_hook (optional) is called from inside the
        backward pass once the adjoints of the DP and of the grounding loss have run (the cotangent of `txt` exists) -- where a
        data-parallel trainer starts reducing its first gradient bucket."""
        if batch_on_device:
            align.step_batch_prepare(lengths, tag, box_mask, factors, pos_for, Q, alpha, vmask, pen, num_token, coef, seed_max)
        drop, ff_masks = draw_masks()
        d0, d3 = (None, None) if drop is None else (drop[:, 0:1], drop[:, 1:4])
        # ---- JointModelBase.forward, DependencyBoxRel._forward, DiscriminativeNDMV._forward: the forward the evaluation step shares ----
        vis_mid, enc_x, vis_feat, pre, x_f, md, ma = step_model.forward(P, batch, layout, dtype, ln_eps, d0=d0, enc_drop=enc_drop, p_enc=p_enc, rng=rng,
                                                                        ff_masks=ff_masks, fused_ff=fused_ff)
        # ---- DependencyBoxRel._vis_forward, joint.py:677-691: the UN-fused x; the potentials are constants of this stage (:252-253) ----
        txt, tmask, tmarg = langfeat.lang_feat_max_tree(None, lengths, md.detach(), ma.detach(), None, None, P["w1"],
                                                        P["w2"], P["b"], keep_viterbi=dep_loss == "viterbi", drop=d3, aux=aux, pre=pre,
                                                        heads=step.forced_heads, keep_partition=dep_loss == "partition")
        if stage_hook is not None:
            txt.register_hook(lambda g_: stage_hook())
        # ---- DependencyBoxRel.loss, joint.py:693-711 ----
        mt, sums = align.grounding_loss_factor_ce(txt, vis_feat, tmask, vmask, tmarg, num_token_f, vis2txt, pen, seg)
        if dep_loss == "gold_rules":
            mx = rules1o.gold_rule_score(md, ma, arc, lengths)    # ldndmv.py:262-275: enll = -(gold rule counts . potentials)
        elif dep_loss == "partition":
            mx = ts.DMV1o([md, ma], lengths).partition            # ldndmv.py:280-281: dep = -partition.sum(); lang_feat_max_tree's pass is reused
        elif step.forced_heads is None:
            mx = ts.DMV1o([md, ma], lengths).max                  # ldndmv.py:277-281: dep = -max.sum(); lang_feat_max_tree's Viterbi pass is reused
        else:
            mx = forced_tree_score(md, ma, step.forced_heads, lengths)   # teacher forcing: the given tree's score in place of the best tree's
        with torch.no_grad():                                     # alpha mt + (1 - alpha) dep, reduce_loss('token'): c_mt mt + sum_b c_max max_b, two launches
            loss = torch.addcmul(torch.dot(mx.view(-1), seed_max), c_mt, mt)
        grads = torch.autograd.grad([mt, mx], leaves, [c_mt, seed_max.view(mx.shape)])
        rng.advance()                                                 # the next step (or graph replay) draws new dropout masks at every site
        # intermediates for the parity tests, DETACHED: a reference to a previous step's autograd graph kept alive across a HIP-graph
        # capture makes torch 2.10 / ROCm 7 crash in capture_end
        step.last = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in dict(
            enc_x=enc_x, vis_mid=vis_mid, x_fused=x_f, merged_dec=md, merged_attach=ma, txt=txt, txt_mask=tmask, txt_marginal=tmarg, vis_feat=vis_feat, sums=sums,
            viterbi_max=mx if dep_loss == "viterbi" else None, dep_score=mx, mt_loss=mt, heads=aux.get("heads")).items()}
        return loss, dict(zip(names, grads)), ()

    step.names, step.P, step.lengths, step.dep_loss, step.arc = names, P, lengths, dep_loss, arc
    # Teacher forcing (parity tests only; None = the reference's behaviour): with a tree given, lang_feat_max_tree reads ITS parents and
    # marginals, and the parser's loss is -score(that tree) instead of -max -- the same function of the parameters the reference
    # differentiates when its own Viterbi tree is that tree (joint.py:256-273 and ldndmv.py:277-281 treat the tree as a constant).  A bf16
    # run whose near-tied attachments flip is thereby compared on the reference's tree: rounding is separated from tree flips.
    step.forced_heads = forced_heads
    step.batch = dict(token=token, tag=tag, box_mask=box_mask, vis_mask=vmask, alpha=alpha, factor_names=factor_names, vis_split=vis_split,
                      factors=factors, pos_for=pos_for, use_pos_prior=use_pos_prior, vis2txt=vis2txt, enc_drop=enc_drop, p_enc=p_enc)
    step.shape = dict(B=B, L=L, R=R, V=V, d=d, h=h, E=E, n_vis=n_vis)
    step.trainable = tuple(k for k in names if k not in ("emb", "vis_box_feat"))
    # `step.on_grad(name, grad)`, if set, is called from inside the backward pass the moment a parameter's (accumulated) gradient exists;
    # step.ready_groups is the order in which that happens
    step.ready_groups = step_model.ready_groups(names)
    step.on_grad = None
    for k in step.trainable:
        P[k].register_hook(lambda g_, k=k: step.on_grad(k, g_) if step.on_grad is not None else None)
    return step

