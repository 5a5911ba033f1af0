"""Drop-in for the reference's `src/model/torch_struct/distributions.py` on the path VLGAE uses.

Same class names, constructor signatures, lazy properties, shapes and constants as the reference
(distributions.py:25-53,116-133,162-174,190-193,245-298), so `from vlgae_amd.torch_struct import
DMV1o, DependencyCRF` replaces `from src.model.torch_struct import DMV1o, DependencyCRF`
(ldndmv.py:21, joint.py:20, dmv.py:16) with no other change.  Every property evaluates through the
HIP kernels; there is no PyTorch implementation of the DP in this package.
"""
import torch
from torch import Tensor
from torch.distributions.distribution import Distribution
from torch.distributions.utils import lazy_property

from . import functional as F
from .dmv import NOCHILD, RIGHT  # noqa: F401  (re-exported like the reference)
from .semirings import NEGINF, LogSemiring, MaxSemiring


def _out_of_scope(name):
    raise NotImplementedError(
        f"StructDistribution.{name}: no caller in VLGAE uses it (only partition / max / argmax / marginals are "
        "reached; SURVEY.md section 2) -- outside the MI355X hot path this package implements.  (Drawing trees is "
        "implemented for DependencyCRF as `sample_heads` / `heads_to_parts` and for DMV1o as `sample_heads` / `log_prob_heads`; entropy, cross-entropy, KL and expected scores as "
        "`tree_entropy` / `tree_cross_entropy` / `tree_kl` / `expected_score` on DependencyCRF and, for the DMV, on DMV1oExpect; the k best trees as `kbest_heads` / `kbest_scores` on DependencyCRF and on DMV1o.  "
        "A DependencyCRF on labeled potentials [B,N,N,L] has all of these except the k best trees, and `argmax_labels` / "
        "`sample_heads(return_labels=True)` for the labels.)")


class StructDistribution(Distribution):
    """Base structured distribution (reference: distributions.py:25-243)."""

    has_enumerate_support = False
    struct = None

    def __init__(self, log_potentials, lengths=None, args={}):
        batch_shape = log_potentials.shape[:1]
        event_shape = log_potentials.shape[1:]
        self.log_potentials = log_potentials
        self.lengths = lengths
        self.args = args
        super().__init__(batch_shape=batch_shape, event_shape=event_shape, validate_args=False)

    # -- the four quantities VLGAE reads ------------------------------------------------------------
    def _sum(self, semiring):
        raise NotImplementedError

    def _marginals(self, semiring):
        raise NotImplementedError

    @lazy_property
    def partition(self):
        "Log-partition function (distributions.py:190-193)."
        return self._sum(LogSemiring)

    @lazy_property
    def max(self):
        "Score of the best structure (distributions.py:116-124)."
        return self._sum(MaxSemiring)

    @lazy_property
    def argmax(self):
        "Best structure as 0/1 parts = Max-semiring marginals (distributions.py:126-133)."
        return self._marginals(MaxSemiring)

    @lazy_property
    def marginals(self):
        "Posterior marginals of the parts (distributions.py:162-174)."
        return self._marginals(LogSemiring)

    @lazy_property
    def mode(self):
        return self.argmax

    # -- reference API with no caller in VLGAE ------------------------------------------------------
    @property
    def entropy(self):
        _out_of_scope("entropy")

    def cross_entropy(self, other):
        _out_of_scope("cross_entropy")

    def kl(self, other):
        _out_of_scope("kl")

    def risk(self, cost):
        _out_of_scope("risk")

    def kmax(self, k):
        _out_of_scope("kmax")

    def topk(self, k):
        _out_of_scope("topk")

    @property
    def count(self):
        _out_of_scope("count")

    def gumbel_crf(self, temperature=1.0):
        _out_of_scope("gumbel_crf")

    def sample(self, sample_shape=torch.Size()):
        _out_of_scope("sample")

    def enumerate_support(self, expand=True):
        _out_of_scope("enumerate_support")


class DMV1o(StructDistribution):
    """First-order DMV with valence (reference: distributions.py:245-265, dmv.py:18-69).

    log_potentials = [dec [B,N,2,2,2], attach [B,N,N,2]] (root-merged, see `merge`); lengths [B].
    partition / max: [B,1].  argmax / marginals: the attach part only, [B,N,N,2] (dmv.py:68-69).
    """

    def __init__(self, log_potentials, lengths, args={}):
        super().__init__(log_potentials[0], lengths=lengths, args=args)
        self.log_potentials = log_potentials

    def _sum(self, semiring):
        dec, attach = self.log_potentials
        return F.dmv1o_sum(dec, attach, self.lengths, semiring.kernel_id)

    def _marginals(self, semiring):
        # helpers.py:118-154 differentiates the semiring sum w.r.t. the potentials and keeps the attach
        # part; the fused kernel returns exactly that gradient.  (Not differentiable a second time:
        # no caller does -- inputs are always detached leaves, joint.py:252-253.)
        dec, attach = self.log_potentials
        _, _, gatt = F.dmv1o_run(dec, attach, self.lengths, semiring.kernel_id, True, want_dec=False)
        return gatt.to(attach.dtype) if attach.dtype == torch.float64 else gatt

    @lazy_property
    def argmax_heads(self):
        """Extension (not in the reference): the best tree as `predicted` heads [B,N], computed on the device.
        Same result as `arc = self.argmax.sum(-1).nonzero(); predicted[arc[:,0], arc[:,2]] = arc[:,1]`
        (joint.py:256-258) without the host synchronisation of `nonzero()`."""
        dec, attach = self.log_potentials
        return F.dmv1o_decode(dec, attach, self.lengths)[1]

    def marginals_and_heads(self, keep_viterbi=False, keep_partition=False):
        """Extension: (`marginals`, `argmax_heads`) with the two DPs overlapped on two HIP streams -- the pair
        lang_feat_max_tree asks for every step (joint.py:251-258).  keep_viterbi=True: the Viterbi pass also produces the
        tree counts and is remembered, so a later `DMV1o(same potentials).max` (the parser's `-max` loss, ldndmv.py:277-281)
        and its backward launch nothing (see functional.dmv1o_marginals_and_heads).  keep_partition=True: the same for `.partition` (the
        parser's marginal loss, ldndmv.py:280-281): the inside-outside pass also writes the dec counts and is remembered."""
        dec, attach = self.log_potentials
        _, gatt, heads = F.dmv1o_marginals_and_heads(dec, attach, self.lengths, keep_viterbi, keep_partition)
        return gatt, heads

    def marginals_and_heads_async(self, keep_viterbi=False):
        """`marginals_and_heads` with BOTH DPs on side streams: returns a handle at once; `handle.wait()` -> (logZ, marginals,
        heads) joins them into the current stream.  Work enqueued in between overlaps the DPs (functional.dmv1o_structure_async)."""
        dec, attach = self.log_potentials
        return F.dmv1o_structure_async(dec, attach, self.lengths, keep_viterbi)

    def sample_heads(self, n, rng=None, u=None, return_log_prob=False):
        """Extension (not in the reference): n trees per sentence drawn from the distribution, as heads [n,B,N] int64 on the device
        (heads[s,b,c] = head of word c, 0 for c = 0 and padding) -- one kernel launch, no host synchronisation.  The semantics of
        `DependencyCRF.sample_heads`: `rng` an `encoders.DeviceRng` whose (seed, step) keys the draws (the caller advances it), `u`
        explicit uniforms [n,B,3,N,N] instead; with neither, the distribution creates and keeps a DeviceRng seeded from
        `torch.initial_seed()` and advances it after each call.  return_log_prob=True: (heads, log_prob [n,B]).  The reference's
        `sample(sample_shape)` (distributions.py:195-217) stays out of scope under that name."""
        dec, attach = self.log_potentials
        own = rng is None and u is None
        if own:
            if getattr(self, "_sample_rng", None) is None:
                from ..encoders import DeviceRng
                self._sample_rng = DeviceRng(torch.initial_seed() & 0x7FFFFFFFFFFFFFFF, dec.device)
            rng = self._sample_rng
        heads, logp, _ = F.dmv1o_sample(dec, attach, self.lengths, n, rng=rng, u=u, want_logp=return_log_prob)
        if own:
            rng.advance()
        return (heads, logp) if return_log_prob else heads

    def log_prob_heads(self, heads):
        """Extension: log p(tree) for head vectors [..., B, N] -> [..., B]: the tree's score (every attachment with its valence and GO
        decision, every STOP) minus `partition`.  Differentiable once with respect to both potentials: the gradient is the tree's
        counts minus the expected counts -- the score-function estimator's term for trees drawn by `sample_heads`."""
        dec, attach = self.log_potentials
        return F.dmv1o_log_prob_heads(dec, attach, self.lengths, heads)

    # -- k-best trees (extension: one launch, functional.dmv1o_kbest).  The reference's `kmax(k)` / `topk(k)` cannot run on a DMV1o at all
    # (KMaxSemiring.sum has no reduction over dimension -2, semirings.py:251) and stay out of scope under those names.
    def kbest_heads(self, k, return_scores=False):
        """The k best trees (1 <= k <= 16) as heads [k,B,N] int64 on the device: k different trees per sentence, also under exact
        ties, best first -- n-best parses for reranking, oracle attachment scores, a look at how peaked the posterior is.
        return_scores=True: (heads, scores [k,B] float32, count [B] int32) -- a sentence with fewer than k trees has count < k, and
        its ranks at or beyond count hold score NEGINF and heads 0.  Row 0 is `argmax_heads` wherever the best tree is unique."""
        dec, attach = self.log_potentials
        heads, scores, count = F.dmv1o_kbest(dec, attach, self.lengths, k)
        return (heads, scores, count) if return_scores else heads

    def kbest_scores(self, k):
        """Scores [k,B] of the k best trees, non-increasing in k (NEGINF where the rank does not exist); scores[0] is `max` up to the
        rounding of its log2-unit arithmetic.  Differentiable once with respect to both potentials: the gradient of scores[k,b] is
        tree (k,b)'s derivation counts (every attachment with its valence and GO decision, every STOP)."""
        dec, attach = self.log_potentials
        return F.dmv1o_kbest_scores(dec, attach, self.lengths, k)[0]

    @staticmethod
    def merge(dec: Tensor, attach: Tensor, root: Tensor, one=0, zero=NEGINF):
        """Root-augmented potentials (distributions.py:253-265): the root is token 0, generates only to
        the right, takes exactly the `root` scores with valence NOCHILD; everything else is `zero`."""
        return F.dmv1o_merge_autograd(dec, attach, root, one, zero)


class DMV1oExpect(DMV1o):
    """Extension (not in the reference): `DMV1o` with the expectation methods `DependencyCRF` has -- same constructor, same properties.
    A class of its own: the surface of `DMV1o` is unchanged.  One dual-number inside-outside launch per distribution
    (functional.dmv1o_expect), exact gradients.  The reference's names (`entropy`, `cross_entropy`, `kl`, `risk`,
    distributions.py:79-114) stay out of scope under those names.  All return [B,1] like `partition` and are differentiable once with
    respect to every potential; `other` may be any `DMV1o` over the same sentences."""

    def expected_score(self, cost):
        """E_p[<cost, tree>] for cost = (cost_dec [B,N,2,2,2], cost_attach [B,N,N,2]), either may be None: the reference's
        `risk([cost_dec, cost_attach])`.  Gradient with respect to the cost: the expected counts."""
        dec, attach = self.log_potentials
        return F.dmv1o_expected_score(dec, attach, self.lengths, cost[0], cost[1])

    def tree_entropy(self):
        "H[p]: the reference's `entropy`."
        dec, attach = self.log_potentials
        return F.dmv1o_entropy(dec, attach, self.lengths)

    def tree_cross_entropy(self, other):
        "H[p, q] with q = `other` (a DMV1o over the same sentences): the reference's `cross_entropy(other)`."
        dec, attach = self.log_potentials
        return F.dmv1o_cross_entropy(dec, attach, other.log_potentials[0], other.log_potentials[1], self.lengths)

    def tree_kl(self, other):
        "KL[p || q] = H[p, q] - H[p]; exactly 0 with zero gradients when both hold the same potentials."
        dec, attach = self.log_potentials
        return F.dmv1o_kl(dec, attach, other.log_potentials[0], other.log_potentials[1], self.lengths)


class DMV1oRules(StructDistribution):
    """Extension: the DMV of `DMV1o`, parameterised by the scorer's rule tables instead of
    merged per-position potentials.  It replaces this block of DiscriminativeNDMV._forward + loss
    (src/model/ldndmv.py:185-209, 277-281)

        attach = attach_rule.gather(2, token...)  -> tril/triu direction select -> function mask
        root   = root_rule.gather(1, token);  merged = DMV1o.merge(dec, attach, root);  DMV1o(merged, lengths)

    with one kernel launch that gathers inside its load stage and returns gradients in rule space.

      attach_rule [B,L,T,2(dir),2(valence)]   log-probs over the T child tokens (ldndmv.py:185)
      dec         [B,L,2,2,2]                 root_rule [T] / [1,T] / [B,T]      token [B,L] int64
      head_mask   [B,L] bool, True = the word takes no children (`function_mask`, ldndmv.py:194-198)
    partition / max: [B,1], differentiable w.r.t. attach_rule, dec, root_rule.  argmax_heads: [B,L+1]."""

    def __init__(self, attach_rule, dec, root_rule, token, lengths, head_mask=None, mask_fill=-1e20, args={}):
        super().__init__(dec, lengths=lengths, args=args)
        self.log_potentials = [attach_rule, dec, root_rule]
        self.token, self.head_mask, self.mask_fill = token, head_mask, mask_fill

    def _sum(self, semiring):
        a, d, r = self.log_potentials
        return F.dmv1o_rules_sum(a, d, r, self.token, self.lengths, self.head_mask, semiring.kernel_id, self.mask_fill)

    def _marginals(self, semiring):
        "Rule-space expected counts (Log) or best-tree rule indicators (Max): the attach_rule part."
        a, d, r = self.log_potentials
        return F.dmv1o_rules_run(a, d, r, self.token, self.lengths, semiring.kernel_id, True, self.head_mask,
                                 False, self.mask_fill)["grad_rule"]

    @lazy_property
    def argmax_heads(self):
        a, d, r = self.log_potentials
        return F.dmv1o_rules_run(a, d, r, self.token, self.lengths, MaxSemiring.kernel_id, False, self.head_mask, True,
                                 self.mask_fill)["heads"]


class DependencyCRF(StructDistribution):
    """Projective single-root dependency CRF (reference: distributions.py:269-298, deptree.py:14-76).

    log_potentials [B,N,N] head -> child with the root at index 0; lengths [B] or None (= N-1).
    partition / max: [B].  argmax / marginals: [B,N,N].

    Labeled: log_potentials [B,N,N,L] head x child x label, 1 <= L <= 255 (deptree.py:19,33-41: the label axis is summed in the
    semiring in front of the DP).  partition / max: [B].  argmax / marginals: [B,N,N,L].  Every extension below takes the labeled
    shape too, except the k best trees; `argmax_labels` and `sample_heads(return_labels=True)` give the labels.
    """

    def __init__(self, log_potentials, lengths=None, args={}, multiroot=False):
        super().__init__(log_potentials, lengths, args)
        assert not multiroot, "multiroot is asserted False by the reference's DP (deptree.py:26-27)"
        self.multiroot = multiroot
        self.labeled = log_potentials.dim() == 4

    def _sum(self, semiring):
        if self.labeled:
            return F.deptree_labeled_sum(self.log_potentials, self.lengths, semiring.kernel_id)
        return F.deptree_sum(self.log_potentials, self.lengths, semiring.kernel_id)

    def _marginals(self, semiring):
        arc = self.log_potentials
        if self.labeled:
            garc = F.deptree_labeled_marginals(arc, self.lengths, semiring.kernel_id)
        else:
            _, garc = F.deptree_run(arc, self.lengths, semiring.kernel_id, True)
        return garc.to(arc.dtype) if arc.dtype == torch.float64 else garc

    @lazy_property
    def _labeled_decode(self):
        return F.deptree_labeled_decode(self.log_potentials, self.lengths)

    @lazy_property
    def argmax_heads(self):
        "Extension: best tree as heads [B,N] on the device (see DMV1o.argmax_heads; MBR decode of ldndmv.py:294-303)."
        if self.labeled:
            return self._labeled_decode[1]
        return F.deptree_decode(self.log_potentials, self.lengths)[1]

    @lazy_property
    def argmax_labels(self):
        """Extension, labeled potentials only: the labels of the best labeled tree, [B,N] int64 on the device -- labels[b,c] is the
        label of the arc `argmax_heads[b,c]` -> c, 0 at c = 0 and in padding.  No host synchronisation."""
        if not self.labeled:
            raise ValueError("argmax_labels: the potentials are unlabeled ([B,N,N]); labeled potentials are [B,N,N,L]")
        return self._labeled_decode[2]

    def _no_labeled_kbest(self):
        raise NotImplementedError(
            "DependencyCRF.kbest_heads / kbest_scores on labeled potentials [B,N,N,L]: the k best *labeled* trees need a K-list of "
            "(score, label) per arc inside the k-best chart (two trees of one shape may differ in a label only), and that chart is not "
            "built.  `kbest_heads` on `potentials.logsumexp(-1)` or `.max(-1).values` ranks the unlabeled trees.")

    def sample_heads(self, n, rng=None, u=None, return_log_prob=False, return_labels=False, u_label=None):
        """Extension (not in the reference): n trees per sentence drawn from the distribution, as heads [n,B,N] int64 on the device
        (heads[s,b,c] = head of word c, 0 for c = 0 and padding) -- one kernel launch, no host synchronisation.  `rng`: an
        `encoders.DeviceRng` whose (seed, step) keys the draws (the same state gives the same trees; the caller advances it);
        `u`: explicit uniforms [n,B,3,N,N] instead.  With neither, the distribution creates and keeps a DeviceRng seeded from
        `torch.initial_seed()` and advances it after each call.  return_log_prob=True: (heads, log_prob [n,B]).
        The reference's `sample(sample_shape)` (distributions.py:195-217) stays out of scope under that name -- it raises, as every
        other unreached method does; `DependencyCRF.heads_to_parts(dist.sample_heads(n))` is its event format.
        Labeled potentials: the tree is drawn from the label-summed arc scores and, with return_labels=True, every arc's label from
        the softmax over its labels: (heads, labels [n,B,N] int64[, log_prob]) -- labels 0 at c = 0 and in padding; log_prob is then
        the labeled tree's.  Explicit uniforms come as the pair `u`, `u_label` [n,B,N]."""
        if (return_labels or u_label is not None) and not self.labeled:
            raise ValueError("sample_heads: labels need labeled potentials [B,N,N,L]")
        if u_label is not None and not return_labels:
            raise ValueError("sample_heads: u_label draws the labels; pass return_labels=True with it")
        own = rng is None and u is None
        if own:
            if getattr(self, "_sample_rng", None) is None:
                from ..encoders import DeviceRng
                self._sample_rng = DeviceRng(torch.initial_seed() & 0x7FFFFFFFFFFFFFFF, self.log_potentials.device)
            rng = self._sample_rng
        if self.labeled and return_labels:
            heads, labels, logp, _ = F.deptree_labeled_sample(self.log_potentials, self.lengths, n, rng=rng, u=u, u_label=u_label,
                                                              want_logp=return_log_prob)
        else:   # (labeled without labels: the marginal over the labels is the tree distribution of the folded arc scores)
            arc = F.label_fold(self.log_potentials.detach(), self.lengths, 0)[0] if self.labeled else self.log_potentials
            heads, logp, _ = F.deptree_sample(arc, self.lengths, n, rng=rng, u=u, want_logp=return_log_prob)
        if own:
            rng.advance()
        out = (heads, labels) if return_labels else (heads,)
        out = out + (logp,) if return_log_prob else out
        return out if len(out) > 1 else out[0]

    # -- k-best trees (extension: one launch, functional.deptree_kbest).  The reference's `kmax(k)` / `topk(k)` (distributions.py:135-156)
    # stay out of scope under those names, as `sample` does next to `sample_heads`.
    def kbest_heads(self, k, return_scores=False):
        """The k best trees (1 <= k <= 16) as heads [k,B,N] int64 on the device: k different trees per sentence, also under exact
        ties, best first; `DependencyCRF.heads_to_parts(dist.kbest_heads(k), lengths)` is the event format of the reference's
        `topk(k)`.  return_scores=True: (heads, scores [k,B] float32, count [B] int32) -- a sentence with fewer than k trees has
        count < k, and its ranks at or beyond count hold score NEGINF and heads 0."""
        if self.labeled:
            self._no_labeled_kbest()
        heads, scores, count = F.deptree_kbest(self.log_potentials, self.lengths, k)
        return (heads, scores, count) if return_scores else heads

    def kbest_scores(self, k):
        """Scores [k,B] of the k best trees, non-increasing in k: the reference's `kmax(k)` wherever the rank exists (NEGINF where it
        does not).  Differentiable once with respect to the potentials: the gradient of scores[k,b] is tree (k,b)'s arc indicators."""
        if self.labeled:
            self._no_labeled_kbest()
        return F.deptree_kbest_scores(self.log_potentials, self.lengths, k)[0]

    # -- expectations (extension: one dual-number inside-outside launch each, exact gradients; functional.deptree_expect) ------------
    # The reference's names (`entropy`, `cross_entropy`, `kl`, `risk`, distributions.py:79-114) stay out of scope under those names,
    # as `sample` does next to `sample_heads`.  All return [B] and are differentiable once with respect to every potential.
    def expected_score(self, cost):
        "E_p[<cost, tree>] for arc costs [B,N,N] (labeled: [B,N,N,L]): the reference's `risk(cost)`."
        if self.labeled:
            return F.deptree_labeled_expected_score(self.log_potentials, self.lengths, cost)
        return F.deptree_expected_score(self.log_potentials, self.lengths, cost)

    def tree_entropy(self):
        "H[p]: the reference's `entropy`."
        if self.labeled:
            return F.deptree_labeled_entropy(self.log_potentials, self.lengths)
        return F.deptree_entropy(self.log_potentials, self.lengths)

    def tree_cross_entropy(self, other):
        "H[p, q] with q = `other` (a DependencyCRF over the same sentences): the reference's `cross_entropy(other)`."
        if self.labeled:
            return F.deptree_labeled_cross_entropy(self.log_potentials, other.log_potentials, self.lengths)
        return F.deptree_cross_entropy(self.log_potentials, other.log_potentials, self.lengths)

    def tree_kl(self, other):
        "KL[p || q] = H[p, q] - H[p]; exactly 0 with zero gradients when both hold the same potentials."
        if self.labeled:
            return F.deptree_labeled_kl(self.log_potentials, other.log_potentials, self.lengths)
        return F.deptree_kl(self.log_potentials, other.log_potentials, self.lengths)

    @staticmethod
    def heads_to_parts(heads, lengths=None, labels=None, num_labels=None):
        """Extension: head vectors [..., B, N] -> 0/1 float32 arc indicators [..., B, N, N] (parts[..., h, c] = 1 iff h is the head of
        word c, 1 <= c <= length; lengths None = N - 1) on the heads' device: the event format of the reference's `sample` /
        `to_parts` (deptree.py:163-186), which `log_prob` accepts.  With `labels` [..., B, N] (and num_labels = L, which no device
        tensor can tell without a host synchronisation): [..., B, N, N, L], parts[..., h, c, l] = 1 iff also l is the label of word c."""
        if labels is not None:
            if num_labels is None:
                raise ValueError("heads_to_parts: labels need num_labels")
            arcs = DependencyCRF.heads_to_parts(heads, lengths)
            hot = torch.nn.functional.one_hot(labels, int(num_labels)).to(torch.float32)   # [..., B, N(child), L]
            return arcs.unsqueeze(-1) * hot.unsqueeze(-3)
        N = heads.shape[-1]
        pos = torch.arange(N, device=heads.device)
        if lengths is None:
            word = (pos >= 1).expand(heads.shape)
        else:
            ln = torch.as_tensor(lengths, device=heads.device).to(torch.int64)
            word = (pos >= 1) & (pos <= ln.unsqueeze(-1))
            word = word.expand(heads.shape)
        parts = torch.zeros(heads.shape + (N,), dtype=torch.float32, device=heads.device)
        return parts.scatter_(-2, heads.unsqueeze(-2), word.to(torch.float32).unsqueeze(-2))

    def log_prob(self, value):
        "log p(tree) for 0/1 arc indicators `value` [..., B, N, N] (labeled: [..., B, N, N, L]) (distributions.py:55-75)."
        score = (self.log_potentials * value.type_as(self.log_potentials)).flatten(-3 if self.labeled else -2).sum(-1)
        return score - self.partition
