"""The gold tree's DMV1o rule counts on the device -- the parser's loss during the rule-supervised initialisation epochs.

With `init_method: 'y'` (config/model/vlgae.yaml:75-76) the reference trains its first `init_epoch` epochs on batches of the
`train_init` set (datamodule/task/dep.py:139-166) with

    enll = -(gold['dec_rule'] * x['dec']).sum() - (gold['attach_rule'] * x['attach']).sum() - (gold['root_rule'] * x['root']).sum()

(src/model/ldndmv.py:262-275), the rule counts built on the host per sentence by generate_rule_1o (dmv_helper/good_init_nn.py:34-77,
wired at ldndmv.py:153-159) and padded as float64 arrays.  Here both halves are kernels (vlgae_amd/csrc/vlg_rules1o.hip; the counting
rules, the reference's `decision[-1]` quirk and the invalid-sentence convention are stated in include/vlgae_amd.h):

    gold_rules(arc, lengths, L)                   the three padded tables, bit-equal to the reference's fields
    gold_rule_score(md, ma, arc, lengths)         [B,1] per-sentence score on the ROOT-MERGED potentials, differentiable in both

so the drop-in line for ldndmv.py:273-275 is

    out['enll'] = -gold_rule_score(x['merged_dec'], x['merged_attach'], gold['arc'], vp.seq_len).sum()

(dec = merged_dec[:,1:], attach = merged_attach[:,1:,1:], root = merged_attach[:,0,1:,NOCHILD]: distributions.py:253-265).
GPU only, like the rest of the package.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _C

MAX_WORDS = 254   # N = L + 1 <= 255, as for the DP


def _arc_lengths(arc, lengths, what):
    _C.require_gpu(arc, what)
    if arc.dim() != 2:
        raise ValueError(f"{what}: arc must be [B, L] (1-based heads, 0 = root), got {tuple(arc.shape)}")
    B = arc.shape[0]
    if arc.dtype != torch.int64 or not arc.is_contiguous():
        arc = arc.to(torch.int64).contiguous()
    if not torch.is_tensor(lengths):
        lengths = torch.as_tensor(lengths)
    if lengths.dtype != torch.int64 or lengths.device != arc.device or not lengths.is_contiguous():
        lengths = lengths.to(device=arc.device, dtype=torch.int64).contiguous()
    if tuple(lengths.shape) != (B,):
        raise ValueError(f"{what}: lengths must have shape ({B},), got {tuple(lengths.shape)}")
    return arc, lengths


def gold_rules(arc, lengths, L, dtype=torch.float64):
    """generate_rule_1o (good_init_nn.py:34-77) of every sentence + LinearPadder / SquarePadder(0), in one launch.
    arc [B, >= max n] int64, lengths [B]; L = the padded width (the batch's max length for the reference's padders).
    Returns (dec_rule [B,L,2,2,2], attach_rule [B,L,L,2], root_rule [B,L]) in `dtype` (float64 like the reference, or float32).
    An invalid sentence (an arc outside [0, n], no arc 0, a length outside [1, L]) gets all-zero tables."""
    arc, lengths = _arc_lengths(arc, lengths, "gold_rules")
    L = int(L)
    if not 1 <= L <= MAX_WORDS:
        raise ValueError(f"gold_rules: L must be in [1, {MAX_WORDS}], got {L}")
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"gold_rules: dtype must be torch.float32 or torch.float64, got {dtype}")
    B = arc.shape[0]
    kw = dict(dtype=dtype, device=arc.device)
    dec, att, root = torch.empty((B, L, 2, 2, 2), **kw), torch.empty((B, L, L, 2), **kw), torch.empty((B, L), **kw)
    _C.check(_C.lib().vlg_dmv1o_gold_rules(_C.ptr(arc), max(1, arc.shape[1]), _C.ptr(lengths), B, L, _C.F64 if dtype == torch.float64 else _C.F32,
                                           _C.ptr(dec), _C.ptr(att), _C.ptr(root), _C.stream_of(arc)), "dmv1o_gold_rules")
    return dec, att, root


def _check_potentials(md, ma, B):
    if md.dim() != 5 or tuple(md.shape[2:]) != (2, 2, 2) or md.shape[0] != B:
        raise ValueError(f"gold_rule_score: merged_dec must be [B,N,2,2,2] with B = {B}, got {tuple(md.shape)}")
    N = md.shape[1]
    if tuple(ma.shape) != (B, N, N, 2):
        raise ValueError(f"gold_rule_score: merged_attach must be [B,N,N,2] = {(B, N, N, 2)}, got {tuple(ma.shape)}")
    if not 2 <= N <= MAX_WORDS + 1:
        raise ValueError(f"gold_rule_score: N = {N} outside [2, {MAX_WORDS + 1}]")
    return N


class _GoldRuleScore(torch.autograd.Function):
    """score[b] = sum(counts_b . potentials_b); backward = g[b] * counts_b written by one launch (no saved tensors but the batch)."""

    @staticmethod
    def forward(ctx, md, ma, arc, lengths):
        B = arc.shape[0]
        N = _check_potentials(md, ma, B)
        if ma.dtype != md.dtype:
            ma = ma.to(md.dtype)
        dt, md_c = _C.in_dtype(md)
        _, ma_c = _C.in_dtype(ma)
        score = torch.empty((B, 1), dtype=torch.float32, device=md.device)
        _C.check(_C.lib().vlg_dmv1o_gold_score(_C.ptr(md_c), _C.ptr(ma_c), _C.ptr(arc), max(1, arc.shape[1]), _C.ptr(lengths), B, N, dt,
                                               _C.ptr(score), _C.stream_of(md)), "dmv1o_gold_score")
        ctx.save_for_backward(arc, lengths)
        ctx.meta = (N, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        ctx.in_dtypes = (md.dtype, ma.dtype)
        return score.double() if md.dtype == torch.float64 else score

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        arc, lengths = ctx.saved_tensors
        N, want_d, want_a = ctx.meta
        if not (want_d or want_a):
            return None, None, None, None
        B = arc.shape[0]
        d0, d1 = ctx.in_dtypes
        out = d0 if d0 == d1 and d0 in (torch.float32, torch.bfloat16) else torch.float32
        g = grad_out if grad_out.dtype == torch.float32 else grad_out.float()
        stride = 1
        if g.dim() and g.stride() == (0,) * g.dim():
            stride = 0                                                 # the expanded scalar of `.sum()`
        elif not g.is_contiguous():
            g = g.contiguous()
        gd = torch.empty((B, N, 2, 2, 2), dtype=out, device=g.device)
        ga = torch.empty((B, N, N, 2), dtype=out, device=g.device)
        _C.check(_C.lib().vlg_dmv1o_gold_score_backward(_C.ptr(arc), max(1, arc.shape[1]), _C.ptr(lengths), B, N, _C.ptr(g), stride,
                                                        _C.BF16 if out == torch.bfloat16 else _C.F32, _C.ptr(gd), _C.ptr(ga), _C.stream_of(g)),
                 "dmv1o_gold_score_backward")
        return (gd.to(d0) if want_d else None), (ga.to(d1) if want_a else None), None, None


def gold_rule_score(merged_dec, merged_attach, arc, lengths):
    """Per-sentence score of the gold tree's rule counts under root-merged DMV1o potentials: [B,1] float32 (float64 for float64
    potentials), differentiable w.r.t. merged_dec [B,N,2,2,2] and merged_attach [B,N,N,2] (float32 / bfloat16; the adjoint is
    g[b] * counts, in the potentials' dtype).  Equals (dec_rule . dec + attach_rule . attach + root_rule . root) per sentence with the
    tables of `gold_rules`; only positions with a nonzero count are read.  An invalid sentence scores NaN with zero gradient."""
    _C.require_gpu(merged_dec, "gold_rule_score")
    arc, lengths = _arc_lengths(arc, lengths, "gold_rule_score")
    return _GoldRuleScore.apply(merged_dec, merged_attach, arc, lengths)
