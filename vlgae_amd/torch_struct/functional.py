"""Autograd-aware entry points over the C ABI (include/vlgae_amd.h).

The reference differentiates its inside loop with autograd (hundreds of AsStridedBackward nodes per
call).  Here the outside pass is part of the same kernel launch as the inside
pass: when any potential requires grad, forward() runs the fused inside+outside kernel and keeps the
unit-upstream expected counts; backward() only scales them by the incoming gradient of logZ.
"""
import threading
import warnings

import torch
from torch.autograd.function import once_differentiable

from .. import _C
from .semirings import NEGINF


_WS_BYTES = {}


def _workspace(op, B, N, semiring, device):
    key = (op, B, N, semiring)
    nbytes = _WS_BYTES.get(key)
    if nbytes is None:
        nbytes = _WS_BYTES[key] = _C.lib().vlg_workspace_bytes(op, B, N, semiring)
    if nbytes == 0:
        return None, 0
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def _lengths(lengths, B, device, allow_none=False):
    if lengths is None:
        if allow_none:
            return None
        raise ValueError("lengths is required")
    if not torch.is_tensor(lengths):
        lengths = torch.as_tensor(lengths)
    if lengths.dtype != torch.int64 or lengths.device != device or not lengths.is_contiguous():
        lengths = lengths.to(device=device, dtype=torch.int64).contiguous()
    if lengths.shape != (B,):
        raise ValueError(f"lengths must have shape ({B},), got {tuple(lengths.shape)}")
    return lengths


def dmv1o_run(dec, attach, lengths, semiring, want_grad, grad_logZ=None, want_dec=True, logZ_shape=None, out=None):
    """Raw launcher.  dec [B,N,2,2,2], attach [B,N,N,2] -> logZ [B] (+ grad_dec, grad_attach fp32).
    want_dec=False: attach counts only (grad_dec is None; the Max semiring then takes the back-pointer walk)."""
    _C.require_gpu(dec, "dmv1o")
    if dec.dim() != 5 or tuple(dec.shape[2:]) != (2, 2, 2):
        raise ValueError(f"dec must be [B,N,2,2,2], got {tuple(dec.shape)}")
    B, N = dec.shape[:2]
    if tuple(attach.shape) != (B, N, N, 2):
        raise ValueError(f"attach must be [B,N,N,2] = {(B, N, N, 2)}, got {tuple(attach.shape)}")
    if dec.dtype != attach.dtype:
        attach = attach.to(dec.dtype)
    dt, dec_c = _C.in_dtype(dec)          # only the storage is read: no detach needed
    _, att_c = _C.in_dtype(attach)
    lengths = _lengths(lengths, B, dec.device)
    L = _C.lib()
    if out is not None:   # caller-owned outputs (allocated on the caller's stream before it switched to a side stream)
        logZ, gdec, gatt = out
    else:
        logZ = torch.empty(logZ_shape or B, dtype=torch.float32, device=dec.device)
    if want_grad:
        if out is None:
            gdec = torch.empty((B, N, 2, 2, 2), dtype=torch.float32, device=dec.device) if want_dec else None
            gatt = torch.empty((B, N, N, 2), dtype=torch.float32, device=dec.device)
        ws, nb = _workspace(_C.OP_DMV1O_INSIDE_OUTSIDE, B, N, semiring, dec.device)
        g = None if grad_logZ is None else grad_logZ.detach().to(torch.float32).reshape(B).contiguous()
        _C.check(L.vlg_dmv1o_inside_outside(_C.ptr(dec_c), _C.ptr(att_c), _C.ptr(lengths), B, N, dt, semiring,
                                            _C.ptr(g), _C.ptr(logZ), _C.ptr(gdec), _C.ptr(gatt), _C.ptr(ws), nb,
                                            _C.stream_of(dec)), "dmv1o_inside_outside")
        return logZ, gdec, gatt
    ws, nb = _workspace(_C.OP_DMV1O_INSIDE, B, N, semiring, dec.device)
    _C.check(L.vlg_dmv1o_inside(_C.ptr(dec_c), _C.ptr(att_c), _C.ptr(lengths), B, N, dt, semiring, _C.ptr(logZ),
                                _C.ptr(ws), nb, _C.stream_of(dec)), "dmv1o_inside")
    return logZ, None, None


def deptree_run(arc, lengths, semiring, want_grad, grad_logZ=None):
    """Raw launcher.  arc [B,N,N] -> logZ [B] (+ grad_arc fp32)."""
    _C.require_gpu(arc, "deptree")
    if arc.dim() != 3:
        raise ValueError("potentials must have dim of 3 (unlabeled)")   # deptree.py:30-31 (labeled potentials go through deptree_labeled_*, which fold them to arc scores first)
    B, N, N2 = arc.shape
    assert N == N2, "Non-square potentials"                              # deptree.py:149
    dt, arc_c = _C.in_dtype(arc)
    lengths = _lengths(lengths, B, arc.device, allow_none=True)
    logZ = torch.empty(B, dtype=torch.float32, device=arc.device)
    L = _C.lib()
    if want_grad:
        garc = torch.empty((B, N, N), dtype=torch.float32, device=arc.device)
        ws, nb = _workspace(_C.OP_DEPTREE_INSIDE_OUTSIDE, B, N, semiring, arc.device)
        g = None if grad_logZ is None else grad_logZ.detach().to(torch.float32).reshape(B).contiguous()
        _C.check(L.vlg_deptree_inside_outside(_C.ptr(arc_c), _C.ptr(lengths), B, N, dt, semiring, _C.ptr(g),
                                              _C.ptr(logZ), _C.ptr(garc), _C.ptr(ws), nb, _C.stream_of(arc)),
                 "deptree_inside_outside")
        return logZ, garc
    ws, nb = _workspace(_C.OP_DEPTREE_INSIDE, B, N, semiring, arc.device)
    _C.check(L.vlg_deptree_inside(_C.ptr(arc_c), _C.ptr(lengths), B, N, dt, semiring, _C.ptr(logZ), _C.ptr(ws), nb,
                                  _C.stream_of(arc)), "deptree_inside")
    return logZ, None


def dmv1o_decode(dec, attach, lengths, out=None):
    """Viterbi tree as a head vector, entirely on the device (no `nonzero()` host sync).
    Returns (best_score [B], heads [B,N] int64): heads[b,c] = head of word c (0 = root token); 0 at c = 0 / padding.
    Equals `predicted` of src/model/joint.py:256-258 and, shifted by one, of ldndmv.py:301-303."""
    _C.require_gpu(dec, "dmv1o_decode")
    B, N = dec.shape[:2]
    if tuple(dec.shape) != (B, N, 2, 2, 2) or tuple(attach.shape) != (B, N, N, 2):
        raise ValueError(f"dec {tuple(dec.shape)} / attach {tuple(attach.shape)}: expected [B,N,2,2,2] / [B,N,N,2]")
    if dec.dtype != attach.dtype:
        attach = attach.to(dec.dtype)
    dt, dec_c = _C.in_dtype(dec)
    _, att_c = _C.in_dtype(attach)
    lengths = _lengths(lengths, B, dec.device)
    if out is None:
        best = torch.empty(B, dtype=torch.float32, device=dec.device)
        heads = torch.empty((B, N), dtype=torch.int64, device=dec.device)
    else:   # caller-owned outputs (dmv1o_marginals_and_heads allocates them on ITS stream before switching to the side stream)
        best, heads = out
    ws, nb = _workspace(_C.OP_DMV1O_INSIDE_OUTSIDE, B, N, _C.SEMIRING_MAX, dec.device)
    _C.check(_C.lib().vlg_dmv1o_decode(_C.ptr(dec_c), _C.ptr(att_c), _C.ptr(lengths), B, N, dt, _C.ptr(best),
                                       _C.ptr(heads), _C.ptr(ws), nb, _C.stream_of(dec)), "dmv1o_decode")
    return best, heads


def dmv1o_viterbi(dec, attach, lengths, out=None):
    """The Max semiring's every output in one launch: (best [B], grad_dec [B,N,2,2,2], grad_attach [B,N,N,2], heads [B,N]).
    The counts are the 0/1 indicators of the best tree (unit upstream gradient) -- what `-DMV1o(...).max.sum()`
    back-propagates (ldndmv.py:277-281) -- and heads is `argmax` as a head vector (joint.py:256-258)."""
    _C.require_gpu(dec, "dmv1o_viterbi")
    B, N = dec.shape[:2]
    if tuple(dec.shape) != (B, N, 2, 2, 2) or tuple(attach.shape) != (B, N, N, 2):
        raise ValueError(f"dec {tuple(dec.shape)} / attach {tuple(attach.shape)}: expected [B,N,2,2,2] / [B,N,N,2]")
    if dec.dtype != attach.dtype:
        attach = attach.to(dec.dtype)
    dt, dec_c = _C.in_dtype(dec)
    _, att_c = _C.in_dtype(attach)
    lengths = _lengths(lengths, B, dec.device)
    if out is None:
        best = torch.empty(B, dtype=torch.float32, device=dec.device)
        gdec = torch.empty((B, N, 2, 2, 2), dtype=torch.float32, device=dec.device)
        gatt = torch.empty((B, N, N, 2), dtype=torch.float32, device=dec.device)
        heads = torch.empty((B, N), dtype=torch.int64, device=dec.device)
    else:
        best, gdec, gatt, heads = out
    ws, nb = _workspace(_C.OP_DMV1O_INSIDE_OUTSIDE, B, N, _C.SEMIRING_MAX, dec.device)
    _C.check(_C.lib().vlg_dmv1o_viterbi(_C.ptr(dec_c), _C.ptr(att_c), _C.ptr(lengths), B, N, dt, None, _C.ptr(best), _C.ptr(gdec),
                                        _C.ptr(gatt), _C.ptr(heads), _C.ptr(ws), nb, _C.stream_of(dec)), "dmv1o_viterbi")
    return best, gdec, gatt, heads


# ---- one Viterbi pass per training step ------------------------------------------------------------------------------------
# lang_feat_max_tree takes `argmax` of the step's potentials (joint.py:256) and the parser's loss takes `-max` of the SAME
# values a few lines later (ldndmv.py:277-281, through a different DMV1o object built on `.detach()`ed aliases).  When the
# first caller asks for it (`marginals_and_heads(keep_viterbi=True)`), the full Viterbi result is remembered here, keyed by
# the identity of the storage it was computed from: the key tensors are kept alive (so their addresses cannot be handed to
# other data) and their version counters are compared (so an in-place update through any alias invalidates the entry; only
# torch operations count -- a raw pointer write by foreign code is invisible, which is why nothing is remembered unasked).
_VITERBI = {}


def _viterbi_key(dec, attach, lengths):
    return (dec.data_ptr(), attach.data_ptr(), lengths.data_ptr(), dec._version, attach._version, lengths._version,
            tuple(dec.shape), dec.dtype, tuple(dec.stride()), tuple(attach.stride()))


def _viterbi_remember(dec, attach, lengths, result, pending=None):
    """pending: the StructureHandle whose side stream is still producing `result` -- a hit joins it into the CURRENT stream
    before the tensors are handed out, so a `.max` taken before (or on another stream than) `handle.wait()` is ordered too."""
    _VITERBI[dec.device] = (_viterbi_key(dec, attach, lengths), (dec.detach(), attach.detach(), lengths), result, pending)


def _viterbi_lookup(dec, attach, lengths):
    if not isinstance(lengths, torch.Tensor):
        return None
    hit = _VITERBI.get(dec.device)
    if hit is None or hit[0] != _viterbi_key(dec, attach, lengths):
        return None
    if hit[3] is not None:
        hit[3].join_current()
    return hit[2]


def viterbi_forget():
    """Drop the remembered Viterbi and partition results (and the references that keep their potentials alive)."""
    _VITERBI.clear()
    _PARTITION.clear()


# The same for the Log semiring: with the marginal loss (`viterbi_training: false`, ldndmv.py:280-281) the parser takes
# `-DMV1o(...).partition.sum()` of the potentials whose inside-outside pass lang_feat_max_tree has just run for the arc marginals
# (joint.py:251-255).  `marginals_and_heads(keep_partition=True)` remembers (logZ, grad_dec, grad_attach) under the key discipline above,
# so that `.partition` and its backward launch no DP.
_PARTITION = {}


def _partition_remember(dec, attach, lengths, result):
    _PARTITION[dec.device] = (_viterbi_key(dec, attach, lengths), (dec.detach(), attach.detach(), lengths), result)


def _partition_lookup(dec, attach, lengths):
    if not isinstance(lengths, torch.Tensor):
        return None
    hit = _PARTITION.get(dec.device)
    if hit is None or hit[0] != _viterbi_key(dec, attach, lengths):
        return None
    return hit[2]


def deptree_decode(arc, lengths=None):
    """Best projective single-root tree of arc scores [B,N,N] as heads [B,N] (see dmv1o_decode).  With `arc` = arc
    marginals this is the MBR decode of src/model/ldndmv.py:294-299."""
    _C.require_gpu(arc, "deptree_decode")
    B, N, N2 = arc.shape
    assert N == N2, "Non-square potentials"
    dt, arc_c = _C.in_dtype(arc)
    lengths = _lengths(lengths, B, arc.device, allow_none=True)
    best = torch.empty(B, dtype=torch.float32, device=arc.device)
    heads = torch.empty((B, N), dtype=torch.int64, device=arc.device)
    ws, nb = _workspace(_C.OP_DEPTREE_INSIDE_OUTSIDE, B, N, _C.SEMIRING_MAX, arc.device)
    _C.check(_C.lib().vlg_deptree_decode(_C.ptr(arc_c), _C.ptr(lengths), B, N, dt, _C.ptr(best), _C.ptr(heads),
                                         _C.ptr(ws), nb, _C.stream_of(arc)), "deptree_decode")
    return best, heads


def _sample_frame(name, device, B, N, n, rng, site, u, want_logp):
    """What deptree_sample and dmv1o_sample share: exactly one of rng and u, the shape of u, the outputs heads [n,B,N] / logp [n,B]
    or None / logZ [B], and the C arguments `rng, site, u, heads, logp, logZ` of vlg_*_sample.  Returns (heads, logp, logZ, u, args);
    u is the contiguous table the arguments point into."""
    if (rng is None) == (u is None):
        raise ValueError(f"{name}: pass exactly one of rng and u")
    if u is not None:
        if tuple(u.shape) != (n, B, 3, N, N) or u.dtype != torch.float32 or u.device != device:
            raise ValueError(f"{name}: u must be float32 [n,B,3,N,N] = {(n, B, 3, N, N)} on {device}")
        u = u.contiguous()
    heads = torch.empty((n, B, N), dtype=torch.int64, device=device)
    logp = torch.empty((n, B), dtype=torch.float32, device=device) if want_logp else None
    logZ = torch.empty(B, dtype=torch.float32, device=device)
    args = (None if rng is None else _C.ptr(rng.state), int(site), _C.ptr(u), _C.ptr(heads), _C.ptr(logp), _C.ptr(logZ))
    return heads, logp, logZ, u, args


def deptree_sample(arc, lengths, n, rng=None, site=0, u=None, want_logp=True):
    """n trees per sentence drawn from the projective CRF of arc scores [B,N,N], in ONE launch (vlg_deptree_sample):
    (heads [n,B,N] int64 as deptree_decode writes them, logp [n,B] float32 or None, logZ [B]).  The uniforms come either from
    `rng` (an encoders.DeviceRng: Philox draws off its device-resident (seed, step), `site` as for the dropout layers) or from the explicit
    table `u` [n,B,3,N,N] float32, read at [s,b,kind,lo,hi] (common random numbers, antithetic draws); exactly one of the two."""
    _C.require_gpu(arc, "deptree_sample")
    if arc.dim() != 3:
        raise ValueError("potentials must have dim of 3 (unlabeled)")
    B, N, N2 = arc.shape
    assert N == N2, "Non-square potentials"
    n = int(n)
    dt, arc_c = _C.in_dtype(arc)
    lengths = _lengths(lengths, B, arc.device, allow_none=True)
    heads, logp, logZ, u, args = _sample_frame("deptree_sample", arc.device, B, N, n, rng, site, u, want_logp)
    L = _C.lib()
    blocks = L.vlg_deptree_sample_blocks(B, N, n) if B > 0 and n > 0 else 1
    ws, nb = _workspace(_C.OP_DEPTREE_INSIDE, B * blocks, N, _C.SEMIRING_LOG, arc.device)
    _C.check(L.vlg_deptree_sample(_C.ptr(arc_c), _C.ptr(lengths), B, N, dt, n, *args, _C.ptr(ws), nb, _C.stream_of(arc)), "deptree_sample")
    return heads, logp, logZ


def dmv1o_sample(dec, attach, lengths, n, rng=None, site=0, u=None, want_logp=True):
    """n trees per sentence drawn from the DMV of root-merged potentials dec [B,N,2,2,2] / attach [B,N,N,2], in ONE launch
    (vlg_dmv1o_sample): (heads [n,B,N] int64 as dmv1o_decode writes them, logp [n,B] float32 or None, logZ [B]).  The uniforms come
    either from `rng` (an encoders.DeviceRng, `site` as for the dropout layers) or from the explicit table `u` [n,B,3,N,N] float32,
    read at [s,b,kind,lo,hi]; exactly one of the two -- the semantics of deptree_sample."""
    _C.require_gpu(dec, "dmv1o_sample")
    if dec.dim() != 5 or tuple(dec.shape[2:]) != (2, 2, 2):
        raise ValueError(f"dec must be [B,N,2,2,2], got {tuple(dec.shape)}")
    B, N = dec.shape[:2]
    if tuple(attach.shape) != (B, N, N, 2):
        raise ValueError(f"attach must be [B,N,N,2] = {(B, N, N, 2)}, got {tuple(attach.shape)}")
    n = int(n)
    if dec.dtype != attach.dtype:
        attach = attach.to(dec.dtype)
    dt, dec_c = _C.in_dtype(dec)
    _, att_c = _C.in_dtype(attach)
    lengths = _lengths(lengths, B, dec.device)
    heads, logp, logZ, u, args = _sample_frame("dmv1o_sample", dec.device, B, N, n, rng, site, u, want_logp)
    L = _C.lib()
    nb = L.vlg_dmv1o_sample_workspace(B, N, n)
    ws = torch.empty(nb, dtype=torch.uint8, device=dec.device) if nb else None
    _C.check(L.vlg_dmv1o_sample(_C.ptr(dec_c), _C.ptr(att_c), _C.ptr(lengths), B, N, dt, n, *args, _C.ptr(ws), nb, _C.stream_of(dec)),
             "dmv1o_sample")
    return heads, logp, logZ


def dmv1o_tree_score(md, ma, heads, lengths, big=1e4):
    """Score of the dependency tree `heads` [B,N] (heads[b,c] = head of word c, 0 = the root token) under root-merged DMV1o potentials
    md [B,N,2,2,2] / ma [B,N,N,2 (head, child, valence)]: [B,1], differentiable w.r.t. both (its gradient is the tree's derivation
    counts).  The counts come from the Max-semiring DP itself on potentials whose arcs (heads[c] -> c) carry a bonus that no other tree
    can make up: the valence of every attachment and every continue / stop decision are functions of the tree, so the arg-max derivation
    of the biased potentials IS the derivation of that tree, under exactly the conventions the kernel uses."""
    from .distributions import DMV1o
    B, N = heads.shape
    with torch.no_grad():
        child = torch.arange(N, device=heads.device)[None].expand(B, -1)
        live = (child >= 1) & (child <= lengths[:, None])
        bonus = torch.zeros((B, N, N), dtype=torch.float32, device=heads.device)
        b_idx = torch.arange(B, device=heads.device)[:, None].expand(-1, N)
        bonus[b_idx[live], heads[live], child[live]] = big
    with torch.enable_grad():
        pot = [md.detach().float().requires_grad_(True), (ma.detach().float() + bonus.unsqueeze(-1)).requires_grad_(True)]
        cd, ca = torch.autograd.grad(DMV1o(pot, lengths).max.sum(), pot)
    ct = torch.float64 if md.dtype == torch.float64 else torch.float32   # (the tests' float64 formulation keeps its precision)
    return ((cd.to(ct) * md.to(ct)).flatten(1).sum(1) + (ca.to(ct) * ma.to(ct)).flatten(1).sum(1)).view(B, 1)


def dmv1o_log_prob_heads(dec, attach, lengths, heads):
    """log p(tree) of head vectors [..., B, N] under the DMV of root-merged potentials: [..., B], the tree's score (dmv1o_tree_score)
    minus the log-partition.  Differentiable once w.r.t. both potentials: the tree's counts minus the expected counts.  Leading
    dimensions fold into the batch (the potentials are repeated for the score's Max-semiring launch; the partition is taken once)."""
    B, N = dec.shape[:2]
    if heads.shape[-2:] != (B, N):
        raise ValueError(f"heads must be [..., B, N] = [..., {B}, {N}], got {tuple(heads.shape)}")
    lead = heads.shape[:-2]
    k = 1
    for d in lead:
        k *= int(d)
    lengths = _lengths(lengths, B, dec.device)
    rep = lambda t: t.unsqueeze(0).expand((k,) + tuple(t.shape)).reshape((k * B,) + tuple(t.shape[1:]))
    score = dmv1o_tree_score(rep(dec), rep(attach), heads.reshape(k * B, N), rep(lengths)).view(lead + (B,))
    return score - dmv1o_sum(dec, attach, lengths, _C.SEMIRING_LOG).reshape(B).to(score.dtype)


_KBEST_WS_BYTES = {}


def _kbest_frame(name, device, B, N, k, workspace_fn):
    """What deptree_kbest and dmv1o_kbest share: the outputs heads [k,B,N] / scores [k,B] / count [B] and the workspace of the launch,
    its size asked of `workspace_fn` (vlg_*_kbest_workspace) once per (name, B, N, k).  Returns (heads, scores, count, ws, nb)."""
    heads = torch.empty((k, B, N), dtype=torch.int64, device=device)
    scores = torch.empty((k, B), dtype=torch.float32, device=device)
    count = torch.empty(B, dtype=torch.int32, device=device)
    nb = _KBEST_WS_BYTES.get((name, B, N, k))
    if nb is None:
        nb = _KBEST_WS_BYTES[(name, B, N, k)] = workspace_fn(B, N, k)
    ws = torch.empty(nb, dtype=torch.uint8, device=device) if nb else None
    return heads, scores, count, ws, nb


def deptree_kbest(arc, lengths, k):
    """The k best projective single-root trees of arc scores [B,N,N], 1 <= k <= 16, in ONE launch (vlg_deptree_kbest):
    (heads [k,B,N] int64 as deptree_decode writes them, scores [k,B] float32 non-increasing in k, count [B] int32).  A rank at or
    beyond count[b] does not exist (short sentence, forbidden arcs): score NEGINF, heads 0.  No host synchronisation."""
    _C.require_gpu(arc, "deptree_kbest")
    if arc.dim() != 3:
        raise ValueError("potentials must have dim of 3 (unlabeled)")
    B, N, N2 = arc.shape
    assert N == N2, "Non-square potentials"
    k = int(k)
    dt, arc_c = _C.in_dtype(arc)
    lengths = _lengths(lengths, B, arc.device, allow_none=True)
    L = _C.lib()
    heads, scores, count, ws, nb = _kbest_frame("deptree_kbest", arc.device, B, N, k, L.vlg_deptree_kbest_workspace)
    _C.check(L.vlg_deptree_kbest(_C.ptr(arc_c), _C.ptr(lengths), B, N, dt, k, _C.ptr(heads), _C.ptr(scores), _C.ptr(count), _C.ptr(ws), nb,
                                 _C.stream_of(arc)), "deptree_kbest")
    return heads, scores, count


class _DepTreeKBestScores(torch.autograd.Function):
    """scores [k,B] of the k best trees; d scores[k,b] / d arc[b,h,c] = 1 on the arcs of tree (k,b), for the ranks that exist."""

    @staticmethod
    def forward(ctx, arc, lengths, k):
        heads, scores, count = deptree_kbest(arc.detach(), lengths, k)
        ctx.save_for_backward(heads, count)
        ctx.arc_shape, ctx.arc_dtype, ctx.lengths = arc.shape, arc.dtype, lengths
        ctx.mark_non_differentiable(heads, count)
        return scores, heads, count

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_scores, _gh, _gc):
        heads, count = ctx.saved_tensors
        K, B, N = heads.shape
        pos = torch.arange(N, device=heads.device)
        ln = pos.new_full((B,), N - 1) if ctx.lengths is None else torch.as_tensor(ctx.lengths, device=heads.device).to(torch.int64)
        word = (pos >= 1) & (pos <= ln.unsqueeze(-1))                                             # [B,N]
        live = torch.arange(K, device=heads.device).unsqueeze(-1) < count.unsqueeze(0)            # [K,B]
        w = grad_scores.to(torch.float32).unsqueeze(-1) * (word.unsqueeze(0) & live.unsqueeze(-1))   # [K,B,N]: grad[k,b] at every word of a live rank
        garc = torch.zeros((B, N, N), dtype=torch.float32, device=heads.device)
        b_idx = torch.arange(B, device=heads.device).view(1, B, 1).expand(K, B, N)
        garc.index_put_((b_idx, heads, pos.view(1, 1, N).expand(K, B, N)), w, accumulate=True)    # += grad[k,b] at [b, heads[k,b,c], c]
        return garc.to(ctx.arc_dtype), None, None


def deptree_kbest_scores(arc, lengths, k):
    "(scores [k,B] differentiable once in arc, heads [k,B,N], count [B])"
    return _DepTreeKBestScores.apply(arc, lengths, k)


def dmv1o_kbest(dec, attach, lengths, k):
    """The k best projective single-root trees of the DMV of root-merged potentials dec [B,N,2,2,2] / attach [B,N,N,2], 1 <= k <= 16,
    in ONE launch (vlg_dmv1o_kbest): (heads [k,B,N] int64 as dmv1o_decode writes them, scores [k,B] float32 non-increasing in k,
    count [B] int32).  A rank at or beyond count[b] does not exist (short sentence, forbidden potentials): score NEGINF, heads 0.
    No host synchronisation."""
    _C.require_gpu(dec, "dmv1o_kbest")
    if dec.dim() != 5 or tuple(dec.shape[2:]) != (2, 2, 2):
        raise ValueError(f"dec must be [B,N,2,2,2], got {tuple(dec.shape)}")
    B, N = dec.shape[:2]
    if tuple(attach.shape) != (B, N, N, 2):
        raise ValueError(f"attach must be [B,N,N,2] = {(B, N, N, 2)}, got {tuple(attach.shape)}")
    k = int(k)
    if dec.dtype != attach.dtype:
        attach = attach.to(dec.dtype)
    dt, dec_c = _C.in_dtype(dec)
    _, att_c = _C.in_dtype(attach)
    lengths = _lengths(lengths, B, dec.device)
    L = _C.lib()
    heads, scores, count, ws, nb = _kbest_frame("dmv1o_kbest", dec.device, B, N, k, L.vlg_dmv1o_kbest_workspace)
    _C.check(L.vlg_dmv1o_kbest(_C.ptr(dec_c), _C.ptr(att_c), _C.ptr(lengths), B, N, dt, k, _C.ptr(heads), _C.ptr(scores), _C.ptr(count),
                               _C.ptr(ws), nb, _C.stream_of(dec)), "dmv1o_kbest")
    return heads, scores, count


def dmv1o_tree_counts(heads, lengths, count=None, weight=None):
    """sum_t weight[t,b] * (derivation counts of the tree heads[t,b,:]) in ONE launch (vlg_dmv1o_tree_counts): heads [T,B,N] int64,
    count [B] int32 or None (only the trees t < count[b]), weight [T,B] float32 or None (1) -> (cnt_dec [B,N,2,2,2], cnt_attach
    [B,N,N,2]) float32.  No atomics: bit-reproducible."""
    _C.require_gpu(heads, "dmv1o_tree_counts")
    if heads.dim() != 3 or heads.dtype != torch.int64:
        raise ValueError(f"heads must be int64 [T,B,N], got {heads.dtype} {tuple(heads.shape)}")
    T, B, N = heads.shape
    heads = heads.contiguous()
    lengths = _lengths(lengths, B, heads.device)
    if count is not None:
        if count.dtype != torch.int32 or tuple(count.shape) != (B,) or count.device != heads.device:
            raise ValueError(f"count must be int32 [{B}] on {heads.device}")
        count = count.contiguous()
    if weight is not None:
        if tuple(weight.shape) != (T, B) or weight.device != heads.device:
            raise ValueError(f"weight must be [T,B] = {(T, B)} on {heads.device}")
        weight = weight.to(torch.float32).contiguous()
    cnt_dec = torch.empty((B, N, 2, 2, 2), dtype=torch.float32, device=heads.device)
    cnt_attach = torch.empty((B, N, N, 2), dtype=torch.float32, device=heads.device)
    _C.check(_C.lib().vlg_dmv1o_tree_counts(_C.ptr(heads), _C.ptr(lengths), _C.ptr(count), _C.ptr(weight), T, B, N, _C.ptr(cnt_dec),
                                            _C.ptr(cnt_attach), _C.stream_of(heads)), "dmv1o_tree_counts")
    return cnt_dec, cnt_attach


class _DMV1oKBestScores(torch.autograd.Function):
    """scores [k,B] of the k best trees; d scores[k,b] / d (dec, attach)[b] = the derivation counts of tree (k,b), for the ranks that
    exist: the backward is one vlg_dmv1o_tree_counts launch weighted by the upstream gradient."""

    @staticmethod
    def forward(ctx, dec, attach, lengths, k):
        heads, scores, count = dmv1o_kbest(dec.detach(), attach.detach(), lengths, k)
        ctx.save_for_backward(heads, count)
        ctx.dtypes, ctx.lengths = (dec.dtype, attach.dtype), lengths
        ctx.mark_non_differentiable(heads, count)
        return scores, heads, count

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_scores, _gh, _gc):
        heads, count = ctx.saved_tensors
        gdec, gatt = dmv1o_tree_counts(heads, ctx.lengths, count, grad_scores)
        return gdec.to(ctx.dtypes[0]), gatt.to(ctx.dtypes[1]), None, None


def dmv1o_kbest_scores(dec, attach, lengths, k):
    "(scores [k,B] differentiable once in dec and attach, heads [k,B,N], count [B])"
    return _DMV1oKBestScores.apply(dec, attach, lengths, k)


def deptree_mbr_decode(marginals, lengths=None):
    """The MBR decode of src/model/ldndmv.py:294-299 from the DMV1o arc marginals [B,N,N,2] (float32: `grad_attach` of the Log
    semiring's inside-outside pass): `DependencyCRF(marginals.sum(-1)).argmax` as (best_score [B], heads [B,N] int64) in ONE DepTree
    launch -- the valence sum is taken in its load stage, no [B,N,N] tensor.  Equals `deptree_decode(marginals.sum(-1))` bit for bit."""
    _C.require_gpu(marginals, "deptree_mbr_decode")
    if marginals.dim() != 4 or marginals.shape[1] != marginals.shape[2] or marginals.shape[3] != 2:
        raise ValueError(f"deptree_mbr_decode: marginals must be [B,N,N,2], got {tuple(marginals.shape)}")
    if marginals.dtype != torch.float32:
        raise ValueError(f"deptree_mbr_decode: marginals must be float32 (the DP writes them so), got {marginals.dtype}")
    B, N = marginals.shape[:2]
    m = marginals.detach().contiguous()
    lengths = _lengths(lengths, B, m.device, allow_none=True)
    best = torch.empty(B, dtype=torch.float32, device=m.device)
    heads = torch.empty((B, N), dtype=torch.int64, device=m.device)
    ws, nb = _workspace(_C.OP_DEPTREE_INSIDE_OUTSIDE, B, N, _C.SEMIRING_MAX, m.device)
    _C.check(_C.lib().vlg_deptree_mbr_decode(_C.ptr(m), _C.ptr(lengths), B, N, _C.ptr(best), _C.ptr(heads), _C.ptr(ws), nb,
                                             _C.stream_of(m)), "deptree_mbr_decode")
    return best, heads


def dmv1o_rules_run(attach_rule, dec, root_rule, token, lengths, semiring, want_grad, head_mask=None, want_heads=False,
                    mask_fill=-1e20, grad_logZ=None):
    """Raw launcher of the rule-table DP (include/vlgae_amd.h: vlg_dmv1o_rules).
    attach_rule [B,L,T,2,2], dec [B,L,2,2,2], root_rule [T] / [1,T] / [B,T], token [B,L] int64, head_mask [B,L] bool.
    Returns dict(logZ [B], grad_rule, grad_dec, grad_root [B,T], heads [B,L+1]) with the requested entries."""
    _C.require_gpu(attach_rule, "dmv1o_rules")
    B, L, T = attach_rule.shape[:3]
    if tuple(attach_rule.shape) != (B, L, T, 2, 2) or tuple(dec.shape) != (B, L, 2, 2, 2) or tuple(token.shape) != (B, L):
        raise ValueError(f"attach_rule {tuple(attach_rule.shape)}, dec {tuple(dec.shape)}, token {tuple(token.shape)}")
    root2 = root_rule.reshape(-1, T)
    if root2.shape[0] not in (1, B):
        raise ValueError(f"root_rule must be [T], [1,T] or [B,T]; got {tuple(root_rule.shape)}")
    dt, rule_c = _C.in_dtype(attach_rule)
    dec_c = dec.detach().to(rule_c.dtype).contiguous()
    root_c = root2.detach().to(rule_c.dtype).contiguous()
    dev = attach_rule.device
    token = token.to(device=dev, dtype=torch.int64).contiguous()
    hm = _C.mask_u8(head_mask, dev)
    lengths = _lengths(lengths, B, dev)
    out = {"logZ": torch.empty(B, dtype=torch.float32, device=dev)}
    g_rule = g_dec = g_root = heads = None
    if want_grad:
        g_rule = torch.empty((B, L, T, 2, 2), dtype=torch.float32, device=dev)
        g_dec = torch.empty((B, L, 2, 2, 2), dtype=torch.float32, device=dev)
        g_root = torch.empty((B, T), dtype=torch.float32, device=dev)
        out.update(grad_rule=g_rule, grad_dec=g_dec, grad_root=g_root)
    if want_heads:
        heads = torch.empty((B, L + 1), dtype=torch.int64, device=dev)
        out["heads"] = heads
    op = _C.OP_DMV1O_INSIDE_OUTSIDE if (want_grad or want_heads) else _C.OP_DMV1O_INSIDE
    ws, nb = _workspace(op, B, L + 1, semiring, dev)
    g = None if grad_logZ is None else grad_logZ.detach().to(torch.float32).reshape(B).contiguous()
    _C.check(_C.lib().vlg_dmv1o_rules(_C.ptr(rule_c), _C.ptr(dec_c), _C.ptr(root_c), int(root2.shape[0] == B and B > 1),
                                      _C.ptr(token), _C.ptr(hm),
                                      _C.ptr(lengths), B, L, T, dt, semiring, float(mask_fill), _C.ptr(g),
                                      _C.ptr(out["logZ"]), _C.ptr(g_rule), _C.ptr(g_dec), _C.ptr(g_root), _C.ptr(heads),
                                      _C.ptr(ws), nb, _C.stream_of(attach_rule)), "dmv1o_rules")
    return out


class _DMV1oRulesSum(torch.autograd.Function):
    """semiring-sum over trees as a function of the scorer's rule tables; backward = rule-space expected counts."""

    @staticmethod
    def forward(ctx, attach_rule, dec, root_rule, token, lengths, head_mask, semiring, mask_fill):
        want = any(ctx.needs_input_grad[:3])
        r = dmv1o_rules_run(attach_rule, dec, root_rule, token, lengths, semiring, want, head_mask, False, mask_fill)
        if want:
            ctx.save_for_backward(r["grad_rule"], r["grad_dec"], r["grad_root"])
        ctx.meta = (attach_rule.dtype, dec.dtype, root_rule.dtype, tuple(root_rule.shape))
        return r["logZ"].unsqueeze(-1)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        g_rule, g_dec, g_root = ctx.saved_tensors
        d0, d1, d2, root_shape = ctx.meta
        g = grad_out.reshape(-1).to(torch.float32)
        gr = (g_rule * g.view(-1, 1, 1, 1, 1)).to(d0) if ctx.needs_input_grad[0] else None
        gd = (g_dec * g.view(-1, 1, 1, 1, 1)).to(d1) if ctx.needs_input_grad[1] else None
        gt = None
        if ctx.needs_input_grad[2]:
            gt = g_root * g.view(-1, 1)
            B, T = gt.shape
            per_sentence = len(root_shape) == 2 and root_shape[0] == B and B > 1
            gt = (gt if per_sentence else gt.sum(0)).reshape(root_shape).to(d2)   # a shared root table sums over the batch
        return gr, gd, gt, None, None, None, None, None


def dmv1o_rules_sum(attach_rule, dec, root_rule, token, lengths, head_mask=None, semiring=0, mask_fill=-1e20):
    return _DMV1oRulesSum.apply(attach_rule, dec, root_rule, token, lengths, head_mask, semiring, mask_fill)


class _DMV1oSum(torch.autograd.Function):
    """semiring-sum over all trees; d/d(potentials) = expected counts (Log) / best tree (Max)."""

    @staticmethod
    def forward(ctx, dec, attach, lengths, semiring):
        want = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        hit = _viterbi_lookup(dec, attach, lengths) if semiring == _C.SEMIRING_MAX and dec.dtype != torch.float64 else None
        phit = _partition_lookup(dec, attach, lengths) if semiring == _C.SEMIRING_LOG and dec.dtype != torch.float64 else None
        if hit is not None:   # this step's Viterbi pass already ran on these very values (marginals_and_heads(keep_viterbi=True))
            best, gdec, gatt, _ = hit
            logZ = best.view(-1, 1)
        elif phit is not None:   # ... or its inside-outside pass, with the dec counts (marginals_and_heads(keep_partition=True))
            lz, gdec, gatt = phit
            logZ = lz.view(-1, 1)
        else:
            logZ, gdec, gatt = dmv1o_run(dec, attach, lengths, semiring, want, logZ_shape=(dec.shape[0], 1))   # [B,1], helpers.py:116
        if want:
            ctx.save_for_backward(gdec, gatt)
            ctx.fwd_thread = threading.get_ident()
        ctx.in_dtypes = (dec.dtype, attach.dtype)
        return logZ.double() if dec.dtype == torch.float64 else logZ

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        _note_backward_thread(ctx)
        gdec, gatt = ctx.saved_tensors
        want_d, want_a = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gd, ga = _scale_counts(gdec if want_d else None, gatt if want_a else None, grad_out, ctx.in_dtypes[0], ctx.in_dtypes[1])
        return gd, ga, None, None


_WARNED_ENGINE_THREAD = False


def _note_backward_thread(ctx):
    """Warn once when backward runs on torch's autograd engine thread instead of the thread that ran forward."""
    global _WARNED_ENGINE_THREAD
    if not _WARNED_ENGINE_THREAD and getattr(ctx, "fwd_thread", None) not in (None, threading.get_ident()):
        _WARNED_ENGINE_THREAD = True
        warnings.warn("vlgae_amd: backward is running on torch's autograd engine thread; the hand-off costs 50-120 us per call, "
                      "more than the fused DP kernel takes. A one-process-per-GPU trainer should call "
                      "vlgae_amd.configure_autograd() (= torch.autograd.set_multithreading_enabled(False)) once at start-up.",
                      RuntimeWarning, stacklevel=2)


def _scale_counts(ca, cb, grad_out, dtype_a, dtype_b):
    """counts * d loss / d logZ, cast to the potentials' dtypes: one launch (vlg_scale_counts) for the fp32 / bf16 cases."""
    first = ca if ca is not None else cb
    if first is None:
        return None, None
    B = first.shape[0]
    dt = dtype_a if ca is not None else dtype_b
    if (ca is not None and cb is not None and dtype_a != dtype_b) or (dt != torch.float32 and dt != torch.bfloat16) or B == 0:
        g = grad_out.reshape(-1).to(torch.float32)
        return tuple(None if c is None else (c * g.view(-1, *([1] * (c.dim() - 1)))).to(d) for c, d in ((ca, dtype_a), (cb, dtype_b)))
    if grad_out.dtype != torch.float32:
        grad_out = grad_out.float()
    stride = 1
    if grad_out.stride() == (0,) * grad_out.dim():
        stride = 0                                                   # the expanded scalar a `.sum()` hands back
    elif not grad_out.is_contiguous():
        grad_out = grad_out.contiguous()
    oa = None if ca is None else torch.empty(ca.shape, dtype=dt, device=ca.device)
    ob = None if cb is None else torch.empty(cb.shape, dtype=dt, device=cb.device)
    _C.check(_C.lib().vlg_scale_counts(_C.ptr(ca), _C.ptr(cb), _C.ptr(grad_out), stride, B, 0 if ca is None else ca.numel() // B,
                                       0 if cb is None else cb.numel() // B, _C.BF16 if dt == torch.bfloat16 else _C.F32, _C.ptr(oa),
                                       _C.ptr(ob), _C.stream_of(first)), "scale_counts")
    return oa, ob


class _DepTreeSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, arc, lengths, semiring):
        want = ctx.needs_input_grad[0]
        logZ, garc = deptree_run(arc, lengths, semiring, want)
        if want:
            ctx.save_for_backward(garc)
        ctx.in_dtype = arc.dtype
        return logZ.to(arc.dtype if arc.dtype == torch.float64 else torch.float32)                  # [B], deptree.py:75

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        (garc,) = ctx.saved_tensors
        return _scale_counts(garc, None, grad_out, ctx.in_dtype, ctx.in_dtype)[0], None, None


def dmv1o_sum(dec, attach, lengths, semiring):
    return _DMV1oSum.apply(dec, attach, lengths, semiring)


def deptree_sum(arc, lengths, semiring):
    return _DepTreeSum.apply(arc, lengths, semiring)


def _expect_frame(name, device, B, N, *, dirs, shapes, shape_error, grad, outs, ws_bytes):
    """What deptree_expect and dmv1o_expect share.  Each given direction of `dirs` is on the GPU and has the shape of its potential
    (`shapes`, in step; `shape_error` opens the message); they go in one storage type -- bf16 only when every one given is bf16, else
    detached float32 -- and contiguous.  logZ [B], ev [B] and the outputs of the shapes `outs` (None: not wanted) are float32 in one
    allocation; the workspace has ws_bytes(B, N, grad) bytes, asked once per (name, B, N, grad).
    Returns (dirs, v_dtype, (logZ, ev, *outputs), ws, nb)."""
    for t, want in zip(dirs, shapes):
        if t is not None:
            _C.require_gpu(t, name)
            if tuple(t.shape) != want:
                raise ValueError(f"{shape_error}, got {tuple(t.shape)}")
    vdt = _C.F32
    given = [t for t in dirs if t is not None]
    if given:
        if all(t.dtype == torch.bfloat16 for t in given):
            vdt = _C.BF16
        else:
            dirs = [None if t is None else t.detach().float() for t in dirs]
        dirs = [None if t is None else (t if t.is_contiguous() else t.contiguous()) for t in dirs]
    out, _ = _C.alloc_f32(device, [(B,), (B,), *outs])
    nb = _WS_BYTES.get((name, B, N, grad))
    if nb is None:
        nb = _WS_BYTES[(name, B, N, grad)] = ws_bytes(B, N, grad)
    return dirs, vdt, out, torch.empty(nb, dtype=torch.uint8, device=device) if nb else None, nb


def deptree_expect(arc, lengths, v=None, v_sub=None, want_mu=False, want_hv=False):
    """Raw launcher of the dual-number DepTree pass (vlg_deptree_expect).  arc [B,N,N]; v, v_sub [B,N,N] or None (= 0): the direction is
    v - v_sub.  Returns (logZ [B], ev [B] = <mu, v - v_sub>, mu [B,N,N] or None, hv [B,N,N] = (Hessian of logZ)(v - v_sub) or None),
    all float32.  want_mu / want_hv select the inside-outside image; without them only the inside pass runs."""
    _C.require_gpu(arc, "deptree_expect")
    if arc.dim() != 3:
        raise ValueError("potentials must have dim of 3 (unlabeled)")
    B, N, N2 = arc.shape
    assert N == N2, "Non-square potentials"
    dt, arc_c = _C.in_dtype(arc)
    shape, L = (B, N, N), _C.lib()
    (v, v_sub), vdt, (logZ, ev, mu, hv), ws, nb = _expect_frame(
        "deptree_expect", arc.device, B, N, dirs=(v, v_sub), shapes=(shape, shape), shape_error=f"direction must be [B,N,N] = {shape}",
        grad=want_mu or want_hv, outs=(shape if want_mu else None, shape if want_hv else None),
        ws_bytes=lambda B, N, grad: L.vlg_workspace_bytes(_C.OP_DEPTREE_EXPECT_GRAD if grad else _C.OP_DEPTREE_EXPECT, B, N, _C.SEMIRING_LOG))
    lengths = _lengths(lengths, B, arc.device, allow_none=True)
    _C.check(L.vlg_deptree_expect(_C.ptr(arc_c), _C.ptr(v), _C.ptr(v_sub), _C.ptr(lengths), B, N, dt, vdt, _C.ptr(logZ), _C.ptr(ev), _C.ptr(mu),
                                  _C.ptr(hv), _C.ptr(ws), nb, _C.stream_of(arc)), "deptree_expect")
    return logZ, ev, mu, hv


def _out_dtype(t):
    return t.dtype if t.dtype == torch.float64 else torch.float32


class _DepTreeExpectedScore(torch.autograd.Function):
    """E_p[<cost, tree>] (the reference's `risk`): value ev, d/d arc = hv = Cov(tree, <cost, tree>), d/d cost = mu."""

    @staticmethod
    def forward(ctx, arc, lengths, cost):
        wa, wc = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        _, ev, mu, hv = deptree_expect(arc, lengths, v=cost, want_mu=wc, want_hv=wa)
        ctx.save_for_backward(hv, mu)
        ctx.in_dtypes = (arc.dtype, cost.dtype)
        return ev.to(_out_dtype(arc))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        hv, mu = ctx.saved_tensors
        ga, gc = _scale_counts(hv, mu, grad_out, *ctx.in_dtypes)
        return ga, None, gc


class _DepTreeEntropy(torch.autograd.Function):
    """H[p] = logZ - <mu, arc>: the direction is the distribution's own potentials; d/d arc = -hv."""

    @staticmethod
    def forward(ctx, arc, lengths):
        want = ctx.needs_input_grad[0]
        logZ, ev, _, hv = deptree_expect(arc, lengths, v=arc, want_hv=want)
        if want:
            ctx.save_for_backward(hv)
        ctx.in_dtype = arc.dtype
        return (logZ - ev).to(_out_dtype(arc))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        (hv,) = ctx.saved_tensors
        return _scale_counts(hv, None, -grad_out, ctx.in_dtype, ctx.in_dtype)[0], None


def _deptree_pq(ctx, arc_p, arc_q, lengths, v_sub):
    """The two launches cross-entropy and KL share: p along v = arc_q (- v_sub), q with no direction.  The q side runs the outside pass
    only when arc_q wants a gradient (a fixed q costs one inside pass): the value pass of the inside-only image and of the
    inside-outside image is the same sequence of operations (vlg_dp_expect.h: expect_fw_span), so on equal potentials the two logZ
    agree bit for bit whichever images ran."""
    wp, wq = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    logZ_p, ev, mu_p, hv = deptree_expect(arc_p, lengths, v=arc_q, v_sub=v_sub, want_mu=wq, want_hv=wp)
    logZ_q, _, mu_q, _ = deptree_expect(arc_q, lengths, want_mu=wq)
    if wq:
        mu_p.sub_(mu_q)          # in place: -(d/d arc_q) = mu_p - mu_q, scaled together with hv by -grad in backward
    ctx.save_for_backward(hv if wp else None, mu_p if wq else None)
    ctx.in_dtypes = (arc_p.dtype, arc_q.dtype)
    return logZ_p, logZ_q, ev


def _deptree_pq_backward(ctx, grad_out):
    hv, dmu = ctx.saved_tensors
    gp, gq = _scale_counts(hv, dmu, -grad_out, *ctx.in_dtypes)
    return gp, gq, None


class _DepTreeCrossEntropy(torch.autograd.Function):
    """H[p,q] = logZ_q - <mu_p, arc_q>; d/d arc_p = -hv, d/d arc_q = mu_q - mu_p."""

    @staticmethod
    def forward(ctx, arc_p, arc_q, lengths):
        _, logZ_q, ev = _deptree_pq(ctx, arc_p, arc_q, lengths, None)
        return (logZ_q - ev).to(_out_dtype(arc_p))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        return _deptree_pq_backward(ctx, grad_out)


class _DepTreeKL(torch.autograd.Function):
    """KL[p||q] = logZ_q - logZ_p - <mu_p, arc_q - arc_p> (the subtraction is the kernel's v - v_sub); gradients as for H[p,q]."""

    @staticmethod
    def forward(ctx, arc_p, arc_q, lengths):
        logZ_p, logZ_q, ev = _deptree_pq(ctx, arc_p, arc_q, lengths, arc_p)
        return (logZ_q - logZ_p - ev).to(_out_dtype(arc_p))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        return _deptree_pq_backward(ctx, grad_out)


def deptree_expected_score(arc, lengths, cost):
    return _DepTreeExpectedScore.apply(arc, lengths, cost)


def deptree_entropy(arc, lengths):
    return _DepTreeEntropy.apply(arc, lengths)


def deptree_cross_entropy(arc_p, arc_q, lengths):
    return _DepTreeCrossEntropy.apply(arc_p, arc_q, lengths)


def deptree_kl(arc_p, arc_q, lengths):
    return _DepTreeKL.apply(arc_p, arc_q, lengths)


# ---- labeled arc potentials phi [B,N,N,L] (deptree.py:19,33-41) ------------------------------------------------------------------------
# The DP reads arc scores [B,N,N]: vlg_label_fold reduces the label axis in the semiring in front of it, vlg_label_expand spreads an
# arc-level gradient back over the labels behind it, vlg_label_draw labels the arcs of sampled trees.  One pass over phi each; no
# [B,N,N,L] temporary besides the result.
def _labeled_in(phi, name):
    _C.require_gpu(phi, name)
    if phi.dim() != 4:
        raise ValueError("labeled potentials must have dim of 4 (head x child x label)")
    B, N, N2, L = phi.shape
    assert N == N2, "Non-square potentials"
    if not 1 <= L <= 255:
        raise ValueError(f"{name}: 1 <= L <= 255 labels (got {L})")
    dt, phi_c = _C.in_dtype(phi)
    return B, N, L, dt, phi_c


def _label_dirs(name, shape, v, v_sub):
    "(v_dtype, v, v_sub) as the kernels take them: both in one storage type (bf16 only when every one given is bf16), contiguous"
    vs = [t for t in (v, v_sub) if t is not None]
    for t in vs:
        _C.require_gpu(t, name)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: direction must be [B,N,N,L] = {tuple(shape)}, got {tuple(t.shape)}")
    if v_sub is not None and v is None:
        raise ValueError(f"{name}: v_sub without v")
    vdt = _C.F32
    if vs:
        if all(t.dtype == torch.bfloat16 for t in vs):
            vdt = _C.BF16
        else:
            v, v_sub = (None if t is None else (t if t.dtype == torch.float32 else t.detach().float()) for t in (v, v_sub))
        v, v_sub = (None if t is None else (t if t.is_contiguous() else t.contiguous()) for t in (v, v_sub))
    return vdt, v, v_sub


def label_fold(phi, lengths, semiring, want_best=False, v=None, v_sub=None):
    """Raw launcher of vlg_label_fold.  phi [B,N,N,L] -> (arc [B,N,N] float32 = logsumexp_l / max_l phi, best [B,N,N] uint8 = the lowest
    label attaining the maximum or None, dbar [B,N,N] float32 = sum_l p_l (v_l - v_sub_l) or None: given iff v is)."""
    B, N, L, dt, phi_c = _labeled_in(phi, "label_fold")
    vdt, v, v_sub = _label_dirs("label_fold", phi.shape, v, v_sub)
    lengths = _lengths(lengths, B, phi.device, allow_none=True)
    (arc, dbar), _ = _C.alloc_f32(phi.device, [(B, N, N), (B, N, N) if v is not None else None])
    best = torch.empty((B, N, N), dtype=torch.uint8, device=phi.device) if want_best else None
    _C.check(_C.lib().vlg_label_fold(_C.ptr(phi_c), _C.ptr(v), _C.ptr(v_sub), _C.ptr(lengths), B, N, L, dt, vdt, semiring, _C.ptr(arc),
                                     _C.ptr(best), _C.ptr(dbar), _C.stream_of(phi)), "label_fold")
    return arc, best, dbar


def label_expand(phi, lengths, semiring, arc, g1, best=None, g2=None, dbar=None, v=None, v_sub=None, scale=None, mode=0, out_dtype=None):
    """Raw launcher of vlg_label_expand: out [B,N,N,L] = scale[b] p_l (g1 + g2 (v_l - v_sub_l - dbar)) (mode 0) or scale[b] g1 p_l
    (mode 1), p_l = exp(phi_l - arc) (Log) or [l == best] (Max); arc / best / dbar as label_fold returned them, g1 / g2 [B,N,N] float32,
    scale [B] or None.  out_dtype: float32 (default) or phi's own bfloat16."""
    B, N, L, dt, phi_c = _labeled_in(phi, "label_expand")
    vdt, v, v_sub = _label_dirs("label_expand", phi.shape, v, v_sub)
    lengths = _lengths(lengths, B, phi.device, allow_none=True)
    odt = _C.BF16 if out_dtype == torch.bfloat16 and dt == _C.BF16 else _C.F32
    out = torch.empty((B, N, N, L), dtype=torch.bfloat16 if odt == _C.BF16 else torch.float32, device=phi.device)
    stride = 1
    if scale is not None:
        scale = scale.detach()
        if scale.dtype != torch.float32:
            scale = scale.float()
        if scale.numel() == 1 or scale.stride() == (0,) * scale.dim():
            stride = 0                                                   # the expanded scalar a `.sum()` hands back
        else:
            scale = scale.reshape(B)
            if not scale.is_contiguous():
                scale = scale.contiguous()
    _C.check(_C.lib().vlg_label_expand(_C.ptr(phi_c), _C.ptr(v), _C.ptr(v_sub), _C.ptr(lengths), B, N, L, dt, vdt, odt, semiring, mode,
                                       _C.ptr(arc), _C.ptr(best), _C.ptr(g1), _C.ptr(g2), _C.ptr(dbar), _C.ptr(scale), stride, _C.ptr(out),
                                       _C.stream_of(phi)), "label_expand")
    return out


def _expand_to(dtype, *args, **kw):
    "label_expand in the storage type of the tensor the gradient belongs to (bf16 directly where the kernel can, else through float32)"
    return label_expand(*args, out_dtype=dtype, **kw).to(dtype)


class _DepTreeLabeledSum(torch.autograd.Function):
    """semiring-sum over all labeled trees: fold, then the DP on the arc scores.  backward spreads the arc counts over the labels
    (softmax over the labels in Log, the best label in Max) with grad_out as the scale: no [B,N,N,L] tensor exists in forward."""

    @staticmethod
    def forward(ctx, phi, lengths, semiring):
        want = ctx.needs_input_grad[0]
        arc, best, _ = label_fold(phi, lengths, semiring, want_best=want and semiring == _C.SEMIRING_MAX)
        if semiring == _C.SEMIRING_MAX:
            # The best tree's score is summed from the folded scores on its arcs, as the samplers sum a tree's score from the input
            # potentials: the DP's own value carries the rounding of its log2-unit charts, this one is exact wherever float32 adds
            # the scores exactly.  (An invalid length keeps the DP's NaN.)
            logZ, garc = deptree_run(arc, lengths, semiring, True)
            logZ = torch.where(torch.isnan(logZ), logZ, torch.where(garc > 0, arc, torch.zeros_like(arc)).sum((1, 2)))
        else:
            logZ, garc = deptree_run(arc, lengths, semiring, want)
        if want:
            ctx.save_for_backward(phi, arc, garc, best)
        ctx.lengths, ctx.semiring = lengths, semiring
        return logZ.to(_out_dtype(phi))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        phi, arc, garc, best = ctx.saved_tensors
        return _expand_to(phi.dtype, phi, ctx.lengths, ctx.semiring, arc, garc, best=best, scale=grad_out), None, None


def deptree_labeled_sum(phi, lengths, semiring):
    return _DepTreeLabeledSum.apply(phi, lengths, semiring)


def deptree_labeled_marginals(phi, lengths, semiring):
    "labeled arc marginals (Log) / the best labeled tree's 0/1 parts (Max): [B,N,N,L] float32 -- fold, inside-outside, expand"
    arc, best, _ = label_fold(phi.detach(), lengths, semiring, want_best=semiring == _C.SEMIRING_MAX)
    _, garc = deptree_run(arc, lengths, semiring, True)
    return label_expand(phi.detach(), lengths, semiring, arc, garc, best=best)


def deptree_labeled_decode(phi, lengths):
    """(best_score [B], heads [B,N], labels [B,N] int64) of the best labeled tree: labels[b,c] = the label of the arc into word c
    (0 at c = 0 and in padding) -- `best` gathered at (heads[c], c) on the device, no host synchronisation."""
    arc, best, _ = label_fold(phi.detach(), lengths, _C.SEMIRING_MAX, want_best=True)
    score, heads = deptree_decode(arc, lengths)
    B, N = heads.shape
    labels = best.view(B, N * N).gather(1, heads * N + torch.arange(N, device=heads.device)).to(torch.int64)
    return score, heads, labels


def deptree_labeled_sample(phi, lengths, n, rng=None, site=0, u=None, u_label=None, want_logp=True):
    """n labeled trees per sentence: (heads [n,B,N], labels [n,B,N] int64, logp [n,B] or None, logZ [B]).  The tree comes from
    deptree_sample on the folded arc scores, the labels from vlg_label_draw under the same (seed, step, site) -- or, with explicit
    uniforms, under u_label [n,B,N] float32 next to the tree sampler's u.  logp is the labeled tree's score minus logZ."""
    B, N, L, dt, phi_c = _labeled_in(phi, "deptree_labeled_sample")
    if (u is None) != (u_label is None):
        raise ValueError("deptree_labeled_sample: explicit uniforms come as the pair u [n,B,3,N,N] and u_label [n,B,N]")
    n = int(n)
    if u_label is not None:
        if tuple(u_label.shape) != (n, B, N) or u_label.dtype != torch.float32 or u_label.device != phi.device:
            raise ValueError(f"deptree_labeled_sample: u_label must be float32 [n,B,N] = {(n, B, N)} on {phi.device}")
        u_label = u_label.contiguous()
    lengths = _lengths(lengths, B, phi.device, allow_none=True)
    arc, _, _ = label_fold(phi_c, lengths, _C.SEMIRING_LOG)
    heads, logp, logZ = deptree_sample(arc, lengths, n, rng=rng, site=site, u=u, want_logp=want_logp)
    labels = torch.empty((n, B, N), dtype=torch.int64, device=phi.device)
    _C.check(_C.lib().vlg_label_draw(_C.ptr(phi_c), _C.ptr(arc), _C.ptr(heads), _C.ptr(lengths), B, N, L, n, dt,
                                     None if rng is None else _C.ptr(rng.state), int(site), _C.ptr(u_label), _C.ptr(labels), _C.ptr(logp),
                                     _C.stream_of(phi)), "label_draw")
    return heads, labels, logp, logZ


class _DepTreeLabeledExpectedScore(torch.autograd.Function):
    """E_p[<cost, labeled tree>]: the fold's dual part cbar is the arc-level cost; d/d phi = p (hv + mu (cost - cbar)), d/d cost = mu p."""

    @staticmethod
    def forward(ctx, phi, lengths, cost):
        wa, wc = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        arc, _, dbar = label_fold(phi, lengths, _C.SEMIRING_LOG, v=cost)
        _, ev, mu, hv = deptree_expect(arc, lengths, v=dbar, want_mu=wa or wc, want_hv=wa)
        ctx.save_for_backward(phi, cost, arc, dbar, mu, hv)
        ctx.lengths = lengths
        return ev.to(_out_dtype(phi))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        phi, cost, arc, dbar, mu, hv = ctx.saved_tensors
        ga = gc = None
        if ctx.needs_input_grad[0]:
            ga = _expand_to(phi.dtype, phi, ctx.lengths, _C.SEMIRING_LOG, arc, hv, g2=mu, dbar=dbar, v=cost, scale=grad_out)
        if ctx.needs_input_grad[2]:
            gc = _expand_to(cost.dtype, phi, ctx.lengths, _C.SEMIRING_LOG, arc, mu, scale=grad_out, mode=1)
        return ga, None, gc


class _DepTreeLabeledEntropy(torch.autograd.Function):
    """H[p] = logZ - <mu, phibar>: the direction is the distribution's own potentials; d/d phi = -p (hv + mu (phi - phibar))."""

    @staticmethod
    def forward(ctx, phi, lengths):
        want = ctx.needs_input_grad[0]
        arc, _, dbar = label_fold(phi, lengths, _C.SEMIRING_LOG, v=phi)
        logZ, ev, mu, hv = deptree_expect(arc, lengths, v=dbar, want_mu=want, want_hv=want)
        if want:
            ctx.save_for_backward(phi, arc, dbar, mu, hv)
        ctx.lengths = lengths
        return (logZ - ev).to(_out_dtype(phi))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        phi, arc, dbar, mu, hv = ctx.saved_tensors
        return _expand_to(phi.dtype, phi, ctx.lengths, _C.SEMIRING_LOG, arc, hv, g2=mu, dbar=dbar, v=phi, scale=-grad_out), None


def _labeled_pq(ctx, phi_p, phi_q, lengths, sub):
    """What labeled cross-entropy and KL share (see _deptree_pq): p folded along v = phi_q (- phi_p when `sub`), q folded without a
    direction; then the launches of the unlabeled path on the arc scores.  On equal potentials the two folds write the same arc scores
    (the direction does not enter them), so the two logZ agree bit for bit and dbar, ev, hv are exactly 0."""
    wp, wq = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    arc_p, _, dbar = label_fold(phi_p, lengths, _C.SEMIRING_LOG, v=phi_q, v_sub=phi_p if sub else None)
    arc_q, _, _ = label_fold(phi_q, lengths, _C.SEMIRING_LOG)
    logZ_p, ev, mu_p, hv = deptree_expect(arc_p, lengths, v=dbar, want_mu=wp or wq, want_hv=wp)
    logZ_q, _, mu_q, _ = deptree_expect(arc_q, lengths, want_mu=wq)
    ctx.save_for_backward(phi_p, phi_q, arc_p, arc_q, dbar, mu_p, hv, mu_q)
    ctx.lengths, ctx.sub = lengths, sub
    return logZ_p, logZ_q, ev


def _labeled_pq_backward(ctx, grad_out):
    "d/d phi_p = -p (hv + mu_p (d - dbar)); d/d phi_q = mu_q q - mu_p p: two mode-1 expands of the same form, so exactly 0 on equal potentials"
    phi_p, phi_q, arc_p, arc_q, dbar, mu_p, hv, mu_q = ctx.saved_tensors
    gp = gq = None
    if ctx.needs_input_grad[0]:
        gp = _expand_to(phi_p.dtype, phi_p, ctx.lengths, _C.SEMIRING_LOG, arc_p, hv, g2=mu_p, dbar=dbar, v=phi_q,
                        v_sub=phi_p if ctx.sub else None, scale=-grad_out)
    if ctx.needs_input_grad[1]:
        gq = label_expand(phi_q, ctx.lengths, _C.SEMIRING_LOG, arc_q, mu_q, scale=grad_out, mode=1)
        gq.sub_(label_expand(phi_p, ctx.lengths, _C.SEMIRING_LOG, arc_p, mu_p, scale=grad_out, mode=1))
        gq = gq.to(phi_q.dtype)
    return gp, gq, None


class _DepTreeLabeledCrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, phi_p, phi_q, lengths):
        _, logZ_q, ev = _labeled_pq(ctx, phi_p, phi_q, lengths, False)
        return (logZ_q - ev).to(_out_dtype(phi_p))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        return _labeled_pq_backward(ctx, grad_out)


class _DepTreeLabeledKL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, phi_p, phi_q, lengths):
        logZ_p, logZ_q, ev = _labeled_pq(ctx, phi_p, phi_q, lengths, True)
        return (logZ_q - logZ_p - ev).to(_out_dtype(phi_p))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        return _labeled_pq_backward(ctx, grad_out)


def _same_labeled_shape(a, b, what):
    if a.dim() != 4 or tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"{what} must be labeled like the potentials: {tuple(b.shape)}, got {tuple(a.shape)}")


def deptree_labeled_expected_score(phi, lengths, cost):
    _same_labeled_shape(cost, phi, "cost")
    return _DepTreeLabeledExpectedScore.apply(phi, lengths, cost)


def deptree_labeled_entropy(phi, lengths):
    return _DepTreeLabeledEntropy.apply(phi, lengths)


def deptree_labeled_cross_entropy(phi_p, phi_q, lengths):
    _same_labeled_shape(phi_q, phi_p, "the other distribution's potentials")
    return _DepTreeLabeledCrossEntropy.apply(phi_p, phi_q, lengths)


def deptree_labeled_kl(phi_p, phi_q, lengths):
    _same_labeled_shape(phi_q, phi_p, "the other distribution's potentials")
    return _DepTreeLabeledKL.apply(phi_p, phi_q, lengths)


def dmv1o_expect(dec, attach, lengths, v=None, v_sub=None, want_mu=False, want_hv=False):
    """Raw launcher of the dual-number DMV1o pass (vlg_dmv1o_expect).  dec [B,N,2,2,2], attach [B,N,N,2] root-merged; v, v_sub: pairs
    (dec-shaped, attach-shaped) or None, either member may be None (= 0): the direction is v - v_sub.  Returns (logZ [B], ev [B] =
    <mu, v - v_sub>, mu_dec, mu_attach, hv_dec, hv_attach), all float32; the mu pair is None unless want_mu, the hv pair = (Hessian of
    logZ)(v - v_sub) None unless want_hv.  Without either only the inside pass runs.  One launch, no host synchronisation."""
    _C.require_gpu(dec, "dmv1o_expect")
    if dec.dim() != 5 or tuple(dec.shape[2:]) != (2, 2, 2):
        raise ValueError(f"dec must be [B,N,2,2,2], got {tuple(dec.shape)}")
    B, N = dec.shape[:2]
    if tuple(attach.shape) != (B, N, N, 2):
        raise ValueError(f"attach must be [B,N,N,2] = {(B, N, N, 2)}, got {tuple(attach.shape)}")
    if dec.dtype != attach.dtype:
        attach = attach.to(dec.dtype)
    dt, dec_c = _C.in_dtype(dec)
    _, att_c = _C.in_dtype(attach)
    dirs = [*(v if v is not None else (None, None)), *(v_sub if v_sub is not None else (None, None))]   # v_dec, v_att, sub_dec, sub_att
    dshape, ashape = (B, N, 2, 2, 2), (B, N, N, 2)
    L = _C.lib()
    dirs, vdt, (logZ, ev, mu_d, mu_a, hv_d, hv_a), ws, nb = _expect_frame(
        "dmv1o_expect", dec.device, B, N, dirs=dirs, shapes=(dshape, ashape) * 2,
        shape_error=f"direction must be (dec-shaped, attach-shaped) = ({dshape}, {ashape})", grad=want_mu or want_hv,
        outs=(dshape if want_mu else None, ashape if want_mu else None, dshape if want_hv else None, ashape if want_hv else None),
        ws_bytes=lambda B, N, grad: L.vlg_dmv1o_expect_workspace(B, N, int(grad)))
    lengths = _lengths(lengths, B, dec.device)
    _C.check(L.vlg_dmv1o_expect(_C.ptr(dec_c), _C.ptr(att_c), _C.ptr(dirs[0]), _C.ptr(dirs[1]), _C.ptr(dirs[2]), _C.ptr(dirs[3]), _C.ptr(lengths),
                                B, N, dt, vdt, _C.ptr(logZ), _C.ptr(ev), _C.ptr(mu_d), _C.ptr(mu_a), _C.ptr(hv_d), _C.ptr(hv_a), _C.ptr(ws), nb,
                                _C.stream_of(dec)), "dmv1o_expect")
    return logZ, ev, mu_d, mu_a, hv_d, hv_a


def _col(t, like):
    "[B] float32 -> [B,1] in the dtype DMV1o.partition returns for these potentials"
    return t.view(-1, 1).to(_out_dtype(like))


class _DMV1oExpectedScore(torch.autograd.Function):
    """E_p[<cost, tree>] (the reference's `risk`): value ev, d/d potentials = hv = Cov(tree, <cost, tree>), d/d cost = mu."""

    @staticmethod
    def forward(ctx, dec, attach, lengths, cost_dec, cost_attach):
        need = ctx.needs_input_grad
        _, ev, mu_d, mu_a, hv_d, hv_a = dmv1o_expect(dec, attach, lengths, v=(cost_dec, cost_attach), want_mu=need[3] or need[4],
                                                     want_hv=need[0] or need[1])
        ctx.save_for_backward(hv_d, hv_a, mu_d, mu_a)
        ctx.in_dtypes = (dec.dtype, attach.dtype, None if cost_dec is None else cost_dec.dtype, None if cost_attach is None else cost_attach.dtype)
        return _col(ev, dec)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        hv_d, hv_a, mu_d, mu_a = ctx.saved_tensors
        need, dts = ctx.needs_input_grad, ctx.in_dtypes
        gd, ga = _scale_counts(hv_d if need[0] else None, hv_a if need[1] else None, grad_out, dts[0], dts[1])
        cd, ca = _scale_counts(mu_d if need[3] else None, mu_a if need[4] else None, grad_out, dts[2], dts[3])
        return gd, ga, None, cd, ca


class _DMV1oEntropy(torch.autograd.Function):
    """H[p] = logZ - <mu, theta>: the direction is the distribution's own potentials; d/d theta = -hv."""

    @staticmethod
    def forward(ctx, dec, attach, lengths):
        want = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        logZ, ev, _, _, hv_d, hv_a = dmv1o_expect(dec, attach, lengths, v=(dec, attach), want_hv=want)
        ctx.save_for_backward(hv_d, hv_a)
        ctx.in_dtypes = (dec.dtype, attach.dtype)
        return _col(logZ - ev, dec)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        hv_d, hv_a = ctx.saved_tensors
        need = ctx.needs_input_grad
        gd, ga = _scale_counts(hv_d if need[0] else None, hv_a if need[1] else None, -grad_out, *ctx.in_dtypes)
        return gd, ga, None


def _dmv1o_pq(ctx, dec_p, att_p, dec_q, att_q, lengths, sub):
    """The two launches cross-entropy and KL share (see _deptree_pq): p along v = theta_q (- theta_p when `sub`), q with no direction.
    The q side runs the outside pass only when q wants a gradient (a fixed q costs one inside pass): the value pass of the inside-only
    image and of the inside-outside image is the same sequence of operations (vlg_dmv_expect.h: dmv_expect_fw_span), so on equal
    potentials the two logZ agree bit for bit whichever images ran."""
    need = ctx.needs_input_grad
    wp, wq = need[0] or need[1], need[2] or need[3]
    logZ_p, ev, mu_d, mu_a, hv_d, hv_a = dmv1o_expect(dec_p, att_p, lengths, v=(dec_q, att_q), v_sub=(dec_p, att_p) if sub else None,
                                                      want_mu=wq, want_hv=wp)
    logZ_q, _, mq_d, mq_a, _, _ = dmv1o_expect(dec_q, att_q, lengths, want_mu=wq)
    if wq:
        mu_d.sub_(mq_d)          # in place: -(d/d theta_q) = mu_p - mu_q, scaled together with hv by -grad in backward
        mu_a.sub_(mq_a)
    ctx.save_for_backward(hv_d, hv_a, mu_d, mu_a)
    ctx.in_dtypes = (dec_p.dtype, att_p.dtype, dec_q.dtype, att_q.dtype)
    return logZ_p, logZ_q, ev


def _dmv1o_pq_backward(ctx, grad_out):
    hv_d, hv_a, dmu_d, dmu_a = ctx.saved_tensors
    need, dts = ctx.needs_input_grad, ctx.in_dtypes
    g = -grad_out
    gpd, gpa = _scale_counts(hv_d if need[0] else None, hv_a if need[1] else None, g, dts[0], dts[1])
    gqd, gqa = _scale_counts(dmu_d if need[2] else None, dmu_a if need[3] else None, g, dts[2], dts[3])
    return gpd, gpa, gqd, gqa, None


class _DMV1oCrossEntropy(torch.autograd.Function):
    """H[p,q] = logZ_q - <mu_p, theta_q>; d/d theta_p = -hv, d/d theta_q = mu_q - mu_p."""

    @staticmethod
    def forward(ctx, dec_p, att_p, dec_q, att_q, lengths):
        _, logZ_q, ev = _dmv1o_pq(ctx, dec_p, att_p, dec_q, att_q, lengths, False)
        return _col(logZ_q - ev, dec_p)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        return _dmv1o_pq_backward(ctx, grad_out)


class _DMV1oKL(torch.autograd.Function):
    """KL[p||q] = logZ_q - logZ_p - <mu_p, theta_q - theta_p> (the subtraction is the kernel's v - v_sub); gradients as for H[p,q]."""

    @staticmethod
    def forward(ctx, dec_p, att_p, dec_q, att_q, lengths):
        logZ_p, logZ_q, ev = _dmv1o_pq(ctx, dec_p, att_p, dec_q, att_q, lengths, True)
        return _col(logZ_q - logZ_p - ev, dec_p)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        return _dmv1o_pq_backward(ctx, grad_out)


def dmv1o_expected_score(dec, attach, lengths, cost_dec=None, cost_attach=None):
    return _DMV1oExpectedScore.apply(dec, attach, lengths, cost_dec, cost_attach)


def dmv1o_entropy(dec, attach, lengths):
    return _DMV1oEntropy.apply(dec, attach, lengths)


def dmv1o_cross_entropy(dec_p, att_p, dec_q, att_q, lengths):
    return _DMV1oCrossEntropy.apply(dec_p, att_p, dec_q, att_q, lengths)


def dmv1o_kl(dec_p, att_p, dec_q, att_q, lengths):
    return _DMV1oKL.apply(dec_p, att_p, dec_q, att_q, lengths)


def dmv1o_merge(dec, attach, root, one=0.0, zero=NEGINF):
    """DMV1o.merge (distributions.py:253-265): root-augmented potentials, always float32."""
    _C.require_gpu(dec, "dmv1o_merge")
    B, Lw = dec.shape[:2]
    if tuple(dec.shape) != (B, Lw, 2, 2, 2) or tuple(attach.shape) != (B, Lw, Lw, 2) or tuple(root.shape) != (B, Lw):
        raise ValueError(f"merge: dec {tuple(dec.shape)}, attach {tuple(attach.shape)}, root {tuple(root.shape)}")
    dt, dec_c = _C.in_dtype(dec)
    attach = attach.detach().to(dec_c.dtype).contiguous()
    root = root.detach().to(dec_c.dtype).contiguous()
    N = Lw + 1
    dec_w = torch.empty((B, N, 2, 2, 2), dtype=torch.float32, device=dec.device)
    att_w = torch.empty((B, N, N, 2), dtype=torch.float32, device=dec.device)
    _C.check(_C.lib().vlg_dmv1o_merge(_C.ptr(dec_c), _C.ptr(attach), _C.ptr(root), B, Lw, dt, float(one), float(zero),
                                      _C.ptr(dec_w), _C.ptr(att_w), _C.stream_of(dec)), "dmv1o_merge")
    return dec_w, att_w


class _Merge(torch.autograd.Function):
    """merge is fill + copy; its adjoint is three slices (the reference gets this from autograd on the
    in-place index assignments of distributions.py:260-264)."""

    @staticmethod
    def forward(ctx, dec, attach, root, one, zero):
        ctx.in_dtypes = (dec.dtype, attach.dtype, root.dtype)
        return dmv1o_merge(dec, attach, root, one, zero)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_dec_w, g_att_w):
        d0, d1, d2 = ctx.in_dtypes
        return (g_dec_w[:, 1:].to(d0), g_att_w[:, 1:, 1:, :].to(d1), g_att_w[:, 0, 1:, 1].to(d2), None, None)


def dmv1o_merge_autograd(dec, attach, root, one=0.0, zero=NEGINF):
    return _Merge.apply(dec, attach, root, one, zero)


_SIDE_STREAMS = {}


def _marginals_viterbi_one_launch(dec, attach, lengths, keep_viterbi, keep_partition=False):
    """Both DPs of `dmv1o_marginals_and_heads` as ONE launch on the current stream (vlg_dmv1o_marginals_viterbi: grid (B, 2), the two
    workgroups of a sentence share a CU): sentences short enough that both passes keep their charts in LDS (N <= 44: twice the larger footprint within 160 KB).  No side
    stream, no events: ~15 us less than the two-stream form at B = 256, L = 40 and nothing for a HIP-graph capture to fork."""
    if tuple(dec.shape[2:]) != (2, 2, 2):
        raise ValueError(f"dec must be [B,N,2,2,2], got {tuple(dec.shape)}")
    B, N = dec.shape[:2]
    if tuple(attach.shape) != (B, N, N, 2):
        raise ValueError(f"attach must be [B,N,N,2] = {(B, N, N, 2)}, got {tuple(attach.shape)}")
    if dec.dtype != attach.dtype:
        attach = attach.to(dec.dtype)
    dt, dec_c = _C.in_dtype(dec)
    _, att_c = _C.in_dtype(attach)
    lengths = _lengths(lengths, B, dec.device)
    dev = dec.device
    logZ, best = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev)
    gatt = torch.empty((B, N, N, 2), dtype=torch.float32, device=dev)
    heads = torch.empty((B, N), dtype=torch.int64, device=dev)
    vdec = torch.empty((B, N, 2, 2, 2), dtype=torch.float32, device=dev) if keep_viterbi else None
    vatt = torch.empty((B, N, N, 2), dtype=torch.float32, device=dev) if keep_viterbi else None
    gdec = torch.empty((B, N, 2, 2, 2), dtype=torch.float32, device=dev) if keep_partition else None
    _C.check(_C.lib().vlg_dmv1o_marginals_viterbi(_C.ptr(dec_c), _C.ptr(att_c), _C.ptr(lengths), B, N, dt, _C.ptr(logZ), _C.ptr(gdec), _C.ptr(gatt),
                                                  _C.ptr(best), _C.ptr(vdec), _C.ptr(vatt), _C.ptr(heads), _C.stream_of(dec)),
             "dmv1o_marginals_viterbi")
    if keep_viterbi:
        _viterbi_remember(dec, attach, lengths, (best, vdec, vatt, heads))
    if keep_partition:
        _partition_remember(dec, attach, lengths, (logZ, gdec, gatt))
    return logZ, gatt, heads


def dmv1o_marginals_and_heads(dec, attach, lengths, keep_viterbi=False, keep_partition=False):
    """What lang_feat_max_tree needs from one sentence batch (joint.py:251-258): the arc marginals
    d logZ / d attach AND the Viterbi heads.  The two are independent DPs over the same potentials; at one
    workgroup per CU each leaves most of the machine idle and their LDS footprints (78 KB + 49 KB at N = 41) fit one
    CU together, so the decode runs on a side HIP stream next to the inside-outside launch and joins before returning.
    Returns (logZ [B], marginals [B,N,N,2], heads [B,N]).

    keep_viterbi=True (training with `viterbi_training`, ldndmv.py:277-281): the side-stream launch is the full Viterbi pass
    (best score + tree counts + heads, 67 us instead of the 57 us walk) and its result is remembered, so the `DMV1o(...).max`
    that the loss takes of the same potentials later in the step launches nothing.

    keep_partition=True (training with the marginal loss, `viterbi_training: false`, ldndmv.py:280-281): the inside-outside pass also
    writes the dec counts and (logZ, grad_dec, grad_attach) is remembered, so a later `DMV1o(same potentials).partition` and its
    backward launch nothing either."""
    _C.require_gpu(dec, "dmv1o_marginals_and_heads")
    if dec.dim() == 5 and _C.lib().vlg_dmv1o_marginals_viterbi_supported(dec.shape[1]):
        return _marginals_viterbi_one_launch(dec, attach, lengths, keep_viterbi, keep_partition)
    cur = torch.cuda.current_stream(dec.device)
    side = _SIDE_STREAMS.get(dec.device)
    if side is None:
        side = _SIDE_STREAMS[dec.device] = torch.cuda.Stream(device=dec.device)
    # The decode's outputs are allocated HERE, on the current stream, and the side stream joins before this returns: every later
    # use, free or reuse of them -- and of the inputs -- is ordered behind the side stream's work by that join, so no
    # `record_stream` bookkeeping is needed (it is what made a HIP-graph capture crash while tensors of an earlier eager
    # step were still alive: the allocator's deferred event handling for recorded streams is not capture-safe).
    B, N = dec.shape[:2]
    best = torch.empty(B, dtype=torch.float32, device=dec.device)
    heads = torch.empty((B, N), dtype=torch.int64, device=dec.device)
    if keep_viterbi or keep_partition:
        lengths = _lengths(lengths, B, dec.device)
    if keep_viterbi:
        vdec = torch.empty((B, N, 2, 2, 2), dtype=torch.float32, device=dec.device)
        vatt = torch.empty((B, N, N, 2), dtype=torch.float32, device=dec.device)
    # The potentials are produced on the current stream: the side stream waits for an event recorded HERE, and the longer of the
    # two launches (the Log-semiring inside-outside pass) is enqueued first -- it starts ~6 us earlier than when it followed the
    # side-stream launch, and the pair ends when it does.
    ready = torch.cuda.Event()
    ready.record(cur)
    logZ, gdec, gatt = dmv1o_run(dec, attach, lengths, _C.SEMIRING_LOG, True, want_dec=keep_partition)
    side.wait_event(ready)
    with torch.cuda.stream(side):
        if keep_viterbi:
            dmv1o_viterbi(dec, attach, lengths, out=(best, vdec, vatt, heads))
        else:
            dmv1o_decode(dec, attach, lengths, out=(best, heads))
    cur.wait_stream(side)
    if keep_viterbi:
        _viterbi_remember(dec, attach, lengths, (best, vdec, vatt, heads))
    if keep_partition:
        _partition_remember(dec, attach, lengths, (logZ, gdec, gatt))
    return logZ, gatt, heads


class StructureHandle:
    """Both DPs of lang_feat_max_tree in flight on two side streams (see dmv1o_structure_async); `wait()` joins them into the
    current stream and returns (logZ [B], marginals [B,N,N,2], heads [B,N])."""

    def __init__(self, streams, outs, device):
        self._streams, self._outs, self._device, self._joined = streams, outs, device, set()

    def join_current(self):
        """Orders the CURRENT stream behind both side streams (idempotent per stream; cheap: two event waits)."""
        cur = torch.cuda.current_stream(self._device)
        if cur not in self._joined:
            for st in self._streams:
                cur.wait_stream(st)
            self._joined.add(cur)

    def wait(self):
        self.join_current()
        return self._outs


_SIDE_STREAMS2 = {}


def dmv1o_structure_async(dec, attach, lengths, keep_viterbi=False):
    """`dmv1o_marginals_and_heads` without occupying the current stream: the Log-semiring inside-outside pass AND the Viterbi
    pass go to two side streams (ordered after what the current stream has enqueued so far: the potentials), and the caller
    keeps enqueueing work that does not need them -- in the training step the attention-fuse, the root row and the encoders'
    projection GEMM (37 us of kernels) run beside the 93 us the DPs take at one workgroup per CU each.  `.wait()` joins.
    Outputs are allocated here, on the current stream (the reasoning of dmv1o_marginals_and_heads applies)."""
    _C.require_gpu(dec, "dmv1o_structure_async")
    dev = dec.device
    cur = torch.cuda.current_stream(dev)
    pair = _SIDE_STREAMS2.get(dev)
    if pair is None:
        pair = _SIDE_STREAMS2[dev] = (torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev))
    B, N = dec.shape[:2]
    lengths = _lengths(lengths, B, dev)
    logZ = torch.empty(B, dtype=torch.float32, device=dev)
    gatt = torch.empty((B, N, N, 2), dtype=torch.float32, device=dev)
    best = torch.empty(B, dtype=torch.float32, device=dev)
    heads = torch.empty((B, N), dtype=torch.int64, device=dev)
    if keep_viterbi:
        vdec = torch.empty((B, N, 2, 2, 2), dtype=torch.float32, device=dev)
        vatt = torch.empty((B, N, N, 2), dtype=torch.float32, device=dev)
    for st in pair:
        st.wait_stream(cur)
    with torch.cuda.stream(pair[0]):
        dmv1o_run(dec, attach, lengths, _C.SEMIRING_LOG, True, want_dec=False, out=(logZ, None, gatt))
    with torch.cuda.stream(pair[1]):
        if keep_viterbi:
            dmv1o_viterbi(dec, attach, lengths, out=(best, vdec, vatt, heads))
        else:
            dmv1o_decode(dec, attach, lengths, out=(best, heads))
    handle = StructureHandle(pair, (logZ, gatt, heads), dev)
    if keep_viterbi:   # the entry carries the handle: a lookup joins the side streams before it returns the hit
        _viterbi_remember(dec, attach, lengths, (best, vdec, vatt, heads), pending=handle)
    return handle
