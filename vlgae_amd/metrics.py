"""Evaluation metrics on the device -- host-side mirror of `metric.update(predict, y, mask)` / `metric.compute()` in
`Pipeline.validation_step` / `validation_epoch_end` (src/pipeline.py:132-151; paths relative to the reference checkout):

    DependencyParsingMetric     src/utility/metric.py:18-61     ucm, uas
    FactorImageMatchingMetric   :64-83                          factor2img/acc
    BoxRelMatchingMetric        :108-208                        box/acc | obj | attr | rel

as sixteen int64 counters that one pair of launches per batch (vlg_eval_metrics) adds into; nothing is read on the host before
`compute()`.  What every counter means is written out next to the C declaration (include/vlgae_amd.h) and, executable, in
tests/eval_restatement.py.  One divergence from the reference, on purpose: BoxRelMatchingMetric raises a shape error for a sentence with
fewer scored tokens than predictions per token (m < min(5, V), metric.py:171 takes `len()` of the token list for the prediction count);
where it runs, every prediction of every scored token is valid, and that is the definition used here for every m >= 1.
`CaptionImageMatchingMetric` belongs to the `on_img` decoder (not the shipped one) and labelled parsing metrics need relation labels
the parser does not predict: neither is here."""
import torch

from . import _C

SLOTS = ("correct_arcs", "total", "n_ucm", "n", "f2i_correct", "f2i_total", "correct_obj", "correct_attr", "correct_rel", "correct_r_rel",
         "total_obj", "total_attr", "total_rel", "processed_token", "n_batches", "loss_sum")   # VLG_EVAL_* of include/vlgae_amd.h
EPS = 1e-12   # metric.py:15


def compute_from_counts(c):
    """`MultiMetric.compute()` (metric.py:266-274: main = parsing, factor2img, box) plus `val_result['loss']` (pipeline.py:149) from a
    dict of counts by SLOTS name.  The reference divides float32 state tensors; here the counts are exact integers and the division is
    Python's (the results agree to float32 rounding)."""
    rel = max(c["correct_rel"], c["correct_r_rel"])                                     # metric.py:199
    return {
        "ucm": 100 * c["n_ucm"] / (c["n"] + EPS),
        "uas": 100 * c["correct_arcs"] / (c["total"] + EPS),
        "factor2img/acc": 100 * c["f2i_correct"] / (c["f2i_total"] + 1e-6),
        "box/acc": 100 * (c["correct_obj"] + c["correct_attr"] + rel) / (c["total_obj"] + c["total_attr"] + c["total_rel"] + EPS),
        "box/obj": 100 * c["correct_obj"] / (c["total_obj"] + EPS),
        "box/attr": 100 * c["correct_attr"] / (c["total_attr"] + EPS),
        "box/rel": 100 * c["correct_rel"] / (c["total_rel"] + EPS),
        "loss": c["loss_sum"] / (c["n_batches"] + 1e-9),
    }


class EvalCounters:
    """The running counters of one evaluation epoch: `reset()` at its start, `update(...)` per batch (two launches, no host
    synchronisation: capturable), `compute()` at its end (the one host read)."""

    def __init__(self, device):
        self.buf = torch.zeros(len(SLOTS), dtype=torch.int64, device=device)

    def reset(self):
        self.buf.zero_()

    def update(self, pred_arc, gold_arc, mask, lengths, factor2img=None, top5=None, vis_box=None, sg_box=None, sg_type=None, sg_mask=None,
               loss=None, factors=()):
        """One batch.  pred_arc [B,L] int64 (any row stride: a view of the decoder's heads [B,L+1] works), gold_arc [B,L] int64,
        mask [B,L] bool / uint8 (the batch's `punct_mask`) or None (= vp.mask, the length mask, built inside the kernel), lengths [B] int64; factor2img [B,Q] / top5 [B,Q,5] int32 as `align.grounding_decode` returns them;
        vis_box [B,R,4], sg_box [B,L,8] (or [B,L,2,4]) float32, sg_type [B,L] int64, sg_mask [B,L] bool: all four or none (a batch
        without `sg_box` skips the box metric, metric.py:123-125); loss: the batch's reduced loss, 0-d float32; factors: which of
        ("rel", "attr", "img") the model's factor layout has beside the objects."""
        dev = self.buf.device
        _C.require_gpu(self.buf, "EvalCounters.update")
        B, L = gold_arc.shape
        if tuple(pred_arc.shape) != (B, L) or pred_arc.dtype != torch.int64 or pred_arc.stride(1) != 1 or pred_arc.stride(0) < L:
            raise ValueError(f"EvalCounters.update: pred_arc must be int64 [B,L] = {(B, L)} with unit column stride, got {pred_arc.dtype} "
                             f"{tuple(pred_arc.shape)} strides {pred_arc.stride()}")
        mask_c = _C.mask_u8(mask, dev)
        sg_mask_c = _C.mask_u8(sg_mask, dev)
        box = (vis_box, sg_box, sg_type, sg_mask_c)
        if any(t is not None for t in box) and (any(t is None for t in box) or top5 is None):
            raise ValueError("EvalCounters.update: vis_box, sg_box, sg_type, sg_mask and top5 go together")
        R = Q = 0
        checks = [("gold_arc", gold_arc, (B, L), torch.int64), ("lengths", lengths, (B,), torch.int64)]
        if mask_c is not None:
            checks.append(("mask", mask_c, (B, L), torch.uint8))
        if factor2img is not None or top5 is not None:
            Q = 2 * (L + 1)
        if factor2img is not None:
            checks.append(("factor2img", factor2img, (B, Q), torch.int32))
        if top5 is not None:
            checks.append(("top5", top5, (B, Q, 5), torch.int32))
        if vis_box is not None:
            R = vis_box.shape[1]
            if sg_box.dim() == 4 and sg_box.is_contiguous():
                sg_box = sg_box.view(B, L, 8)
            checks += [("vis_box", vis_box, (B, R, 4), torch.float32), ("sg_box", sg_box, (B, L, 8), torch.float32),
                       ("sg_type", sg_type, (B, L), torch.int64), ("sg_mask", sg_mask_c, (B, L), torch.uint8)]
        if loss is not None:
            checks.append(("loss", loss, (), torch.float32))
        for name, t, shape, dt in checks:
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"EvalCounters.update: {name} must be contiguous {dt} {shape} on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        if pred_arc.device != dev:
            raise ValueError(f"EvalCounters.update: pred_arc on {pred_arc.device}, counters on {dev}")
        lib = _C.lib()
        nbytes = lib.vlg_eval_metrics_workspace(B)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _C.check(lib.vlg_eval_metrics(_C.ptr(pred_arc), pred_arc.stride(0), _C.ptr(gold_arc), _C.ptr(mask_c), _C.ptr(lengths), _C.ptr(factor2img),
                                      _C.ptr(top5), _C.ptr(vis_box), _C.ptr(sg_box), _C.ptr(sg_type), _C.ptr(sg_mask_c), _C.ptr(loss), B, L, Q, R,
                                      int("rel" in factors), int("attr" in factors), int("img" in factors), _C.ptr(ws), nbytes,
                                      _C.ptr(self.buf), _C.stream_of(self.buf)), "eval_metrics")

    def counts(self):
        """The counters by name, read on the host (synchronises): integers, and `loss_sum` as the float64 it is."""
        vals = self.buf.tolist()
        out = dict(zip(SLOTS[:-1], vals))
        out["loss_sum"] = self.buf[-1:].view(torch.float64).item()
        return out

    def compute(self):
        """The reference's metric dict for everything `update` has seen since `reset()`: ucm, uas, factor2img/acc, box/acc, box/obj,
        box/attr, box/rel, loss."""
        return compute_from_counts(self.counts())
