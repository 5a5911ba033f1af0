"""The evaluation counters restated in numpy, as the reference EXECUTES them (src/utility/metric.py of the reference: DependencyParsingMetric.update
:29-39, FactorImageMatchingMetric.update :70-80 on the kept rows of txt_mask, BoxRelMatchingMetric.update :122-193).  Pinned on reference-made
fixtures by tests/test_eval_metrics.py; the GPU tests compare vlg_eval_metrics with it on inputs no fixture covers.

One definition the reference does not give: a sentence with fewer scored tokens than predictions per token (m < K = min(5, V)) makes
BoxRelMatchingMetric raise (metric.py:171 takes len() of the token list as the prediction count).  Where it runs (m >= K) all K predictions of
every scored token are valid; that is the rule here for every m >= 1."""
import numpy as np

COUNTS = ("correct_arcs", "total", "n_ucm", "n", "f2i_correct", "f2i_total", "correct_obj", "correct_attr", "correct_rel", "correct_r_rel",
          "total_obj", "total_attr", "total_rel", "processed_token")


def iou(p, g):
    """_one_by_one_iou (metric.py:228-250) of box pairs [..., 4], float32 in its operation order."""
    p, g = np.asarray(p, np.float32), np.asarray(g, np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        area1 = (p[..., 2] - p[..., 0]) * (p[..., 3] - p[..., 1])
        area2 = (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1])
        wh = np.maximum(np.minimum(p[..., 2:], g[..., 2:]) - np.maximum(p[..., :2], g[..., :2]), np.float32(0))
        inter = wh[..., 0] * wh[..., 1]
        union = area1 + area2 - inter
        return inter / union


def column_types(cols, R, factors):
    """Factor layout obj | rel | attr | img -> (type, first box, second box) of top-5 columns (joint.py:596-622, metric.py:155-167)."""
    cols = np.asarray(cols, np.int64)
    typ, bi, bj = np.zeros_like(cols), np.zeros_like(cols), np.zeros_like(cols)
    off = R
    obj = (cols >= 0) & (cols < R)
    typ[obj], bi[obj], bj[obj] = 1, cols[obj], cols[obj]
    if "rel" in factors:
        m = (cols >= off) & (cols < off + R * R)
        typ[m], bi[m], bj[m] = 3, (cols[m] - off) // R, (cols[m] - off) % R
        off += R * R
    if "attr" in factors:
        m = (cols >= off) & (cols < off + R)
        typ[m], bi[m], bj[m] = 2, cols[m] - off, cols[m] - off
    return typ, bi, bj


def eval_counts(pred, gold, mask, lengths, factor2img=None, top5=None, vis_box=None, sg_box=None, sg_type=None, sg_mask=None, factors=()):
    """The counters one batch adds: a dict of Python ints by COUNTS name."""
    pred, gold, mask = np.asarray(pred), np.asarray(gold), np.asarray(mask).astype(bool)
    B, L = gold.shape
    c = dict.fromkeys(COUNTS, 0)
    ok = (pred == gold) & mask
    c["correct_arcs"], c["total"], c["n"] = int(ok.sum()), int(mask.sum()), B
    c["n_ucm"] = int((ok.sum(1) == mask.sum(1)).sum())
    if factor2img is not None:
        N = L + 1
        for b in range(B):
            n = int(min(max(int(lengths[b]), 0), L))
            rows = list(range(1, n + 1)) + list(range(N + 1, N + n + 1))
            c["f2i_total"] += len(rows)
            c["f2i_correct"] += int(sum(int(factor2img[b, q]) == b for q in rows))
    if sg_box is None:
        return c
    R = vis_box.shape[1]
    V = R + ("rel" in factors) * R * R + ("attr" in factors) * R + ("img" in factors)
    K = min(5, V)
    sg_box = np.asarray(sg_box, np.float32).reshape(B, L, 2, 4)
    sg_type, sg_mask = np.asarray(sg_type), np.asarray(sg_mask).astype(bool)
    c["processed_token"] = int(mask.sum())
    for k, v in (("total_obj", 1), ("total_attr", 2), ("total_rel", 3)):
        c[k] = int((sg_type == v).sum())
    for b in range(B):
        m = int(mask[b].sum())
        for t in range(min(m, L)):
            if not sg_mask[b, t]:
                continue
            typ, bi, bj = column_types(top5[b, t + 1, :K], R, factors)
            p0, p1 = vis_box[b, bi], vis_box[b, bj]                      # [K,4]
            g0, g1 = sg_box[b, t, 0][None], sg_box[b, t, 1][None]
            raw0, raw1 = iou(p0, g0) > 0.5, iou(p1, g1) > 0.5
            swp0, swp1 = iou(p0, g1) > 0.5, iou(p1, g0) > 0.5
            gt = int(sg_type[b, t])
            oa = bool((raw0 & (typ < 3)).any()) and gt > 0 and typ[0] > 0
            rel = bool((raw0 & raw1 & (typ == 3)).any())
            rrel = bool((swp0 & swp1 & (typ == 3)).any())
            c["correct_obj"] += int(oa and gt == 1)
            c["correct_attr"] += int(oa and gt == 2)
            c["correct_rel"] += int(rel and gt == 3)
            c["correct_r_rel"] += int(rrel and gt == 3)
    return c


def add_counts(a, b):
    return {k: a[k] + b[k] for k in COUNTS}
