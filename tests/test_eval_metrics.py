"""CPU: the evaluation metrics' definition.  The numpy restatement (tests/eval_restatement.py) of the counters equals what the reference's own
DependencyParsingMetric / FactorImageMatchingMetric / BoxRelMatchingMetric accumulated over two consecutive batches (fixtures made by
tests/golden/make_golden_eval.py, which runs those classes), integer for integer; `metrics.compute_from_counts` reproduces their `compute()`
dict; the new C entry points validate their arguments on the host.  The GPU tests (test_eval_step_gpu.py) hold the kernel to the same
fixtures and, beyond them, to the restatement."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest

from conftest import ROOT
from eval_restatement import COUNTS, add_counts, eval_counts

GOLDEN = os.path.join(ROOT, "tests", "golden")
METRIC_FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "evalmetric_*.npz")))
STEP_FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "evalstep_*.npz")))


def batch_of(z, i):
    """Keyword arguments of eval_counts for batch i of an evalmetric_* fixture."""
    kw = dict(pred=z[f"pred_arc_{i}"], gold=z[f"gold_arc_{i}"], mask=z[f"mask_{i}"], lengths=z[f"lengths_{i}"], factor2img=z[f"factor2img_{i}"],
              top5=z[f"top5_{i}"], factors=tuple(str(f) for f in z["factors"]))
    if f"sg_box_{i}" in z.files:
        kw.update(vis_box=z[f"vis_box_{i}"], sg_box=z[f"sg_box_{i}"], sg_type=z[f"sg_type_{i}"], sg_mask=z[f"sg_mask_{i}"])
    return kw


def test_fixtures_exist():
    assert len(METRIC_FIXTURES) == 3 and len(STEP_FIXTURES) == 2, (METRIC_FIXTURES, STEP_FIXTURES)


@pytest.mark.parametrize("path", METRIC_FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_restatement_equals_the_reference_counters(path):
    z = np.load(path)
    assert tuple(z["counter_names"]) == COUNTS
    total = dict.fromkeys(COUNTS, 0)
    for i in range(2):
        kw = batch_of(z, i)
        if "sg_box" in kw:   # the reference only runs where every sentence has at least K scored tokens
            assert (kw["mask"].sum(1) >= 5).all()
        total = add_counts(total, eval_counts(**kw))
        assert [total[k] for k in COUNTS] == z[f"counters_{i}"].tolist(), (i, total, dict(zip(COUNTS, z[f"counters_{i}"].tolist())))
    if "sg_box_0" in z.files:   # the fixture exercises all four correct_* counters
        assert all(total[k] > 0 for k in ("correct_obj", "correct_attr", "correct_rel", "correct_r_rel"))
    check_compute(total, [float(z["loss_0"]), float(z["loss_1"])], json.loads(str(z["compute"])))


def check_compute(counts, losses, want):
    from vlgae_amd import metrics
    loss_sum = 0.0
    for v in losses:             # float64 adds of float32 values, in batch order: Python's sum of `.item()`s
        loss_sum += float(np.float32(v))
    got = metrics.compute_from_counts(dict(counts, n_batches=len(losses), loss_sum=loss_sum))
    assert set(got) == set(want) == {"ucm", "uas", "factor2img/acc", "box/acc", "box/obj", "box/attr", "box/rel", "loss"}
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-6, abs=1e-30), (k, got[k], v)
    assert got["loss"] == want["loss"]   # the same float64 arithmetic


@pytest.mark.parametrize("path", STEP_FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_restatement_equals_the_reference_counters_of_the_eval_step(path):
    """The same on the reference's whole eval step: its decoded heads, top-5 columns and factor -> image, through its metric classes,
    the same batch twice."""
    z = np.load(path)
    t = np.load(path.replace("evalstep_", "trainstep_"))
    factors = tuple(str(f) for f in t["factor_names"][1:])
    kw = dict(pred=z["arc_viterbi"], gold=z["gold_arc"], mask=z["mask"], lengths=t["lengths"], factor2img=z["factor2img"], top5=z["top5"], factors=factors)
    if bool(z["with_sg"]):
        kw.update(vis_box=z["vis_box"], sg_box=z["sg_box"], sg_type=z["sg_type"], sg_mask=z["sg_mask"])
        assert (z["mask"].sum(1) >= 5).all()
    one = eval_counts(**kw)
    assert [one[k] for k in COUNTS] == z["counters_0"].tolist()
    two = add_counts(one, one)
    assert [two[k] for k in COUNTS] == z["counters_1"].tolist()
    check_compute(two, [float(z["loss"])] * 2, json.loads(str(z["compute"])))
    # the lists `write_prediction` gets: align.grounding_lists on the fixture's index arrays = the reference's own lists
    import torch
    from vlgae_amd import align
    rows = z["txt_mask"]
    live = np.take_along_axis(z["logit"], z["top5"].astype(np.int64), -1) > -1e5     # ranks with a dead (tied) value have no defined column
    lists = align.grounding_lists(torch.from_numpy(z["top5"]), torch.from_numpy(z["factor2img"]), torch.from_numpy(rows), list(t["factor_names"]),
                                  t["vis_split"].tolist())
    want = json.loads(str(z["txt_to_factor"]))
    keep_live = [[live[b, q] for q in np.flatnonzero(rows[b])] for b in range(len(rows))]
    for b, (got_b, want_b) in enumerate(zip(lists["txt_to_factor"], want)):
        assert len(got_b) == len(want_b)
        for q, (g_row, w_row) in enumerate(zip(got_b, want_b)):
            for k, (g_item, w_item) in enumerate(zip(g_row, w_row)):
                if keep_live[b][q][k]:
                    assert g_item[0] == w_item[0] and (list(g_item[1]) if isinstance(g_item[1], tuple) else g_item[1]) == w_item[1], (b, q, k)
    assert [[int(v) for v in row] for row in lists["txt_to_img"]] == json.loads(str(z["txt_to_img"]))


def test_short_sentences_and_corner_cases_of_the_definition():
    """m < K (the reference raises there; the definition here: every prediction of every scored token is valid), an empty mask (counts
    for ucm), a punctuation hole (the FIRST m words are scored, not the masked positions), type-0 first prediction, 0 / 0 IoU."""
    R, L = 3, 4
    vis_box = np.array([[[0, 0, 1, 1], [2, 2, 3, 3], [0, 0, 0, 0]]], np.float32)
    top5 = np.zeros((1, 2 * (L + 1), 5), np.int32)
    top5[0, 1] = [0, 1, 2, 3, 4]          # token 0: obj 0 first
    top5[0, 2] = [12, 0, 1, 2, 3]         # token 1: the image factor first (V - 1 = 3 + 9 + 0 + 1 - 1 = 12), obj 0 second
    top5[0, 3] = [3 + 0 * 3 + 1, 0, 1, 2, 5]   # token 2: rel (0, 1) first
    sg_box = np.zeros((1, L, 8), np.float32)
    sg_box[0, 0, :4] = [0, 0, 1, 1]
    sg_box[0, 1, :4] = [0, 0, 1, 1]
    sg_box[0, 2] = [2, 2, 3, 3, 0, 0, 1, 1]   # the pair swapped: r_rel
    sg_type = np.array([[1, 1, 3, 2]])
    kw = dict(gold=np.array([[0, 1, 2, 3]]), lengths=np.array([4]), top5=top5, vis_box=vis_box, sg_box=sg_box, sg_type=sg_type, sg_mask=sg_type != 0,
              factors=("rel", "img"), factor2img=np.zeros((1, 10), np.int32))
    c = eval_counts(pred=np.array([[0, 1, 2, 0]]), mask=np.array([[1, 1, 1, 0]], bool), **kw)   # m = 3 < K = 5
    assert (c["correct_obj"], c["correct_rel"], c["correct_r_rel"], c["total_obj"], c["total_attr"], c["total_rel"]) == (1, 0, 1, 2, 1, 1)
    assert (c["n_ucm"], c["correct_arcs"], c["total"], c["processed_token"], c["f2i_total"], c["f2i_correct"]) == (1, 3, 3, 3, 8, 8)
    c = eval_counts(pred=np.array([[0, 1, 2, 0]]), mask=np.array([[0, 1, 1, 0]], bool), **kw)   # a hole at word 0: words 0 and 1 are scored
    assert (c["correct_obj"], c["correct_r_rel"], c["total"]) == (1, 0, 2)
    c = eval_counts(pred=np.array([[9, 9, 9, 9]]), mask=np.zeros((1, 4), bool), **kw)
    assert (c["n_ucm"], c["total"], c["correct_obj"], c["processed_token"]) == (1, 0, 0, 0)
    sg_box[0, 0, :4] = 0                      # gold and prediction both empty boxes: 0 / 0, not a match
    top5[0, 1, 0] = 2
    kw["top5"] = top5[:, :, [0, 0, 0, 0, 0]]
    c = eval_counts(pred=np.array([[0, 1, 2, 0]]), mask=np.array([[1, 0, 0, 0]], bool), **kw)
    assert c["correct_obj"] == 0


def test_compute_arithmetic_from_given_counts():
    from vlgae_amd import metrics
    c = dict(correct_arcs=30, total=40, n_ucm=1, n=8, f2i_correct=5, f2i_total=20, correct_obj=3, correct_attr=1, correct_rel=2, correct_r_rel=4,
             total_obj=6, total_attr=4, total_rel=10, processed_token=40, n_batches=2, loss_sum=3.0)
    got = metrics.compute_from_counts(c)
    assert got["ucm"] == pytest.approx(12.5) and got["uas"] == pytest.approx(75.0) and got["factor2img/acc"] == pytest.approx(25.0, rel=1e-6)
    assert got["box/acc"] == pytest.approx(100 * (3 + 1 + 4) / 20) and got["box/rel"] == pytest.approx(20.0)   # acc takes max(rel, r_rel); rel does not
    assert got["box/obj"] == pytest.approx(50.0) and got["box/attr"] == pytest.approx(25.0) and got["loss"] == pytest.approx(1.5)
    zero = metrics.compute_from_counts(dict.fromkeys(metrics.SLOTS, 0))
    assert all(v == 0 for v in zero.values())          # the EPS / 1e-6 / 1e-9 in the denominators: no division by zero before the first batch
    # EvalCounters reads its buffer the same way (a host tensor can be read; updating needs the GPU)
    import torch
    ec = metrics.EvalCounters(torch.device("cpu"))
    ec.buf[:15] = torch.tensor([c[k] for k in metrics.SLOTS[:15]])
    ec.buf[15:].view(torch.float64)[0] = 3.0
    assert ec.compute() == got and ec.counts()["loss_sum"] == 3.0
    ec.reset()
    assert ec.compute() == zero
    with pytest.raises(RuntimeError, match="MI355X"):
        ec.update(torch.zeros(1, 2, dtype=torch.int64), torch.zeros(1, 2, dtype=torch.int64), torch.ones(1, 2, dtype=torch.bool), torch.tensor([2]))


def test_new_entry_points_validate_on_the_host():
    from vlgae_amd.build import build_library
    build_library()
    from vlgae_amd import _C
    lib = _C.lib()
    one = ctypes.c_void_p(64)
    need = lib.vlg_eval_metrics_workspace(4)
    assert need > 0 and need % 256 == 0 and lib.vlg_eval_metrics_workspace(0) == 0 and lib.vlg_eval_metrics_workspace(8) >= 2 * need - 256
    em = lib.vlg_eval_metrics
    ok = lambda **kw: [kw.get("pred", one), kw.get("ld", 6), one, one, one, kw.get("f2i", one), kw.get("top5", one), kw.get("vis_box", one),
                       kw.get("sg_box", one), one, one, None, kw.get("B", 4), kw.get("L", 6), kw.get("Q", 14), kw.get("R", 5), 1, 1, 0,
                       kw.get("ws", one), kw.get("ws_bytes", need), kw.get("counters", one), None]
    assert em(*ok(B=0)) == 0                                                           # empty batch: nothing to do
    assert em(*ok(B=-1)) == 0x1001 and em(*ok(L=0)) == 0x1001
    assert em(*ok(ld=5)) == 0x1001 and b"ld_pred" in lib.vlg_last_error()
    assert em(*ok(pred=None)) == 0x1003 and em(*ok(counters=None)) == 0x1003
    assert em(*ok(sg_box=None)) == 0x1003 and b"go together" in lib.vlg_last_error()
    assert em(*ok(top5=None)) == 0x1003
    assert em(*ok(Q=13)) == 0x1001 and b"query rows" in lib.vlg_last_error()
    assert em(*ok(R=0)) == 0x1001
    assert em(*ok(ws_bytes=need - 1)) == 0x1004 and em(*ok(ws=None)) == 0x1004
    mbr = lib.vlg_deptree_mbr_decode
    assert mbr(one, one, 4, 1, one, one, None, 0, None) == 0x1001 and mbr(one, one, 4, 300, one, one, None, 0, None) == 0x1001
    assert mbr(None, one, 4, 8, one, one, None, 0, None) == 0x1003 and mbr(one, one, 4, 8, one, None, None, 0, None) == 0x1003
    assert mbr(one, one, 0, 8, one, one, None, 0, None) == 0
    assert mbr(one, one, 4, 200, one, one, None, 0, None) == 0x1004                     # long sentences spill: the workspace is checked first
