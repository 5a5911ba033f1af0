"""CPU: the gold-tree rule counts of the parser's rule-supervised initialisation epochs (vlgae_amd/rules1o.py, vlg_rules1o.hip).

  * the goldrules_* fixtures (generate_rule_1o + the padders, run by tests/golden/make_golden_init.py) against an independent numpy
    restatement of the counting rules -- this pins the reference's `decision[-1]` quirk;
  * the initstep_* fixtures: the reference's enll (gold rules . unmerged potentials) equals the count . potential sum read off the
    ROOT-MERGED potentials, the layout `gold_rule_score` reads;
  * the new C-ABI entries' argument errors, with no GPU; `train_step.build`'s and the Python API's validation."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden_files, golden_ids, load

LEFT, RIGHT, HASCHILD, NOCHILD, GO, STOP = 0, 1, 0, 1, 0, 1


def np_rules(arc, n, L):
    """The counting rules as written in include/vlgae_amd.h (vlg_dmv1o_gold_rules): (dec [L,2,2,2], attach [L,L,2], root [L]) float64."""
    dec, att, root = np.zeros((L, 2, 2, 2)), np.zeros((L, L, 2)), np.zeros(L)
    a = [int(x) for x in arc[:n]]
    if not 1 <= n <= L or any(x < 0 or x > n for x in a) or 0 not in a:
        return dec, att, root
    head = [x - 1 for x in a]
    left = [min([c for c in range(n) if head[c] == h and c < h], default=h) for h in range(n)]     # leftmost left child, else itself
    right = [max([c for c in range(n) if head[c] == h and c > h], default=h) for h in range(n)]    # rightmost right child, else itself
    for c, h in enumerate(head):
        if h >= 0:
            d = LEFT if c < h else RIGHT
            v = NOCHILD if (left if d == LEFT else right)[h] == c else HASCHILD
            att[h, c, v] += 1
            dec[h, d, v, GO] += 1
        else:   # the reference's decision[-1]
            dec[n - 1, RIGHT, NOCHILD if c == n - 1 else HASCHILD, GO] += 1
        dec[c, LEFT, NOCHILD if left[c] == c else HASCHILD, STOP] += 1
        dec[c, RIGHT, NOCHILD if right[c] == c else HASCHILD, STOP] += 1
    root[a.index(0)] = 1
    return dec, att, root


def np_batch_rules(arc, lengths, L):
    got = [np_rules(arc[b], int(lengths[b]), L) for b in range(len(lengths))]
    return tuple(np.stack([g[i] for g in got]) for i in range(3))


@pytest.mark.parametrize("path", golden_files("goldrules_"), ids=golden_ids("goldrules_"))
def test_goldrules_fixtures_match_the_restatement(path):
    g = load(path)
    L = g["dec_rule"].shape[1]
    dec, att, root = np_batch_rules(g["arc"], g["lengths"], L)
    assert np.array_equal(dec, g["dec_rule"]) and np.array_equal(att, g["attach_rule"]) and np.array_equal(root, g["root_rule"])


def test_goldrules_fixture_pins_the_root_quirk():
    """decision[-1]: every root child adds a GO of the LAST word to the right, NOCHILD only for the last word itself."""
    g = load(golden_files("goldrules_B10_L6")[0])
    for b, n in enumerate(g["lengths"]):
        arc = g["arc"][b, :n]
        own = sum(1 for c in range(n) if arc[c] - 1 == n - 1 and c > n - 1)   # (none: nothing lies right of the last word)
        roots = [c for c in range(n) if arc[c] == 0]
        assert g["dec_rule"][b, n - 1, RIGHT, NOCHILD, GO] == own + (n - 1 in roots)
        assert g["dec_rule"][b, n - 1, RIGHT, HASCHILD, GO] == sum(1 for c in roots if c != n - 1)
        assert g["root_rule"][b].sum() == 1 and g["root_rule"][b, roots[0]] == 1


@pytest.mark.parametrize("path", golden_files("initstep_"), ids=golden_ids("initstep_"))
def test_initstep_enll_on_merged_potentials(path):
    """The reference's enll (ldndmv.py:273-275, unmerged dec / attach / root) = -sum(counts . merged potentials) with dec = md[:,1:],
    attach = ma[:,1:,1:], root = ma[:,0,1:,NOCHILD]: the drop-in formula of rules1o.gold_rule_score, in float64 on the fixture."""
    g = load(path)
    md, ma = g["merged_dec"].astype(np.float64), g["merged_attach"].astype(np.float64)
    L = md.shape[1] - 1
    dec, att, root = np_batch_rules(g["arc"], g["lengths"], L)
    score = (dec * np.where(dec != 0, md[:, 1:], 0)).sum() + (att * np.where(att != 0, ma[:, 1:, 1:], 0)).sum() + \
        (root * np.where(root != 0, ma[:, 0, 1:, NOCHILD], 0)).sum()
    assert abs(-score - float(g["enll"])) <= 1e-6 * abs(float(g["enll"])), (-score, float(g["enll"]))
    assert int(g["init_epoch"]) > 0 and bool(g["viterbi_training"])


@pytest.fixture(scope="module")
def lib():
    from vlgae_amd.build import build_library
    build_library()
    from vlgae_amd import _C
    return _C.lib()


def test_gold_entries_argument_errors(lib):
    one = ctypes.c_void_p(16)
    # rule tables: L in [1, 254], ld_arc >= 1, out_dtype f32 / f64, no null buffers; B = 0 is a no-op
    assert lib.vlg_dmv1o_gold_rules(one, 4, one, 2, 0, 0, one, one, one, None) == 0x1001
    assert lib.vlg_dmv1o_gold_rules(one, 4, one, 2, 255, 0, one, one, one, None) == 0x1001 and b"254" in lib.vlg_last_error()
    assert lib.vlg_dmv1o_gold_rules(one, 0, one, 2, 4, 0, one, one, one, None) == 0x1001
    assert lib.vlg_dmv1o_gold_rules(one, 4, one, -1, 4, 0, one, one, one, None) == 0x1001
    assert lib.vlg_dmv1o_gold_rules(one, 4, one, 2, 4, 1, one, one, one, None) == 0x1002          # bf16 tables: not offered
    assert lib.vlg_dmv1o_gold_rules(one, 4, one, 2, 4, 2, one, None, one, None) == 0x1003
    assert lib.vlg_dmv1o_gold_rules(None, 4, None, 0, 4, 2, None, None, None, None) == 0
    # score: 2 <= N <= 255, in_dtype f32 / bf16
    assert lib.vlg_dmv1o_gold_score(one, one, one, 4, one, 2, 1, 0, one, None) == 0x1001
    assert lib.vlg_dmv1o_gold_score(one, one, one, 4, one, 2, 256, 0, one, None) == 0x1001 and b"255" in lib.vlg_last_error()
    assert lib.vlg_dmv1o_gold_score(one, one, one, 4, one, 2, 5, 2, one, None) == 0x1002
    assert lib.vlg_dmv1o_gold_score(one, one, one, 4, one, 2, 5, 1, None, None) == 0x1003
    assert lib.vlg_dmv1o_gold_score(None, None, None, 4, None, 0, 5, 0, None, None) == 0
    # adjoint: g_stride 0 / 1, out_dtype f32 / bf16
    assert lib.vlg_dmv1o_gold_score_backward(one, 4, one, 2, 5, one, 2, 0, one, one, None) == 0x1001
    assert lib.vlg_dmv1o_gold_score_backward(one, 4, one, 2, 300, one, 1, 0, one, one, None) == 0x1001
    assert lib.vlg_dmv1o_gold_score_backward(one, 4, one, 2, 5, one, 1, 2, one, one, None) == 0x1002
    assert lib.vlg_dmv1o_gold_score_backward(one, 4, one, 2, 5, None, 1, 0, one, one, None) == 0x1003
    assert lib.vlg_dmv1o_gold_score_backward(None, 4, None, 0, 5, None, 0, 1, None, None, None) == 0


def test_python_api_has_no_cpu_path():
    from vlgae_amd import rules1o
    arc, lengths = torch.zeros(2, 3, dtype=torch.int64), torch.tensor([3, 2])
    with pytest.raises(RuntimeError, match="no CPU path"):
        rules1o.gold_rules(arc, lengths, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rules1o.gold_rule_score(torch.zeros(2, 4, 2, 2, 2), torch.zeros(2, 4, 4, 2), arc, lengths)


def test_train_step_build_validates_dep_loss_before_gpu_work():
    from vlgae_amd import train_step
    cpu = torch.device("cpu")   # nothing is allocated before these checks: no device is needed to see them fail
    with pytest.raises(ValueError, match="dep_loss"):
        train_step.build(2, 4, 3, cpu, dep_loss="marginal")
    with pytest.raises(ValueError, match="arc"):
        train_step.build(2, 4, 3, cpu, dep_loss="gold_rules")
    with pytest.raises(ValueError, match="arc"):
        train_step.build(2, 4, 3, cpu, dep_loss="gold_rules", given=dict(lengths=torch.tensor([4, 2])))
    for mode in ("viterbi", "partition"):
        with pytest.raises(ValueError, match="only read with dep_loss='gold_rules'"):
            train_step.build(2, 4, 3, cpu, dep_loss=mode, given=dict(arc=torch.zeros(2, 4, dtype=torch.int64)))
    with pytest.raises(TypeError):
        train_step.build(2, 4, 3, cpu, wiring="r3", dep_loss="partition")
    assert train_step.DEP_LOSSES == ("viterbi", "gold_rules", "partition")
