#!/usr/bin/env python3
"""Golden vectors of the parser's two other losses, produced by RUNNING THE REFERENCE (like make_golden.py, which this script imports
and does not change).  Run from the repo root:   python tests/golden/make_golden_init.py

  goldrules_*.npz   generate_rule_1o (src/model/dmv_helper/good_init_nn.py:34-77) of hand-picked and random arc vectors, padded as
                    LinearPadder / SquarePadder(0) pad them (their `np.float` is gone from current numpy: the same padding is written
                    out here, float64).  Stored: arc [B,L] (0 past n), lengths, dec_rule, attach_rule, root_rule.
  initstep_*.npz    make_golden.trainstep_cases' whole training step with `src.trainer.current_epoch` (0) < `init_epoch` (5), `dmv=None`:
                    DiscriminativeNDMV.loss (ldndmv.py:262-275) takes enll = -(gold rules . potentials), the gold rules being
                    generate_rule_1o of a random tree per sentence (one root, possibly non-projective).  Extra fields: arc, enll.
  margstep_*.npz    the same step after the init epochs with viterbi_training=False: -DMV1o(...).partition.sum() (ldndmv.py:280-281).

The step fixtures keep trainstep_cases' two small shapes (B <= 4, L <= 9, h 64); its L = 40 case is computed and not stored.
trainstep_cases is driven unchanged: the reference's `DiscriminativeNDMV.loss` is wrapped (the schedule flags, the gold rules, and an
alias `nll` of `enll` for the field that function stores), `np.savez_compressed` is redirected to the new names, and a gradient
that does not exist in the init step (the merged potentials are not read by enll) is stored as an empty array.
"""
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import _ref_import  # noqa: E402

INIT_EPOCH = 5    # config/model/vlgae.yaml:75-76


def _pad(rules, L, square):
    out = np.zeros((len(rules), L, L, *rules[0].shape[2:]) if square else (len(rules), L, *rules[0].shape[1:]), dtype=np.float64)
    for b, r in enumerate(rules):
        n = r.shape[0]
        if square:
            out[b, :n, :n] = r
        else:
            out[b, :n] = r
    return out


def _rules(arcs):
    from src.model.dmv_helper.good_init_nn import generate_rule_1o
    L = max(len(a) for a in arcs)
    got = [generate_rule_1o([int(x) for x in a]) for a in arcs]
    return dict(dec_rule=_pad([r["dec_rule"] for r in got], L, False), attach_rule=_pad([r["attach_rule"] for r in got], L, True),
                root_rule=_pad([r["root_rule"] for r in got], L, False))


def _arc_array(arcs, L):
    out = np.zeros((len(arcs), L), dtype=np.int64)
    for b, a in enumerate(arcs):
        out[b, :len(a)] = a
    return out


def random_tree(rng, n):
    """One root; every other word attaches to a word placed before it in a random order (non-projective trees included)."""
    order = rng.permutation(n)
    arc = np.zeros(n, dtype=np.int64)
    for i in range(1, n):
        arc[order[i]] = order[rng.integers(0, i)] + 1
    return arc


def goldrules_cases():
    cases = {
        "goldrules_B10_L6_cases": [
            [0],                    # n = 1
            [2, 0],                 # n = 2, the root child at n-1
            [0, 1],                 # n = 2, the root child elsewhere
            [2, 0, 4, 2, 4, 5],     # projective
            [3, 4, 0, 3, 1],        # non-projective ((2 -> 0) crosses (3 -> 1))
            [0, 1, 0, 3, 0, 5],     # several roots, the last word not among them
            [4, 4, 4, 0],           # the root child at n-1 with left children
            [0, 2, 2, 3],           # a self-loop (word 1 heads itself)
            [0, 3, 2, 3],           # a cycle (1 <-> 2) beside the root
            [6, 6, 0, 2, 6, 0],     # two roots, the second at n-1
        ],
    }
    rng = np.random.default_rng(1)
    lengths = [80, 1, 2, 37, 64, 13, 80, 5]
    rand = [random_tree(rng, n) for n in lengths]
    rand[3][[0, 5]] = 0                       # a second and third root
    rand[6][79] = 80                          # a self-loop at n-1 (word 79 had a head; the tree keeps one root elsewhere)
    if not (rand[6] == 0).any():
        rand[6][0] = 0
    cases["goldrules_B8_L80_s1"] = rand
    _ref_import.import_joint()
    for name, arcs in cases.items():
        L = max(len(a) for a in arcs)
        r = _rules(arcs)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), arc=_arc_array(arcs, L), lengths=np.array([len(a) for a in arcs], np.int64), **r)
        print(name, {k: v.shape for k, v in r.items()}, "root-child quirk rows:", int(r["dec_rule"][:, :, 1, :, 0].sum()))


def step_cases(mode):
    """mode 'init': initstep_*; 'marg': margstep_* (see the module docstring)."""
    src, _ = _ref_import.import_joint()
    from src.model import ldndmv
    ND = ldndmv.DiscriminativeNDMV
    real_loss, real_savez, real_np = ND.loss, np.savez_compressed, mg._np
    rng = np.random.default_rng(7)
    rec = {}

    def loss(self, x, gold, vp):
        self.cfg.init_epoch, self.cfg.viterbi_training = INIT_EPOCH, mode != "marg"
        src.trainer = NS(current_epoch=0 if mode == "init" else 100)
        if mode == "init":
            arcs = [random_tree(rng, int(n)) for n in vp.seq_len]
            r = _rules(arcs)
            L = x["dec"].shape[1]
            assert r["dec_rule"].shape[1] == L    # the batch has a sentence of the full length (trainstep_cases: lengths[0] = L)
            gold = dict(gold, **{k: torch.from_numpy(v) for k, v in r.items()})
            rec["arc"] = _arc_array(arcs, L)
        total, out = real_loss(self, x, gold, vp)
        if mode == "init":
            rec["enll"] = out["enll"].detach().numpy()
            out = dict(out, nll=out["enll"])      # (trainstep_cases stores parts["nll"] as `dep_loss`)
        return total, out

    def savez(path, **kw):
        name = os.path.basename(path)
        if "_L40_" in name:
            return
        prefix = "initstep_" if mode == "init" else "margstep_"
        extra = dict(arc=rec["arc"], enll=rec["enll"]) if mode == "init" else {}
        real_savez(os.path.join(HERE, name.replace("trainstep_", prefix)), **kw, **extra, init_epoch=np.int64(INIT_EPOCH),
                   viterbi_training=np.bool_(mode != "marg"))

    ND.loss, np.savez_compressed = loss, savez
    mg._np = lambda t: np.zeros(0, np.float32) if t is None else real_np(t)
    try:
        mg.trainstep_cases()
    finally:
        ND.loss, np.savez_compressed, mg._np = real_loss, real_savez, real_np


if __name__ == "__main__":
    goldrules_cases()
    step_cases("init")
    step_cases("marg")
