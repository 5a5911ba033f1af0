#!/usr/bin/env python3
"""Golden vectors of the k-best trees of DMV1o, produced by RUNNING THE REFERENCE in float64 (like make_golden_kbest.py).
Run from the repo root:   python tests/golden/make_golden_dmv_kbest.py

The reference has no k-max for the DMV (on a DMV1o its `kmax` / `topk` stop in KMaxSemiring.sum), so the vectors are made differently:

  dmvkbest_B3_N6_s0.npz, dmvkbest_B4_N5_s1.npz: float64 dec [B,N,2,2,2] / attach [B,N,N,2] (the exactly-representable recipe of
  tests/dmv_kbest_restatement.py: potentials), ragged lengths [B] (words <= 5, one sentence of length 1 in each).  EVERY projective
  single-root tree of every sentence is scored by the reference's own `DMV1o(...).max` on potentials whose attach is -1e9 off the
  tree: `values` [T,B] sorted in descending order (-inf where the sentence has fewer than T trees; T = the most any sentence has),
  `heads` [T,B,N] the trees in that order (a stable sort over the order of enumeration), `ntrees` [B].
  dmvkbest_B2_N41_s2.npz: one N = 41 batch with the reference's `max` as `values` [1,B] and its `argmax` as `heads` [1,B,N].
  Arrays only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import  # noqa: E402
from dmv_kbest_restatement import all_trees, potentials  # noqa: E402

SMALL = ((3, 6, 0), (4, 5, 1))
OFF_TREE = -1e9


def small_case(ts, B, N, seed):
    rng = np.random.default_rng(seed)
    dec, attach = potentials(rng, B, N)
    lengths = rng.integers(2, N, size=B)
    lengths[0], lengths[-1] = N - 1, 1
    trees = [all_trees(int(L)) for L in lengths]
    T = max(len(t) for t in trees)
    values = np.full((T, B), -np.inf)
    heads = np.zeros((T, B, N), np.int64)
    for b, L in enumerate(lengths):
        n = len(trees[b])
        forced = np.full((n, N, N, 2), OFF_TREE)
        for t, h in enumerate(trees[b]):
            c = np.arange(1, L + 1)
            forced[t, h[c], c] = attach[b, h[c], c]
        d = torch.tensor(np.broadcast_to(dec[b], (n, N, 2, 2, 2)).copy())
        v = ts.DMV1o([d, torch.tensor(forced)], torch.full((n,), int(L))).max.detach().numpy().reshape(n)
        order = np.argsort(-v, kind="stable")
        values[:n, b] = v[order]
        for k, t in enumerate(order):
            heads[k, b, :L + 1] = trees[b][t]
    return dict(dec=dec, attach=attach, lengths=lengths.astype(np.int64), values=values, heads=heads,
                ntrees=np.array([len(t) for t in trees], np.int64))


def long_case(ts, B, N, seed):
    rng = np.random.default_rng(seed)
    dec, attach = potentials(rng, B, N)
    lengths = np.array([N - 1, (N - 1) // 2], np.int64)[:B]
    dist = ts.DMV1o([torch.tensor(dec, requires_grad=True), torch.tensor(attach, requires_grad=True)], torch.tensor(lengths))
    values = dist.max.detach().numpy().reshape(1, B)
    parts = dist.argmax.detach().numpy().sum(-1)   # [B,N,N] (head, child)
    heads = np.zeros((1, B, N), np.int64)
    for b, L in enumerate(lengths):
        h, c = np.nonzero(parts[b] > 0.5)
        assert sorted(c) == list(range(1, L + 1)), (b, c)
        heads[0, b, c] = h
    return dict(dec=dec, attach=attach, lengths=lengths, values=values, heads=heads)


def main():
    ts = _ref_import.import_torch_struct()
    for B, N, seed in SMALL:
        path = os.path.join(HERE, f"dmvkbest_B{B}_N{N}_s{seed}.npz")
        np.savez_compressed(path, **small_case(ts, B, N, seed))
        print(path, os.path.getsize(path), "bytes")
    path = os.path.join(HERE, "dmvkbest_B2_N41_s2.npz")
    np.savez_compressed(path, **long_case(ts, 2, 41, 2))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
