#!/usr/bin/env python3
"""Golden vectors of the k-best trees of DependencyCRF, produced by RUNNING THE REFERENCE in float64 (like make_golden.py).
Run from the repo root:   python tests/golden/make_golden_kbest.py

  kbest_B3_N6_K4_s0.npz, kbest_B4_N12_K8_s1.npz, kbest_B2_N41_K16_s2.npz: float64 arc [B,N,N] (the exactly-representable recipe of
  tests/kbest_restatement.py: potentials), ragged lengths [B] (one sentence of length 1 in each), `values` [K+1,B] = the reference's
  `kmax(K + 1)` and `heads` [K,B,N] = its `topk(K)` as head vectors (0 where the rank does not exist; `exists` [K,B] says which do).
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
from kbest_restatement import potentials  # noqa: E402

CASES = ((3, 6, 4, 0), (4, 12, 8, 1), (2, 41, 16, 2))


def case(ts, B, N, K, seed):
    rng = np.random.default_rng(seed)
    arc = potentials(rng, (B, N, N))
    lengths = rng.integers(2, N, size=B)
    lengths[0], lengths[-1] = N - 1, 1
    ln = torch.tensor(lengths)
    values = ts.DependencyCRF(torch.tensor(arc), ln).kmax(K + 1).detach().numpy()
    parts = ts.DependencyCRF(torch.tensor(arc), ln).topk(K).detach().numpy()   # [K,B,N,N], (head, child)
    exists = values[:K] > -5e4   # the reference pads with -1e5 per missing operand; a tree of this recipe scores >= -4 (N - 1)
    heads = np.zeros((K, B, N), np.int64)
    for k in range(K):
        for b in range(B):
            if exists[k, b]:
                h, c = np.nonzero(parts[k, b] > 0.5)
                assert sorted(c) == list(range(1, lengths[b] + 1)), (k, b, c)
                heads[k, b, c] = h
    return dict(arc=arc, lengths=lengths.astype(np.int64), values=values, heads=heads, exists=exists)


def main():
    ts = _ref_import.import_torch_struct()
    for B, N, K, seed in CASES:
        path = os.path.join(HERE, f"kbest_B{B}_N{N}_K{K}_s{seed}.npz")
        np.savez_compressed(path, **case(ts, B, N, K, seed))
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
