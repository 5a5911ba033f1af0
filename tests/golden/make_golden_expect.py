#!/usr/bin/env python3
"""Golden vectors of the expectation quantities of DependencyCRF, produced by RUNNING THE REFERENCE in float64 (like make_golden.py).
Run from the repo root:   python tests/golden/make_golden_expect.py

  expect_B3_N6_s0.npz, expect_B4_N12_s1.npz, expect_B2_N41_s2.npz: float64 arc_p, arc_q, cost [B,N,N] and ragged lengths [B] (one
  sentence of length 1 in each), with the reference's `entropy`, `cross_entropy(q)` and `risk(cost)`, `kl` stored as
  cross_entropy - entropy (the reference's own `kl` is not a yardstick: its KLDivergenceSemiring disagrees with that difference), and
  the autograd gradients of each with respect to every input: g_<quantity>_<input>.  Arrays only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402

CASES = ((3, 6, 0), (4, 12, 1), (2, 41, 2))


def case(ts, B, N, seed):
    rng = np.random.default_rng(seed)
    arc_p, arc_q, cost = (rng.standard_normal((B, N, N)) for _ in range(3))
    lengths = rng.integers(2, N, size=B)
    lengths[0], lengths[-1] = N - 1, 1
    out = dict(arc_p=arc_p, arc_q=arc_q, cost=cost, lengths=lengths.astype(np.int64))
    ln = torch.tensor(lengths)

    def leaves():
        return [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (arc_p, arc_q, cost)]

    def keep(name, value, inputs):
        out[name] = value.detach().numpy().copy()
        grads = torch.autograd.grad(value.sum(), [t for _, t in inputs])
        for (iname, _), g in zip(inputs, grads):
            out[f"g_{name}_{iname}"] = g.numpy().copy()

    p, q, c = leaves()
    keep("entropy", ts.DependencyCRF(p, ln).entropy, [("arc_p", p)])
    p, q, c = leaves()
    keep("cross_entropy", ts.DependencyCRF(p, ln).cross_entropy(ts.DependencyCRF(q, ln)), [("arc_p", p), ("arc_q", q)])
    p, q, c = leaves()
    keep("risk", ts.DependencyCRF(p, ln).risk(c), [("arc_p", p), ("cost", c)])
    p, q, c = leaves()
    dp, dq = ts.DependencyCRF(p, ln), ts.DependencyCRF(q, ln)
    keep("kl", dp.cross_entropy(dq) - dp.entropy, [("arc_p", p), ("arc_q", q)])
    return out


def main():
    ts = _ref_import.import_torch_struct()
    for B, N, seed in CASES:
        path = os.path.join(HERE, f"expect_B{B}_N{N}_s{seed}.npz")
        np.savez_compressed(path, **case(ts, B, N, seed))
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
