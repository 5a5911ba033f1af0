#!/usr/bin/env python3
"""Golden vectors of DependencyCRF on LABELED potentials [B,N,N,L], produced by RUNNING THE REFERENCE in float64 (like make_golden.py).
Run from the repo root:   python tests/golden/make_golden_labeled.py

  labeled_B3_N6_L4_s0.npz, labeled_B4_N12_L5_s1.npz, labeled_B2_N41_L7_s2.npz: float64 phi, other, cost [B,N,N,L] (the exactly
  representable recipe of tests/labeled_restatement.py: potentials -- no two equal labels in a row), ragged lengths [B] (one sentence
  of length 1 in each), and the reference's partition, max [B], marginals, argmax [B,N,N,L], entropy, cross_entropy (against
  `other`), kl (stored as cross_entropy - entropy, as make_golden_expect.py does) and risk (against `cost`) [B].  The two small cases also hold the autograd gradients of the sum over the batch of each:
  grad_<name> w.r.t. phi, grad_<name>_other / grad_risk_cost w.r.t. the second argument.  Arrays only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import  # noqa: E402
from labeled_restatement import potentials  # noqa: E402

CASES = ((3, 6, 4, 0, True), (4, 12, 5, 1, True), (2, 41, 7, 2, False))


def case(ts, B, N, L, seed, grads):
    rng = np.random.default_rng(seed)
    phi, other, cost = (potentials(rng, (B, N, N, L)) for _ in range(3))
    lengths = rng.integers(2, N, size=B)
    lengths[0], lengths[-1] = N - 1, 1
    ln = torch.tensor(lengths)
    out = dict(phi=phi, other=other, cost=cost, lengths=lengths.astype(np.int64))

    def leaves():
        return [torch.tensor(x, requires_grad=True) for x in (phi, other, cost)]

    quantities = {
        "partition": lambda p, q, c: ts.DependencyCRF(p, ln).partition,
        "max": lambda p, q, c: ts.DependencyCRF(p, ln).max,
        "entropy": lambda p, q, c: ts.DependencyCRF(p, ln).entropy,
        # (as in make_golden_expect.py: the reference's own `kl` is not a yardstick -- its KLDivergenceSemiring disagrees with this difference)
        "kl": lambda p, q, c: ts.DependencyCRF(p, ln).cross_entropy(ts.DependencyCRF(q, ln)) - ts.DependencyCRF(p, ln).entropy,
        "cross_entropy": lambda p, q, c: ts.DependencyCRF(p, ln).cross_entropy(ts.DependencyCRF(q, ln)),
        "risk": lambda p, q, c: ts.DependencyCRF(p, ln).risk(c),
    }
    for name, fn in quantities.items():
        p, q, c = leaves()
        val = fn(p, q, c)
        out[name] = val.detach().numpy().reshape(B)
        if grads:
            val.sum().backward()
            out["grad_" + name] = p.grad.numpy()
            if name in ("kl", "cross_entropy"):
                out[f"grad_{name}_other"] = q.grad.numpy()
            if name == "risk":
                out["grad_risk_cost"] = c.grad.numpy()
    out["marginals"] = ts.DependencyCRF(torch.tensor(phi), ln).marginals.detach().numpy()
    out["argmax"] = ts.DependencyCRF(torch.tensor(phi), ln).argmax.detach().numpy()
    return out


def main():
    ts = _ref_import.import_torch_struct()
    for B, N, L, seed, grads in CASES:
        path = os.path.join(HERE, f"labeled_B{B}_N{N}_L{L}_s{seed}.npz")
        np.savez_compressed(path, **case(ts, B, N, L, seed, grads))
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
