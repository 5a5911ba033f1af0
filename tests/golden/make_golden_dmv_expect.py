#!/usr/bin/env python3
"""Golden vectors of the expectation quantities of DMV1o, produced by RUNNING THE REFERENCE in float64 (like make_golden_expect.py).
Run from the repo root:   python tests/golden/make_golden_dmv_expect.py

  dmvexpect_B3_N6_s0.npz, dmvexpect_B4_N12_s1.npz, dmvexpect_B2_N41_s2.npz: float64 root-merged potentials dec_p, dec_q
  [B,N,2,2,2] and att_p, att_q [B,N,N,2] (the reference's DMV1o.merge of random unmerged ones), costs cost_dec, cost_att of the same
  shapes, and ragged lengths [B] (one sentence of length 1 in each), with the reference's `entropy`, `cross_entropy(q)` and
  `risk([cost_dec, cost_att])`, `kl` stored as cross_entropy - entropy (the reference's own `kl` is not a yardstick: its
  KLDivergenceSemiring disagrees with that difference), and the autograd gradients of the first three with respect to every input:
  g_<quantity>_<input>.  Values are [B] (the reference returns [B,1]).  Arrays only.
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
    L = N - 1
    t = lambda *shape: torch.tensor(rng.standard_normal(shape))

    def merged():
        dec, att = ts.DMV1o.merge(t(B, L, 2, 2, 2), t(B, L, L, 2), t(B, L))
        return dec.double().numpy().copy(), att.double().numpy().copy()   # (merge returns float32: the values are kept, in float64 arrays)

    (dec_p, att_p), (dec_q, att_q) = merged(), merged()
    cost_dec, cost_att = t(B, N, 2, 2, 2).numpy(), t(B, N, N, 2).numpy()
    lengths = rng.integers(2, N, size=B)
    lengths[0], lengths[-1] = N - 1, 1
    arrays = dict(dec_p=dec_p, att_p=att_p, dec_q=dec_q, att_q=att_q, cost_dec=cost_dec, cost_att=cost_att)
    out = dict(arrays, lengths=lengths.astype(np.int64))
    ln = torch.tensor(lengths)

    def leaves():
        return {k: torch.tensor(x, dtype=torch.float64, requires_grad=True) for k, x in arrays.items()}

    def keep(name, value, x, inputs):
        out[name] = value.detach().numpy().reshape(B).copy()
        for iname, g in zip(inputs, torch.autograd.grad(value.sum(), [x[k] for k in inputs])):
            out[f"g_{name}_{iname}"] = g.numpy().copy()

    x = leaves()
    keep("entropy", ts.DMV1o([x["dec_p"], x["att_p"]], ln).entropy, x, ("dec_p", "att_p"))
    x = leaves()
    keep("cross_entropy", ts.DMV1o([x["dec_p"], x["att_p"]], ln).cross_entropy(ts.DMV1o([x["dec_q"], x["att_q"]], ln)), x,
         ("dec_p", "att_p", "dec_q", "att_q"))
    x = leaves()
    keep("risk", ts.DMV1o([x["dec_p"], x["att_p"]], ln).risk([x["cost_dec"], x["cost_att"]]), x, ("dec_p", "att_p", "cost_dec", "cost_att"))
    out["kl"] = out["cross_entropy"] - out["entropy"]
    return out


def main():
    ts = _ref_import.import_torch_struct()
    for B, N, seed in CASES:
        path = os.path.join(HERE, f"dmvexpect_B{B}_N{N}_s{seed}.npz")
        np.savez_compressed(path, **case(ts, B, N, seed))
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
