"""GPU: the short image after round 10 -- outside-pass lane groups from the group table (G = 4, 8, 10, 12, 16, 32, 64; a wavefront's
last lanes idle at G = 10, 12) and the inside pass's closed piece for the widths 1 and 2 -- against the general image, bit for bit.

The embedding method of test_dmv_short_image_gpu.py / test_dmv_short_inside_gpu.py: a batch at tensor width N <= 41 launches the short
image; the same batch embedded into N = 42 tensors filled with the semiring zero launches the general image, which this round does
not touch.  The outside pass has no cross-lane reduction and the closed piece evaluates the two-lane butterflies' one fmaxf and one
add in one lane, so logZ, grad_dec and grad_attach agree in every bit on the common region.

Cases:
  * N = 41 with every length 1 ... 40 in one launch (B = 40): every piece of the table, every piece edge, empty pieces;
  * tight charts, N = len + 1 (other chart pitches), for the sentence lengths on both sides of every new piece edge: the longest
    width's span count 32 | 33, 24 | 25, 20 | 21, 16 | 17 (where the G = 8, 10, 12, 16 pieces begin to be cut by capacity) and the
    widths 2 | 3 (where the closed piece of the inside pass ends); each such N again with every length below it in the batch;
  * float32 and bf16 storage;
  * Log with the outside pass (unit and non-unit cotangent), Log inside only, Max with the back-pointer walk;
  * random potentials, potentials on a grid of 0.5 (exact ties between split points), -inf on a tenth of the arcs;
  * every launch twice: the second call must return identical bits.
"""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

pytestmark = pytest.mark.gpu

SR_LOG, SR_MAX = 0, 1
WIDE = 42   # one past kShortN: the general image
# N = Ne of the longest sentence: 41, then both sides of every edge (longest width's spans N - 2 ... : N - 1 = 33 | 32, ...; widths 3 | 2)
WIDTHS = [41, 34, 33, 26, 25, 22, 21, 18, 17, 4, 3]
DTYPES = [torch.float32, torch.bfloat16]
KINDS = ["random", "ties", "neginf"]


@pytest.fixture(scope="module")
def Fn():
    import vlgae_amd.torch_struct.functional as F
    return F


@pytest.fixture(scope="module")
def oracle_mod():
    import oracle
    oracle.build()
    return oracle


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def merged(oracle_mod, N, seed, kind):
    """every length 1 ... N - 1 once, as merged potentials [B,N,2,2,2], [B,N,N,2], and a non-unit cotangent [B]"""
    rng = np.random.default_rng(seed)
    L = N - 1
    lengths = np.arange(1, N, dtype=np.int64)
    B = len(lengths)
    dec = np.log(rng.dirichlet(np.ones(2), (B, L, 2, 2))).astype(np.float32)
    attach = rng.standard_normal((B, L, L, 2)).astype(np.float32)
    root = np.log(rng.dirichlet(np.ones(L), B)).astype(np.float32)
    md, ma = oracle_mod.dmv1o_merge(dec, attach, root)
    forbid = None
    if kind == "ties":      # a grid of 0.5 (exact in bf16 too): sums tie
        md, ma = (np.round(md * 2) / 2).astype(np.float32), (np.round(ma * 2) / 2).astype(np.float32)
    elif kind == "neginf":  # the chain 0 -> 1 -> 2 -> ... is left alone, so every sentence keeps a finite tree
        forbid = rng.random(ma.shape[:3]) < 0.1
        forbid[:, np.arange(N - 1), np.arange(1, N)] = False
        ma = ma.copy()
        ma[forbid] = -np.inf
    g = (0.25 + 2.5 * rng.random(B)).astype(np.float32)
    return md, ma, lengths, g, forbid


def embedded(a, fill, square):
    """a [B,N,...] (square: [B,N,N,...]) placed in the leading corner of a WIDE tensor filled with `fill`"""
    B, n = a.shape[:2]
    out = np.full((B, WIDE, WIDE) + a.shape[3:] if square else (B, WIDE) + a.shape[2:], fill, a.dtype)
    if square:
        out[:, :n, :n] = a
    else:
        out[:, :n] = a
    return out


def corner(x, N, square):
    if x.dim() == 1:
        return x
    return x[:, :N, :N] if square else x[:, :N]


MODES = ("log_counts", "log_counts_g", "log_inside", "max_walk")


def run_modes(Fn, md, ma, lengths, g, dtype):
    d, a, ln, gl = t(md).to(dtype), t(ma).to(dtype), t(lengths), t(g)
    out = {
        "log_counts": Fn.dmv1o_run(d, a, ln, SR_LOG, True),                    # logZ, grad_dec, grad_attach: unit cotangent
        "log_counts_g": Fn.dmv1o_run(d, a, ln, SR_LOG, True, grad_logZ=gl),    # non-unit cotangent
        "log_inside": Fn.dmv1o_run(d, a, ln, SR_LOG, False)[:1],
        "max_walk": Fn.dmv1o_viterbi(d, a, ln)[:3],                            # best score, its tree's counts
    }
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", WIDTHS)
def test_short_image_equals_general_image(Fn, oracle_mod, N, kind, dtype):
    md, ma, lengths, g, forbid = merged(oracle_mod, N, 1000 + 10 * N + KINDS.index(kind), kind)
    zero = np.float32(oracle_mod.NEGINF)
    short = run_modes(Fn, md, ma, lengths, g, dtype)
    again = run_modes(Fn, md, ma, lengths, g, dtype)
    wide = run_modes(Fn, embedded(md, zero, False), embedded(ma, zero, True), lengths, g, dtype)
    what = f"N={N} {kind}"
    for mode in MODES:
        assert bool(torch.isfinite(short[mode][0]).all()), f"{what} {mode}: value not finite"
        for k, (s, s2, w) in enumerate(zip(short[mode], again[mode], wide[mode])):   # (value, grad_dec [B,N,2,2,2], grad_attach [B,N,N,2])
            c = corner(w, N, square=(k == 2))
            assert s.shape == c.shape, f"{what} {mode}: output {k} has shape {tuple(s.shape)}"
            assert torch.equal(s, s2), f"{what} {mode}: output {k} differs between two calls"
            assert torch.equal(s, c), f"{what} {mode}: output {k} differs between the short and the general image"
    assert torch.equal(short["log_inside"][0], short["log_counts"][0])
    assert torch.equal(short["log_counts_g"][0], short["log_counts"][0])
    for mode in ("log_counts", "log_counts_g"):
        assert bool(torch.isfinite(short[mode][1]).all()) and bool(torch.isfinite(short[mode][2]).all()), f"{what} {mode}: counts not finite"
    if forbid is not None:
        assert float(short["log_counts"][2][t(forbid)].abs().max()) == 0.0, "a forbidden arc has a non-zero expected count"
    # the best tree has one head per word
    assert torch.equal(short["max_walk"][2].sum((1, 2, 3)), t(lengths).to(torch.float32))
