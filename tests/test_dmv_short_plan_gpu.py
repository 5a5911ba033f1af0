"""GPU: the short image after round 11 -- the outside pass's stationary cells kept in registers over a piece (xa read once per piece,
its adjoint word summed in a register and written through) -- against the general image, bit for bit, at EVERY tensor width of the
short image.

The embedding method of test_dmv_short_sched_gpu.py: a batch at tensor width N <= 41 launches the short image; the same batch embedded
into N = 42 tensors filled with the semiring zero launches the general image, which this round does not touch.  The earlier tests
cover 11 of the 40 widths; what a lane holds over a piece depends on the chart pitch P = (N + 1) | 1 and on where the pieces of
every sentence length begin and end, so here every N = 2 ... 41 runs with every length 1 ... N - 1 in one batch.

  * modes: Log with the outside pass and a non-unit cotangent, Log inside only, Max with the back-pointer walk;
  * float32 and bf16 storage;
  * random potentials, and -inf on a tenth of the arcs with the chain 0 -> 1 -> 2 ... kept;
  * every launch twice: the second call must return identical bits (a register that outlives its piece, a cell left over from the
    launch before, would show here).
"""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

pytestmark = pytest.mark.gpu

SR_LOG = 0
WIDE = 42   # one past kShortN: the general image
WIDTHS = list(range(2, 42))
DTYPES = [torch.float32, torch.bfloat16]
KINDS = ["random", "neginf"]
MODES = ("log_counts_g", "log_inside", "max_walk")


@pytest.fixture(scope="module")
def Fn():
    import vlgae_amd.torch_struct.functional as F
    return F


@pytest.fixture(scope="module")
def oracle_mod():
    import oracle
    oracle.build()
    return oracle


@pytest.fixture(scope="module")
def batches(oracle_mod):
    """(N, kind) -> merged potentials of every length 1 ... N - 1, made once and shared by both storage types"""
    made = {}

    def get(N, kind):
        if (N, kind) not in made:
            rng = np.random.default_rng(1100 + 10 * N + KINDS.index(kind))
            L = N - 1
            lengths = np.arange(1, N, dtype=np.int64)
            B = len(lengths)
            dec = np.log(rng.dirichlet(np.ones(2), (B, L, 2, 2))).astype(np.float32)
            attach = rng.standard_normal((B, L, L, 2)).astype(np.float32)
            root = np.log(rng.dirichlet(np.ones(L), B)).astype(np.float32)
            md, ma = oracle_mod.dmv1o_merge(dec, attach, root)
            forbid = None
            if kind == "neginf":   # the chain 0 -> 1 -> 2 -> ... is left alone, so every sentence keeps a finite tree
                forbid = rng.random(ma.shape[:3]) < 0.1
                forbid[:, np.arange(N - 1), np.arange(1, N)] = False
                ma = ma.copy()
                ma[forbid] = -np.inf
            g = (0.25 + 2.5 * rng.random(B)).astype(np.float32)
            made[(N, kind)] = (md, ma, lengths, g, forbid)
        return made[(N, kind)]

    return get


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


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


def run_modes(Fn, md, ma, lengths, g, dtype):
    d, a, ln, gl = t(md).to(dtype), t(ma).to(dtype), t(lengths), t(g)
    return {
        "log_counts_g": Fn.dmv1o_run(d, a, ln, SR_LOG, True, grad_logZ=gl),    # logZ, grad_dec, grad_attach: non-unit cotangent
        "log_inside": Fn.dmv1o_run(d, a, ln, SR_LOG, False)[:1],
        "max_walk": Fn.dmv1o_viterbi(d, a, ln)[:3],                            # best score, its tree's counts
    }


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_short_image_equals_general_image_at_every_width(Fn, oracle_mod, batches, kind, dtype):
    zero = np.float32(oracle_mod.NEGINF)
    for N in WIDTHS:
        md, ma, lengths, g, forbid = batches(N, kind)
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
        assert torch.equal(short["log_inside"][0], short["log_counts_g"][0])
        assert bool(torch.isfinite(short["log_counts_g"][1]).all()) and bool(torch.isfinite(short["log_counts_g"][2]).all()), f"{what}: counts not finite"
        if forbid is not None:
            assert float(short["log_counts_g"][2][t(forbid)].abs().max()) == 0.0, f"{what}: a forbidden arc has a non-zero expected count"
        # the best tree has one head per word
        assert torch.equal(short["max_walk"][2].sum((1, 2, 3)), t(lengths).to(torch.float32)), f"{what}: the best tree is not a tree"
