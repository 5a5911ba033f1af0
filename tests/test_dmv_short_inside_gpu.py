"""GPU: the short-sentence image's inside pass on per-segment addresses (dmv_fw_segment_p), against the general image, bit for bit.

The embedding method of test_dmv_short_image_gpu.py: a batch at tensor width N <= 41 launches the short image; the same batch
embedded into N = 42 tensors filled with the semiring zero launches the general image.  The two run the same adds, maxes,
exponentials and logarithms on the same operands in the same order, so every returned tensor agrees in every bit on the common
region, for float32 and bf16 potentials.  What that file leaves out and this one adds:

  * the modes the inside pass serves besides Log with counts: Log without an outside pass, Max with counts and heads (the
    back-pointer bytes are stored from the inside pass), Max without;
  * tensor widths N = 2, 3, 5, 9, 17, 25, 33, 41, each with a batch of every length 1 ... N - 1: chart pitches other than 43,
    every segment edge of make_sched, spans that end inside a segment (their lanes keep stepping addresses they no longer use),
    the masked root cell at every width;
  * Max with potentials rounded to multiples of 0.5, so that split points tie: the first index must win through the term masks;
  * Log with -inf arcs sprinkled over a batch in which every sentence keeps a finite tree.
"""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

pytestmark = pytest.mark.gpu

SR_LOG, SR_MAX = 0, 1
WIDE = 42   # one past kShortN: the general image
WIDTHS = [2, 3, 5, 9, 17, 25, 33, 41]
DTYPES = [torch.float32, torch.bfloat16]


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


def merged(oracle_mod, N, seed):
    """every length 1 ... N - 1 once, as merged potentials [B,N,2,2,2], [B,N,N,2]"""
    rng = np.random.default_rng(seed)
    L = N - 1
    lengths = np.arange(1, N, dtype=np.int64)
    B = len(lengths)
    dec = np.log(rng.dirichlet(np.ones(2), (B, L, 2, 2))).astype(np.float32)
    attach = rng.standard_normal((B, L, L, 2)).astype(np.float32)
    root = np.log(rng.dirichlet(np.ones(L), B)).astype(np.float32)
    md, ma = oracle_mod.dmv1o_merge(dec, attach, root)
    return md, ma, lengths


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
    """the common region of a WIDE-wide result: [B] as it is, [B,WIDE,...] -> [:, :N], [B,WIDE,WIDE,...] -> [:, :N, :N]"""
    if x.dim() == 1:
        return x
    return x[:, :N, :N] if square else x[:, :N]


def run_modes(Fn, md, ma, lengths, dtype, modes):
    """{mode: tuple of tensors} for one set of potentials at its own tensor width"""
    d, a, ln = t(md).to(dtype), t(ma).to(dtype), t(lengths)
    out = {}
    if "log_inside" in modes:
        out["log_inside"] = Fn.dmv1o_run(d, a, ln, SR_LOG, False)[:1]
    if "log_counts" in modes:
        out["log_counts"] = Fn.dmv1o_run(d, a, ln, SR_LOG, True)
    if "max_inside" in modes:
        out["max_inside"] = Fn.dmv1o_run(d, a, ln, SR_MAX, False)[:1]
    if "max_counts_heads" in modes:
        out["max_counts_heads"] = Fn.dmv1o_viterbi(d, a, ln)
    torch.cuda.synchronize()
    return out


def check_short_equals_general(Fn, oracle_mod, md, ma, lengths, dtype, modes, what):
    N = md.shape[1]
    zero = np.float32(oracle_mod.NEGINF)
    short = run_modes(Fn, md, ma, lengths, dtype, modes)
    wide = run_modes(Fn, embedded(md, zero, False), embedded(ma, zero, True), lengths, dtype, modes)
    for mode in modes:
        assert bool(torch.isfinite(short[mode][0]).all()), f"{what} {mode}: value not finite"
        for k, (s, w) in enumerate(zip(short[mode], wide[mode])):
            c = corner(w, N, square=(k == 2))   # (value, grad_dec [B,N,2,2,2], grad_attach [B,N,N,2], heads [B,N])
            assert s.shape == c.shape, f"{what} {mode}: output {k} has shape {tuple(s.shape)}"
            assert torch.equal(s, c), f"{what} {mode}: output {k} differs between the short and the general image"
    return short


ALL_MODES = ("log_inside", "log_counts", "max_inside", "max_counts_heads")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("N", WIDTHS)
def test_every_mode_at_every_width(Fn, oracle_mod, N, dtype):
    md, ma, lengths = merged(oracle_mod, N, 100 + N)
    assert len(lengths) <= 40
    short = check_short_equals_general(Fn, oracle_mod, md, ma, lengths, dtype, ALL_MODES, f"N={N}")
    # the inside-only launches return what the fused ones return
    assert torch.equal(short["log_inside"][0], short["log_counts"][0])
    assert torch.equal(short["max_inside"][0], short["max_counts_heads"][0])
    best, gdec, gatt, heads = short["max_counts_heads"]
    # the best tree has one head per word: len arcs, and heads names them
    assert torch.equal(gatt.sum((1, 2, 3)), t(lengths).to(torch.float32))
    assert bool(((heads != 0).sum(1) <= t(lengths)).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_max_with_tied_split_points(Fn, oracle_mod, dtype):
    """potentials on a grid of 0.5 (exact in bf16 too): sums tie, and both images must break every tie for the first index"""
    md, ma, lengths = merged(oracle_mod, 41, 7)
    md, ma = (np.round(md * 2) / 2).astype(np.float32), (np.round(ma * 2) / 2).astype(np.float32)
    check_short_equals_general(Fn, oracle_mod, md, ma, lengths, dtype, ("max_inside", "max_counts_heads"), "ties")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_log_with_forbidden_arcs(Fn, oracle_mod, dtype):
    """-inf on a tenth of the arcs; the chain 0 -> 1 -> 2 -> ... is left alone, so every sentence keeps a finite tree"""
    md, ma, lengths = merged(oracle_mod, 41, 8)
    rng = np.random.default_rng(9)
    N = ma.shape[1]
    forbid = rng.random(ma.shape[:3]) < 0.1
    forbid[:, np.arange(N - 1), np.arange(1, N)] = False
    ma = ma.copy()
    ma[forbid] = -np.inf
    short = check_short_equals_general(Fn, oracle_mod, md, ma, lengths, dtype, ("log_inside", "log_counts"), "-inf arcs")
    lz, gd, ga = short["log_counts"]
    assert bool(torch.isfinite(ga).all()) and bool(torch.isfinite(gd).all())
    assert float(ga[t(forbid)].abs().max()) == 0.0, "a forbidden arc has a non-zero expected count"
