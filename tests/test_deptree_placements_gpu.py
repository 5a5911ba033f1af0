"""DepTree (deptree_kernel / dep_run) at every chart placement of DepLayout, against the fp64 CPU oracle.

DepLayout keeps one sentence's charts in LDS while they fit the 160 KiB budget and moves a growing set of them to the caller's
workspace beyond it.  Widths N at which the placement changes (vlg_dp_core.h: DepLayout, chart_pitch):

  launch                                   all in LDS   mode 1                    mode 2            mode 3
  Log inside-outside                       N <= 82      83-116 (C, I, S in ws)    117-142 (+ gI)    143-255 (everything)
  Max walk (decode, max + gradient, MBR)   N <= 106     107-126 (gI in ws)        127-255 (values and back-pointers too)
  inside only                              N <= 142     143-255 (C, I in ws)

test_placement_boundaries_are_where_the_cases_assume pins that table; the cases below sit on both sides of every boundary
and at the largest supported width.

Tolerances:
  logZ / best score   logz_tol (2e-5 relative) for the Log semiring, 1e-5 relative for Max-semiring values
  marginals           min(6e-4, max(MARG_TOL, 6 * e32)): the project's rule for long DMV sentences.  e32 is the error of the
                      SEQUENTIAL fp32 oracle against the fp64 oracle on the same inputs -- a property of the reference.
  column sums         min(6e-4, max(1e-4, 6 * c32)), c32 the fp32 oracle's own deviation of a column sum from one: the same
                      rule over the 1e-4 that the DepTree tests at N <= 150 use.  Sums are taken in float64 on the host.
  weighted launch     upstream weights lie in [0.25, 1]: the adjoints are linear in the weight, so the unit bound holds.
  Max semiring        one-hot and heads exact where the fp32 and fp64 oracle agree on the arg-max (asserted per case)
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MARG_TOL = 5e-5
SR_LOG, SR_MAX = 0, 1


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def t(a, dtype=None):
    x = torch.from_numpy(np.array(a)).to(dev())   # a copy: the shared references are read-only
    return x if dtype is None else x.to(dtype)


def logz_tol(ref):
    return 2e-5 * np.maximum(1.0, np.abs(ref))


@pytest.fixture(scope="module")
def Fn():
    from vlgae_amd import _C
    from vlgae_amd.torch_struct import functional
    _C.lib()   # must load: the product has no fallback
    return functional


def ragged_lengths(rng, N, B=5):
    """the full width, the two shortest sentences, the rest from [N/2, N)"""
    ln = rng.integers(max(1, N // 2), N, B)
    ln[0], ln[1], ln[2] = N - 1, 1, min(2, N - 1)
    return ln.astype(np.int64)


def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def log_reference(oracle, arc, lengths, w=None):
    """fp64 results, the tolerances that come from the fp32 oracle, and (with w) the weighted fp64 gradient"""
    z64, g64 = oracle.deptree(arc, lengths, "log", np.float64)
    _, g32 = oracle.deptree(arc, lengths, "log", np.float32)
    e32 = float(np.abs(g32 - g64).max())
    c32 = 0.0
    for b, n in enumerate(lengths):
        c32 = max(c32, float(np.abs(g32[b].astype(np.float64).sum(0)[1:n + 1] - 1.0).max()))
    gw = None if w is None else oracle.deptree(arc, lengths, "log", np.float64, glogZ=w)[1]
    ref = dict(z=z64, g=g64, gw=gw, e32=e32, c32=c32, bound=min(6e-4, max(MARG_TOL, 6 * e32)), col_tol=min(6e-4, max(1e-4, 6 * c32)))
    frozen(z64, g64, gw)
    return ref


def check_log(tag, lz, g, lengths, ref, g_ref=None):
    """logZ, marginals, column sums, exact zeros outside the sentence; prints the figures before it asserts"""
    lz, g = lz.detach().cpu().numpy(), g.detach().cpu().numpy()
    g_ref = ref["g"] if g_ref is None else g_ref
    err = float(np.abs(g - g_ref).max())
    zerr = float((np.abs(lz - ref["z"]) / logz_tol(ref["z"])).max())
    cerr = 0.0
    for b, n in enumerate(lengths):
        if g_ref is ref["g"]:
            cerr = max(cerr, float(np.abs(g[b].astype(np.float64).sum(0)[1:n + 1] - 1.0).max()))
        assert not g[b, :, 0].any() and not g[b, :, n + 1:].any() and not g[b, n + 1:, :].any(), (tag, b)
        assert not np.diagonal(g[b]).any(), (tag, b)
    print(f"[deptree] {tag}: marginal err {err:.2e} (bound {ref['bound']:.2e}, e32 {ref['e32']:.2e}), column-sum err {cerr:.2e} "
          f"(tol {ref['col_tol']:.2e}, c32 {ref['c32']:.2e}), logZ err / tol {zerr:.2f}")
    assert np.all(np.isfinite(lz)) and zerr <= 1.0, (tag, zerr)
    assert err <= ref["bound"], (tag, err, ref["bound"])
    assert cerr <= ref["col_tol"], (tag, cerr, ref["col_tol"])
    return err


def heads_of(onehot, lengths):
    """head vector of a [B,N,N] indicator tensor (exactly one head per word inside the sentence, none outside)"""
    B, N = onehot.shape[:2]
    heads = np.zeros((B, N), np.int64)
    for b, n in enumerate(lengths):
        assert np.array_equal(onehot[b].sum(0)[1:n + 1], np.ones(n)) and onehot[b].sum() == n, b
        heads[b, 1:n + 1] = onehot[b].argmax(0)[1:n + 1]
    return heads


def tree_score(arc, heads, n):
    return float(sum(np.float64(arc[heads[c], c]) for c in range(1, n + 1)))


# ------------------------------------------------------------------------------------------------ A: the placement table
def chart_pitch(N):
    return (N + 1) | 1


def align16(x):
    return (x + 15) & ~15


def ws_expected(N, bytes_per_cell):
    """one chart per entry, each rounded up to 16 bytes on its own"""
    cells = N * chart_pitch(N)
    return sum(align16(cells * b) for b in bytes_per_cell)


LOG_IO = {0: [], 1: [4, 4, 4], 2: [4, 4, 4, 4], 3: [4, 4, 4, 4, 4, 4]}   # C, I, S | + gI | + gCc, gCi
MAX_WALK = {0: [], 1: [4], 2: [4, 4, 1, 1, 4]}                            # gI | C, I, bpS, bpC, gI
INSIDE = {0: [], 1: [4, 4]}                                               # C, I


@pytest.mark.parametrize("op,sr,table,edges", [
    ("io", SR_LOG, LOG_IO, [(2, 0), (41, 0), (42, 0), (82, 0), (83, 1), (116, 1), (117, 2), (142, 2), (143, 3), (255, 3)]),
    ("io", SR_MAX, MAX_WALK, [(2, 0), (106, 0), (107, 1), (126, 1), (127, 2), (255, 2)]),
    ("inside", SR_LOG, INSIDE, [(142, 0), (143, 1), (255, 1)]),
    ("inside", SR_MAX, INSIDE, [(142, 0), (143, 1), (255, 1)]),
], ids=["log_inside_outside", "max_walk", "log_inside", "max_inside"])
def test_placement_boundaries_are_where_the_cases_assume(op, sr, table, edges):
    """vlg_workspace_bytes reads the launchers' own plan (dp_plan<DepLayout>): the per-sentence workspace names the placement mode.
    If a layout change moves a boundary, this fails instead of the cases below quietly running in another mode."""
    from vlgae_amd import _C
    code = _C.OP_DEPTREE_INSIDE_OUTSIDE if op == "io" else _C.OP_DEPTREE_INSIDE
    for N, mode in edges:
        got = int(_C.lib().vlg_workspace_bytes(code, 1, N, sr))
        assert got == ws_expected(N, table[mode]), (op, sr, N, mode, got)
        assert int(_C.lib().vlg_workspace_bytes(code, 3, N, sr)) == 3 * got
        assert len({ws_expected(N, v) for v in table.values()}) == len(table)   # the size tells the modes apart


# ------------------------------------------------------------------------------------------------ B: Log semiring
LOG_CASES = [(82, 1.0), (83, 1.0), (116, 1.0), (117, 1.0), (142, 1.0), (143, 1.0), (255, 1.0), (83, 6.0), (117, 6.0), (143, 6.0)]


@functools.lru_cache(maxsize=None)
def _log_case(N, scale):
    import oracle
    rng = np.random.default_rng(7000 + 10 * N + int(scale))
    lengths = ragged_lengths(rng, N)
    arc = (rng.standard_normal((len(lengths), N, N)) * scale).astype(np.float32)
    w = rng.uniform(0.25, 1.0, len(lengths)).astype(np.float32)
    frozen(arc, lengths, w)
    return arc, lengths, w, log_reference(oracle, arc, lengths, w)


@pytest.mark.parametrize("N,scale", LOG_CASES, ids=[f"N{n}_scale{int(s)}" for n, s in LOG_CASES])
def test_deptree_log_placements_vs_oracle(Fn, oracle_mod, N, scale):
    """Log inside-outside on both sides of 82/83 (all in LDS -> mode 1), 116/117 (-> mode 2), 142/143 (-> mode 3) and at 255, with
    peaky scores (standard deviation 6) in each workspace mode; unit and weighted upstream; bit-reproducible.  At 142, 143 and
    255 the inside-only launch (its own boundary is 142/143) in both semirings.

    Observed marginal error / its bound on an MI355X, unit upstream (column-sum error / its tolerance in brackets):
      scale 1   N = 82   1.18e-5 / 5.00e-5 (1.73e-5 / 1.0e-4)     N = 83   1.26e-5 / 6.91e-5 (1.62e-5 / 1.0e-4)
                N = 116  6.98e-6 / 5.00e-5 (8.39e-6 / 1.0e-4)     N = 117  5.66e-6 / 7.97e-5 (7.24e-6 / 1.02e-4)
                N = 142  5.21e-6 / 5.12e-5 (6.64e-6 / 1.0e-4)     N = 143  7.84e-6 / 5.57e-5 (9.35e-6 / 1.0e-4)
                N = 255  2.00e-5 / 1.45e-4 (2.69e-5 / 2.0e-4)
      scale 6   N = 83   7.00e-5 / 3.19e-4 (7.07e-5 / 3.19e-4)    N = 117  1.71e-4 / 6.00e-4 (1.75e-4 / 6.0e-4)
                N = 143  2.12e-4 / 6.00e-4 (2.12e-4 / 6.0e-4)
    The weighted launch stays below the unit one in every case (4.5e-6 ... 1.44e-4).  The kernel's error is 0.4 to 2.2 times
    the sequential fp32 oracle's own (e32) throughout: no placement stands out."""
    arc, lengths, w, ref = _log_case(N, scale)
    a, ln = t(arc), t(lengths)
    lz, g = Fn.deptree_run(a, ln, SR_LOG, True)
    check_log(f"log N={N} scale={scale:g}", lz, g, lengths, ref)
    lz2, g2 = Fn.deptree_run(a, ln, SR_LOG, True)
    assert torch.equal(lz2, lz) and torch.equal(g2, g)                       # bit-reproducible
    lzw, gw = Fn.deptree_run(a, ln, SR_LOG, True, grad_logZ=t(w))
    assert torch.equal(lzw, lz)
    check_log(f"log N={N} scale={scale:g} weighted", lzw, gw, lengths, ref, ref["gw"])
    if scale == 1.0 and N in (142, 143, 255):
        zi = Fn.deptree_run(a, ln, SR_LOG, False)[0].cpu().numpy()
        assert np.all(np.abs(zi - ref["z"]) <= logz_tol(ref["z"]))
        zm = Fn.deptree_run(a, ln, SR_MAX, False)[0].cpu().numpy()
        qm = oracle_mod.deptree(arc, lengths, "max", np.float64, grad=False)[0]
        assert np.all(np.abs(zm - qm) <= logz_tol(qm))


# ------------------------------------------------------------------------------------------------ C: Max semiring and decode
@functools.lru_cache(maxsize=None)
def _max_case(N):
    import oracle
    rng = np.random.default_rng(8000 + N)
    lengths = ragged_lengths(rng, N)
    arc = rng.standard_normal((len(lengths), N, N)).astype(np.float32)
    z64, g64 = oracle.deptree(arc, lengths, "max", np.float64)
    _, g32 = oracle.deptree(arc, lengths, "max", np.float32)
    frozen(arc, lengths, z64, g64, g32)
    return arc, lengths, z64, g64, g32


@pytest.mark.parametrize("N", [106, 107, 126, 127, 255])
def test_deptree_max_placements_vs_oracle(Fn, oracle_mod, N):
    """Max semiring with its back-pointer walk on both sides of 106/107 (all in LDS -> gI in the workspace) and 126/127 (-> values
    and back-pointers too) and at 255: score to 1e-5 relative, the one-hot equal to the oracle's arg-max indicators, decode heads
    equal to the one-hot, a projective single-root tree per sentence."""
    arc, lengths, z64, g64, g32 = _max_case(N)
    assert np.array_equal(g32, g64.astype(np.float32)), "precondition: the fp32 and fp64 oracle agree on the arg-max"
    a, ln = t(arc), t(lengths)
    mz, onehot = Fn.deptree_run(a, ln, SR_MAX, True)
    assert np.all(np.abs(mz.cpu().numpy() - z64) <= 1e-5 * np.maximum(1.0, np.abs(z64)))
    assert np.array_equal(onehot.cpu().numpy(), g64.astype(np.float32))
    best, heads = Fn.deptree_decode(a, ln)
    assert torch.equal(best, mz)
    h = heads.cpu().numpy()
    assert np.array_equal(h, heads_of(g64, lengths))
    for b, n in enumerate(lengths):
        assert oracle_mod.is_projective_tree(h[b], int(n)), b


# ------------------------------------------------------------------------------------------------ D: one batch, every placement
D_LENGTHS = np.array([60, 1, 2, 37, 45], np.int64)


@functools.lru_cache(maxsize=None)
def _embed_case():
    import oracle
    rng = np.random.default_rng(6100)
    arc = rng.standard_normal((len(D_LENGTHS), 61, 61)).astype(np.float32)
    w = rng.uniform(0.25, 1.0, len(D_LENGTHS)).astype(np.float32)
    frozen(arc, w)
    return arc, log_reference(oracle, arc, D_LENGTHS, w)


def embedded(a, N):
    """the [B,n,n] batch in the top-left corner of a zero [B,N,N] one"""
    out = np.zeros((a.shape[0], N, N), a.dtype)
    out[:, :a.shape[1], :a.shape[2]] = a
    return out


@pytest.mark.parametrize("N", [61, 83, 117, 143])
def test_deptree_same_sentences_across_log_placements(Fn, N):
    """One ragged batch (longest sentence 60 words) as it is and embedded in zero-padded widths that run in workspace modes 1, 2 and
    3: each meets the bound of its own 61-wide reference; rows and columns past the sentence are exact zeros (check_log).

    Observed marginal error on an MI355X: 2.29e-6 at each of the four widths (bound 5.00e-5), column sums within 3.42e-6."""
    arc, ref = _embed_case()
    wide = dict(ref, g=embedded(ref["g"], N))
    lz, g = Fn.deptree_run(t(embedded(arc, N)), t(D_LENGTHS), SR_LOG, True)
    assert tuple(g.shape) == (len(D_LENGTHS), N, N)
    check_log(f"embedded log N={N}", lz, g, D_LENGTHS, wide)
    if N > 61:
        assert float(g[:, 61:, :].abs().max()) == 0.0 and float(g[:, :, 61:].abs().max()) == 0.0


@pytest.mark.parametrize("N", [107, 127])
def test_deptree_same_sentences_across_max_placements(Fn, oracle_mod, N):
    """The same batch under the Max semiring: no reduction-order rounding and a positional tie rule, so score, one-hot and heads
    of the embedded batch equal those of the 61-wide launch bit for bit."""
    arc, _ = _embed_case()
    ln = t(D_LENGTHS)
    mz0, oh0 = Fn.deptree_run(t(arc), ln, SR_MAX, True)
    best0, heads0 = Fn.deptree_decode(t(arc), ln)
    mz, oh = Fn.deptree_run(t(embedded(arc, N)), ln, SR_MAX, True)
    best, heads = Fn.deptree_decode(t(embedded(arc, N)), ln)
    assert torch.equal(mz, mz0) and torch.equal(best, best0) and torch.equal(best, mz)
    assert torch.equal(oh[:, :61, :61], oh0) and float(oh.sum()) == float(oh0.sum()) == float(D_LENGTHS.sum())
    assert torch.equal(heads[:, :61], heads0) and int(heads[:, 61:].abs().max()) == 0
    h = heads.cpu().numpy()
    for b, n in enumerate(D_LENGTHS):
        assert oracle_mod.is_projective_tree(h[b], int(n)), b


# ------------------------------------------------------------------------------------------------ E: bf16 storage
@pytest.mark.parametrize("N", [41, 81, 100, 150])
def test_deptree_bf16_arcs(Fn, oracle_mod, N):
    """The bf16 instantiations of both semirings (short image, all in LDS, Log mode 1 / Max all in LDS, Log mode 3 / Max mode 2).
    The oracle runs on the rounded values.  bf16 scores repeat, so the Max semiring's tree is checked by value, not by identity.

    Observed marginal error on an MI355X: N = 41 1.99e-6, 81 4.45e-6, 100 5.55e-6 (bound 5.00e-5 each), 150 1.34e-5 (bound 6.72e-5)."""
    rng = np.random.default_rng(9000 + N)
    lengths = ragged_lengths(rng, N)
    a16 = torch.from_numpy(rng.standard_normal((len(lengths), N, N)).astype(np.float32)).bfloat16()
    arc = a16.float().numpy()
    a16, ln = a16.to(dev()), t(lengths)
    ref = log_reference(oracle_mod, arc, lengths)
    lz, g = Fn.deptree_run(a16, ln, SR_LOG, True)
    assert g.dtype == torch.float32
    check_log(f"bf16 log N={N}", lz, g, lengths, ref)
    q = oracle_mod.deptree(arc, lengths, "max", np.float64, grad=False)[0]
    mz, onehot = Fn.deptree_run(a16, ln, SR_MAX, True)
    best, heads = Fn.deptree_decode(a16, ln)
    assert torch.equal(best, mz)
    assert np.all(np.abs(mz.cpu().numpy() - q) <= 1e-5 * np.maximum(1.0, np.abs(q)))
    h = heads.cpu().numpy()
    assert np.array_equal(heads_of(onehot.cpu().numpy(), lengths), h)
    for b, n in enumerate(lengths):
        assert oracle_mod.is_projective_tree(h[b], int(n)), b
        assert not h[b, n + 1:].any() and h[b, 0] == 0
        assert abs(tree_score(arc[b], h[b], int(n)) - q[b]) <= 1e-5 * max(1.0, abs(q[b])), b


# ------------------------------------------------------------------------------------------------ F: -inf arcs
@pytest.mark.parametrize("N", [13, 120])
def test_deptree_minus_inf_arcs(Fn, oracle_mod, N):
    """-inf arcs (a caller masking with float('-inf')) act as probability zero: the same results as the finite sentinel -1e12 in
    their place, everything finite, exactly zero marginal on a killed arc, and a decoded tree that uses none.  About a quarter of
    the arcs are killed, never one of the root's, and the chain 0 -> 1 -> 2 ... survives, so every sentence keeps a tree.

    Observed marginal error on an MI355X: N = 13 6.2e-7, N = 120 1.11e-5 (bounds 5.00e-5, 6.08e-5)."""
    rng = np.random.default_rng(300 + N)
    lengths = ragged_lengths(rng, N, 6)
    B = len(lengths)
    arc = rng.standard_normal((B, N, N)).astype(np.float32)
    kill = rng.random((B, N, N)) < 0.25
    kill[:, 0, :] = False
    kill[:, np.arange(N - 1), np.arange(1, N)] = False
    a_inf, a_fin = arc.copy(), arc.copy()
    a_inf[kill] = -np.inf
    a_fin[kill] = -1e12
    ln = t(lengths)
    lz1, g1 = Fn.deptree_run(t(a_inf), ln, SR_LOG, True)
    lz2, g2 = Fn.deptree_run(t(a_fin), ln, SR_LOG, True)
    assert bool(torch.isfinite(lz1).all() and torch.isfinite(g1).all())
    assert torch.allclose(lz1, lz2, rtol=1e-6, atol=1e-5) and torch.allclose(g1, g2, atol=1e-6)
    ref = log_reference(oracle_mod, a_fin, lengths)   # the oracle itself returns NaN on -inf
    check_log(f"-inf arcs N={N}", lz1, g1, lengths, ref)
    assert float(g1[t(kill)].abs().max()) == 0.0
    q = oracle_mod.deptree(a_fin, lengths, "max", np.float64, grad=False)[0]
    best, heads = Fn.deptree_decode(t(a_inf), ln)
    assert np.all(np.abs(best.cpu().numpy() - q) <= 1e-5 * np.maximum(1.0, np.abs(q)))
    h = heads.cpu().numpy()
    for b, n in enumerate(lengths):
        assert oracle_mod.is_projective_tree(h[b], int(n)), b
        assert not any(kill[b, h[b, c], c] for c in range(1, n + 1)), b


# ------------------------------------------------------------------------------------------------ G: invalid lengths
@pytest.mark.parametrize("N", [6, 120])
def test_deptree_invalid_lengths(Fn, N):
    """Lengths 0 and N are no sentences: NaN score, zero grad_arc, zero heads, in every launch kind; their valid neighbours get the
    bits of a launch without them."""
    rng = np.random.default_rng(400 + N)
    arc = t(rng.standard_normal((5, N, N)).astype(np.float32))
    lengths = np.array([N - 1, 0, N // 2, N, 2 if N > 2 else 1], np.int64)
    bad, ok = [1, 3], [0, 2, 4]
    ln, ln_ok = t(lengths), t(lengths[ok])
    for sr in (SR_LOG, SR_MAX):
        lz, g = Fn.deptree_run(arc, ln, sr, True)
        lz_ok, g_ok = Fn.deptree_run(arc[ok].contiguous(), ln_ok, sr, True)
        assert bool(torch.isnan(lz[bad]).all()) and float(g[bad].abs().max()) == 0.0
        assert bool(torch.isfinite(lz[ok]).all()) and torch.equal(lz[ok], lz_ok) and torch.equal(g[ok], g_ok)
        zi = Fn.deptree_run(arc, ln, sr, False)[0]
        assert bool(torch.isnan(zi[bad]).all()) and torch.equal(zi[ok], Fn.deptree_run(arc[ok].contiguous(), ln_ok, sr, False)[0])
    best, heads = Fn.deptree_decode(arc, ln)
    best_ok, heads_ok = Fn.deptree_decode(arc[ok].contiguous(), ln_ok)
    assert bool(torch.isnan(best[bad]).all()) and int(heads[bad].abs().max()) == 0
    assert torch.equal(best[ok], best_ok) and torch.equal(heads[ok], heads_ok)
    assert int((heads[0, 1:] > 0).sum()) == N - 2


# ------------------------------------------------------------------------------------------------ H: ties
@pytest.mark.parametrize("N", [10, 110])
@pytest.mark.parametrize("pattern", ["all_zero", "root_is_nobodys_child"])
def test_deptree_ties_take_first_argmax(Fn, oracle_mod, N, pattern):
    """All-equal arcs: every tree ties, and torch.max's backward goes to the FIRST maximal index (test_emu_ties_take_first_argmax
    has the DMV form of the pattern): the device's back-pointers give the oracle's tree exactly."""
    arc = np.zeros((3, N, N), np.float32)
    if pattern == "root_is_nobodys_child":
        arc[:, :, 0] = -1e12
    lengths = np.array([N - 1, N // 2, 2], np.int64)
    z32, g32 = oracle_mod.deptree(arc, lengths, "max", np.float32)
    mz, onehot = Fn.deptree_run(t(arc), t(lengths), SR_MAX, True)
    best, heads = Fn.deptree_decode(t(arc), t(lengths))
    assert np.array_equal(mz.cpu().numpy(), z32) and torch.equal(best, mz)
    assert np.array_equal(onehot.cpu().numpy(), g32)
    assert np.array_equal(heads.cpu().numpy(), heads_of(g32, lengths))
