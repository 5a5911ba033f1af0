"""vlg_linear_wgrad (gemm_tn_kernel / gemm_tn3_kernel / the reductions, vlgae_amd/csrc/vlg_gemm.hip) at every split plan and row count:
the case table and the restated plan come from tests/test_wgrad_plans.py, which pins each case to the path its id names.

Exact operands.  Every product and every partial sum, in any order, is exactly representable in float32, so a float32 result must equal
the float64 reference BIT FOR BIT and a bf16 result must equal that reference rounded once -- no tolerance:
  bf16 operands      integers in [-3, 3], a quarter of them zero
  float32 operands   one operand on the same integer grid (its lo part is zero), the other m * 2^-8 with integer |m| < 1024: hi = bf16(v) and
                     lo = v - hi are both exact multiples of 2^-8 and mostly both non-zero, so a_hi b + a_lo b is the exact product; run
                     with the two-part operand as dy (the a_lo b_hi term) and again as x (the a_hi b_lo term)
  bit budget         asserted per case from the float64 reference alone: max(|dy|^T |x|) and the column sums of |dy| and |x|, in units of
                     the grid step, stay below 2^22.  A condition on the inputs, not a bound on the result.

Guards.  The C ABI is called directly so the test owns every buffer: operands are rows [16, 16 + K) and the leading columns of a
[K + 32, columns + 16] tensor whose other elements are NaN; the workspace holds exactly vlg_linear_wgrad_workspace(K, M, N) bytes of 0xFF
(NaN as float32) with a 256-byte tail the library is not told about; d_weight is columns [16, 16 + N) of an [M, N + 40] NaN tensor, d_bias
and x_colsum sit in NaN vectors with 8 elements on each side.  A read of anything the plan does not cover turns a result into NaN, a
missing write leaves one, a stray write removes one from a guard.  Every call is repeated (same bits) and run once more through
align.linear_wgrad on the same views (taken in place; same bits).

Ordinary data.  test_small_k_rounding_data holds the small-K plans to the bounds of test_linear_wgrad_partial_tiles /
test_linear_wgrad_float32_operands (tests/test_gpu_parity.py), unchanged.
"""
import functools

import pytest
import torch

from test_wgrad_plans import CASES, STAGE, case_id, describe, plan_bytes, plan_of, workspace_restated

pytestmark = pytest.mark.gpu

NAN = float("nan")
BF, F32 = torch.bfloat16, torch.float32


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from vlgae_amd import _C
    return _C.lib()   # must load: the product has no fallback


# ---------------------------------------------------------------------------------------------------------------- exact operands
INT_GRID = torch.tensor([-3., -2., -1., 0., 0., 1., 2., 3.], dtype=torch.float64)     # a quarter zero


def int_grid(gen, rows, cols):
    return INT_GRID[torch.randint(0, 8, (rows, cols), generator=gen)]


def two_part_grid(gen, rows, cols):
    return torch.randint(-1023, 1024, (rows, cols), generator=gen).double() * 2.0 ** -8


@functools.lru_cache(maxsize=4)     # a set serves the consecutive cases of one size (three kinds of column sum); nothing keeps the rest alive
def exact_operands(ops, K, M, N):
    """[(label, dy [K,M], x [K,N], grid step)] as float64 on the host: one pair for bf16 operands, both role assignments for float32"""
    gen = torch.Generator().manual_seed(1000003 * K + 1009 * M + N + (7 if ops == "f32" else 0))
    if ops == "bf16":
        return [("integers", int_grid(gen, K, M), int_grid(gen, K, N), 1.0)]
    two_dy, two_x = two_part_grid(gen, K, M), two_part_grid(gen, K, N)
    for v in (two_dy, two_x):   # lo exact; hi and lo both non-zero wherever m has more than 8 significant bits (half of the draws)
        hi = v.float().bfloat16().double()
        assert (v.numel() < 1000 or float(((v != hi) & (hi != 0)).double().mean()) > 0.4) and torch.equal((v - hi).float().bfloat16().double(), v - hi)
    return [("dy two-part", two_dy, int_grid(gen, K, N), 2.0 ** -8), ("x two-part", int_grid(gen, K, M), two_x, 2.0 ** -8)]


def reference(dy64, x64, step):
    """float64 results and the bit-budget condition that makes them exact in float32 whatever the order of summation"""
    ref = dict(w=dy64.t() @ x64, bias=dy64.sum(0), colsum=x64.sum(0))
    budget = max(float((dy64.abs().t() @ x64.abs()).max()), float(dy64.abs().sum(0).max()), float(x64.abs().sum(0).max())) / step
    assert budget < 2 ** 22, budget
    for v in ref.values():
        assert torch.equal(v.float().double(), v)
    return ref


# ---------------------------------------------------------------------------------------------------------------- guarded buffers
def guarded_operand(vals, dtype):
    K, C = vals.shape
    full = torch.full((K + 32, C + 16), NAN, dtype=dtype, device=dev())
    view = full[16:16 + K, :C]
    view.copy_(vals.to(dtype))
    assert view.stride(1) == 1 and view.stride(0) % 8 == 0 and view.data_ptr() % 16 == 0     # what align.linear_wgrad takes in place
    return full, view


def guarded_outputs(M, N, second, odt):
    wide = torch.full((M, N + 40), NAN, dtype=odt, device=dev())
    vecs = {}
    for name, n in (("bias", M), ("colsum", N)):
        if second in (name, "both"):
            vecs[name] = torch.full((n + 16,), NAN, dtype=odt, device=dev())
    return wide, vecs


def check_outputs(tag, wide, vecs, M, N, ref, odt):
    """the written regions equal the reference exactly (rounded once for bf16 results); every guard element is still NaN"""
    for name, got, full, want in [("d_weight", wide[:, 16:16 + N], wide, ref["w"])] + [(k, v[8:-8], v, ref[k]) for k, v in vecs.items()]:
        want = want.float().to(odt)
        got = got.cpu()
        if not torch.equal(got, want):
            bad = (got != want) | torch.isnan(got)
            where = bad.nonzero()[0].tolist()
            at = tuple(where)
            raise AssertionError(f"{tag}: {name} differs from the float64 reference in {int(bad.sum())} of {bad.numel()} elements "
                                 f"({int(torch.isnan(got).sum())} NaN); first at {where}: got {float(got[at])}, want {float(want[at])}")
        assert int(torch.isnan(full).sum()) == full.numel() - want.numel(), f"{tag}: a guard element of {name} was written"


def same_bits(tag, first, other):
    """two result sets, guards included, bit for bit (NaN guards compare as their bit patterns)"""
    for (name, a), b in zip([("d_weight", first[0])] + sorted(first[1].items()), [other[0]] + [v for _, v in sorted(other[1].items())]):
        bits = torch.int32 if a.dtype == F32 else torch.int16
        assert torch.equal(a.view(bits), b.view(bits)), f"{tag}: {name} differs from the first call's bits"


def call_cabi(lib, dy, x, K, M, N, ws, nbytes, wide, vecs):
    from vlgae_amd import _C
    idt = _C.BF16 if dy.dtype == BF else _C.F32
    odt = _C.BF16 if wide.dtype == BF else _C.F32
    dw = wide[:, 16:16 + N]
    inner = {k: v[8:-8] for k, v in vecs.items()}
    _C.check(lib.vlg_linear_wgrad(_C.ptr(dy), dy.stride(0), _C.ptr(x), x.stride(0), K, M, N, idt, _C.ptr(ws), nbytes, odt, _C.ptr(dw), dw.stride(0),
                                  _C.ptr(inner.get("bias")), _C.ptr(inner.get("colsum")), _C.stream_of(dy)), "linear_wgrad")


def run_exact_case(lib, c):
    from vlgae_amd import align
    K, M, N = c.K, c.M, c.N
    p = plan_of(c.ops, K, M, N, c.second)
    print(f"[wgrad] {case_id(c)}: {c.ops} operands, {describe(p)}")
    assert (p.tile, p.S, p.full_stages, p.last_stages, p.last_rows) == (c.tile,) + c.claim      # (test_wgrad_plans.py says which cases moved)
    nbytes = int(lib.vlg_linear_wgrad_workspace(K, M, N))
    assert nbytes == workspace_restated(K, M, N) and plan_bytes(p, M, N) <= nbytes
    dtype = BF if c.ops == "bf16" else F32
    for label, dy64, x64, step in exact_operands(c.ops, K, M, N):
        ref = reference(dy64, x64, step)
        dy_full, dy = guarded_operand(dy64, dtype)
        x_full, x = guarded_operand(x64, dtype)
        for odt in (F32, BF) if c.bf16_out else (F32,):
            tag = f"{case_id(c)} [{label}, {'bf16' if odt == BF else 'float32'} results]"
            ws = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device=dev())
            wide, vecs = guarded_outputs(M, N, c.second, odt)
            call_cabi(lib, dy, x, K, M, N, ws, nbytes, wide, vecs)
            check_outputs(tag, wide, vecs, M, N, ref, odt)
            assert int((ws[nbytes:] != 0xFF).sum()) == 0, f"{tag}: a write behind the workspace"
            # once more, into fresh outputs over the used workspace: the same bits
            wide2, vecs2 = guarded_outputs(M, N, c.second, odt)
            call_cabi(lib, dy, x, K, M, N, ws, nbytes, wide2, vecs2)
            same_bits(tag + " repeated", (wide, vecs), (wide2, vecs2))
            check_outputs(tag + " repeated", wide2, vecs2, M, N, ref, odt)
            assert int((ws[nbytes:] != 0xFF).sum()) == 0, f"{tag}: a write behind the workspace"
            if c.second != "both":   # the Python entry on the same views (both sums at once exist only in the C ABI)
                wide3, vecs3 = guarded_outputs(M, N, c.second, odt)
                second = vecs3[c.second][8:-8] if vecs3 else None
                dw, _ = align.linear_wgrad(dy, x, want_bias=c.second == "bias", want_x_colsum=c.second == "colsum", out=(wide3[:, 16:16 + N], second))
                assert dw.data_ptr() == wide3[:, 16:16 + N].data_ptr()
                same_bits(tag + " through align.linear_wgrad", (wide, vecs), (wide3, vecs3))
                check_outputs(tag + " through align.linear_wgrad", wide3, vecs3, M, N, ref, odt)
        # the operands are as they were, their guards included
        for full, vals in ((dy_full, dy64), (x_full, x64)):
            assert torch.equal(full[16:16 + K, :vals.shape[1]].cpu().double(), vals) and int(torch.isnan(full).sum()) == full.numel() - vals.numel()


@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_exact_operands_every_plan(lib, c):
    """Every case of the table (see test_wgrad_plans.py for the path each id names): bit-equal to float64, guards untouched, repeatable,
    the same through align.linear_wgrad; a third of the cases also with bf16 results (the exact value rounded once); float32 operands in both
    role assignments of the two-part operand."""
    run_exact_case(lib, c)


def test_lazy_group_exact_operands(lib):
    """A lazy WgradGroup -- one grid per kernel image (vlg_linear_wgrad_partial_group), one grouped reduction -- on exact operands: every
    item equals its float64 reference bit for bit (test_linear_wgrad_lazy_group_equals_single_launches shows equality with the single
    launches only).  In this order: three S = 1 items on the 64-tile, two 128-tile items whose last split is one row, one large item, one
    float32 item (its own launch), then K = 257 items until the 64-tile class exceeds one launch's 8 items and the reductions exceed 12."""
    from vlgae_amd import align
    items = [("bf16", 1, 72, 136, "bias"), ("bf16", 5, 72, 136, "colsum"), ("bf16", 129, 72, 136, "none"),
             ("bf16", 129, 256, 512, "bias"), ("bf16", 257, 264, 520, "colsum"), ("bf16", 4099, 72, 136, "bias"), ("f32", 33, 264, 520, "bias")]
    items += [("bf16", 257, 72, 136, ("bias", "colsum", "none")[i % 3]) for i in range(5)] + [("bf16", 257, 64, 64, "bias"), ("bf16", 257, 8, 8, "colsum")]
    plans = [plan_of(ops, K, M, N, second) for ops, K, M, N, second in items]
    for it, p in zip(items, plans):
        print(f"[wgrad] group item {it}: {describe(p)}")
    assert [p.S for p in plans[:3]] == [1, 1, 1] and all(p.tile == 64 for p in plans[:3])
    assert all(p.tile == 128 and p.S >= 2 and p.last_rows == 1 for p in plans[3:5]) and plans[6].tile == 128 and plans[6].last_rows == 1 + STAGE["f32", 128]
    assert sum(p.tile == 64 and it[0] == "bf16" for it, p in zip(items, plans)) > 8 and len(items) > 12
    wg = align.WgradGroup(lazy=True)
    outs, refs, keep = [], [], []
    for ops, K, M, N, second in items:
        label, dy64, x64, step = exact_operands(ops, K, M, N)[0]
        refs.append(reference(dy64, x64, step))
        (_, dy), (_, x) = guarded_operand(dy64, BF if ops == "bf16" else F32), guarded_operand(x64, BF if ops == "bf16" else F32)
        keep.append((dy, x))
        outs.append(align.linear_wgrad(dy, x, want_bias=second == "bias", want_x_colsum=second == "colsum", defer=wg))
    wg.flush()
    for it, (dw, vec), ref in zip(items, outs, refs):
        assert torch.equal(dw.cpu().double(), ref["w"]), it
        assert (vec is None) == (it[4] == "none") and (vec is None or torch.equal(vec.cpu().double(), ref[it[4]])), it


ROUNDING = [(ops, M, N, K) for ops, M, N in (("bf16", 72, 136), ("f32", 72, 136), ("bf16", 264, 520)) for K in (1, 5, 129, 257, 385)]


@pytest.mark.parametrize("ops,M,N,K", ROUNDING, ids=[f"{o}_{m}x{n}_K{k}" for o, m, n, k in ROUNDING])
def test_small_k_rounding_data(lib, ops, M, N, K):
    """Random normal operands at the small row counts, under the bounds of test_linear_wgrad_partial_tiles (bf16: 1e-5 max|ref| + 1e-3; the
    column sum of x 1e-3) and test_linear_wgrad_float32_operands (2e-5 max|ref|; + 1e-9 / + 1e-6 for the two column sums), as they are."""
    from vlgae_amd import align
    print(f"[wgrad] rounding {ops} {M}x{N} K={K}: {describe(plan_of(ops, K, M, N, 'bias'))}")
    gen = torch.Generator().manual_seed(31 * K + M + (1 if ops == "f32" else 0))
    if ops == "bf16":
        dy_full, x_full = torch.randn(K, M + 16, generator=gen).to(dev(), BF), torch.randn(K, N + 16, generator=gen).to(dev(), BF)
    else:
        dy_full = (torch.randn(K, M + 16, generator=gen) * torch.rand(K, 1, generator=gen) * 1e-3).to(dev())     # cotangent-sized values
        x_full = torch.randn(K, N + 16, generator=gen).to(dev())
    dy, x = dy_full[:, :M], x_full[:, :N]
    dw, db = align.linear_wgrad(dy, x)
    _, xs = align.linear_wgrad(dy, x, want_x_colsum=True)
    rw, rb, rx = dy.double().t() @ x.double(), dy.double().sum(0), x.double().sum(0)
    ew, eb, ex = (float((a.double() - b).abs().max()) for a, b in ((dw, rw), (db, rb), (xs, rx)))
    mw, mb, mx = float(rw.abs().max()), float(rb.abs().max()), float(rx.abs().max())
    print(f"[wgrad]   d_weight err {ew:.3e} (max|ref| {mw:.3e}), d_bias err {eb:.3e} (max|ref| {mb:.3e}), x_colsum err {ex:.3e} (max|ref| {mx:.3e})")
    if ops == "bf16":
        assert ew <= 1e-5 * mw + 1e-3 and eb <= 1e-5 * mb + 1e-3 and ex <= 1e-3
    else:
        assert ew <= 2e-5 * mw and eb <= 2e-5 * mb + 1e-9 and ex <= 2e-5 * mx + 1e-6
