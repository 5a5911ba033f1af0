"""CPU: the split-K plan of vlg_linear_wgrad (plan_tn / tn_big, vlgae_amd/csrc/vlg_gemm.hip) restated in Python, pinned against the
library where the library shows it without a GPU, and the case table of tests/test_wgrad_plans_gpu.py with the class every case claims.

plan_tn turns (K, M, N, operand type, which column sums) into a tile shape, a stage depth, a split count S, the rows per split KC and a
grid of tiles x ceil(S / 8) x 8 workgroups.  The kernel bodies branch on what comes out:

  image          64-tile or 128-tile, bf16 (gemm_tn_kernel) or float32 operands (gemm_tn3_kernel); stage depth 128 / 64 / 64 / 32 rows
  full_stages    stages of a full split (KC / stage); the 64-tile bf16 image runs two stages per trip and an odd one behind the loop
  last_stages    stages of the last split (the only one when S = 1): its parity picks the same tail
  last_rows      rows of the last split; last_rows % stage != 0 is a SHORT last stage -- zeros from out-of-range buffer loads (bf16) or
                 from a per-row predicate (float32)
  S % 8 != 0     workgroups of the last group of eight splits that return at once

The K of a weight gradient is the number of token rows of the batch -- whatever the token-budget sampler produced, down to a single short
sentence -- so every one of these is reached in production.  CASES below holds the smallest sizes at which each exists; the numbers every
row claims were worked out from plan_tn as it stands, test_cases_are_in_the_class_their_name_claims re-derives them, and a change of the
plan constants fails here first instead of moving the GPU cases off their boundaries unnoticed.
"""
import collections
import ctypes
import re

import pytest

VLG_TN_WGS = 256        # workgroups a product is split into (tiles x row splits)
VLG_TN_BIG_MIN = 8      # 128-tiles an output must have to take the 128-tile kernel
STAGE = {("bf16", 64): 128, ("bf16", 128): 64, ("f32", 64): 64, ("f32", 128): 32}   # contraction rows per LDS stage

Plan = collections.namedtuple("Plan", "tile stage tiles KC S full_stages last_rows last_stages grid")


def cdiv(a, b):
    return (a + b - 1) // b


def tn_big(M, N):
    return M >= 128 and N >= 128 and cdiv(M, 128) * cdiv(N, 128) >= VLG_TN_BIG_MIN


def plan_tn(K, M, N, big, f32=False):
    tile = 128 if big else 64
    stage = STAGE["f32" if f32 else "bf16", tile]
    tiles = cdiv(M, tile) * cdiv(N, tile)
    S = cdiv(VLG_TN_WGS, tiles)
    max_s = cdiv(K, 2 * stage)                      # at least two stages per split
    S = max(1, min(S, max_s))
    KC = cdiv(cdiv(K, S), stage) * stage            # whole stages per split
    S = cdiv(K, KC)
    last_rows = K - (S - 1) * KC
    return Plan(tile, stage, tiles, KC, S, KC // stage, last_rows, cdiv(last_rows, stage), tiles * cdiv(S, 8) * 8)


def plan_of(ops, K, M, N, second):
    """the plan vlg_linear_wgrad takes: the 128-tile carries one kind of column sum, so both at once fall back to the 64-tile"""
    return plan_tn(K, M, N, tn_big(M, N) and second != "both", ops == "f32")


def plan_bytes(p, M, N):
    return 4 * p.S * (M * N + M + N)


def workspace_restated(K, M, N):
    """vlg_linear_wgrad_workspace: the largest of the plans any operand type / tile shape may take"""
    if K < 1 or M < 8 or N < 8 or M % 8 or N % 8:
        return 0
    return max(plan_bytes(plan_tn(K, M, N, big, f32), M, N) for f32 in (False, True) for big in ((False, True) if tn_big(M, N) else (False,)))


def describe(p):
    return f"{p.tile}-tile stage {p.stage}: S={p.S} KC={p.KC} full/last stages {p.full_stages}/{p.last_stages} last_rows={p.last_rows} grid={p.grid} ({p.tiles} tiles)"


# ---------------------------------------------------------------------------------------------------------------- the case table
# (operands, tile, output shapes, which column sums, {K: (S, full_stages, last_stages, last_rows)})
ONE = ("bias", "colsum", "none")     # d_bias only, x_colsum only, neither: the three 128-tile images; the 64-tile image carries both sums
SMALL64 = {1: (1, 1, 1, 1), 5: (1, 1, 1, 5), 127: (1, 1, 1, 127), 128: (1, 1, 1, 128),              # S = 1, one stage, short or exactly full
           129: (1, 2, 2, 129), 255: (1, 2, 2, 255), 256: (1, 2, 2, 256),                          # S = 1, two stages, the second short or full
           257: (2, 2, 1, 1), 383: (2, 2, 1, 127), 384: (2, 2, 1, 128),                            # S = 2, a one-stage (odd) last split beside a two-stage split
           385: (2, 2, 2, 129)}                                                                    # S = 2, the last split's second stage holds one row
SMALL128 = {1: (1, 1, 1, 1), 63: (1, 1, 1, 63), 64: (1, 1, 1, 64), 65: (1, 2, 2, 65),              # stage 64, one register set
            129: (2, 2, 1, 1), 257: (3, 2, 1, 1), 385: (4, 2, 1, 1), 2049: (17, 2, 1, 1)}          # S = 2, 3, 4, 17: last split of one row, S % 8 != 0
ROWS = [
    ("bf16", 64, [(8, 8), (64, 64), (72, 136)], ONE, SMALL64),
    ("bf16", 64, [(512, 8)], ONE, {10496: (28, 3, 1, 128),       # three stages per split (odd full split) and a one-stage last split, every stage full
                                   10369: (28, 3, 1, 1)}),       # ... with a last split of one row
    ("bf16", 64, [(72, 136)], ONE, {4099: (17, 2, 1, 3)}),       # S above 8 (three groups of eight, the last of one split), a three-row last split
    ("bf16", 128, [(256, 512), (264, 520)], ONE, SMALL128),      # 8 tiles (exactly VLG_TN_BIG_MIN) and 15 tiles with partial edges
    # image selection: both sides of tn_big
    ("bf16", 64, [(256, 384), (120, 1024)], ONE, {257: (2, 2, 1, 1)}),      # 6 tiles of 128; M < 128
    ("bf16", 128, [(128, 1024), (1024, 128)], ONE, {257: (3, 2, 1, 1)}),    # 8 tiles of 128 either way round
    # both column sums on an output big enough for the 128-tile: only through the C ABI, on the 64-tile image
    ("bf16", 64, [(256, 512)], ("both",), {129: (1, 2, 2, 129), 2049: (6, 3, 2, 129)}),
    # float32 operands (gemm_tn3_kernel)
    ("f32", 64, [(8, 8), (72, 136)], ONE, SMALL128),             # stage 64: the plan of the bf16 128-tile at these K
    ("f32", 128, [(256, 512), (264, 520)], ONE, {1: (1, 1, 1, 1), 31: (1, 1, 1, 31), 32: (1, 1, 1, 32), 33: (1, 2, 2, 33), 127: (2, 2, 2, 63),
                                                 129: (3, 2, 1, 1), 257: (5, 2, 1, 1)}),
    ("f32", 128, [(256, 512)], ONE, {2049: (22, 3, 2, 33)}),     # 8 tiles: S capped by the workgroup count, three stages per split
    ("f32", 128, [(264, 520)], ONE, {2049: (17, 4, 1, 1)}),      # 15 tiles
]

Case = collections.namedtuple("Case", "ops tile M N K second claim bf16_out")


def _cases():
    out = []
    for ops, tile, shapes, seconds, by_k in ROWS:
        for M, N in shapes:
            for K, claim in by_k.items():
                for second in seconds:
                    i = len(out)     # a third of them also with bf16 results: one of every three, moving through the kinds of column sum
                    out.append(Case(ops, tile, M, N, K, second, claim, (i + i // 3) % 3 == 0))
    return out


CASES = _cases()


def case_id(c):
    S, full, last, rows = c.claim
    return f"{c.ops}_t{c.tile}_{c.M}x{c.N}_K{c.K}_{c.second}_S{S}_f{full}_l{last}_r{rows}"


def klass(tile, stage, S, full, last, rows):
    """what the kernel bodies branch on"""
    return dict(tile=tile, S=S, full_stages_odd=bool(full & 1), last_stages_odd=bool(last & 1), short_last_stage=rows % stage != 0,
                partial_group_of_eight=S % 8 != 0)


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.fixture(scope="module")
def lib():
    from vlgae_amd.build import build_library
    build_library()            # hipcc cross-compiles for gfx950 without a GPU
    from vlgae_amd import _C
    return _C.lib()


def test_cases_are_in_the_class_their_name_claims():
    """Every case of the GPU file: the restated plan gives the image, the split count, the stage counts of a full and of the last split
    and the last split's rows that the table (and so the case's id) claims.  If a plan constant changes, this names the cases that moved."""
    moved = []
    for c in CASES:
        p = plan_of(c.ops, c.K, c.M, c.N, c.second)
        S, full, last, rows = c.claim
        want = klass(c.tile, STAGE[c.ops, c.tile], S, full, last, rows)
        got = klass(p.tile, p.stage, p.S, p.full_stages, p.last_stages, p.last_rows)
        if got != want or (p.S, p.full_stages, p.last_stages, p.last_rows) != c.claim:
            moved.append(f"{case_id(c)}: the plan is now {describe(p)}; class {got}, the case claims {want}")
    assert not moved, "cases that left the path they were written for:\n  " + "\n  ".join(moved)
    assert len({case_id(c) for c in CASES}) == len(CASES)


def test_case_table_covers_every_path():
    """The paths the kernel bodies distinguish, each held by at least one case (from the claims alone)."""
    def has(ops, tile, **want):
        return any(c.ops == ops and c.tile == tile and all(klass(tile, STAGE[ops, tile], *c.claim)[k] == v for k, v in want.items()) for c in CASES)
    for ops, tile in STAGE:
        assert has(ops, tile, S=1, short_last_stage=True) and has(ops, tile, S=1, short_last_stage=False), (ops, tile)
        assert has(ops, tile, last_stages_odd=True, short_last_stage=True) and has(ops, tile, last_stages_odd=False, short_last_stage=True), (ops, tile)
        assert has(ops, tile, S=2) and has(ops, tile, partial_group_of_eight=True), (ops, tile)
        assert any(c.ops == ops and c.tile == tile and c.claim[0] > 8 for c in CASES), (ops, tile)          # more than one group of eight splits
        assert any(c.ops == ops and c.tile == tile and c.claim[0] >= 2 and c.claim[3] == 1 for c in CASES), (ops, tile)   # a last split of one row
    # the two-register-set pipeline: an odd full split, an odd full split beside an odd last one, even beside odd, even beside even
    assert has("bf16", 64, full_stages_odd=True, last_stages_odd=True) and has("bf16", 64, full_stages_odd=False, last_stages_odd=True)
    assert has("bf16", 64, full_stages_odd=False, last_stages_odd=False) and has("bf16", 64, full_stages_odd=True, last_stages_odd=False)
    # both sides of tn_big, and the fallback with both column sums
    assert tn_big(256, 512) and tn_big(128, 1024) and tn_big(1024, 128) and not tn_big(256, 384) and not tn_big(120, 1024)
    assert any(c.second == "both" and c.tile == 64 and tn_big(c.M, c.N) for c in CASES)
    assert abs(sum(c.bf16_out for c in CASES) * 3 - len(CASES)) <= 3 and {c.second for c in CASES if c.bf16_out} == {"bias", "colsum", "none", "both"}


def test_workspace_equals_the_largest_restated_plan(lib):
    """vlg_linear_wgrad_workspace(K, M, N) = max over the plans it considers (both operand types; both tile shapes when tn_big) of
    4 S (M N + M + N): over the whole case table, K = 1 .. 600 for three output shapes, and 0 for the shapes it refuses."""
    q = lib.vlg_linear_wgrad_workspace
    for c in CASES:
        assert q(c.K, c.M, c.N) == workspace_restated(c.K, c.M, c.N), case_id(c)
        p = plan_of(c.ops, c.K, c.M, c.N, c.second)
        assert 0 < plan_bytes(p, c.M, c.N) <= q(c.K, c.M, c.N), case_id(c)             # the plan the call takes fits
    for M, N in ((8, 8), (72, 136), (264, 520)):
        for K in range(1, 601):
            assert q(K, M, N) == workspace_restated(K, M, N), (K, M, N, describe(plan_tn(K, M, N, False)))
    for K, M, N in ((0, 64, 64), (-1, 64, 64), (256, 0, 64), (256, 64, 0), (256, -8, 64), (256, 64, -8), (256, 4, 64), (256, 64, 4), (256, 20, 72),
                    (256, 72, 20), (256, 65, 64), (256, 64, 127)):
        assert q(K, M, N) == 0 == workspace_restated(K, M, N), (K, M, N)


def test_restated_plan_invariants():
    """What the kernels rely on, for every K up to 600 and the table's own sizes: whole stages per split, every split non-empty, the splits
    cover K exactly, at least two stages per full split once there is more than one split, a grid of whole groups of eight."""
    sizes = {(c.ops, c.K, c.M, c.N, c.second) for c in CASES}
    sizes |= {(ops, K, M, N, "bias") for ops in ("bf16", "f32") for M, N in ((8, 8), (72, 136), (264, 520)) for K in range(1, 601)}
    for ops, K, M, N, second in sizes:
        p = plan_of(ops, K, M, N, second)
        assert p.KC % p.stage == 0 and p.S >= 1 and 1 <= p.last_rows <= p.KC and (p.S - 1) * p.KC + p.last_rows == K, (ops, K, M, N)
        assert p.S == 1 or p.full_stages >= 2, (ops, K, M, N)
        assert p.grid % 8 == 0 and p.grid >= p.tiles * p.S, (ops, K, M, N)


def test_linear_wgrad_argument_edges_on_the_host(lib):
    """K = 0, a workspace one byte short, row strides that are no multiple of 8 or below the column count: refused before any launch
    (tests/test_cabi.py holds the dtype check and the multiple-of-8 workspace query of this entry)."""
    K, M, N = 257, 72, 136
    need = lib.vlg_linear_wgrad_workspace(K, M, N)
    big = (2049, 256, 512)
    # Every call below is refused before any launch, so the pointer is never used.  This file also runs where a GPU is present: there the
    # pointer is a real buffer large enough for every operand, workspace and output of both shapes, so that a host check weakened
    # later turns into a failing assertion here and not into a launch on a made-up address.
    import torch
    if torch.cuda.is_available():
        held = torch.zeros(max(need, lib.vlg_linear_wgrad_workspace(*big)) + 4 * (big[0] + 32) * (big[2] + 40), dtype=torch.uint8, device="cuda:0")
        one = ctypes.c_void_p(held.data_ptr())
    else:
        one = ctypes.c_void_p(64)

    def call(K=K, ld_dy=M + 16, ld_x=N + 16, ws=need, in_dtype=1, second=(one, None), ld_dw=N + 40):
        return lib.vlg_linear_wgrad(one, ld_dy, one, ld_x, K, M, N, in_dtype, one, ws, 0, one, ld_dw, second[0], second[1], None)

    def needed(rc):
        """the size the refusal of an EMPTY workspace names: every short call below is checked against it first, so none can reach a launch"""
        assert rc == 0x1004
        return int(re.search(rb"needs a (\d+)-byte workspace", lib.vlg_last_error()).group(1))

    for in_dtype in (0, 1):
        assert call(K=0, in_dtype=in_dtype) == 0x1001 and b"K >= 1" in lib.vlg_last_error()
        own = plan_bytes(plan_of("f32" if in_dtype == 0 else "bf16", K, M, N, "bias"), M, N)      # what this call needs: at most the query's answer
        assert 0 < own <= need and needed(call(ws=0, in_dtype=in_dtype)) == own
        assert call(ws=own - 1, in_dtype=in_dtype) == 0x1004 and b"workspace" in lib.vlg_last_error()
        assert call(ld_dy=M + 4, in_dtype=in_dtype) == 0x1001 and b"row strides" in lib.vlg_last_error()       # not a multiple of 8
        assert call(ld_x=N + 4, in_dtype=in_dtype) == 0x1001
        assert call(ld_dy=M - 8, in_dtype=in_dtype) == 0x1001 and call(ld_x=N - 8, in_dtype=in_dtype) == 0x1001   # below the column count
        assert call(ld_dw=N - 8, in_dtype=in_dtype) == 0x1001
    # the workspace bound is the plan's own: both column sums on a 128-tile output take the 64-tile plan, and its size is what is checked
    K, M, N = big
    args = (one, M + 16, one, N + 16, K, M, N, 1, one)
    both, single = (plan_bytes(plan_of("bf16", K, M, N, second), M, N) for second in ("both", "bias"))
    assert single != both and max(single, both) <= lib.vlg_linear_wgrad_workspace(K, M, N)
    assert needed(lib.vlg_linear_wgrad(*args, 0, 0, one, N, one, one, None)) == both and lib.vlg_linear_wgrad(*args, both - 1, 0, one, N, one, one, None) == 0x1004
    assert needed(lib.vlg_linear_wgrad(*args, 0, 0, one, N, one, None, None)) == single and lib.vlg_linear_wgrad(*args, single - 1, 0, one, N, one, None, None) == 0x1004
