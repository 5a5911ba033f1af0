"""CPU: DMV1o tree sampling (DMV1o.sample_heads) without a GPU -- the float64 restatement of the rule pinned on the reference-made
fixtures, the walk of vlgae_amd/csrc/vlg_dmv_sample.h under the host emulator (tests/emu/emu_dmv_sample.cpp), the same emulator as a
stand-alone program under AddressSanitizer + UBSan, the C ABI's host-side contract and the Python surface.

Steering (tests/dmv_sample_restatement.py): the float64 restatement writes, for a chosen tree, the midpoint of the wanted split's
interval into the uniform table; the float32 walk must then return exactly that tree.  Potentials are 0.25 randn, root-merged; every
steered split keeps a conditional probability of at least 0.01 (asserted, no target excluded): both chains as they are, the root's child
at the positions whose root split reaches that floor, the other trees grown through splits of probability >= 0.02.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dmv_sample_restatement as D
from conftest import GOLDEN, ROOT, golden_files, golden_ids, load

HERE = os.path.join(ROOT, "tests", "emu")
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "emu_dmv_sample.cpp")
DEPS = [SRC, os.path.join(HERE, "emu_dp.cpp"), os.path.join(HERE, "emu_sample_common.h")] + [
    os.path.join(ROOT, "vlgae_amd", "csrc", f) for f in ("vlg_dp_core.h", "vlg_dmv_sample.h", "vlg_sample_common.h")]
FLOOR = 0.01
SHAPE, DTYPE, WORKSPACE, NULL = 0x1001, 0x1002, 0x1004, 0x1005
LDS_BUDGET = 160 * 1024


def _build(out, extra):
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", *extra, SRC, "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def emu():
    return ctypes.CDLL(_build(os.path.join(BUILD, "libvlg_emu_dmv_sample.so"), ["-fPIC", "-shared"]))


@pytest.fixture(scope="module")
def lib():
    from vlgae_amd.build import build_library
    build_library()
    from vlgae_amd import _C
    return _C.lib()


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def merged_fixture(g):
    "the fixture's potentials root-merged, float64"
    return D.merge64(g["dec"].astype(np.float64), g["attach"].astype(np.float64), g["root"].astype(np.float64))


# ---- 1. the restatement, pinned on what the reference computed ------------------------------------------------------------------------------
@pytest.mark.parametrize("path", golden_files("dmv_"), ids=golden_ids("dmv_"))
def test_restatement_inside_pass_and_best_tree_match_the_reference(path):
    g = load(path)
    dec, attach = merged_fixture(g)
    for b, L in enumerate(int(x) for x in g["lengths"]):
        charts = D.inside64(dec[b], attach[b], L)
        assert abs(D.log_partition(charts, L) - g["logZ64"][b, 0]) <= 1e-9
        score, _, cd, ca = D.tree_score(dec[b], attach[b], g["predicted"][b], L)
        assert abs(score - g["max64"][b, 0]) <= 1e-9
        if "maxgrad_dec64" in g:   # (the fixtures of the largest cases store no gradients)
            assert np.array_equal(cd, g["maxgrad_dec64"][b]) and np.array_equal(ca, g["maxgrad_attach64"][b])


@pytest.mark.parametrize("name", ("dmv_B5_L7_s2", "dmv_B3_L2_s4", "dmv_B3_L1_s3"))
def test_restatement_tree_scores_sum_to_the_partition_function(name):
    "every projective single-root tree of every sentence of <= 6 words (7 words: 38 s of enumeration, left out)"
    g = load(os.path.join(GOLDEN, name + ".npz"))
    dec, attach = merged_fixture(g)
    seen = 0
    for b, L in enumerate(int(x) for x in g["lengths"]):
        if L > 6:
            continue
        scores = [D.tree_score(dec[b], attach[b], t, L)[0] for t in D.all_trees(L)]
        assert len(scores) == {1: 1, 2: 2, 3: 7, 4: 30, 5: 143, 6: 728}[L]
        assert abs(np.logaddexp.reduce(scores) - g["logZ64"][b, 0]) <= 1e-9
        seen += 1
    assert seen >= 3


# ---- 2. the walk under the emulator -------------------------------------------------------------------------------------------------------
def steered_case(N, seed, count=12):
    "(dec [N,2,2,2], attach [N,N,2], targets [S,N], u [S,3,N,N], pmin, rows' charts) for one sentence of full length"
    rng = np.random.default_rng(seed)
    L = N - 1
    dec, attach = (x[0] for x in D.merge64(*D.random_unmerged(rng, 1, L)))
    charts = D.inside64(dec, attach, L)
    rows = D.steered_rows(dec, attach, L, count, rng, FLOOR, charts)
    return dec, attach, np.stack([D.pad_heads(h, N) for _, _, h in rows]), np.stack([u for u, _, _ in rows]), min(p for _, p, _ in rows), charts


def run_emu(emu, dec, attach, lengths, u, order=0):
    B, N = dec.shape[:2]
    S = u.shape[0]
    dec, attach, u = (np.ascontiguousarray(x, np.float32) for x in (dec, attach, u))
    ln = np.ascontiguousarray(lengths, np.int64)
    heads = np.full((S, B, N), -1, np.int64)
    logp, logZ = np.full((S, B), np.nan, np.float32), np.full(B, np.nan, np.float32)
    assert emu.emu_dmv1o_sample(_p(dec), _p(attach), _p(ln), B, N, 0, S, _p(u), _p(heads), _p(logp), _p(logZ), 16, order) == 0
    return heads, logp, logZ


def first_workspace_n(lib):
    "the smallest N whose charts the launcher keeps in the workspace"
    return next(N for N in range(2, 256) if lib.vlg_dmv1o_sample_workspace(1, N, 1) > 0)


@pytest.mark.parametrize("N", (2, 3, 6, 41, 66, "last_lds", "first_ws"))
def test_emulator_returns_steered_trees(emu, lib, N):
    if isinstance(N, str):
        N = first_workspace_n(lib) - (1 if N == "last_lds" else 0)
    assert emu.emu_dmv_sample_placement(N) == (1 if lib.vlg_dmv1o_sample_workspace(1, N, 1) else 0)   # the emulator carves as the launcher plans
    dec, attach, targets, u, pmin, charts = steered_case(N, seed=200 + N, count=12 if N <= 66 else 4)
    print(f"N={N}: {len(targets)} steered trees, smallest conditional probability {pmin:.4f}")
    assert pmin >= FLOOR
    L = N - 1
    before = emu.emu_canary_trips()
    heads, logp, logZ = run_emu(emu, dec[None], attach[None], [L], u[:, None], order=2 if N <= 6 else 0)
    assert np.array_equal(heads[:, 0], targets)
    assert emu.emu_canary_trips() == before == 0
    lz = D.log_partition(charts, L)
    assert abs(logZ[0] - lz) <= 2e-5 * max(1.0, abs(lz))
    for s in range(len(targets)):
        score, mag, _, _ = D.tree_score(dec, attach, targets[s], L)
        assert abs(logp[s, 0] - (score - lz)) <= 2e-5 * max(1.0, abs(lz)) + (4 * L + 1) * 2.0 ** -23 * mag


def test_emulator_both_placements_at_one_size(emu):
    "the workspace placement forced at N = 41: both charts in the second arena, only the staged dec and the stack in the first"
    dec, attach, targets, u, pmin, _ = steered_case(41, seed=7, count=4)
    assert pmin >= FLOOR
    emu.emu_set_dmv_sample_mode(1)
    try:
        heads, _, _ = run_emu(emu, dec[None], attach[None], [40], u[:, None])
    finally:
        emu.emu_set_dmv_sample_mode(-1)
    assert np.array_equal(heads[:, 0], targets) and emu.emu_canary_trips() == 0


def test_emulator_short_sentence_in_a_wide_batch_and_bad_lengths(emu):
    "ragged lengths: charts of a short sentence inside a wider tensor; an invalid length gives heads 0, logp NaN, logZ NaN"
    N = 9
    rng = np.random.default_rng(5)
    dec, attach = D.merge64(*D.random_unmerged(rng, 4, N - 1))
    lengths = [5, 0, 1, N]
    u = np.full((2, 4, 3, N, N), np.nan, np.float32)
    want = np.zeros((2, 4, N), np.int64)
    for s in range(2):
        u[s, 0], _, h = D.steer(dec[0], attach[0], 5, pick=D.floor_pick(rng, 0.02))
        want[s, 0] = D.pad_heads(h, N)
        u[s, 2], _, h = D.steer(dec[2], attach[2], 1, D.right_chain(1))
        want[s, 2] = D.pad_heads(h, N)
    heads, logp, logZ = run_emu(emu, dec, attach, lengths, u)
    assert np.array_equal(heads, want) and emu.emu_canary_trips() == 0
    assert np.isnan(logp[:, [1, 3]]).all() and np.isnan(logZ[[1, 3]]).all() and np.isfinite(logp[:, [0, 2]]).all()


def test_nan_uniform_takes_the_last_split_of_positive_weight(emu):
    "a NaN uniform (and u within an ulp of 1) falls through to the largest r with w_r > 0 -- never to a forbidden split"
    N, L = 6, 5
    rng = np.random.default_rng(11)
    dec, attach = (x[0] for x in D.merge64(*D.random_unmerged(rng, 1, L)))
    attach[0, 4:, :] = -np.inf                               # the root's child cannot be word 4 or 5
    u = np.full((2, 1, 3, N, N), np.nan, np.float32)
    u[1] = np.nextafter(np.float32(1), np.float32(0))
    heads, logp, _ = run_emu(emu, dec[None], attach[None], [L], u)
    for s in range(2):
        assert D.is_tree(heads[s, 0], L) and np.isfinite(logp[s, 0])
        assert list(heads[s, 0]).index(0, 1) == 3             # root -> 3: the last root split that has weight
    assert np.array_equal(heads[0, 0], D.walk(dec, np.where(np.isinf(attach), -1e30, attach), L, np.ones((3, N, N))))


# ---- 3. sanitizers: the emulator as a stand-alone program -----------------------------------------------------------------------------------
def test_standalone_program_under_asan_ubsan(tmp_path):
    exe = _build(os.path.join(BUILD, "emu_dmv_sample_san"), ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                                                              "-fno-sanitize-recover=undefined", "-DEMU_DMV_SAMPLE_MAIN"])
    for N in (41, 66):
        dec, attach, targets, u, pmin, _ = steered_case(N, seed=200 + N, count=4)
        assert pmin >= FLOOR
        case = tmp_path / f"case{N}.bin"
        with open(case, "wb") as f:
            np.array([1, N, len(targets)], np.int32).tofile(f)
            np.array([N - 1], np.int64).tofile(f)
            dec.astype(np.float32).tofile(f)
            attach.astype(np.float32).tofile(f)
            np.ascontiguousarray(u[:, None], np.float32).tofile(f)
            np.ascontiguousarray(targets[:, None], np.int64).tofile(f)
        r = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "mismatches=0 canary_trips=0" in r.stdout, r.stdout + r.stderr


# ---- 4. C ABI -------------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_host_side_validation(lib):
    from vlgae_amd import _C
    for name in ("vlg_dmv1o_sample", "vlg_dmv1o_sample_blocks", "vlg_dmv1o_sample_workspace", "vlg_dmv1o_sample_lds_bytes"):
        assert hasattr(lib, name) and name in _C.SIGNATURES
    one = ctypes.c_void_p(16)   # any non-null pointer: validation must return before it is dereferenced (no GPU here)
    f = lib.vlg_dmv1o_sample
    assert f(one, one, one, 2, 8, 0, 4, one, 0, one, one, one, one, None, 0, None) == NULL        # both sources
    assert b"exactly one" in lib.vlg_last_error()
    assert f(one, one, one, 2, 8, 0, 4, None, 0, None, one, one, one, None, 0, None) == NULL      # neither
    assert f(None, one, one, 2, 8, 0, 4, one, 0, None, one, one, one, None, 0, None) == NULL      # no dec
    assert f(one, None, one, 2, 8, 0, 4, one, 0, None, one, one, one, None, 0, None) == NULL      # no attach
    assert f(one, one, None, 2, 8, 0, 4, one, 0, None, one, one, one, None, 0, None) == NULL      # no lengths
    assert f(one, one, one, 2, 8, 0, 4, one, 0, None, None, one, one, None, 0, None) == NULL      # no heads
    assert f(one, one, one, 2, 8, 0, 0, one, 0, None, one, one, one, None, 0, None) == SHAPE      # S < 1
    assert f(one, one, one, 2, 1, 0, 4, one, 0, None, one, one, one, None, 0, None) == SHAPE
    assert f(one, one, one, 2, 256, 0, 4, one, 0, None, one, one, one, None, 0, None) == SHAPE
    assert f(one, one, one, 2, 8, 7, 4, one, 0, None, one, one, one, None, 0, None) == DTYPE
    assert f(None, None, None, 0, 8, 0, 4, None, 0, None, None, None, None, None, 0, None) == 0   # empty batch: no-op
    assert lib.vlg_version() == _C.ABI_VERSION == 145


def _align16(x):
    return (x + 15) & ~15


def test_size_queries_and_launcher_agree_for_every_n(lib):
    """DmvLayout's forward-only plan restated: both float2 charts and the staged dec in LDS where they fit 160 KiB, else the charts in the
    workspace; the walk's eight 16-int stacks (512 B) behind them must fit wherever the charts do.  The workspace query is that stride
    times B Y, and the launcher refuses one byte less."""
    one = ctypes.c_void_p(16)
    ws_ns = []
    for N in range(2, 256):
        chart = _align16(N * ((N + 1) | 1) * 8)
        all_lds = 2 * chart + _align16(32 * N)
        in_lds = all_lds <= LDS_BUDGET
        lds = lib.vlg_dmv1o_sample_lds_bytes(N)
        assert lds == (all_lds if in_lds else _align16(32 * N)) + 8 * 16 * 4, N
        assert lds <= LDS_BUDGET, N
        stride = lib.vlg_dmv1o_sample_workspace(1, N, 1)
        assert stride == (0 if in_lds else 2 * chart), N
        for B, S in ((1, 1), (3, 64), (5, 4096), (300, 9)):
            Y = lib.vlg_dmv1o_sample_blocks(B, N, S)
            need = lib.vlg_dmv1o_sample_workspace(B, N, S)
            assert need == stride * B * Y, (N, B, S)
            if need:
                assert lib.vlg_dmv1o_sample(one, one, one, B, N, 0, S, one, 0, None, one, one, one, one, need - 1, None) == WORKSPACE
                assert lib.vlg_dmv1o_sample(one, one, one, B, N, 0, S, one, 0, None, one, one, one, None, need, None) == WORKSPACE
        if stride:
            ws_ns.append(N)
    assert ws_ns == list(range(ws_ns[0], 256)) and ws_ns[0] == first_workspace_n(lib) == 100   # N = 99 is the last all-LDS size: 672 bytes spare
    assert lib.vlg_dmv1o_sample_lds_bytes(99) == LDS_BUDGET - 672 + 512
    for bad in ((0, 41, 8), (4, 41, 0), (4, 1, 8), (4, 256, 8)):
        assert lib.vlg_dmv1o_sample_workspace(*bad) == 0 and lib.vlg_dmv1o_sample_blocks(*bad) == 1
    assert lib.vlg_dmv1o_sample_lds_bytes(1) == 0 and lib.vlg_dmv1o_sample_lds_bytes(256) == 0


def test_block_plan(lib):
    """Y fills the device once -- 256 CUs x the workgroups of this N that share a CU (as many as the LDS holds, four at most; one where the
    charts live in the workspace) -- and is capped by the samples: a wavefront owns whole samples, so ceil(S / 8) blocks have one each."""
    blocks = lib.vlg_dmv1o_sample_blocks
    for N, per_cu in ((41, 4), (66, 2), (99, 1), (100, 1), (200, 1), (255, 1)):
        assert per_cu == (1 if lib.vlg_dmv1o_sample_workspace(1, N, 1) else min(4, LDS_BUDGET // lib.vlg_dmv1o_sample_lds_bytes(N)))
        fill = 256 * per_cu
        for B in (1, 3, 4, 100, 255, 256, 1024, 4096):
            ys = [blocks(B, N, S) for S in (1, 2, 8, 9, 64, 65, 512, 4096, 1 << 20, 1 << 21)]
            assert all(y >= 1 for y in ys) and ys == sorted(ys), (N, B, ys)                    # monotone in S ...
            assert ys[-1] == ys[-2] == max(1, fill // B), (N, B, ys)                            # ... up to its cap
            assert ys[0] == 1 and ys[3] == min(2, max(1, fill // B))                            # never more blocks than ceil(S / 8)
        assert blocks(fill, N, 1 << 20) == 1 and blocks(4096, N, 1 << 20) == 1                  # B alone fills the device
        assert blocks(4, N, 4096) * 4 >= 256                                                    # a small batch with many samples still fills it


# ---- 5. Python surface ----------------------------------------------------------------------------------------------------------------------
def test_python_surface():
    import torch
    from vlgae_amd import train_step
    from vlgae_amd.torch_struct import DMV1o, functional as F
    assert callable(DMV1o.sample_heads) and callable(DMV1o.log_prob_heads)
    assert callable(F.dmv1o_sample) and callable(F.dmv1o_log_prob_heads) and callable(F.dmv1o_tree_score)
    assert callable(train_step.forced_tree_score)
    dist = DMV1o([torch.zeros(1, 3, 2, 2, 2), torch.zeros(1, 3, 3, 2)], torch.tensor([2]))
    with pytest.raises(NotImplementedError, match="sample_heads"):
        dist.sample()
    with pytest.raises(NotImplementedError, match="tree_entropy"):
        dist.sample()
    with pytest.raises(RuntimeError, match="no CPU path"):       # a missing kernel path is an error, never an eager fall-back
        dist.sample_heads(2, u=torch.zeros(2, 1, 3, 3, 3))
