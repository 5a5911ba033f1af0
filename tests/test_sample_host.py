"""CPU: tree sampling (DependencyCRF.sample_heads) without a GPU -- the C ABI's host-side contract, the walk of
vlgae_amd/csrc/vlg_dp_sample.h under the host emulator (tests/emu/emu_sample.cpp), and the same emulator as a stand-alone program under
AddressSanitizer + UBSan.

Steering (tests/sample_restatement.py): the float64 restatement of the sampling rule writes, for a chosen tree, the midpoint of the wanted
split's interval into the uniform table; the float32 walk must then return exactly that tree.  Every steered split keeps a conditional
probability of at least 0.01 (asserted): half of that, the distance from the midpoint to the interval's ends, is three orders of
magnitude above what float32 charts of N <= 66 can be off by.  To leave that room for "the root's child at EVERY position" -- with random
potentials the middle positions have probability ~1/500 at N = 66, the count of trees alone favours the ends -- the root's arc scores
are re-weighted so that the root's child is uniform over the positions (1 / len >= 1 / 65); the chains are steered as they are, the
other trees grow through splits of probability >= 0.02.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sample_restatement as R
from conftest import ROOT

HERE = os.path.join(ROOT, "tests", "emu")
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "emu_sample.cpp")
DEPS = [SRC, os.path.join(HERE, "emu_dp.cpp"), os.path.join(HERE, "emu_sample_common.h")] + [
    os.path.join(ROOT, "vlgae_amd", "csrc", f) for f in ("vlg_dp_core.h", "vlg_dp_sample.h", "vlg_sample_common.h")]
NS = (2, 3, 6, 41, 66)


def _build(out, extra):
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", *extra, SRC, "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def emu():
    return ctypes.CDLL(_build(os.path.join(BUILD, "libvlg_emu_sample.so"), ["-fPIC", "-shared"]))


@pytest.fixture(scope="module")
def lib():
    from vlgae_amd.build import build_library
    build_library()
    from vlgae_amd import _C
    return _C.lib()


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def uniform_root(arc, length):
    "arc with the root's row shifted so that every position is the root's child with probability 1 / length"
    I, C = R.inside64(arc, length)
    t, r = R.terms(I, C, 2, 0, length)
    out = np.array(arc, np.float32)
    out[0, r] -= (t - t.max()).astype(np.float32)
    return out


def steered_case(N, seed, n_random=20, sweep=True):
    """(arc [N,N], targets [S,N], u [S,3,N,N], pmin) for one sentence of full length: both chains, the root's child at every position,
    n_random random trees."""
    rng = np.random.default_rng(seed)
    L = N - 1
    arc = uniform_root(0.5 * rng.standard_normal((N, N)), L)
    rows = [R.steer(arc, L, R.left_chain(L)), R.steer(arc, L, R.right_chain(L))]
    if sweep:
        rows += [R.steer(arc, L, pick=R.floor_pick(rng, 0.02, root_child=p, length=L)) for p in range(1, L + 1)]
    rows += [R.steer(arc, L, pick=R.floor_pick(rng, 0.02)) for _ in range(n_random)]
    for k, (_, _, h) in enumerate(rows[2:2 + L] if sweep else []):
        assert h[k + 1] == 0 and R.is_tree(h, L)
    return arc, np.stack([R.pad_heads(h, N) for _, _, h in rows]), np.stack([u for u, _, _ in rows]), min(p for _, p, _ in rows)


def run_emu(emu, arc, lengths, u, order=0):
    B, N = arc.shape[:2]
    S = u.shape[0]
    arc, u = np.ascontiguousarray(arc, np.float32), np.ascontiguousarray(u, np.float32)
    ln = np.ascontiguousarray(lengths, np.int64)
    heads = np.full((S, B, N), -1, np.int64)
    logp, logZ = np.full((S, B), np.nan, np.float32), np.full(B, np.nan, np.float32)
    assert emu.emu_deptree_sample(_p(arc), _p(ln), B, N, 0, S, _p(u), _p(heads), _p(logp), _p(logZ), 16, order) == 0
    return heads, logp, logZ


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_host_side_validation(lib):
    from vlgae_amd import _C
    assert hasattr(lib, "vlg_deptree_sample") and hasattr(lib, "vlg_deptree_sample_blocks")
    assert "vlg_deptree_sample" in _C.SIGNATURES and "vlg_deptree_sample_blocks" in _C.SIGNATURES
    one = ctypes.c_void_p(16)   # any non-null pointer: validation must return before it is dereferenced (no GPU here)
    f = lib.vlg_deptree_sample
    SHAPE, DTYPE, WORKSPACE, NULL = 0x1001, 0x1002, 0x1004, 0x1005
    assert f(one, one, 2, 8, 0, 4, one, 0, one, one, one, one, None, 0, None) == NULL       # both sources
    assert b"exactly one" in lib.vlg_last_error()
    assert f(one, one, 2, 8, 0, 4, None, 0, None, one, one, one, None, 0, None) == NULL     # neither
    assert f(None, one, 2, 8, 0, 4, one, 0, None, one, one, one, None, 0, None) == NULL     # no potentials
    assert f(one, one, 2, 8, 0, 4, one, 0, None, None, one, one, None, 0, None) == NULL     # no heads
    assert f(one, one, 2, 8, 0, 0, one, 0, None, one, one, one, None, 0, None) == SHAPE     # S < 1
    assert f(one, one, 2, 1, 0, 4, one, 0, None, one, one, one, None, 0, None) == SHAPE
    assert f(one, one, 2, 300, 0, 4, one, 0, None, one, one, one, None, 0, None) == SHAPE
    assert f(one, one, 2, 8, 7, 4, one, 0, None, one, one, one, None, 0, None) == DTYPE
    assert f(None, None, 0, 8, 0, 4, None, 0, None, None, None, None, None, 0, None) == 0   # empty batch: no-op
    # long sentences keep their charts in the workspace of the inside pass, one slice per block of the (B, Y) grid
    Y = lib.vlg_deptree_sample_blocks(2, 200, 64)
    need = lib.vlg_workspace_bytes(_C.OP_DEPTREE_INSIDE, 2 * Y, 200, 0)
    assert Y > 1 and need > 0
    assert f(one, one, 2, 200, 0, 64, one, 0, None, one, one, one, one, need - 1, None) == WORKSPACE
    assert f(one, one, 2, 200, 0, 64, one, 0, None, one, one, one, None, 0, None) == WORKSPACE
    assert lib.vlg_version() == _C.ABI_VERSION


def test_block_plan(lib):
    """Y fills the device once -- 256 CUs x the workgroups of this N that share a CU (as many as the LDS holds, four at most; one where the
    charts live in the workspace) -- and is capped by the samples: a wavefront owns whole samples, so ceil(S / 8) blocks have one each."""
    blocks = lib.vlg_deptree_sample_blocks
    for N, per_cu in ((41, 4), (100, 2), (142, 1), (200, 1), (255, 1)):
        fill = 256 * per_cu
        for B in (1, 3, 4, 100, 255, 256, 1024, 4096):
            ys = [blocks(B, N, S) for S in (1, 2, 8, 9, 64, 65, 512, 4096, 1 << 20, 1 << 21)]
            assert all(y >= 1 for y in ys) and ys == sorted(ys), (N, B, ys)                    # monotone in S ...
            assert ys[-1] == ys[-2] == max(1, fill // B), (N, B, ys)                            # ... up to its cap
            assert ys[0] == 1 and ys[3] == min(2, max(1, fill // B))                            # never more blocks than ceil(S / 8)
        assert blocks(fill, N, 1 << 20) == 1 and blocks(4096, N, 1 << 20) == 1                  # B alone fills the device
        assert blocks(4, N, 4096) * 4 >= 256                                                    # a small batch with many samples still fills it
    assert blocks(0, 41, 8) == 1 and blocks(4, 41, 0) == 1 and blocks(4, 300, 8) == 1


def test_python_surface():
    from vlgae_amd.torch_struct import DependencyCRF
    import torch
    assert callable(DependencyCRF.sample_heads)
    heads = torch.tensor([[[0, 2, 0, 2, 0]], [[0, 0, 1, 2, 0]]])                # [S=2, B=1, N=5], length 3
    parts = DependencyCRF.heads_to_parts(heads, lengths=torch.tensor([3]))
    assert parts.shape == (2, 1, 5, 5) and parts.dtype == torch.float32
    want = torch.zeros(2, 1, 5, 5)
    for s, (h, c) in [(0, (2, 1)), (0, (0, 2)), (0, (2, 3)), (1, (0, 1)), (1, (1, 2)), (1, (2, 3))]:
        want[s, 0, h, c] = 1
    assert torch.equal(parts, want)
    assert DependencyCRF.heads_to_parts(heads[0]).sum() == 4                    # lengths None: every position 1 ... N-1 is a word
    with pytest.raises(NotImplementedError, match="sample_heads"):
        DependencyCRF(torch.zeros(1, 3, 3)).sample()


# ---- the walk under the emulator -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
def test_emulator_returns_steered_trees(emu, N):
    arc, targets, u, pmin = steered_case(N, seed=100 + N)
    print(f"N={N}: {len(targets)} steered trees, smallest conditional probability {pmin:.4f}")
    assert pmin >= 0.01
    L = N - 1
    before = emu.emu_canary_trips()
    heads, logp, logZ = run_emu(emu, arc[None], [L], u[:, None], order=2 if N <= 6 else 0)
    assert np.array_equal(heads[:, 0], targets)
    assert emu.emu_canary_trips() == before == 0
    I, C = R.inside64(arc, L)
    assert abs(logZ[0] - C[0, L]) <= 2e-5 * max(1.0, abs(C[0, L]))
    for s in (0, 1, len(targets) - 1):
        score, mag = R.tree_score(arc, targets[s], L)
        assert abs(logp[s, 0] - (score - C[0, L])) <= 2e-5 * max(1.0, abs(C[0, L])) + L * 2.0 ** -23 * mag


def test_emulator_short_sentence_in_a_wide_batch_and_bad_length(emu):
    "ragged lengths: charts of a short sentence inside a wider tensor; an invalid length gives heads 0, logp NaN, logZ NaN"
    N = 9
    rng = np.random.default_rng(5)
    arc = (0.5 * rng.standard_normal((3, N, N))).astype(np.float32)
    lengths = [5, 0, 1]
    u = np.full((2, 3, 3, N, N), np.nan, np.float32)
    want = np.zeros((2, 3, N), np.int64)
    for s in range(2):
        u[s, 0], _, h = R.steer(arc[0], 5, pick=R.floor_pick(rng, 0.02))
        want[s, 0] = R.pad_heads(h, N)
        u[s, 2], _, h = R.steer(arc[2], 1, R.right_chain(1))
        want[s, 2] = R.pad_heads(h, N)
    heads, logp, logZ = run_emu(emu, arc, lengths, u)
    assert np.array_equal(heads, want) and emu.emu_canary_trips() == 0
    assert np.isnan(logp[:, 1]).all() and np.isnan(logZ[1]) and np.isfinite(logp[:, [0, 2]]).all()


def test_emulator_charts_in_the_workspace(emu):
    "the placement of long sentences: both charts in the second arena, only the walk's stack in the first"
    arc, targets, u, pmin = steered_case(41, seed=7, n_random=3, sweep=False)
    assert pmin >= 0.01
    emu.emu_set_dep_mode(1)
    try:
        heads, _, _ = run_emu(emu, arc[None], [40], u[:, None])
    finally:
        emu.emu_set_dep_mode(0)
    assert np.array_equal(heads[:, 0], targets) and emu.emu_canary_trips() == 0


def test_nan_uniform_takes_the_last_split_of_positive_weight(emu):
    "a NaN uniform (and u within an ulp of 1) falls through to the largest r with w_r > 0 -- never to a forbidden split"
    N, L = 6, 5
    rng = np.random.default_rng(11)
    arc = (0.5 * rng.standard_normal((N, N))).astype(np.float32)
    arc[0, 4:] = -np.inf                                   # the root's child cannot be word 4 or 5
    u = np.full((2, 1, 3, N, N), np.nan, np.float32)
    u[1] = np.nextafter(np.float32(1), np.float32(0))
    heads, logp, _ = run_emu(emu, arc[None], [L], u)
    for s in range(2):
        assert R.is_tree(heads[s, 0], L) and np.isfinite(logp[s, 0])
        assert list(heads[s, 0]).index(0, 1) == 3           # root -> 3: the last root split that has weight
    assert np.array_equal(heads[0, 0], R.walk(np.where(np.isinf(arc), -1e30, arc), L, np.ones((3, N, N))))


# ---- sanitizers: the emulator as a stand-alone program ----------------------------------------------------------------------------------
def test_standalone_program_under_asan_ubsan(tmp_path):
    exe = _build(os.path.join(BUILD, "emu_sample_san"), ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                                                          "-fno-sanitize-recover=undefined", "-DEMU_SAMPLE_MAIN"])
    for N in (41, 66):
        arc, targets, u, pmin = steered_case(N, seed=100 + N, n_random=1, sweep=False)   # both chains and a random tree
        assert pmin >= 0.01 and len(targets) == 3
        case = tmp_path / f"case{N}.bin"
        with open(case, "wb") as f:
            np.array([1, N, 3], np.int32).tofile(f)
            np.array([N - 1], np.int64).tofile(f)
            arc.astype(np.float32).tofile(f)
            np.ascontiguousarray(u[:, None], np.float32).tofile(f)
            np.ascontiguousarray(targets[:, None], np.int64).tofile(f)
        r = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "mismatches=0 canary_trips=0" in r.stdout, r.stdout + r.stderr
