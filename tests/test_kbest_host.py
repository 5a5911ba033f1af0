"""CPU: the k best dependency trees (DependencyCRF.kbest_heads / kbest_scores) without a GPU -- the float64 restatement against the
reference's fixtures and brute force, the bodies of vlgae_amd/csrc/vlg_dp_kbest.h under the host emulator (tests/emu/emu_kbest.cpp) at
every placement mode, the same emulator as a stand-alone program under AddressSanitizer + UBSan, the C ABI's host-side contract, and
the layout / placement table.

Potentials are the exactly-representable recipe of tests/kbest_restatement.py, so float32 scores are compared bit for bit.
"""
import ctypes
import functools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import kbest_restatement as R
from conftest import GOLDEN, ROOT, load

HERE = os.path.join(ROOT, "tests", "emu")
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "emu_kbest.cpp")
DEPS = [SRC, os.path.join(HERE, "emu_dp.cpp"), os.path.join(HERE, "emu_kbest_common.h")] + [
    os.path.join(ROOT, "vlgae_amd", "csrc", f) for f in ("vlg_dp_core.h", "vlg_dp_kbest.h")]
NS = (2, 3, 6, 12, 41, 66)
KS = (1, 2, 3, 4, 5, 8, 9, 16)
FIXTURES = (("kbest_B3_N6_K4_s0", 4), ("kbest_B4_N12_K8_s1", 8), ("kbest_B2_N41_K16_s2", 16))
LDS = 160 * 1024
# the largest N with everything in LDS / with only the back-pointer charts in the workspace, per code image KC
PLACEMENT = {1: (115, 142), 2: (81, 100), 4: (57, 70), 8: (40, 49), 16: (28, 34)}


def _build(out, extra):
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", *extra, SRC, "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def emu():
    return ctypes.CDLL(_build(os.path.join(BUILD, "libvlg_emu_kbest.so"), ["-fPIC", "-shared"]))


@pytest.fixture(scope="module")
def lib():
    from vlgae_amd.build import build_library
    build_library()
    from vlgae_amd import _C
    return _C.lib()


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def run_emu(emu, arc, lengths, K, mode, nt=16, order=0, bf16=False):
    B, N = arc.shape[:2]
    a = np.ascontiguousarray(arc, np.float32)
    if bf16:
        assert not (a.view(np.uint32) & 0xFFFF).any()
        a = (a.view(np.uint32) >> 16).astype(np.uint16)
    ln = np.ascontiguousarray(lengths, np.int64)
    heads = np.full((K, B, N), -1, np.int64)
    scores, count = np.full((K, B), np.nan, np.float32), np.full(B, -1, np.int32)
    assert emu.emu_deptree_kbest(_p(a), _p(ln), B, N, int(bf16), K, mode, _p(heads), _p(scores), _p(count), nt, order) == 0
    return heads, scores, count


def ragged(N):
    return [N - 1, 1, max(1, (N - 1) // 2)]


@functools.lru_cache(maxsize=None)
def case(N, bf16):
    "potentials, lengths and the unpruned float64 restatement at K' = 17, once per (N, dtype); drawn again until the tie cap holds"
    for draw in range(8):
        rng = np.random.default_rng(7000 + 2 * N + bf16 + 1000 * draw)
        arc = R.potentials(rng, (3, N, N), bf16=bf16)
        ref = [R.kbest_dp(arc[b], L, 17) for b, L in enumerate(ragged(N))]
        if R.tied_share(ref) <= 0.25:
            break
    return arc, ragged(N), ref


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K", FIXTURES)
def test_restatement_equals_the_reference_fixtures(name, K):
    g = load(os.path.join(GOLDEN, name + ".npz"))
    assert g["lengths"].min() == 1 and g["values"].shape[0] == K + 1
    n_cmp = 0
    for b, L in enumerate(g["lengths"]):
        v, h, c = R.kbest_dp(g["arc"][b], int(L), K + 1)
        ref = g["values"][:, b]
        ex = ref > -5e4   # the reference pads a missing rank with -1e5 per missing operand
        assert c == ex.sum() and np.array_equal(ex[:K], g["exists"][:, b])
        assert np.array_equal(v[ex], ref[ex]) and np.all(v[~ex] == R.NEGINF)
        vp, hp, cp = R.kbest_dp(g["arc"][b], int(L), K + 1, prune=True)   # the pruning bound loses nothing
        assert np.array_equal(v, vp) and np.array_equal(h, hp) and c == cp
        for k in range(min(c, K)):
            assert R.is_tree(h[k], int(L)) and R.tree_score(g["arc"][b], h[k], int(L)) == v[k]
            if (k == 0 or ref[k - 1] > ref[k]) and ref[k] > ref[k + 1]:
                assert np.array_equal(h[k], g["heads"][k, b]), (b, k)
                n_cmp += 1
    assert n_cmp >= 0.75 * g["exists"].sum()


@pytest.mark.parametrize("L", (1, 2, 3, 4, 5, 6))
def test_restatement_equals_brute_force(L):
    arc = R.potentials(np.random.default_rng(40 + L), (7, 7))
    s, h = R.brute_force(arc, L)
    assert len(s) == R.TREE_COUNTS[L]
    v, hh, c = R.kbest_dp(arc, L, 16)
    assert c == min(16, len(s)) and np.array_equal(v[:c], s[:c]) and np.all(v[c:] == R.NEGINF) and not hh[c:].any()
    assert len({tuple(x) for x in hh[:c]}) == c and all(R.is_tree(x, L) for x in hh[:c])
    for k in range(c):
        if (k == 0 or s[k - 1] > s[k]) and (k + 1 == len(s) or s[k] > s[k + 1]):
            assert np.array_equal(hh[k], h[k])


# ---- the kernel bodies under the emulator ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("N", NS)
def test_emulator_at_every_placement(emu, N, bf16):
    """Every K at every placement mode (the spilled modes forced at small N, with a NaN-filled second arena as the workspace).  Lane
    groups of up to 8 lanes at N <= 12 (nt = 16), up to 2 at N = 41, single lanes at N = 66 -- the emulator's cross-lane steps are
    barriers of host threads, and the wide groups cost seconds there."""
    arc, lengths, ref = case(N, bf16)
    nt = 16 if N <= 12 else 4 if N <= 41 else 2
    for K in KS:
        first = None
        for mode in (0, 1, 2):
            heads, scores, count = run_emu(emu, arc, lengths, K, mode, nt=nt, order=mode, bf16=bf16)
            R.check_kbest(arc, lengths, K, heads, scores, count, ref)
            if first is None:
                first = (heads, scores, count)
            assert all(np.array_equal(x, y) for x, y in zip(first, (heads, scores, count)))   # placement and lane order change nothing
        h16 = run_emu(emu, arc, lengths, 16, -1, nt=nt, bf16=bf16) if K == KS[0] else h16
        assert np.array_equal(first[0], h16[0][:K]) and np.array_equal(first[1].view(np.uint32), h16[1][:K].view(np.uint32))   # prefix
    assert emu.emu_canary_trips() == 0


def test_emulator_lane_groups_and_orders_agree(emu):
    arc, lengths, ref = case(12, False)
    base = run_emu(emu, arc, lengths, 9, 0, nt=2)
    for nt, order in ((4, 1), (8, 2), (16, 3), (32, 5)):
        got = run_emu(emu, arc, lengths, 9, 0, nt=nt, order=order)
        assert all(np.array_equal(x, y) for x, y in zip(base, got)), (nt, order)


def test_emulator_ties_forbidden_arcs_and_bad_lengths(emu):
    N, K = 9, 16
    heads, scores, count = run_emu(emu, np.zeros((1, N, N)), [N - 1], K, 1)
    assert count[0] == K and np.all(scores == 0.0) and len({tuple(h) for h in heads[:, 0]}) == K
    assert all(R.is_tree(h, N - 1) for h in heads[:, 0])
    base = R.potentials(np.random.default_rng(2), (N, N))
    chain = np.full((N, N), -np.inf)
    for c in range(1, N):
        chain[c - 1, c] = base[c - 1, c]
    orphan = base.copy()
    orphan[:, 4] = -1e20
    heads, scores, count = run_emu(emu, np.stack([chain, orphan, base, base]), [N - 1, N - 1, 0, N], 8, 2)
    assert list(count) == [1, 0, 0, 0]
    assert np.array_equal(heads[0, 0], np.concatenate([[0], np.arange(N - 1)])) and not heads[1:, 0].any() and not heads[:, 1:].any()
    assert np.all(scores[1:, 0] == np.float32(R.NEGINF)) and np.all(scores[:, 1] == np.float32(R.NEGINF)) and np.all(np.isnan(scores[:, 2:]))
    assert emu.emu_canary_trips() == 0


def test_standalone_program_under_asan_ubsan(emu, tmp_path):
    exe = _build(os.path.join(BUILD, "emu_kbest_san"), ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                                                         "-fno-sanitize-recover=undefined", "-DEMU_KBEST_MAIN"])
    for N, K, mode in ((6, 4, 0), (12, 16, 2), (41, 8, 1)):
        arc, lengths, _ = case(N, False)
        heads, scores, _ = run_emu(emu, arc, lengths, K, mode, nt=8, order=2)
        path = tmp_path / f"case{N}.bin"
        with open(path, "wb") as f:
            f.write(struct.pack("4i", 3, N, K, mode))
            f.write(np.asarray(lengths, np.int64).tobytes())
            f.write(np.ascontiguousarray(arc, np.float32).tobytes())
            f.write(scores.tobytes())
            f.write(heads.tobytes())
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "mismatches=0 canary_trips=0" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_host_side_validation(lib):
    from vlgae_amd import _C
    assert hasattr(lib, "vlg_deptree_kbest") and hasattr(lib, "vlg_deptree_kbest_workspace")
    assert "vlg_deptree_kbest" in _C.SIGNATURES and "vlg_deptree_kbest_workspace" in _C.SIGNATURES
    one = ctypes.c_void_p(16)   # any non-null pointer: validation must return before it is dereferenced (no GPU here)
    f = lib.vlg_deptree_kbest
    SHAPE, DTYPE, WORKSPACE, NULL = 0x1001, 0x1002, 0x1004, 0x1005
    for N in (1, 0, 256, 300):
        assert f(one, one, 2, N, 0, 4, one, one, one, None, 0, None) == SHAPE
    for K in (0, -1, 17):
        assert f(one, one, 2, 8, 0, K, one, one, one, None, 0, None) == SHAPE
    assert f(one, one, 2, 8, 7, 4, one, one, one, None, 0, None) == DTYPE
    assert f(one, one, 2, 8, 2, 4, one, one, one, None, 0, None) == DTYPE
    assert f(None, one, 2, 8, 0, 4, one, one, one, None, 0, None) == NULL
    assert f(one, one, 2, 8, 0, 4, None, one, one, None, 0, None) == NULL
    assert f(one, one, 2, 8, 0, 4, one, None, one, None, 0, None) == NULL
    assert f(None, None, 0, 8, 0, 4, None, None, None, None, 0, None) == 0   # empty batch: no-op
    assert f(one, one, 2, 255, 1, 16, one, one, one, None, 0, None) == WORKSPACE
    assert lib.vlg_version() == _C.ABI_VERSION == 145


def test_workspace_query_and_launcher_agree(lib):
    one = ctypes.c_void_p(16)
    q, f = lib.vlg_deptree_kbest_workspace, lib.vlg_deptree_kbest
    assert q(1, 2, 1) == 0 and q(1, 255, 16) > 0
    assert q(0, 200, 8) == 0 and q(2, 1, 8) == 0 and q(2, 256, 8) == 0 and q(2, 100, 0) == 0 and q(2, 100, 17) == 0
    refused = 0
    for K in (1, 8, 16):
        for N in range(2, 256):
            need = q(2, N, K)
            assert need == 2 * q(1, N, K) and q(5, N, K) == 5 * q(1, N, K)   # linear in B
            if need:
                assert f(one, one, 2, N, 0, K, one, one, one, one, need - 1, None) == 0x1004
                assert str(need).encode() in lib.vlg_last_error()
                refused += 1
    assert refused == sum(255 - PLACEMENT[KC][0] for KC in (1, 8, 16))


# ---- layout --------------------------------------------------------------------------------------------------------------------------------
def layout(N, KC, mode):
    "KbestLayout restated: (lds_bytes, ws_bytes)"
    cells = N * ((N + 1) | 1)
    size = {True: 0, False: 0}
    for nbytes, in_lds in ((cells * KC * 4, mode < 2), (cells * KC * 4, mode < 2), (cells * KC * 2, mode < 1), (cells * KC * 2, mode < 1),
                           (8 * 32 * 4, True)):
        size[in_lds] = (size[in_lds] + nbytes + 15) & ~15
    return size[True], size[False]


def test_layout_and_placement_table(emu, lib):
    emu.emu_kbest_plan.restype = None
    out = (ctypes.c_longlong * 4)()
    for K in range(1, 17):
        KC = next(c for c in (1, 2, 4, 8, 16) if K <= c)
        for N in range(2, 256):
            mode = next((m for m in (0, 1) if layout(N, KC, m)[0] <= LDS), 2)
            lds, ws = layout(N, KC, mode)
            emu.emu_kbest_plan(N, K, out)
            assert tuple(out) == (KC, mode, lds, ws), (N, K, tuple(out))
            assert lds <= LDS and lib.vlg_deptree_kbest_workspace(3, N, K) == 3 * ws
            a, b = PLACEMENT[KC]
            assert mode == (0 if N <= a else 1 if N <= b else 2), (N, K, mode)


def test_python_surface():
    import torch
    from vlgae_amd.torch_struct import DependencyCRF
    from vlgae_amd.torch_struct import functional as F
    assert callable(DependencyCRF.kbest_heads) and callable(DependencyCRF.kbest_scores) and callable(F.deptree_kbest)
    dist = DependencyCRF(torch.zeros(1, 3, 3))
    for name in ("kmax", "topk"):
        with pytest.raises(NotImplementedError, match="kbest_heads") as e:
            getattr(dist, name)(2)
        assert re.search("sample_heads", str(e.value)) and re.search("tree_entropy", str(e.value))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dist.kbest_heads(2)
