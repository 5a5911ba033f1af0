"""CPU: the k best trees of the valence DMV (DMV1o.kbest_heads / kbest_scores) and their adjoint (vlg_dmv1o_tree_counts) without a GPU --
the float64 restatement against the reference-made fixtures and brute force, the bodies of vlgae_amd/csrc/vlg_dmv_kbest.h under the host
emulator (tests/emu/emu_dmv_kbest.cpp) at every placement mode, the same emulator as a stand-alone program under AddressSanitizer +
UBSan, the C ABI's host-side contract, and the layout / placement table.

Potentials are the exactly-representable recipe of tests/dmv_kbest_restatement.py, so float32 scores are compared bit for bit.
"""
import ctypes
import functools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import dmv_kbest_restatement as R
from conftest import GOLDEN, ROOT, load
from dmv_sample_restatement import tree_score

HERE = os.path.join(ROOT, "tests", "emu")
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "emu_dmv_kbest.cpp")
DEPS = [SRC, os.path.join(HERE, "emu_dp.cpp"), os.path.join(HERE, "emu_kbest_common.h")] + [
    os.path.join(ROOT, "vlgae_amd", "csrc", f) for f in ("vlg_dp_core.h", "vlg_dp_kbest.h", "vlg_dmv_kbest.h")]
NS = (2, 3, 6, 12, 41, 66)
KS = (1, 2, 3, 4, 5, 8, 9, 16)
LDS = 160 * 1024
# the largest N with everything in LDS / with only the back-pointer charts in the workspace, per code image KC
PLACEMENT = {1: (78, 89), 2: (60, 70), 4: (44, 52), 8: (32, 38), 16: (22, 28)}


def _build(out, extra):
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", *extra, SRC, "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def emu():
    return ctypes.CDLL(_build(os.path.join(BUILD, "libvlg_emu_dmv_kbest.so"), ["-fPIC", "-shared"]))


@pytest.fixture(scope="module")
def lib():
    from vlgae_amd.build import build_library
    build_library()
    from vlgae_amd import _C
    return _C.lib()


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _bits(a, bf16):
    a = np.ascontiguousarray(a, np.float32)
    if bf16:
        assert not (a.view(np.uint32) & 0xFFFF).any()
        a = (a.view(np.uint32) >> 16).astype(np.uint16)
    return a


def run_emu(emu, dec, attach, lengths, K, mode, nt=16, order=0, bf16=False):
    B, N = attach.shape[:2]
    d, a = _bits(dec, bf16), _bits(attach, bf16)
    ln = np.ascontiguousarray(lengths, np.int64)
    heads = np.full((K, B, N), -1, np.int64)
    scores, count = np.full((K, B), np.nan, np.float32), np.full(B, -1, np.int32)
    assert emu.emu_dmv1o_kbest(_p(d), _p(a), _p(ln), B, N, int(bf16), K, mode, _p(heads), _p(scores), _p(count), nt, order) == 0
    return heads, scores, count


def emu_counts(emu, heads, lengths, count, weight, N):
    T, B = heads.shape[:2]
    h, ln = np.ascontiguousarray(heads, np.int64), np.ascontiguousarray(lengths, np.int64)
    c = None if count is None else np.ascontiguousarray(count, np.int32)
    w = None if weight is None else np.ascontiguousarray(weight, np.float32)
    cd, ca = np.full((B, N, 2, 2, 2), np.nan, np.float32), np.full((B, N, N, 2), np.nan, np.float32)
    assert emu.emu_dmv1o_tree_counts(_p(h), _p(ln), _p(c), _p(w), T, B, N, _p(cd), _p(ca)) == 0
    return cd, ca


def ragged(N):
    return [N - 1, 1, max(1, (N - 1) // 2)]


@functools.lru_cache(maxsize=None)
def case(N, bf16):
    "potentials, lengths and the unpruned float64 restatement at K' = 17, once per (N, dtype); drawn again until the tie cap holds"
    for draw in range(8):
        rng = np.random.default_rng(9000 + 2 * N + bf16 + 1000 * draw)
        dec, attach = R.potentials(rng, 3, N, bf16=bf16)
        ref = [R.dmv_kbest_dp(dec[b], attach[b], L, 17) for b, L in enumerate(ragged(N))]
        if R.tied_share(ref) <= 0.25:
            break
    return dec, attach, ragged(N), ref


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("dmvkbest_B3_N6_s0", "dmvkbest_B4_N5_s1"))
def test_restatement_equals_the_reference_fixtures(name):
    "every tree of every sentence, scored by the reference's own DMV1o.max on forced potentials: values and, where separated, heads"
    g = load(os.path.join(GOLDEN, name + ".npz"))
    assert g["lengths"].min() == 1 and g["lengths"].max() <= 5
    n_cmp = 0
    for b, L in enumerate(g["lengths"]):
        nt = int(g["ntrees"][b])
        assert nt == R.TREE_COUNTS[int(L)]
        ref = g["values"][:nt, b]
        K = min(17, nt + 1)
        v, h, c = R.dmv_kbest_dp(g["dec"][b], g["attach"][b], int(L), K)
        n = min(K, nt)
        assert c == n and np.array_equal(v[:n], ref[:n]) and np.all(v[n:] == R.NEGINF)
        vp, hp, cp = R.dmv_kbest_dp(g["dec"][b], g["attach"][b], int(L), K, prune=True)   # the pruning bound loses nothing
        assert np.array_equal(v, vp) and np.array_equal(h, hp) and c == cp
        for k in range(n):
            assert R.is_tree(h[k], int(L)) and R.score(g["dec"][b], g["attach"][b], h[k], int(L))[0] == v[k]
            if (k == 0 or ref[k - 1] > ref[k]) and (k + 1 == nt or ref[k] > ref[k + 1]):
                assert np.array_equal(h[k], g["heads"][k, b]), (b, k)
                n_cmp += 1
    assert n_cmp >= 0.75 * sum(min(17, int(t)) for t in g["ntrees"])


def test_restatement_rank_zero_is_the_reference_argmax():
    g = load(os.path.join(GOLDEN, "dmvkbest_B2_N41_s2.npz"))
    for b, L in enumerate(g["lengths"]):
        v, h, c = R.dmv_kbest_dp(g["dec"][b], g["attach"][b], int(L), 2, prune=True)
        assert c == 2 and v[0] == g["values"][0, b] and v[0] > v[1] and np.array_equal(h[0], g["heads"][0, b])


@pytest.mark.parametrize("L", (1, 2, 3, 4, 5, 6))
def test_restatement_equals_brute_force(L):
    dec, attach = R.potentials(np.random.default_rng(40 + L), 1, 7)
    s, h = R.brute_force(dec[0], attach[0], L)
    assert len(s) == R.TREE_COUNTS[L] and len({tuple(x) for x in h}) == len(s)
    v, hh, c = R.dmv_kbest_dp(dec[0], attach[0], L, 16)
    assert c == min(16, len(s)) and (c < 16) == (len(s) < 16)
    assert np.array_equal(v[:c], s[:c]) and np.all(v[c:] == R.NEGINF) and not hh[c:].any()
    assert len({tuple(x) for x in hh[:c]}) == c and all(R.is_tree(x, L) for x in hh[:c])
    for k in range(c):
        if (k == 0 or s[k - 1] > s[k]) and (k + 1 == len(s) or s[k] > s[k + 1]):
            assert np.array_equal(hh[k], h[k])


# ---- the kernel bodies under the emulator ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("N", NS)
def test_emulator_at_every_placement(emu, N, bf16):
    """Every K at every placement mode (the spilled modes forced at small N, with a NaN-filled second arena as the workspace), bit for
    bit with the restatement.  Lane groups of up to 8 lanes at N <= 12 (nt = 16), up to 2 at N = 41, single lanes at N = 66."""
    dec, attach, lengths, ref = case(N, bf16)
    nt = 16 if N <= 12 else 4 if N <= 41 else 2
    for K in KS:
        first = None
        for mode in (0, 1, 2):
            heads, scores, count = run_emu(emu, dec, attach, lengths, K, mode, nt=nt, order=mode, bf16=bf16)
            R.check_dmv_kbest(dec, attach, lengths, K, heads, scores, count, ref)
            if first is None:
                first = (heads, scores, count)
            assert all(np.array_equal(x, y) for x, y in zip(first, (heads, scores, count)))   # placement and lane order change nothing
        h16 = run_emu(emu, dec, attach, lengths, 16, -1, nt=nt, bf16=bf16) if K == KS[0] else h16
        assert np.array_equal(first[0], h16[0][:K]) and np.array_equal(first[1].view(np.uint32), h16[1][:K].view(np.uint32))   # prefix
    assert emu.emu_canary_trips() == 0


@pytest.mark.parametrize("KC", (1, 2, 4, 8, 16))
def test_emulator_both_sides_of_each_boundary(emu, KC):
    "the plan's own placement (mode -1) at the last N of one mode and the first of the next, for the image KC"
    a, b = PLACEMENT[KC]
    rng = np.random.default_rng(300 + KC)
    for N in (a, a + 1, b, b + 1):
        dec, attach = R.potentials(rng, 2, N)
        lengths = [N - 1, 2]
        ref = [R.dmv_kbest_dp(dec[i], attach[i], L, KC + 1, prune=True) for i, L in enumerate(lengths)]
        heads, scores, count = run_emu(emu, dec, attach, lengths, KC, -1, nt=2)
        R.check_dmv_kbest(dec, attach, lengths, KC, heads, scores, count, ref, tie_cap=None)
    assert emu.emu_canary_trips() == 0


def test_emulator_lane_groups_and_orders_agree(emu):
    dec, attach, lengths, ref = case(12, False)
    base = run_emu(emu, dec, attach, lengths, 9, 0, nt=2)
    for nt, order in ((4, 1), (8, 2), (16, 3), (32, 5)):
        got = run_emu(emu, dec, attach, lengths, 9, 0, nt=nt, order=order)
        assert all(np.array_equal(x, y) for x, y in zip(base, got)), (nt, order)


def test_emulator_ties_forbidden_potentials_and_bad_lengths(emu):
    N, K = 9, 16
    heads, scores, count = run_emu(emu, np.zeros((1, N, 2, 2, 2)), np.zeros((1, N, N, 2)), [N - 1], K, 1)
    assert count[0] == K and np.all(scores == 0.0) and len({tuple(h) for h in heads[:, 0]}) == K
    assert all(R.is_tree(h, N - 1) for h in heads[:, 0])
    dec, attach = R.potentials(np.random.default_rng(2), 1, N)
    dec, base = dec[0], attach[0]
    chain = np.full((N, N, 2), -np.inf)                # only the right chain 0 -> 1 -> 2 -> ... is allowed
    for c in range(1, N):
        chain[c - 1, c] = base[c - 1, c]
    orphan = base.copy()                               # word 4 has no head at all
    orphan[:, 4] = -1e20
    nostop = dec.copy()                                # word 3 may never stop to its right without a child, nor with one
    nostop[3, 1, :, 1] = -1e12
    heads, scores, count = run_emu(emu, np.stack([dec, dec, nostop, dec, dec]), np.stack([chain, orphan, base, base, base]),
                                   [N - 1, N - 1, N - 1, 0, N], 8, 2)
    assert list(count) == [1, 0, 0, 0, 0]
    want = np.concatenate([[0], np.arange(N - 1)])
    assert np.array_equal(heads[0, 0], want) and not heads[1:, 0].any() and not heads[:, 1:].any()
    assert scores[0, 0] == np.float32(R.score(dec, base, want, N - 1)[0])
    assert np.all(scores[1:, 0] == np.float32(R.NEGINF)) and np.all(scores[:, 1:3] == np.float32(R.NEGINF)) and np.all(np.isnan(scores[:, 3:]))
    assert emu.emu_canary_trips() == 0


def test_standalone_program_under_asan_ubsan(emu, tmp_path):
    exe = _build(os.path.join(BUILD, "emu_dmv_kbest_san"), ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                                                             "-fno-sanitize-recover=undefined", "-DEMU_DMV_KBEST_MAIN"])
    for N, K, mode in ((6, 4, 0), (12, 16, 2), (41, 8, 1)):
        dec, attach, lengths, _ = case(N, False)
        heads, scores, count = run_emu(emu, dec, attach, lengths, K, mode, nt=8, order=2)
        cd, ca = emu_counts(emu, heads, lengths, count, None, N)
        path = tmp_path / f"case{N}.bin"
        with open(path, "wb") as f:
            f.write(struct.pack("4i", 3, N, K, mode))
            f.write(np.asarray(lengths, np.int64).tobytes())
            f.write(np.ascontiguousarray(dec, np.float32).tobytes())
            f.write(np.ascontiguousarray(attach, np.float32).tobytes())
            f.write(scores.tobytes())
            f.write(heads.tobytes())
            f.write(cd.tobytes())
            f.write(ca.tobytes())
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "mismatches=0 canary_trips=0" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ---- tree counts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", (1, 2, 3, 4, 5))
def test_tree_counts_of_every_tree(emu, L):
    "the restated counts and the kernel's lane body against tree_score's counts, for every tree of L words"
    N = 7
    trees = R.all_trees(L)
    heads = np.zeros((len(trees), 1, N), np.int64)
    for t, h in enumerate(trees):
        heads[t, 0, :L + 1] = h
    dec, attach = R.potentials(np.random.default_rng(L), 1, N)
    for t in range(len(trees)):
        _, _, cd, ca = tree_score(dec[0], attach[0], heads[t, 0], L)
        for got in (R.tree_counts(heads[t:t + 1], [L], None, None, N), emu_counts(emu, heads[t:t + 1], [L], None, None, N)):
            assert np.array_equal(got[0][0], cd) and np.array_equal(got[1][0], ca), (t, heads[t, 0])
        assert cd.sum() + ca.sum() == 4 * L + 1
    w = (2.0 ** np.random.default_rng(L).integers(-3, 4, (len(trees), 1))).astype(np.float32)
    want = R.tree_counts(heads, [L], None, w, N)
    got = emu_counts(emu, heads, [L], None, w, N)
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])
    total = sum(float(x) for x in w[:, 0])
    assert got[0].sum() + got[1].sum() == (4 * L + 1) * total   # power-of-two weights: every sum is exact


def test_tree_counts_skip_absent_ranks_and_bad_entries(emu):
    N, L = 8, 5
    trees = R.all_trees(L)[:4]
    heads = np.zeros((4, 3, N), np.int64)
    for t, h in enumerate(trees):
        heads[t, :, :L + 1] = h
    heads[1, 1, 2] = 2          # names itself
    heads[2, 1, 3] = L + 1      # outside the sentence
    heads[3, 1, 4] = -5
    heads[:, :, L + 1:] = 99    # padding is never read as a word
    count = np.array([2, 4, 4], np.int32)
    lengths = [L, L, N]         # the last one is no sentence
    cd, ca = emu_counts(emu, heads, lengths, count, None, N)
    want = R.tree_counts(heads, lengths, count, None, N)
    assert np.array_equal(cd, want[0]) and np.array_equal(ca, want[1])
    both = R.tree_counts(heads[:2, :1], [L], None, None, N)
    assert np.array_equal(cd[0], both[0][0]) and np.array_equal(ca[0], both[1][0])   # ranks t >= count contribute nothing
    assert ca[1].sum() == 4 * L - 3 and not cd[2].any() and not ca[2].any()
    assert emu.emu_canary_trips() == 0


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_host_side_validation(lib):
    from vlgae_amd import _C
    for name in ("vlg_dmv1o_kbest", "vlg_dmv1o_kbest_workspace", "vlg_dmv1o_tree_counts"):
        assert hasattr(lib, name) and name in _C.SIGNATURES
    one = ctypes.c_void_p(16)   # any non-null pointer: validation must return before it is dereferenced (no GPU here)
    f = lib.vlg_dmv1o_kbest
    SHAPE, DTYPE, WORKSPACE, NULL = 0x1001, 0x1002, 0x1004, 0x1005
    for N in (1, 0, 256, 300):
        assert f(one, one, one, 2, N, 0, 4, one, one, one, None, 0, None) == SHAPE
    for K in (0, -1, 17):
        assert f(one, one, one, 2, 8, 0, K, one, one, one, None, 0, None) == SHAPE
    assert f(one, one, one, 2, 8, 7, 4, one, one, one, None, 0, None) == DTYPE
    assert f(one, one, one, 2, 8, 2, 4, one, one, one, None, 0, None) == DTYPE
    for missing in (0, 1, 2, 7, 8):   # dec, attach, lengths, heads, scores
        args = [one, one, one, 2, 8, 0, 4, one, one, one, None, 0, None]
        args[missing] = None
        assert f(*args) == NULL
    assert f(None, None, None, 0, 8, 0, 4, None, None, None, None, 0, None) == 0   # empty batch: no-op
    assert f(one, one, one, 2, 255, 1, 16, one, one, one, None, 0, None) == WORKSPACE
    g = lib.vlg_dmv1o_tree_counts
    for N in (1, 256):
        assert g(one, one, None, None, 3, 2, N, one, one, None) == SHAPE
    assert g(one, one, None, None, -1, 2, 8, one, one, None) == SHAPE
    for missing in (0, 1, 7, 8):      # heads, lengths, cnt_dec, cnt_attach
        args = [one, one, None, None, 3, 2, 8, one, one, None]
        args[missing] = None
        assert g(*args) == NULL
    assert g(None, None, None, None, 3, 0, 8, None, None, None) == 0


def test_workspace_query_and_launcher_agree(lib):
    one = ctypes.c_void_p(16)
    q, f = lib.vlg_dmv1o_kbest_workspace, lib.vlg_dmv1o_kbest
    assert q(1, 2, 1) == 0 and q(1, 255, 16) > 0
    assert q(0, 200, 8) == 0 and q(2, 1, 8) == 0 and q(2, 256, 8) == 0 and q(2, 100, 0) == 0 and q(2, 100, 17) == 0
    refused = 0
    for K in (1, 8, 16):
        for N in range(2, 256):
            need = q(2, N, K)
            assert need == 2 * q(1, N, K) and q(5, N, K) == 5 * q(1, N, K)   # linear in B
            if need:
                assert f(one, one, one, 2, N, 0, K, one, one, one, one, need - 1, None) == 0x1004
                assert str(need).encode() in lib.vlg_last_error()
                refused += 1
    assert refused == sum(255 - PLACEMENT[KC][0] for KC in (1, 8, 16))


# ---- layout --------------------------------------------------------------------------------------------------------------------------------
def layout(N, KC, mode):
    "DmvKbestLayout restated: (lds_bytes, ws_bytes)"
    cells = N * ((N + 1) | 1)
    size = {True: 0, False: 0}
    for nbytes, in_lds in ((cells * KC * 8, mode < 2), (cells * KC * 4, mode < 2), (cells * 8, mode < 2), (cells * KC * 2, mode < 1),
                           (cells * KC * 4, mode < 1), (8 * 32 * 4, True)):
        size[in_lds] = (size[in_lds] + nbytes + 15) & ~15
    return size[True], size[False]


def test_layout_and_placement_table(emu, lib):
    emu.emu_dmv_kbest_plan.restype = None
    out = (ctypes.c_longlong * 4)()
    for K in range(1, 17):
        KC = next(c for c in (1, 2, 4, 8, 16) if K <= c)
        for N in range(2, 256):
            mode = next((m for m in (0, 1) if layout(N, KC, m)[0] <= LDS), 2)
            lds, ws = layout(N, KC, mode)
            emu.emu_dmv_kbest_plan(N, K, out)
            assert tuple(out) == (KC, mode, lds, ws), (N, K, tuple(out))
            assert lds <= LDS and lib.vlg_dmv1o_kbest_workspace(3, N, K) == 3 * ws
            a, b = PLACEMENT[KC]
            assert mode == (0 if N <= a else 1 if N <= b else 2), (N, K, mode)


def test_python_surface():
    import torch
    from vlgae_amd.torch_struct import DMV1o
    from vlgae_amd.torch_struct import functional as F
    assert callable(DMV1o.kbest_heads) and callable(DMV1o.kbest_scores)
    assert callable(F.dmv1o_kbest) and callable(F.dmv1o_kbest_scores) and callable(F.dmv1o_tree_counts)
    dist = DMV1o([torch.zeros(1, 3, 2, 2, 2), torch.zeros(1, 3, 3, 2)], torch.tensor([2]))
    for name in ("kmax", "topk"):
        with pytest.raises(NotImplementedError, match="kbest_heads") as e:
            getattr(dist, name)(2)
        assert re.search("DMV1o", str(e.value))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dist.kbest_heads(2)
