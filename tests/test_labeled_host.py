"""CPU: DependencyCRF on labeled potentials [B,N,N,L] without a GPU -- the float64 restatement (tests/labeled_restatement.py) against
the reference's fixtures and against brute force over every labeled tree, the label-draw body of vlgae_amd/csrc/vlg_label_draw.h under
the host emulator (tests/emu/emu_label.cpp; the same emulator as a stand-alone program under AddressSanitizer + UBSan), the C ABI's
host-side contract (header against the ctypes table, argument-check codes, the lane-group table) and the Python surface.
"""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import labeled_restatement as R
import sample_restatement as S
from conftest import GOLDEN, ROOT, load

HERE = os.path.join(ROOT, "tests", "emu")
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "emu_label.cpp")
DEPS = [SRC, os.path.join(HERE, "emu_dp.cpp"), os.path.join(HERE, "emu_sample_common.h")] + [
    os.path.join(ROOT, "vlgae_amd", "csrc", f) for f in ("vlg_dp_core.h", "vlg_sample_common.h", "vlg_label_draw.h")]
FIXTURES = ("labeled_B3_N6_L4_s0", "labeled_B4_N12_L5_s1", "labeled_B2_N41_L7_s2")
TOL = 1e-11   # the bound of test_oracle_golden


def _build(out, extra):
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", *extra, SRC, "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def emu():
    return ctypes.CDLL(_build(os.path.join(BUILD, "libvlg_emu_label.so"), ["-fPIC", "-shared"]))


@pytest.fixture(scope="module")
def lib():
    from vlgae_amd.build import build_library
    build_library()
    from vlgae_amd import _C
    return _C.lib()


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


# ---- 1. the restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_equals_the_reference_fixtures(name):
    g = load(os.path.join(GOLDEN, name + ".npz"))
    assert g["lengths"].min() == 1 and g["phi"].dtype == np.float64
    L = g["phi"].shape[-1]
    assert all(len(set(row)) == L for t in ("phi", "other", "cost") for row in g[t].reshape(-1, L))   # no label ties
    worst = {}

    def cmp(key, got, b):
        worst[key] = max(worst.get(key, 0.0), float(np.abs(np.asarray(got) - g[key][b]).max()))

    for b, ln in enumerate(g["lengths"]):
        q = R.log_quantities(g["phi"][b], int(ln), g["other"][b], g["cost"][b])
        m = R.max_quantities(g["phi"][b], int(ln))
        for key in ("partition", "marginals", "entropy", "kl", "cross_entropy", "risk"):
            cmp(key, q[key], b)
        cmp("max", m["max"], b)
        assert np.array_equal(m["argmax"], g["argmax"][b])
        assert m["max"] == R.labeled_score(g["phi"][b], m["heads"], m["labels"], int(ln))
        if "grad_partition" in g:
            cmp("grad_partition", q["marginals"], b)
            assert np.array_equal(m["argmax"], g["grad_max"][b])
            for key in ("entropy", "kl", "cross_entropy", "risk"):
                cmp("grad_" + key, q[key + "_grad"], b)
            cmp("grad_kl_other", q["kl_grad_other"], b)
            cmp("grad_cross_entropy_other", q["cross_entropy_grad_other"], b)
            cmp("grad_risk_cost", q["risk_grad_cost"], b)
    print(name, {k: f"{v:.1e}" for k, v in worst.items()})
    assert ("grad_partition" in g) == (name != FIXTURES[-1])
    assert max(worst.values()) <= TOL, worst


@pytest.mark.parametrize("length", (1, 2, 3, 4))
def test_restatement_equals_brute_force_over_labeled_trees(length):
    phi = R.potentials(np.random.default_rng(300 + length), (5, 5, 3))
    logZ, marg, H, score, heads, labels = R.brute(phi, length)
    n = length + 1
    q = R.log_quantities(phi, length)
    m = R.max_quantities(phi, length)
    assert abs(q["partition"] - logZ) <= 1e-12 and abs(q["entropy"] - H) <= 1e-11
    assert np.abs(q["marginals"][:n, :n] - marg).max() <= 1e-12 and not q["marginals"][n:].any() and not q["marginals"][:, n:].any()
    assert m["max"] == score and np.array_equal(m["heads"][:n], heads) and np.array_equal(m["labels"][:n], labels)


def test_restatement_masks_ties_and_forbidden_labels():
    rng = np.random.default_rng(5)
    N, L, ln = 6, 5, 3
    phi = R.potentials(rng, (N, N, L))
    base = R.fold(phi, ln, "log", v=phi)
    dirty = phi.copy()
    dirty[~R.read_mask(N, ln)] = np.nan                                  # never-read cells: anything
    for a, b in zip(base, R.fold(dirty, ln, "log", v=dirty)):
        assert np.array_equal(a, b)
    assert np.all(base[0][~R.read_mask(N, ln)] == R.ZERO) and not base[1][~R.read_mask(N, ln)].any()
    assert np.array_equal(R.fold(phi, ln, "log", v=phi, v_sub=phi)[2], np.zeros((N, N)))   # dbar of a zero direction: exactly 0
    phi[1, 2] = -np.inf                                                  # a row without an allowed label
    phi[2, 3, 1] = -np.inf                                               # one forbidden label among finite ones
    phi[0, 1, :] = [1.0, 2.0, 2.0, 0.5, 2.0]                             # a planted tie: the lowest index wins
    arc, best, dbar, p = R.fold(phi, ln, "log", v=phi)
    assert arc[1, 2] == -np.inf and best[1, 2] == 0 and dbar[1, 2] == 0 and not p[1, 2].any()
    assert p[2, 3, 1] == 0 and abs(p[2, 3].sum() - 1) < 1e-15 and np.isfinite(dbar[2, 3])
    assert best[0, 1] == 1 and R.fold(phi, ln, "max")[0][0, 1] == 2.0
    assert np.all(np.isfinite(R.log_quantities(phi, ln)["entropy_grad"]))


# ---- 2. the draw body under the emulator --------------------------------------------------------------------------------------------------
def run_emu(emu, phi, heads, lengths, u_label, arc=None, logp=None, bf16=False):
    B, N, _, L = phi.shape
    S = heads.shape[0]
    a = np.ascontiguousarray(phi, np.float32)
    if bf16:
        assert not (a.view(np.uint32) & 0xFFFF).any()
        a = (a.view(np.uint32) >> 16).astype(np.uint16)
    labels = np.full((S, B, N), -1, np.int64)
    arc = None if arc is None else np.ascontiguousarray(arc, np.float32)
    before = emu.emu_canary_trips()
    assert emu.emu_label_draw(_p(a), _p(arc), _p(np.ascontiguousarray(heads, np.int64)), _p(np.ascontiguousarray(lengths, np.int64)), B, N, L, S,
                              int(bf16), _p(np.ascontiguousarray(u_label, np.float32)), _p(labels), _p(logp)) == 0
    assert emu.emu_canary_trips() == before == 0
    return labels


def draw_case(N, L, samples, seed, bf16=False):
    "phi [3,N,N,L], random trees heads [samples,3,N] over ragged lengths, the generator"
    rng = np.random.default_rng(seed)
    lengths = np.array([N - 1, 1, max(1, (N - 1) // 2)])
    phi = R.potentials(rng, (3, N, N, L), bf16=bf16)
    heads = np.stack([np.stack([S.pad_heads(S.random_tree(int(ln), rng), N) for ln in lengths]) for _ in range(samples)])
    return phi, heads, lengths, rng


@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("N,L", ((2, 1), (4, 2), (6, 3), (6, 7), (12, 40), (7, 64), (5, 65), (4, 255)))
def test_emulated_draw_equals_the_restated_rule(emu, N, L, bf16):
    """Steered: u_label is the midpoint of a chosen label's interval, so float32 and float64 land on the same label; the one-lane wave
    runs the rule's sequential sums, one term per chunk."""
    S_ = 4
    phi, heads, lengths, rng = draw_case(N, L, S_, 900 + 7 * N + L, bf16)
    if L > 1:
        phi[0, :, :, L // 2] = -np.inf                   # a forbidden label is never drawn (it is no target: its weight is 0)
    target = np.zeros((S_, 3, N), np.int64)
    u = np.full((S_, 3, N), np.nan, np.float32)
    pmin = 1.0
    for s in range(S_):
        for b, ln in enumerate(lengths):
            for c in range(1, int(ln) + 1):
                row = phi[b, heads[s, b, c], c]
                ok = np.nonzero(np.exp(row - row.max()) >= 1e-3)[0]
                t = int(rng.choice(ok))
                u[s, b, c], p = R.steer_label(row, t)
                target[s, b, c], pmin = t, min(pmin, p)
                assert R.draw_label(row, u[s, b, c]) == t
    assert pmin > 1e-5   # half an interval is far above float32's cum / total error (L 2^-24)
    got = run_emu(emu, phi, heads, lengths, u, bf16=bf16)
    assert np.array_equal(got, target)
    assert L == 1 or not np.any(got[:, 0] == L // 2)


def test_emulated_draw_edges_and_logp(emu):
    N, L = 6, 4
    phi, heads, lengths, rng = draw_case(N, L, 2, 77)
    lengths = np.array([N - 1, 1, 0])                    # the last one is no sentence
    heads[:, 1] = 0
    heads[:, 2] = 0
    heads[1, 0] = 0                                      # a tree the sampler gave up on (5 words, all heads 0)
    u = np.zeros((2, 3, N), np.float32)                  # u = 0: the first label of weight > 0
    phi[0, :, :, 0] = -np.inf
    arc = R.fold_batch(phi, np.array([N - 1, 1, 1]))[0]
    logp = np.zeros((2, 3), np.float32)
    logp[1, 0] = np.nan
    got = run_emu(emu, phi, heads, lengths, u, arc=arc, logp=logp)
    assert not got[1, 0].any() and np.isnan(logp[1, 0]) and not got[:, 2].any() and not got[:, :, 0].any()
    assert np.all(got[0, 0, 1:] == 1) and got[0, 1, 1] == 0 and not got[0, 1, 2:].any()
    want = sum(phi[0, heads[0, 0, c], c, 1] - arc[0, heads[0, 0, c], c] for c in range(1, N))
    assert abs(logp[0, 0] - want) <= 1e-5 * (N - 1) * 8
    ones = np.nextafter(np.float32(1), np.float32(0)) * np.ones((2, 3, N), np.float32)   # u -> 1: the last label of weight > 0
    assert np.all(run_emu(emu, phi, heads, lengths, ones)[0, 0, 1:] == L - 1)
    nan = np.full((2, 3, N), np.nan, np.float32)
    assert np.all(run_emu(emu, phi, heads, lengths, nan)[0, 0, 1:] == L - 1)


def test_standalone_program_under_asan_ubsan(emu, tmp_path):
    exe = _build(os.path.join(BUILD, "emu_label_san"), ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                                                         "-fno-sanitize-recover=undefined", "-DEMU_LABEL_MAIN"])
    for N, L in ((6, 3), (12, 65), (5, 255)):
        phi, heads, lengths, rng = draw_case(N, L, 3, 11 * N + L)
        u = rng.random((3, 3, N)).astype(np.float32)
        labels = run_emu(emu, phi, heads, lengths, u)
        path = tmp_path / f"case{N}_{L}.bin"
        with open(path, "wb") as f:
            f.write(struct.pack("4i", 3, N, L, 3))
            f.write(np.asarray(lengths, np.int64).tobytes())
            f.write(np.ascontiguousarray(phi, np.float32).tobytes())
            f.write(np.ascontiguousarray(heads, np.int64).tobytes())
            f.write(u.tobytes())
            f.write(labels.tobytes())
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "mismatches=0 canary_trips=0" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ---- 3. C ABI -----------------------------------------------------------------------------------------------------------------------------
NAMES = ("vlg_label_fold", "vlg_label_expand", "vlg_label_draw", "vlg_label_lanes")


def test_header_agrees_with_the_ctypes_table(lib):
    from vlgae_amd import _C
    text = open(os.path.join(ROOT, "include", "vlgae_amd.h")).read()
    kinds = {ctypes.c_void_p: "ptr", ctypes.c_int: "int", ctypes.c_uint: "unsigned"}
    for name in NAMES:
        assert hasattr(lib, name) and name in _C.SIGNATURES
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", text)
        assert m, name
        declared = ["ptr" if "*" in a else "unsigned" if a.split()[0] == "unsigned" else a.split()[0] for a in m.group(1).split(",")]
        res, args = _C.SIGNATURES[name]
        assert res is ctypes.c_int and [kinds[a] for a in args] == declared, name
    assert lib.vlg_version() == _C.ABI_VERSION


def test_argument_check_codes(lib):
    one = ctypes.c_void_p(16)   # any non-null pointer: validation must return before it is dereferenced (no GPU here)
    SHAPE, DTYPE, ARG = 0x1001, 0x1002, 0x1003
    fold, expand, draw = lib.vlg_label_fold, lib.vlg_label_expand, lib.vlg_label_draw

    def f(phi=one, v=None, v_sub=None, B=2, N=8, L=5, dt=0, vdt=0, sr=0, arc=one, best=None, dbar=None):
        return fold(phi, v, v_sub, one, B, N, L, dt, vdt, sr, arc, best, dbar, None)

    def e(phi=one, v=None, v_sub=None, B=2, N=8, L=5, dt=0, vdt=0, odt=0, sr=0, mode=0, arc=one, best=None, g1=one, stride=1, out=one):
        return expand(phi, v, v_sub, one, B, N, L, dt, vdt, odt, sr, mode, arc, best, g1, None, None, None, stride, out, None)

    def d(phi=one, arc=None, heads=one, B=2, N=8, L=5, S=3, dt=0, rng=one, u=None, labels=one, logp=None):
        return draw(phi, arc, heads, one, B, N, L, S, dt, rng, 0, u, labels, logp, None)

    for call in (f, e, d):
        for N in (1, 0, 256):
            assert call(N=N) == SHAPE
        for L in (0, -1, 256):
            assert call(L=L) == SHAPE
        assert call(B=-1) == SHAPE and call(dt=2) == DTYPE and call(dt=7) == DTYPE
        assert call(phi=None) == ARG
        assert call(phi=None, B=0) == 0                                      # empty batch: a no-op before any pointer is looked at
    assert f(vdt=3) == DTYPE and f(sr=2) == ARG and f(arc=None) == ARG
    assert f(sr=1, dbar=one) == ARG and f(v_sub=one) == ARG
    assert e(vdt=3) == DTYPE and e(odt=1) == DTYPE and e(dt=1, odt=2) == DTYPE and e(mode=2) == ARG and e(stride=2) == ARG
    assert e(sr=1) == ARG and e(g1=None) == ARG and e(out=None) == ARG and e(arc=None) == ARG and e(v_sub=one) == ARG
    assert d(S=0) == SHAPE and d(rng=None) == ARG and d(u=one) == ARG and d(heads=None) == ARG and d(labels=None) == ARG
    assert d(logp=one) == ARG
    assert b"label_draw" in lib.vlg_last_error()
    assert f(B=1 << 30, N=255, L=255) == SHAPE and b"workgroups" in lib.vlg_last_error()
    assert f(B=1100, N=255, L=255) == SHAPE and e(B=1100, N=255, L=255) == SHAPE      # 1100 x 16257 tiles of four rows: past 2^24 - 1 workgroups
    assert d(B=1 << 20, S=64) == SHAPE and b"workgroups" in lib.vlg_last_error()         # 2^26 (sample, sentence) pairs, four per workgroup


def plan(L, bf16):
    "vlg_label.hip: label_plan restated -- (lanes per row, vector image)"
    es = 2 if bf16 else 4
    vec = (L * es) % 16 == 0
    E, KS = (16 // es, 2) if vec else (1, 4)
    need = -(-L // (E * KS))
    G = 1
    while G < need:
        G *= 2
    return G, vec


def test_lane_group_table(lib):
    for bf16 in (False, True):
        table = {}
        for L in range(1, 256):
            G, vec = plan(L, bf16)
            assert lib.vlg_label_lanes(L, int(bf16)) == (G | (0x100 if vec else 0)), (L, bf16)
            assert G <= 64 and G * (2 * (8 if bf16 else 4) if vec else 4) >= L
            table.setdefault((G, vec), []).append(L)
        assert {G for G, _ in table} == {1, 2, 4, 8, 16, 32, 64}
    assert lib.vlg_label_lanes(0, 0) == 0 and lib.vlg_label_lanes(256, 0) == 0 and lib.vlg_label_lanes(8, 2) == 0


# ---- 4. the Python surface ----------------------------------------------------------------------------------------------------------------
def test_python_surface():
    import torch
    from vlgae_amd.torch_struct import DependencyCRF
    from vlgae_amd.torch_struct import functional as F
    for name in ("label_fold", "label_expand", "deptree_labeled_sum", "deptree_labeled_marginals", "deptree_labeled_decode", "deptree_labeled_sample",
                 "deptree_labeled_expected_score", "deptree_labeled_entropy", "deptree_labeled_cross_entropy", "deptree_labeled_kl"):
        assert callable(getattr(F, name))
    dist = DependencyCRF(torch.zeros(1, 3, 3, 2))
    assert dist.labeled and not DependencyCRF(torch.zeros(1, 3, 3)).labeled
    for call in (lambda: dist.kbest_heads(2), lambda: dist.kbest_scores(2)):
        with pytest.raises(NotImplementedError, match="labeled") as err:
            call()
        assert "K-list" in str(err.value) and "not" in str(err.value)
    with pytest.raises(NotImplementedError, match="labeled potentials"):
        dist.kmax(2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dist.partition
    with pytest.raises(ValueError, match="unlabeled"):
        DependencyCRF(torch.zeros(1, 3, 3)).argmax_labels
    with pytest.raises(ValueError, match="labeled potentials"):
        DependencyCRF(torch.zeros(1, 3, 3)).sample_heads(1, return_labels=True)
    with pytest.raises(ValueError, match="return_labels"):
        dist.sample_heads(1, u=torch.zeros(1, 1, 3, 3, 3), u_label=torch.zeros(1, 1, 3))
    heads = torch.tensor([[[0, 2, 0, 2], [0, 0, 1, 0]]])
    labels = torch.tensor([[[0, 1, 2, 0], [0, 2, 1, 0]]])
    parts = DependencyCRF.heads_to_parts(heads, torch.tensor([3, 2]), labels=labels, num_labels=3)
    assert parts.shape == (1, 2, 4, 4, 3) and parts.sum() == 5
    assert parts[0, 0, 2, 1, 1] == 1 and parts[0, 0, 0, 2, 2] == 1 and parts[0, 0, 2, 3, 0] == 1 and parts[0, 1, 0, 1, 2] == 1 and parts[0, 1, 1, 2, 1] == 1
    assert torch.equal(parts.sum(-1), DependencyCRF.heads_to_parts(heads, torch.tensor([3, 2])))
    with pytest.raises(ValueError, match="num_labels"):
        DependencyCRF.heads_to_parts(heads, labels=labels)
