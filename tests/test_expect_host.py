"""CPU: expectations under DependencyCRF (expected_score / tree_entropy / tree_cross_entropy / tree_kl) without a GPU -- the float64
restatement of the dual-number rule against the reference's fixtures and against enumeration, the kernel's body under the host emulator
(tests/emu/emu_expect.cpp) at both arenas, the same emulator as a stand-alone program under AddressSanitizer + UBSan, the C ABI's
host-side contract at every N, and the Python surface.

Tolerances (tests/expect_restatement.py): against the float64 restatement, the floor of each output or 6 x the float32 restatement's own
error.  Largest error / bound the emulator reached: logZ 0.004, ev 0.003, mu 0.10, hv 0.09 (printed per case).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import expect_restatement as E
from conftest import ROOT

HERE = os.path.join(ROOT, "tests", "emu")
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "emu_expect.cpp")
DEPS = [SRC, os.path.join(HERE, "emu_dp.cpp"), os.path.join(HERE, "emu_expect_common.h")] + [os.path.join(ROOT, "vlgae_amd", "csrc", f) for f in ("vlg_dp_core.h", "vlg_dp_expect.h")]
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("expect_B3_N6_s0", "expect_B4_N12_s1", "expect_B2_N41_s2")
NS = (2, 3, 6, 41, 58, 101)


def _build(out, extra):
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", *extra, SRC, "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def emu():
    return ctypes.CDLL(_build(os.path.join(BUILD, "libvlg_emu_expect.so"), ["-fPIC", "-shared"]))


@pytest.fixture(scope="module")
def lib():
    from vlgae_amd.build import build_library
    build_library()
    from vlgae_amd import _C
    return _C.lib()


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def ragged(N):
    return np.array([N - 1, 1, max(1, (N - 1) // 2)], np.int64)


def case(N, seed, lengths=None):
    rng = np.random.default_rng(seed)
    arc = rng.standard_normal((3, N, N)).astype(np.float32)
    v = (0.5 * rng.standard_normal((3, N, N))).astype(np.float32)
    return arc, v, ragged(N) if lengths is None else np.asarray(lengths, np.int64)


def run_emu(emu, arc, lengths, v=None, v_sub=None, mode=0, grad=True, order=0):
    B, N = arc.shape[:2]
    arc = np.ascontiguousarray(arc, np.float32)
    v, v_sub = (None if t is None else np.ascontiguousarray(t, np.float32) for t in (v, v_sub))
    logZ, ev = np.full(B, 7.0, np.float32), np.full(B, 7.0, np.float32)
    mu = np.full((B, N, N), 7.0, np.float32) if grad else None
    hv = np.full((B, N, N), 7.0, np.float32) if grad else None
    before = emu.emu_canary_trips()
    assert emu.emu_deptree_expect(_p(arc), _p(v), _p(v_sub), _p(np.ascontiguousarray(lengths, np.int64)), B, N, mode, _p(logZ), _p(ev),
                                  _p(mu), _p(hv), 16, order) == 0
    assert emu.emu_canary_trips() == before == 0
    return logZ, ev, mu, hv


def check(tag, got, arc, lengths, v=None, v_sub=None):
    r = E.ratios(got, arc, lengths, v, v_sub)
    print(f"{tag}: error / bound " + " ".join(f"{k} {x:.3f}" for k, x in r.items()))
    assert all(x <= 1.0 for x in r.values()), (tag, r)
    return r


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float(np.abs(np.asarray(a) - b).max() / max(1.0, np.abs(b).max()))


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_the_reference(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    p, q, c, ln = z["arc_p"], z["arc_q"], z["cost"], z["lengths"]
    assert 1 in ln and p.dtype == np.float64
    lzq, _, muq, _ = E.dual_batch(q, ln)
    lz, ev, mu, hv = E.dual_batch(p, ln, p)
    errs = [_rel(lz - ev, z["entropy"]), _rel(-hv, z["g_entropy_arc_p"])]
    lz, ev, mu, hv = E.dual_batch(p, ln, q)
    errs += [_rel(lzq - ev, z["cross_entropy"]), _rel(-hv, z["g_cross_entropy_arc_p"]), _rel(muq - mu, z["g_cross_entropy_arc_q"])]
    lz, ev, mu, hv = E.dual_batch(p, ln, q, p)
    errs += [_rel(lzq - lz - ev, z["kl"]), _rel(-hv, z["g_kl_arc_p"]), _rel(muq - mu, z["g_kl_arc_q"])]
    assert np.all(z["kl"] >= 0) and _rel(z["kl"], z["cross_entropy"] - z["entropy"]) == 0.0
    lz, ev, mu, hv = E.dual_batch(p, ln, c)
    errs += [_rel(ev, z["risk"]), _rel(hv, z["g_risk_arc_p"]), _rel(mu, z["g_risk_cost"])]
    print(name, "largest relative error", max(errs))
    assert max(errs) <= 1e-10, errs


@pytest.mark.parametrize("length", (1, 2, 3, 4, 5))
def test_restatement_matches_enumeration(length):
    rng = np.random.default_rng(length)
    N, n = length + 2, length + 1
    arc, v = rng.standard_normal((N, N)), rng.standard_normal((N, N))
    logZ, ev, mu, hv, H, gH = E.brute(arc, length, v)
    lz, e, m, h = E.dual(arc, length, v)
    assert max(abs(lz - logZ), abs(e - ev), np.abs(m[:n, :n] - mu).max(), np.abs(h[:n, :n] - hv).max()) <= 1e-11
    assert not m[n:].any() and not m[:, n:].any() and not h[n:].any() and not h[:, n:].any()
    lz, e, m, h = E.dual(arc, length, arc)                     # entropy: the direction is the potentials themselves
    assert abs(lz - e - H) <= 1e-11 and np.abs(-h[:n, :n] - gH).max() <= 1e-11
    if length == 1:
        assert H == 0.0 and not h.any()


def test_restated_plan_boundaries():
    "twelve charts fit the LDS up to N = 57, four up to N = 100; every N has a plan within the LDS"
    assert [N for N in range(2, 256) if E.plan(N, True)[0] == 0][-1] == 57 and [N for N in range(2, 256) if E.plan(N, False)[0] == 0][-1] == 100
    assert all(E.plan(N, g)[1] <= E.LDS_BUDGET for N in range(2, 256) for g in (False, True))
    assert E.boundaries() == sorted(set(E.boundaries())) and 58 in E.boundaries() and 101 in E.boundaries()


# ---- 2. the kernel's body under the emulator ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("mode", (0, 3))
def test_emulator_matches_the_restatement(emu, N, mode):
    "mode 0: every chart in the first arena; mode 3: every chart in the second (the workspace placement)"
    arc, v, ln = case(N, 10 + N)
    got = run_emu(emu, arc, ln, v, mode=mode, order=2 if N <= 6 else 0)
    check(f"emu N={N} mode={mode}", got, arc, ln, v)
    fw = run_emu(emu, arc, ln, v, mode=min(mode, 2), grad=False)
    assert np.array_equal(fw[0], got[0]) and np.array_equal(fw[1], got[1])       # the forward-only body: the same values


def test_emulator_orders_agree(emu):
    "no intra-phase race: the serialisation order of the lanes inside a phase does not change a bit"
    arc, v, ln = case(12, 3)
    a = run_emu(emu, arc, ln, v, order=0)
    for order in (1, 2, 5):
        b = run_emu(emu, arc, ln, v, order=order)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), order


@pytest.mark.parametrize("mode", (1, 2))
def test_emulator_mixed_placements(emu, mode):
    arc, v, ln = case(41, 77)
    got = run_emu(emu, arc, ln, v, mode=mode)
    assert all(np.array_equal(x, y) for x, y in zip(got, run_emu(emu, arc, ln, v, mode=0)))


def test_emulator_forbidden_arcs_null_direction_and_bad_length(emu):
    N = 12
    rng = np.random.default_rng(4)
    arc, v, _ = case(N, 4)
    forbid = rng.random((3, N, N)) < 0.2
    forbid[:, np.arange(N - 1), np.arange(1, N)] = False      # the chain 0 -> 1 -> 2 ... stays allowed: the support is not empty
    arc[forbid] = -np.inf
    v[forbid] = 1e30                                          # garbage where nothing may be read
    ln = np.array([N - 1, 0, 5], np.int64)                    # the middle one is not a sentence
    got = run_emu(emu, arc, ln, v)
    check("emu forbidden", got, arc, ln, v)
    assert not got[2][forbid].any() and not got[3][forbid].any()
    assert np.isnan(got[0][1]) and np.isnan(got[1][1]) and np.isfinite(got[0][[0, 2]]).all()
    ln = ragged(N)
    lz, ev, mu, hv = run_emu(emu, arc, ln, None)              # no direction: ev = 0, hv = 0 exactly, logZ and mu unchanged
    assert not ev.any() and not hv.any()
    ref = run_emu(emu, arc, ln, v)
    assert np.array_equal(lz, ref[0]) and np.array_equal(mu, ref[2])
    same = run_emu(emu, arc, ln, v, v_sub=v)                  # v - v_sub = 0 exactly (the finite part)
    assert not same[1].any() and not same[3].any()


# ---- 3. sanitizers: the emulator as a stand-alone program -----------------------------------------------------------------------------
def test_standalone_program_under_asan_ubsan(tmp_path):
    exe = _build(os.path.join(BUILD, "emu_expect_san"), ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                                                         "-fno-sanitize-recover=undefined", "-DEMU_EXPECT_MAIN"])
    for N in (41, 58):
        arc, v, ln = case(N, 20 + N)
        mode = E.plan(N, True)[0]
        case_file, out_file = tmp_path / f"case{N}.bin", tmp_path / f"out{N}.bin"
        with open(case_file, "wb") as f:
            np.array([3, N, mode], np.int32).tofile(f)
            ln.tofile(f)
            arc.tofile(f)
            v.tofile(f)
        r = subprocess.run([exe, str(case_file), str(out_file)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "canary_trips=0" in r.stdout, r.stdout + r.stderr
        flat = np.fromfile(out_file, np.float32)
        got = (flat[:3], flat[3:6], flat[6:6 + 3 * N * N].reshape(3, N, N), flat[6 + 3 * N * N:].reshape(3, N, N))
        check(f"sanitized emu N={N} mode={mode}", got, arc, ln, v)


# ---- 4. C ABI -------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_host_side_validation(lib):
    from vlgae_amd import _C
    assert hasattr(lib, "vlg_deptree_expect") and "vlg_deptree_expect" in _C.SIGNATURES
    assert (_C.OP_DEPTREE_EXPECT, _C.OP_DEPTREE_EXPECT_GRAD) == (4, 5)
    one = ctypes.c_void_p(16)   # any non-null pointer: validation must return before it is dereferenced (no GPU here)
    f = lib.vlg_deptree_expect
    SHAPE, DTYPE, NULL, WORKSPACE = 0x1001, 0x1002, 0x1003, 0x1004
    assert f(one, one, one, one, 2, 1, 0, 0, one, one, one, one, None, 0, None) == SHAPE
    assert f(one, one, one, one, 2, 256, 0, 0, one, one, one, one, None, 0, None) == SHAPE and b"255" in lib.vlg_last_error()
    assert f(one, one, one, one, 2, 8, 7, 0, one, one, one, one, None, 0, None) == DTYPE
    assert f(one, one, one, one, 2, 8, 0, 7, one, one, one, one, None, 0, None) == DTYPE and b"v_dtype" in lib.vlg_last_error()
    assert f(None, one, one, one, 2, 8, 0, 0, one, one, one, one, None, 0, None) == NULL
    assert f(one, one, one, one, 2, 8, 0, 0, None, one, one, one, None, 0, None) == NULL
    assert f(None, None, None, None, 0, 8, 0, 0, None, None, None, None, None, 0, None) == 0          # empty batch: no-op
    assert f(one, None, None, None, 2, 200, 1, 1, one, None, None, one, None, 0, None) == WORKSPACE    # optional pointers may be null
    q = lib.vlg_workspace_bytes
    for op in (_C.OP_DEPTREE_EXPECT, _C.OP_DEPTREE_EXPECT_GRAD):
        assert q(op, 3, 2, 0) == 0 and q(op, 3, 255, 0) > 0 and q(op, 3, 255, 1) == 0 and q(op, 0, 255, 0) == 0
    assert q(99, 4, 41, 0) == 0


def test_workspace_query_launcher_and_restated_layout_agree_at_every_width(lib):
    """Both ops, every N in 2 ... 255: the query equals the restated layout's workspace, the restated LDS part fits 160 KiB, and one byte
    less than the query is refused with VLG_ERR_WORKSPACE naming the size.  (Never a sufficient size: that would launch.)"""
    from vlgae_amd import _C
    one, B = ctypes.c_void_p(16), 3
    f, q = lib.vlg_deptree_expect, lib.vlg_workspace_bytes
    for grad, op in ((False, _C.OP_DEPTREE_EXPECT), (True, _C.OP_DEPTREE_EXPECT_GRAD)):
        spilled = 0
        for N in range(2, 256):
            mode, lds, ws = E.plan(N, grad)
            need = q(op, B, N, 0)
            assert need == ws * B and lds <= 160 * 1024, (grad, N, mode, need, ws, lds)
            if need:
                spilled += 1
                for mu, hv in (((one, None), (None, one), (one, one)) if grad else ((None, None),)):
                    assert f(one, one, None, one, B, N, 0, 0, one, one, mu, hv, one, need - 1, None) == 0x1004, (grad, N)
                    assert str(need).encode() in lib.vlg_last_error()
                assert f(one, one, None, one, B, N, 0, 0, one, one, one if grad else None, None, None, 0, None) == 0x1004
        assert spilled > 0
    assert q(_C.OP_DEPTREE_EXPECT_GRAD, 1, 57, 0) == 0 < q(_C.OP_DEPTREE_EXPECT_GRAD, 1, 58, 0)
    assert q(_C.OP_DEPTREE_EXPECT, 1, 100, 0) == 0 < q(_C.OP_DEPTREE_EXPECT, 1, 101, 0)


# ---- 5. Python surface ----------------------------------------------------------------------------------------------------------------
def test_python_surface():
    import torch
    from vlgae_amd.torch_struct import DependencyCRF, DMV1o, functional as F
    for name in ("expected_score", "tree_entropy", "tree_cross_entropy", "tree_kl"):
        assert callable(getattr(DependencyCRF, name)) and not hasattr(DMV1o, name)
    for name in ("deptree_expect", "deptree_expected_score", "deptree_entropy", "deptree_cross_entropy", "deptree_kl"):
        assert callable(getattr(F, name))
    d = DependencyCRF(torch.zeros(1, 3, 3))
    with pytest.raises(NotImplementedError, match="sample_heads"):
        d.entropy
    for call in (lambda: d.cross_entropy(d), lambda: d.kl(d), lambda: d.risk(torch.zeros(1, 3, 3))):
        with pytest.raises(NotImplementedError, match="tree_entropy"):
            call()
    with pytest.raises(RuntimeError, match="MI355X"):       # no CPU path
        d.tree_entropy()
