"""CPU: expectations under DMV1o (DMV1oExpect: expected_score / tree_entropy / tree_cross_entropy / tree_kl) without a GPU -- the float64 restatement
of the dual-number rule against the reference's fixtures and against enumeration over every tree with its valences, the restated
layout and plan against the library's size query at every N, the kernel's body under the host emulator (tests/emu/emu_dmv_expect.cpp)
at every placement, the same emulator as a stand-alone program under AddressSanitizer + UBSan, the C ABI's host-side contract, and the
Python surface.

Tolerances (tests/dmv_expect_restatement.py, the family's bounds of tests/expect_restatement.py): against the float64 restatement, the
floor of each output or 6 x the float32 restatement's own error.  Largest error / bound the emulator reached: logZ 0.006, ev 0.002,
mu_dec 0.055, mu_att 0.051, hv_dec 0.027, hv_att 0.025 (printed per case).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dmv_expect_restatement as E
from conftest import ROOT

HERE = os.path.join(ROOT, "tests", "emu")
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "emu_dmv_expect.cpp")
DEPS = [SRC, os.path.join(HERE, "emu_dp.cpp"), os.path.join(HERE, "emu_expect_common.h")] + [os.path.join(ROOT, "vlgae_amd", "csrc", f)
                                                   for f in ("vlg_dp_core.h", "vlg_dp_expect.h", "vlg_dmv_expect.h")]
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("dmvexpect_B3_N6_s0", "dmvexpect_B4_N12_s1", "dmvexpect_B2_N41_s2")
SHAPE, DTYPE, ARG, WORKSPACE = 0x1001, 0x1002, 0x1003, 0x1004


def _build(out, extra):
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", *extra, SRC, "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def emu():
    return ctypes.CDLL(_build(os.path.join(BUILD, "libvlg_emu_dmv_expect.so"), ["-fPIC", "-shared"]))


@pytest.fixture(scope="module")
def lib():
    from vlgae_amd.build import build_library
    build_library()
    from vlgae_amd import _C
    return _C.lib()


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def run_emu(emu, dec, attach, lengths, v=None, v_sub=None, mode=0, grad=True, order=0, want=(True, True, True, True)):
    "(logZ, ev, mu_dec, mu_att, hv_dec, hv_att); `want` selects the four optional outputs of the inside-outside image"
    B, N = dec.shape[:2]
    dec, attach = _f32(dec), _f32(attach)
    vd, va = (_f32(t) for t in (v or (None, None)))
    sd, sa = (_f32(t) for t in (v_sub or (None, None)))
    logZ, ev = np.full(B, 7.0, np.float32), np.full(B, 7.0, np.float32)
    outs = [np.full(s, 7.0, np.float32) if grad and w else None for s, w in zip((dec.shape, attach.shape, dec.shape, attach.shape), want)]
    before = emu.emu_canary_trips()
    assert emu.emu_dmv1o_expect(_p(dec), _p(attach), _p(vd), _p(va), _p(sd), _p(sa), _p(np.ascontiguousarray(lengths, np.int64)), B, N, mode,
                                _p(logZ), _p(ev), *[_p(o) for o in outs], 16, order) == 0
    assert emu.emu_canary_trips() == before == 0
    return (logZ, ev, *outs)


def check(tag, got, dec, attach, lengths, v=None, v_sub=None):
    r = E.ratios(got, dec, attach, lengths, v, v_sub)
    print(f"{tag}: error / bound " + " ".join(f"{k} {x:.3f}" for k, x in r.items()))
    assert all(x <= 1.0 for x in r.values()), (tag, r)
    return r


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float(np.abs(np.asarray(a) - b).max() / max(1.0, np.abs(b).max()))


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_the_reference(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    p, q, c, ln = (z["dec_p"], z["att_p"]), (z["dec_q"], z["att_q"]), (z["cost_dec"], z["cost_att"]), z["lengths"]
    assert 1 in ln and p[0].dtype == np.float64
    lzq, _, mqd, mqa, _, _ = E.dual_batch(*q, ln)
    lz, ev, _, _, hd, ha = E.dual_batch(*p, ln, p)
    errs = [_rel(lz - ev, z["entropy"]), _rel(-hd, z["g_entropy_dec_p"]), _rel(-ha, z["g_entropy_att_p"])]
    lz, ev, md, ma, hd, ha = E.dual_batch(*p, ln, q)
    errs += [_rel(lzq - ev, z["cross_entropy"]), _rel(-hd, z["g_cross_entropy_dec_p"]), _rel(-ha, z["g_cross_entropy_att_p"]),
             _rel(mqd - md, z["g_cross_entropy_dec_q"]), _rel(mqa - ma, z["g_cross_entropy_att_q"])]
    lz, ev, md, ma, hd, ha = E.dual_batch(*p, ln, q, p)   # KL: the gradients are those of cross_entropy - entropy
    errs += [_rel(lzq - lz - ev, z["kl"]), _rel(-hd, z["g_cross_entropy_dec_p"] - z["g_entropy_dec_p"]),
             _rel(-ha, z["g_cross_entropy_att_p"] - z["g_entropy_att_p"]), _rel(mqd - md, z["g_cross_entropy_dec_q"]),
             _rel(mqa - ma, z["g_cross_entropy_att_q"])]
    assert np.all(z["kl"] >= 0) and _rel(z["kl"], z["cross_entropy"] - z["entropy"]) == 0.0
    lz, ev, md, ma, hd, ha = E.dual_batch(*p, ln, c)
    errs += [_rel(ev, z["risk"]), _rel(hd, z["g_risk_dec_p"]), _rel(ha, z["g_risk_att_p"]), _rel(md, z["g_risk_cost_dec"]),
             _rel(ma, z["g_risk_cost_att"])]
    print(name, "largest relative error", max(errs))
    assert max(errs) <= 1e-10, errs


@pytest.mark.parametrize("length", (1, 2, 3, 4, 5))
def test_restatement_matches_enumeration(length):
    N, n = length + 2, length + 1
    dec, attach, v = E.case(N, length, B=1)
    dec, attach, v = dec[0].astype(np.float64), attach[0].astype(np.float64), tuple(t[0].astype(np.float64) for t in v)
    logZ, ev, mud, mua, hvd, hva, H, gHd, gHa = E.brute(dec, attach, length, v)
    lz, e, md, ma, hd, ha = E.dual(dec, attach, length, v)
    assert max(abs(lz - logZ), abs(e - ev), np.abs(md[:n] - mud).max(), np.abs(ma[:n, :n] - mua).max(), np.abs(hd[:n] - hvd).max(),
               np.abs(ha[:n, :n] - hva).max()) <= 1e-11
    for t in (md, hd):
        assert not t[n:].any()
    for t in (ma, ha):
        assert not t[n:].any() and not t[:, n:].any()
    lz, e, _, _, hd, ha = E.dual(dec, attach, length, (dec, attach))   # entropy: the direction is the potentials themselves
    assert abs(lz - e - H) <= 1e-11 and np.abs(-hd[:n] - gHd).max() <= 1e-11 and np.abs(-ha[:n, :n] - gHa).max() <= 1e-11
    if length == 1:
        assert H == 0.0 and not hd.any() and not ha.any()


# ---- 2. layout and plan ----------------------------------------------------------------------------------------------------------------
def test_restated_plan_boundaries():
    "80 bytes per cell fit the LDS up to N = 44, 32 bytes up to N = 70 (the benchmark shape N = 41 is inside both); every N has a plan"
    fits = lambda grad: [N for N in range(2, 256) if E.plan(N, grad)[0] == 0][-1]
    assert (fits(True), fits(False)) == (44, 70)
    assert all(E.plan(N, g)[1] <= E.LDS_BUDGET for N in range(2, 256) for g in (False, True))
    assert E.boundaries() == [45, 63, 71, 81, 99] and (E.first_workspace_n(True), E.first_workspace_n(False)) == (45, 71)
    assert [E.plan(N, True)[0] for N in (44, 45, 62, 63, 80, 81, 255)] == [0, 1, 1, 2, 2, 3, 3]
    assert [E.plan(N, False)[0] for N in (70, 71, 98, 99, 255)] == [0, 1, 1, 2, 2]
    assert 41 * 43 * 80 + 41 * 64 <= E.layout(41, True, 0)[0] == 143744 and E.layout(41, True, 0)[1] == 0   # the benchmark shape: 80 B per cell + staging, each chart padded to 16 B


def test_workspace_query_launcher_and_restated_layout_agree_at_every_width(lib):
    """Both images, every N in 2 ... 255: the query equals the restated layout's workspace, and one byte less than the query is refused
    with VLG_ERR_WORKSPACE naming the size.  (Never a sufficient size: that would launch.)"""
    one, B = ctypes.c_void_p(16), 3
    f, q = lib.vlg_dmv1o_expect, lib.vlg_dmv1o_expect_workspace
    for grad in (False, True):
        spilled = 0
        for N in range(2, 256):
            mode, lds, ws = E.plan(N, grad)
            need = q(B, N, int(grad))
            assert need == ws * B and lds <= 160 * 1024, (grad, N, mode, need, ws, lds)
            if need:
                spilled += 1
                outs = ((one, None, None, None), (None, one, None, None), (None, None, one, None), (None, None, None, one),
                        (one, one, one, one)) if grad else ((None,) * 4,)
                for o in (outs if N in (45, 63, 81, 255) else outs[-1:]):
                    assert f(one, one, one, one, None, None, one, B, N, 0, 0, one, one, *o, one, need - 1, None) == WORKSPACE, (grad, N)
                    assert str(need).encode() in lib.vlg_last_error()
                assert f(one, one, one, None, None, None, one, B, N, 0, 0, one, one, *outs[-1], None, 0, None) == WORKSPACE
        assert spilled > 0
    assert q(1, 44, 1) == 0 < q(1, 45, 1) and q(1, 70, 0) == 0 < q(1, 71, 0)
    assert q(0, 255, 1) == 0 and q(3, 1, 1) == 0 and q(3, 256, 1) == 0      # out of range: 0


# ---- 3. the kernel's body under the emulator ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,mode", [(2, 0), (3, 0), (6, 0), (6, 1), (6, 2), (6, 3), (13, 0), (13, 3), (24, 1), (24, 2)])
def test_emulator_matches_the_restatement(emu, N, mode):
    "every placement of the inside-outside image, with both arenas allocated exactly as laid out; the forward-only image beside it"
    dec, attach, v = E.case(N, 10 + N)
    ln = E.ragged(N)
    got = run_emu(emu, dec, attach, ln, v, mode=mode, order=2 if N <= 6 else 0)
    check(f"emu N={N} mode={mode}", got, dec, attach, ln, v)
    fw = run_emu(emu, dec, attach, ln, v, mode=min(mode, 2), grad=False)
    assert np.array_equal(fw[0], got[0]) and np.array_equal(fw[1], got[1])       # the forward-only body: the same bits
    assert all(o is None for o in fw[2:])


def test_emulator_benchmark_shape(emu):
    N = 41
    dec, attach, v = E.case(N, 41, B=1)
    ln = np.array([N - 1], np.int64)
    got = run_emu(emu, dec, attach, ln, v)
    check("emu N=41", got, dec, attach, ln, v)
    fw = run_emu(emu, dec, attach, ln, v, grad=False)
    assert np.array_equal(fw[0], got[0]) and np.array_equal(fw[1], got[1])


def test_emulator_orders_and_placements_agree(emu):
    "no intra-phase race: the serialisation order of the lanes inside a phase, and where the charts live, do not change a bit"
    dec, attach, v = E.case(12, 3)
    ln = E.ragged(12)
    a = run_emu(emu, dec, attach, ln, v, order=0)
    for order, mode in ((1, 0), (2, 1), (5, 2), (3, 3)):
        b = run_emu(emu, dec, attach, ln, v, order=order, mode=mode)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), (order, mode)


def test_emulator_each_optional_output_alone(emu):
    dec, attach, v = E.case(9, 5)
    ln = E.ragged(9)
    full = run_emu(emu, dec, attach, ln, v)
    for k in range(4):
        want = tuple(i == k for i in range(4))
        got = run_emu(emu, dec, attach, ln, v, want=want)
        assert np.array_equal(got[0], full[0]) and np.array_equal(got[1], full[1]) and np.array_equal(got[2 + k], full[2 + k])


def test_emulator_forbidden_entries_null_direction_and_bad_length(emu):
    N = 12
    rng = np.random.default_rng(4)
    dec, attach, v = E.case(N, 4)
    forbid = rng.random(attach.shape) < 0.2
    forbid[:, np.arange(N - 1), np.arange(1, N)] = False      # the chain 0 -> 1 -> 2 ... stays allowed: the support is not empty
    attach[forbid] = -np.inf
    merged_zero = attach <= -5e11                             # what DMV1o.merge wrote (and the -inf entries)
    v[1][merged_zero] = 1e30                                  # garbage where nothing may be read
    v[0][dec <= -5e11] = 1e30
    ln = np.array([N - 1, 0, 5], np.int64)                    # the middle one is not a sentence
    got = run_emu(emu, dec, attach, ln, v)
    check("emu forbidden", got, dec, attach, ln, v)
    assert not got[3][merged_zero].any() and not got[5][merged_zero].any()
    assert not got[2][dec <= -5e11].any() and not got[4][dec <= -5e11].any()
    assert np.isnan(got[0][1]) and np.isnan(got[1][1]) and np.isfinite(got[0][[0, 2]]).all()
    ln = E.ragged(N)
    null = run_emu(emu, dec, attach, ln, None)                # no direction: ev = 0, hv = 0 exactly, logZ and mu unchanged
    assert not null[1].any() and not null[4].any() and not null[5].any()
    ref = run_emu(emu, dec, attach, ln, v)
    assert all(np.array_equal(null[k], ref[k]) for k in (0, 2, 3))
    same = run_emu(emu, dec, attach, ln, v, v_sub=v)          # v - v_sub = 0 exactly (the finite part)
    assert not same[1].any() and not same[4].any() and not same[5].any()
    kl = run_emu(emu, dec, attach, ln, (dec, attach), v_sub=(dec, attach))   # the direction of tree_kl(p, p)
    assert not kl[1].any() and not kl[4].any() and not kl[5].any()


def test_emulator_structural_identities(emu):
    N = 12
    dec, attach, v = E.case(N, 8)
    ln = E.ragged(N)
    lz, ev, md, ma, hd, ha = (np.asarray(t, np.float64) for t in run_emu(emu, dec, attach, ln, v))
    for b, length in enumerate(ln):
        n = int(length) + 1
        dd, da = E.direction(dec[b], attach[b], int(length), (v[0][b], v[1][b]))
        assert abs(ev[b] - (md[b] * dd).sum() - (ma[b] * da).sum()) <= 1e-4 * max(1.0, (np.abs(md[b] * dd)).sum() + np.abs(ma[b] * da).sum())
        assert np.abs(ma[b, :, 1:n].sum((0, 2)) - 1).max() <= 1e-4 and np.abs(ha[b].sum((0, 2))).max() <= 1e-4   # every word has one head
        assert np.abs(md[b, 1:n, :, :, 1].sum(-1) - 1).max() <= 1e-4 and np.abs(hd[b, :, :, :, 1].sum(-1)).max() <= 1e-4   # every side stops once
        left = np.tril(np.ones((N, N)), -1)[:, :, None]
        for t_dec, t_att in ((md[b], ma[b]), (hd[b], ha[b])):
            assert np.abs(t_dec[:, 0, :, 0] - (t_att * left).sum(1)).max() <= 1e-5
            assert np.abs(t_dec[:, 1, :, 0] - (t_att * (1 - left)).sum(1)).max() <= 1e-5


# ---- 4. sanitizers: the emulator as a stand-alone program -----------------------------------------------------------------------------
def test_standalone_program_under_asan_ubsan(tmp_path):
    exe = _build(os.path.join(BUILD, "emu_dmv_expect_san"), ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                                                             "-fno-sanitize-recover=undefined", "-DEMU_DMV_EXPECT_MAIN"])
    for N, mode in ((13, 0), (10, 1), (10, 2), (13, 3)):
        dec, attach, v = E.case(N, 20 + N)
        ln = E.ragged(N)
        case_file, out_file = tmp_path / f"case{N}_{mode}.bin", tmp_path / f"out{N}_{mode}.bin"
        with open(case_file, "wb") as f:
            np.array([3, N, mode], np.int32).tofile(f)
            ln.tofile(f)
            for t in (dec, attach, v[0], v[1]):
                np.ascontiguousarray(t, np.float32).tofile(f)
        r = subprocess.run([exe, str(case_file), str(out_file)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "canary_trips=0" in r.stdout, r.stdout + r.stderr
        flat = np.fromfile(out_file, np.float32)
        sizes = [3, 3, dec.size, attach.size, dec.size, attach.size]
        parts = np.split(flat, np.cumsum(sizes)[:-1])
        got = (parts[0], parts[1], parts[2].reshape(dec.shape), parts[3].reshape(attach.shape), parts[4].reshape(dec.shape),
               parts[5].reshape(attach.shape))
        check(f"sanitized emu N={N} mode={mode}", got, dec, attach, ln, v)


# ---- 5. C ABI -------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_host_side_validation(lib):
    from vlgae_amd import _C
    assert lib.vlg_version() == 145 == _C.ABI_VERSION
    assert hasattr(lib, "vlg_dmv1o_expect") and "vlg_dmv1o_expect" in _C.SIGNATURES and "vlg_dmv1o_expect_workspace" in _C.SIGNATURES
    one = ctypes.c_void_p(16)   # any non-null pointer: validation must return before it is dereferenced (no GPU here)
    f = lib.vlg_dmv1o_expect
    tail = (one, one, one, one, one, one, None, 0, None)       # logZ, ev, mu_dec, mu_attach, hv_dec, hv_attach, ws, ws_bytes, stream
    assert f(one, one, one, one, one, one, one, 2, 1, 0, 0, *tail) == SHAPE
    assert f(one, one, one, one, one, one, one, 2, 256, 0, 0, *tail) == SHAPE and b"255" in lib.vlg_last_error()
    assert f(one, one, one, one, one, one, one, -1, 8, 0, 0, *tail) == SHAPE
    assert f(one, one, one, one, one, one, one, 2, 8, 7, 0, *tail) == DTYPE
    assert f(one, one, one, one, one, one, one, 2, 8, 0, 7, *tail) == DTYPE and b"v_dtype" in lib.vlg_last_error()
    assert f(None, one, one, one, one, one, one, 2, 8, 0, 0, *tail) == ARG
    assert f(one, None, one, one, one, one, one, 2, 8, 0, 0, *tail) == ARG
    assert f(one, one, one, one, one, one, one, 2, 8, 0, 0, None, *tail[1:]) == ARG
    assert f(None, None, None, None, None, None, None, 0, 8, 0, 0, None, None, None, None, None, None, None, 0, None) == 0   # empty batch: no-op
    assert f(one, one, None, None, None, None, one, 2, 200, 1, 1, one, None, None, None, None, one, None, 0, None) == WORKSPACE   # optional pointers may be null
    assert f(one, one, None, None, None, None, one, 2, 200, 1, 1, one, None, None, None, None, None, None, 0, None) == WORKSPACE   # forward only
    q = lib.vlg_workspace_bytes          # the op enum of vlg_workspace_bytes is unchanged: the size query is its own function
    assert q(6, 3, 255, 0) == 0 and (_C.OP_DEPTREE_EXPECT, _C.OP_DEPTREE_EXPECT_GRAD) == (4, 5)


# ---- 6. Python surface ----------------------------------------------------------------------------------------------------------------
def test_python_surface():
    import torch
    from vlgae_amd import torch_struct as ts
    from vlgae_amd.torch_struct import DMV1o, DMV1oExpect, functional as F
    assert issubclass(DMV1oExpect, DMV1o) and "DMV1oExpect" in ts.__all__
    for name in ("expected_score", "tree_entropy", "tree_cross_entropy", "tree_kl"):
        assert callable(getattr(DMV1oExpect, name)) and not hasattr(DMV1o, name)      # the surface of DMV1o itself is unchanged
    for name in ("dmv1o_expect", "dmv1o_expected_score", "dmv1o_entropy", "dmv1o_cross_entropy", "dmv1o_kl"):
        assert callable(getattr(F, name))
    pots, ln = [torch.zeros(1, 3, 2, 2, 2), torch.zeros(1, 3, 3, 2)], torch.tensor([2])
    d, plain = DMV1oExpect(pots, ln), DMV1o(pots, ln)
    with pytest.raises(NotImplementedError, match="DMV1oExpect"):
        d.entropy
    for call in (lambda: d.cross_entropy(d), lambda: d.kl(d), lambda: d.risk([None, None])):
        with pytest.raises(NotImplementedError, match="tree_entropy"):
            call()
    for call in (d.tree_entropy, lambda: d.tree_kl(plain), lambda: d.tree_cross_entropy(plain),
                 lambda: d.expected_score((None, torch.zeros(1, 3, 3, 2)))):
        with pytest.raises(RuntimeError, match="MI355X"):       # no CPU path
            call()
