"""CPU: the check sequence vlg_deptree_expect and vlg_dmv1o_expect share (vlgae_amd/csrc/vlg_expect_kernels.h: expect_entry).  One table of
refused calls against both entry points: the return code and the whole vlg_last_error text of each, as recorded from the library before
the two entry points were folded onto one frame -- the order of the checks, the codes and the messages are part of the C ABI's contract.
No call here can launch: every one is refused (or is the empty batch) before a pointer is dereferenced."""
import ctypes

import pytest

SHAPE, DTYPE, ARG, WORKSPACE = 0x1001, 0x1002, 0x1003, 0x1004
B = 3
ONE = ctypes.c_void_p(16)   # any non-null pointer


@pytest.fixture(scope="module")
def lib():
    from vlgae_amd.build import build_library
    build_library()
    from vlgae_amd import _C
    return _C.lib()


def _deptree(lib, pot=ONE, lengths=ONE, B=B, N=8, in_dtype=0, v_dtype=0, logZ=ONE, grad=False, ws=None, ws_bytes=0):
    return lib.vlg_deptree_expect(pot, ONE, None, lengths, B, N, in_dtype, v_dtype, logZ, ONE, ONE if grad else None, None, ws, ws_bytes, None)


def _dmv1o(lib, pot=ONE, lengths=ONE, B=B, N=8, in_dtype=0, v_dtype=0, logZ=ONE, grad=False, ws=None, ws_bytes=0, attach=ONE):
    return lib.vlg_dmv1o_expect(pot, attach, ONE, ONE, None, None, lengths, B, N, in_dtype, v_dtype, logZ, ONE, None, ONE if grad else None, None,
                                None, ws, ws_bytes, None)


def _need(lib, op, N, grad):
    from vlgae_amd import _C
    if op == "deptree_expect":
        return lib.vlg_workspace_bytes(_C.OP_DEPTREE_EXPECT_GRAD if grad else _C.OP_DEPTREE_EXPECT, B, N, 0)
    return lib.vlg_dmv1o_expect_workspace(B, N, int(grad))


def _first_spilled(lib, op, grad):
    return next(N for N in range(2, 256) if _need(lib, op, N, grad))


def table(lib, op):
    """{case: (return code, vlg_last_error text)} of the refused calls of one entry point"""
    f = {"deptree_expect": _deptree, "dmv1o_expect": _dmv1o}[op]
    out = {}

    def call(case, **kw):
        rc = f(lib, **kw)
        out[case] = (rc, lib.vlg_last_error().decode())

    call("B < 0", B=-1)
    call("N = 1", N=1)
    call("N = 256", N=256)
    call("bad in_dtype", in_dtype=7)
    call("bad v_dtype", v_dtype=7)
    call("bad in_dtype and v_dtype", in_dtype=7, v_dtype=7)            # in_dtype is checked first
    call("bad v_dtype, null potentials", v_dtype=7, pot=None)           # the types before the pointers
    call("null potentials", pot=None)
    call("null logZ", logZ=None)
    if op == "dmv1o_expect":            # its other required pointers, each alone
        call("null attach", attach=None)
        call("null lengths", lengths=None)
    for grad in (False, True):
        N = _first_spilled(lib, op, grad)
        need = _need(lib, op, N, grad)
        tag = f"grad={int(grad)} N={N}"
        call(f"one byte short, {tag}", N=N, grad=grad, ws=ONE, ws_bytes=need - 1)
        call(f"null workspace, {tag}", N=N, grad=grad, ws=None, ws_bytes=need)
        call(f"null lengths, {tag}", N=N, grad=grad, lengths=None, ws=None, ws_bytes=0)   # DepTree: optional, so the next check speaks
        call(f"null logZ before the workspace, {tag}", N=N, grad=grad, logZ=None, ws=None, ws_bytes=0)
    return out


# table(lib, op) of the library of the commit before the fold
RECORDED = {
    "deptree_expect": {
        'B < 0': (0x1001, 'deptree_expect: need B >= 0 and N >= 2 (got B=-1 N=8)'),
        'N = 1': (0x1001, 'deptree_expect: need B >= 0 and N >= 2 (got B=3 N=1)'),
        'N = 256': (0x1001, 'deptree_expect: N=256 exceeds the supported maximum of 255'),
        'bad in_dtype': (0x1002, 'deptree_expect: in_dtype 7'),
        'bad v_dtype': (0x1002, 'deptree_expect: v_dtype 7'),
        'bad in_dtype and v_dtype': (0x1002, 'deptree_expect: in_dtype 7'),
        'bad v_dtype, null potentials': (0x1002, 'deptree_expect: v_dtype 7'),
        'null potentials': (0x1003, 'deptree_expect: null buffer (arc and logZ are required)'),
        'null logZ': (0x1003, 'deptree_expect: null buffer (arc and logZ are required)'),
        'one byte short, grad=0 N=101': (0x1004, 'deptree_expect: N=101 needs a 249696-byte workspace (got 249695); see vlg_workspace_bytes'),
        'null workspace, grad=0 N=101': (0x1004, 'deptree_expect: N=101 needs a 249696-byte workspace (got 249696); see vlg_workspace_bytes'),
        'null lengths, grad=0 N=101': (0x1004, 'deptree_expect: N=101 needs a 249696-byte workspace (got 0); see vlg_workspace_bytes'),
        'null logZ before the workspace, grad=0 N=101': (0x1003, 'deptree_expect: null buffer (arc and logZ are required)'),
        'one byte short, grad=1 N=58': (0x1004, 'deptree_expect: N=58 needs a 246528-byte workspace (got 246527); see vlg_workspace_bytes'),
        'null workspace, grad=1 N=58': (0x1004, 'deptree_expect: N=58 needs a 246528-byte workspace (got 246528); see vlg_workspace_bytes'),
        'null lengths, grad=1 N=58': (0x1004, 'deptree_expect: N=58 needs a 246528-byte workspace (got 0); see vlg_workspace_bytes'),
        'null logZ before the workspace, grad=1 N=58': (0x1003, 'deptree_expect: null buffer (arc and logZ are required)'),
    },
    "dmv1o_expect": {
        'B < 0': (0x1001, 'dmv1o_expect: need B >= 0 and N >= 2 (got B=-1 N=8)'),
        'N = 1': (0x1001, 'dmv1o_expect: need B >= 0 and N >= 2 (got B=3 N=1)'),
        'N = 256': (0x1001, 'dmv1o_expect: N=256 exceeds the supported maximum of 255'),
        'bad in_dtype': (0x1002, 'dmv1o_expect: in_dtype 7'),
        'bad v_dtype': (0x1002, 'dmv1o_expect: v_dtype 7'),
        'bad in_dtype and v_dtype': (0x1002, 'dmv1o_expect: in_dtype 7'),
        'bad v_dtype, null potentials': (0x1002, 'dmv1o_expect: v_dtype 7'),
        'null potentials': (0x1003, 'dmv1o_expect: null buffer (dec, attach, lengths and logZ are required)'),
        'null logZ': (0x1003, 'dmv1o_expect: null buffer (dec, attach, lengths and logZ are required)'),
        'null attach': (0x1003, 'dmv1o_expect: null buffer (dec, attach, lengths and logZ are required)'),
        'null lengths': (0x1003, 'dmv1o_expect: null buffer (dec, attach, lengths and logZ are required)'),
        'one byte short, grad=0 N=71': (0x1004, 'dmv1o_expect: N=71 needs a 248832-byte workspace (got 248831); see vlg_workspace_bytes'),
        'null workspace, grad=0 N=71': (0x1004, 'dmv1o_expect: N=71 needs a 248832-byte workspace (got 248832); see vlg_workspace_bytes'),
        'null lengths, grad=0 N=71': (0x1003, 'dmv1o_expect: null buffer (dec, attach, lengths and logZ are required)'),
        'null logZ before the workspace, grad=0 N=71': (0x1003, 'dmv1o_expect: null buffer (dec, attach, lengths and logZ are required)'),
        'one byte short, grad=1 N=45': (0x1004, 'dmv1o_expect: N=45 needs a 253920-byte workspace (got 253919); see vlg_workspace_bytes'),
        'null workspace, grad=1 N=45': (0x1004, 'dmv1o_expect: N=45 needs a 253920-byte workspace (got 253920); see vlg_workspace_bytes'),
        'null lengths, grad=1 N=45': (0x1003, 'dmv1o_expect: null buffer (dec, attach, lengths and logZ are required)'),
        'null logZ before the workspace, grad=1 N=45': (0x1003, 'dmv1o_expect: null buffer (dec, attach, lengths and logZ are required)'),
    },
}


@pytest.mark.parametrize("op", sorted(RECORDED))
def test_refused_calls_keep_their_code_and_message(lib, op):
    got = table(lib, op)
    assert sorted(got) == sorted(RECORDED[op])
    for case, want in RECORDED[op].items():
        assert got[case] == want, (op, case, got[case], want)
    assert all(rc in (SHAPE, DTYPE, ARG, WORKSPACE) for rc, _ in got.values())


@pytest.mark.parametrize("f", (_deptree, _dmv1o))
def test_empty_batch_returns_before_any_pointer_check(lib, f):
    assert f(lib, B=0, pot=None, lengths=None, logZ=None) == 0
    assert f(lib, B=0, pot=None, lengths=None, logZ=None, N=255, grad=True, ws=None, ws_bytes=0) == 0   # nor is a workspace asked for
    assert f(lib, B=0, N=1) == SHAPE and f(lib, B=0, in_dtype=7) == DTYPE and f(lib, B=0, v_dtype=7) == DTYPE   # but behind shape and types
