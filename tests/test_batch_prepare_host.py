"""CPU: the C-ABI entries of the batch-on-device training step (vlg_step_batch_prepare, vlg_grounding_loss_ntok) validate their arguments
on the host, before any HIP call, and the Python wrapper refuses buffers the launch would overrun."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from vlgae_amd.build import build_library
    build_library()
    from vlgae_amd import _C
    return _C.lib()


def test_abi_version(lib):
    from vlgae_amd import _C
    assert lib.vlg_version() == 145 == _C.ABI_VERSION


def test_batch_prepare_validates_on_the_host(lib):
    one = ctypes.c_void_p(64)
    prep = lib.vlg_step_batch_prepare
    args = lambda **kw: [kw.get("lengths", one), kw.get("tag", one), one, kw.get("B", 2), kw.get("L", 5), kw.get("R", 3), kw.get("Q", 12), 1, 1, 1,
                         kw.get("pobj", one), kw.get("nobj", 3), one, 2, one, 1, 100.0, 0.5, kw.get("vmask", one), kw.get("pen", one), one, one,
                         one, None]
    assert prep(*args(B=0)) == 0                                              # empty batch: nothing to do
    assert prep(*args(B=-1)) == 0x1001
    assert prep(*args(L=0)) == 0x1001 and prep(*args(R=0)) == 0x1001 and prep(*args(R=5000)) == 0x1001
    assert prep(*args(Q=5)) == 0x1001 and b"L + 1" in lib.vlg_last_error()   # the prior table needs rows 1..L
    assert prep(*args(lengths=None)) == 0x1003 and prep(*args(vmask=None)) == 0x1003
    assert prep(*args(tag=None)) == 0x1003 and b"tags" in lib.vlg_last_error()
    assert prep(*args(pobj=None)) == 0x1003 and b"POS" in lib.vlg_last_error()
    assert prep(*args(nobj=-1)) == 0x1003


def test_grounding_loss_ntok_validates_on_the_host(lib):
    one = ctypes.c_void_p(64)
    gl = lib.vlg_grounding_loss_ntok
    need = lib.vlg_grounding_loss_workspace(3, 14, 9)
    a = lambda **kw: [kw.get("txt", one), one, None, None, one, kw.get("pen", None), None, 0, 3, 14, 9, kw.get("d", 32), kw.get("dt", 0), -1e20,
                      kw.get("nt", one), 1.0, one, kw.get("ws", need), one, None, None, None]
    assert gl(*a(nt=None)) == 0x1003 and b"num_token" in lib.vlg_last_error()
    assert gl(*a(d=48)) == 0x1001 and b"d=48" in lib.vlg_last_error()
    assert gl(*a(dt=3)) == 0x1002 and gl(*a(txt=None)) == 0x1003
    assert gl(*a(pen=one)) == 0x1003 and b"segments" in lib.vlg_last_error()
    assert gl(*a(ws=need - 1)) == 0x1004


def test_wrapper_refuses_mismatched_buffers():
    """align.step_batch_prepare checks every buffer's shape / type before the launch (CPU tensors: the checks come first)."""
    from vlgae_amd import align
    B, L, R = 3, 4, 2
    ok = dict(lengths=torch.ones(B, dtype=torch.int64), tag=torch.zeros(B, L, dtype=torch.int64), box_mask=torch.ones(B, R, dtype=torch.bool),
              factors=("rel", "attr", "img"), pos_for={}, Q=2 * (L + 1), alpha=0.5, vmask=torch.empty(B, R + R * R + R + 1, dtype=torch.bool),
              pen=torch.empty(B, 2 * (L + 1), 4), num_token=torch.empty(()), coef=torch.empty(2), seed_max=torch.empty(B))
    for k, v in (("vmask", torch.empty(B, R + R * R + R, dtype=torch.bool)), ("pen", torch.empty(B, 2 * (L + 1), 3)), ("seed_max", torch.empty(B + 1)),
                 ("coef", torch.empty(3)), ("num_token", torch.empty(1)), ("lengths", torch.ones(B, dtype=torch.int32)),
                 ("box_mask", torch.ones(B + 1, R, dtype=torch.bool)), ("tag", torch.zeros(B, L)), ("Q", L),
                 ("pos_for", {"obj": torch.tensor([1], dtype=torch.int32)})):
        with pytest.raises(ValueError):
            align.step_batch_prepare(**dict(ok, **{k: v}))
    # the consistent set passes every check and stops only at the device requirement (host tensors never reach the launch)
    with pytest.raises(RuntimeError, match="MI355X"):
        align.step_batch_prepare(**ok)
    with pytest.raises(RuntimeError, match="MI355X"):
        align.step_batch_prepare(**dict(ok, pen=None, pos_for={"obj": torch.tensor([0, 1])}))
