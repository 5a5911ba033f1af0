"""The workspace vlg_workspace_bytes asks for is enough and is not overrun: every DP entry point that spills, called through the C ABI
with a workspace of exactly the queried size between two 4 KiB guard bands.

Each case runs at the smallest width at which its layout spills (the edge tables of test_dmv_placements_gpu.py and
test_deptree_placements_gpu.py):

  layout     Log inside-outside   Max walk   inside only
  DMV1o      N = 63               N = 77     N = 100
  DepTree    N = 83               N = 107    N = 143

B = 3 ragged sentences, the first of full length, float32 inputs.  Guards and workspace start as the byte 0xA5; afterwards both guards
must be intact and every output must equal, bit for bit, what the Python wrapper (vlgae_amd.torch_struct.functional, which owns its
workspace) returns for the same inputs -- so the kernels read nothing of the workspace that they did not write.

The rule-table entry runs at T = 5, so words share tokens and grad_rule / grad_root are sums of fp32 atomics (vlg_dp_core.h:
RuleIO::st_attach).  They are compared bit for bit like every other output: at this shape one workgroup's atomics arrive in one order
(200 launches of the Log-semiring gradient form gave one result on an MI355X); under the Max semiring the counts are sums of ones,
exact in any order.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD, FILL, B, T = 4096, 0xA5, 3, 5
SR_LOG, SR_MAX = 0, 1


def lengths_of(N):
    return torch.tensor([N - 1, 1, N // 2], dtype=torch.int64)


class Guarded:
    """`need` bytes between two guard bands, all 0xA5"""
    def __init__(self, need, dev):
        assert need > 0, "the case must spill"
        self.buf = torch.full((GUARD + need + GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.need = need
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + GUARD)

    def intact(self):
        return bool((self.buf[:GUARD] == FILL).all()) and bool((self.buf[GUARD + self.need:] == FILL).all())


def same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and torch.equal(g, w), k


def dmv_inputs(N, dev):
    g = torch.Generator().manual_seed(100 + N)
    dec = torch.randn(B, N, 2, 2, 2, generator=g).log_softmax(-1)
    return dec.to(dev), torch.randn(B, N, N, 2, generator=g).to(dev), lengths_of(N).to(dev)


def run_dmv(kind, N, dev, Fn, _C, L):
    dec, att, ln = dmv_inputs(N, dev)
    f32, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)
    z, gd, ga, heads = torch.empty(B, **f32), torch.empty(B, N, 2, 2, 2, **f32), torch.empty(B, N, N, 2, **f32), torch.empty(B, N, **i64)
    p, s = _C.ptr, _C.stream_of(dec)
    if kind == "log_inside_outside":
        ws = Guarded(L.vlg_workspace_bytes(_C.OP_DMV1O_INSIDE_OUTSIDE, B, N, SR_LOG), dev)
        _C.check(L.vlg_dmv1o_inside_outside(p(dec), p(att), p(ln), B, N, 0, SR_LOG, None, p(z), p(gd), p(ga), ws.ptr, ws.need, s), kind)
        same((z, gd, ga), Fn.dmv1o_run(dec, att, ln, SR_LOG, True))
    elif kind == "max_inside_outside":
        ws = Guarded(L.vlg_workspace_bytes(_C.OP_DMV1O_INSIDE_OUTSIDE, B, N, SR_MAX), dev)
        _C.check(L.vlg_dmv1o_inside_outside(p(dec), p(att), p(ln), B, N, 0, SR_MAX, None, p(z), p(gd), p(ga), ws.ptr, ws.need, s), kind)
        same((z, gd, ga), Fn.dmv1o_run(dec, att, ln, SR_MAX, True))
    elif kind == "viterbi":
        ws = Guarded(L.vlg_workspace_bytes(_C.OP_DMV1O_INSIDE_OUTSIDE, B, N, SR_MAX), dev)
        _C.check(L.vlg_dmv1o_viterbi(p(dec), p(att), p(ln), B, N, 0, None, p(z), p(gd), p(ga), p(heads), ws.ptr, ws.need, s), kind)
        same((z, gd, ga, heads), Fn.dmv1o_viterbi(dec, att, ln))
    elif kind == "decode":
        ws = Guarded(L.vlg_workspace_bytes(_C.OP_DMV1O_INSIDE_OUTSIDE, B, N, SR_MAX), dev)
        _C.check(L.vlg_dmv1o_decode(p(dec), p(att), p(ln), B, N, 0, p(z), p(heads), ws.ptr, ws.need, s), kind)
        same((z, heads), Fn.dmv1o_decode(dec, att, ln))
    else:
        sr = SR_LOG if kind == "log_inside" else SR_MAX
        ws = Guarded(L.vlg_workspace_bytes(_C.OP_DMV1O_INSIDE, B, N, sr), dev)
        _C.check(L.vlg_dmv1o_inside(p(dec), p(att), p(ln), B, N, 0, sr, p(z), ws.ptr, ws.need, s), kind)
        same((z,), Fn.dmv1o_run(dec, att, ln, sr, False)[:1])
    return ws


def run_rules(kind, N, dev, Fn, _C, L):
    Lw = N - 1
    g = torch.Generator().manual_seed(200 + N)
    rule = torch.randn(B, Lw, T, 2, 2, generator=g).to(dev)
    dec = torch.randn(B, Lw, 2, 2, 2, generator=g).log_softmax(-1).to(dev)
    root = torch.randn(T, generator=g).log_softmax(-1).to(dev)
    token = torch.randint(0, T, (B, Lw), generator=g).to(dev)
    ln = lengths_of(N).to(dev)
    sr = SR_LOG if kind.startswith("log") else SR_MAX
    grads, heads = kind.endswith("gradients"), kind.endswith("heads")
    f32 = dict(dtype=torch.float32, device=dev)
    z = torch.empty(B, **f32)
    gr, gd, g0 = (torch.empty(B, Lw, T, 2, 2, **f32), torch.empty(B, Lw, 2, 2, 2, **f32), torch.empty(B, T, **f32)) if grads else (None, None, None)
    h = torch.empty(B, N, dtype=torch.int64, device=dev) if heads else None
    op = _C.OP_DMV1O_INSIDE_OUTSIDE if grads or heads else _C.OP_DMV1O_INSIDE
    ws = Guarded(L.vlg_workspace_bytes(op, B, N, sr), dev)
    p = _C.ptr
    _C.check(L.vlg_dmv1o_rules(p(rule), p(dec), p(root), 0, p(token), None, p(ln), B, Lw, T, 0, sr, -1e20, None, p(z), p(gr), p(gd), p(g0), p(h),
                               ws.ptr, ws.need, _C.stream_of(rule)), kind)
    want = Fn.dmv1o_rules_run(rule, dec, root, token, ln, sr, grads, want_heads=heads)
    got = dict(logZ=z, grad_rule=gr, grad_dec=gd, grad_root=g0, heads=h)
    assert sorted(want) == sorted(k for k, v in got.items() if v is not None)
    same([got[k] for k in sorted(want)], [want[k] for k in sorted(want)])
    return ws


def run_dep(kind, N, dev, Fn, _C, L):
    g = torch.Generator().manual_seed(300 + N)
    arc = torch.randn(B, N, N, generator=g).to(dev)
    ln = lengths_of(N).to(dev)
    f32, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)
    z, garc, heads = torch.empty(B, **f32), torch.empty(B, N, N, **f32), torch.empty(B, N, **i64)
    p, s = _C.ptr, _C.stream_of(arc)
    if kind in ("log_inside_outside", "max_inside_outside"):
        sr = SR_LOG if kind.startswith("log") else SR_MAX
        ws = Guarded(L.vlg_workspace_bytes(_C.OP_DEPTREE_INSIDE_OUTSIDE, B, N, sr), dev)
        _C.check(L.vlg_deptree_inside_outside(p(arc), p(ln), B, N, 0, sr, None, p(z), p(garc), ws.ptr, ws.need, s), kind)
        same((z, garc), Fn.deptree_run(arc, ln, sr, True))
    elif kind == "decode":
        ws = Guarded(L.vlg_workspace_bytes(_C.OP_DEPTREE_INSIDE_OUTSIDE, B, N, SR_MAX), dev)
        _C.check(L.vlg_deptree_decode(p(arc), p(ln), B, N, 0, p(z), p(heads), ws.ptr, ws.need, s), kind)
        same((z, heads), Fn.deptree_decode(arc, ln))
    elif kind == "mbr_decode":
        marg = torch.rand(B, N, N, 2, generator=g).to(dev)
        ws = Guarded(L.vlg_workspace_bytes(_C.OP_DEPTREE_INSIDE_OUTSIDE, B, N, SR_MAX), dev)
        _C.check(L.vlg_deptree_mbr_decode(p(marg), p(ln), B, N, p(z), p(heads), ws.ptr, ws.need, s), kind)
        same((z, heads), Fn.deptree_mbr_decode(marg, ln))
    elif kind == "sample":
        S = 2
        u = torch.rand(S, B, 3, N, N, generator=g).to(dev)
        hs, logp = torch.empty(S, B, N, **i64), torch.empty(S, B, **f32)
        Y = L.vlg_deptree_sample_blocks(B, N, S)
        ws = Guarded(L.vlg_workspace_bytes(_C.OP_DEPTREE_INSIDE, B * Y, N, SR_LOG), dev)
        _C.check(L.vlg_deptree_sample(p(arc), p(ln), B, N, 0, S, None, 0, p(u), p(hs), p(logp), p(z), ws.ptr, ws.need, s), kind)
        same((hs, logp, z), Fn.deptree_sample(arc, ln, S, u=u))
    else:
        sr = SR_LOG if kind == "log_inside" else SR_MAX
        ws = Guarded(L.vlg_workspace_bytes(_C.OP_DEPTREE_INSIDE, B, N, sr), dev)
        _C.check(L.vlg_deptree_inside(p(arc), p(ln), B, N, 0, sr, p(z), ws.ptr, ws.need, s), kind)
        same((z,), Fn.deptree_run(arc, ln, sr, False)[:1])
    return ws


CASES = [(run_dmv, "log_inside_outside", 63), (run_dmv, "max_inside_outside", 77), (run_dmv, "viterbi", 77), (run_dmv, "decode", 77),
         (run_dmv, "log_inside", 100), (run_dmv, "max_inside", 100),
         (run_rules, "log_gradients", 63), (run_rules, "max_gradients", 77), (run_rules, "max_heads", 77), (run_rules, "log_inside", 100),
         (run_dep, "log_inside_outside", 83), (run_dep, "max_inside_outside", 107), (run_dep, "decode", 107), (run_dep, "mbr_decode", 107),
         (run_dep, "log_inside", 143), (run_dep, "max_inside", 143), (run_dep, "sample", 143)]


@pytest.mark.parametrize("run,kind,N", CASES, ids=[f"{r.__name__[4:]}_{k}_N{n}" for r, k, n in CASES])
def test_queried_workspace_is_enough_and_not_overrun(run, kind, N):
    from vlgae_amd import _C
    from vlgae_amd.torch_struct import functional as Fn
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    dev = torch.device("cuda:0")
    ws = run(kind, N, dev, Fn, _C, _C.lib())
    torch.cuda.synchronize()
    assert ws.intact(), (kind, N)
