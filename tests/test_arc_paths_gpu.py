"""The arc encoder's trilinear contraction (vlgae_amd/csrc/vlg_arc.hip) at every route, split plan and row boundary, through the C ABI
(vlg_trilinear, vlg_trilinear_ws, vlg_trilinear_backward, vlg_trilinear_backward_g), against a float64 reference.  The case table, the
restated dispatch and the inputs come from tests/test_arc_paths.py, which pins every case to the route its id names; here the route of each
case is re-derived under the device's own CU count before it runs, so a case never silently runs another kernel.

Exact set (CASES).  child, parent, w and g are integers in [-4, 4] / 4: every output of every route must EQUAL float32 of the float64
reference bit for bit (tests/test_arc_paths.py asserts the bound on the partial sums from the shapes).  The reference is the C oracle
(oracle.cpu_oracle.arc_encoder / arc_encoder_backward, float64) for M <= 4096 and float64 torch on the device in row chunks of 2048 above
(einsum('mx,xhy->mhy') then einsum('mhy,my->mh'); the three adjoints through autograd): the rows of the table with M = lo / hi (the
RT-targeting rows: M in 6145 .. 24576), M = 10496, 18945, 26113 and 43521 use the device reference, every other row the oracle.

Guards.  The C ABI is called directly so that the test owns every buffer.  Every operand, every output and the workspace sit between NaN
bands of 64 elements; the operands with their bands are compared with a copy taken before the call; output regions are prefilled with 3e38
and the workspace interior with NaN, so a row or slab that a kernel reads but no earlier launch of the same call wrote (the Mp - M padding
rows of the transposed copies, the partial slab of an empty row chunk, the per-workgroup maxima) reaches an output as NaN.  Every call is
made a second time into fresh outputs with the workspace prefilled with zeros: the same bits, the atomic two-range forms included.

Rounding set (ROUNDING).  One case per kernel image on normal(0, 0.5) features, w / sqrt(X Y), rounded to bf16 for the bf16 images (the
cotangent too, as the product hands it over); the fp16-parts images on the magnitude-spread inputs of
test_arc_trilinear_float32_on_fp16_parts.  |got - ref64| <= max(tol max(1, |ref|max), 4 e32) with tol = 1e-4 (2e-6, and 1e-5 of every row's
own largest entry for the row-wise results, on the fp16-parts images) and e32 the float32 C oracle's own error against float64 on the same
inputs; it is computed for the forward cases up to M = 4096 and for the backward ones where M X H Y <= 5e8 (the oracle's cost); elsewhere
(the RT 6 / RT 4 rows and the float32 backward at 128^3) the first term stands alone, which only tightens the bound.  d_w of the bf16
images gets one more term: tri_dw_kernel and tri_dw2_kernel round the A operand c[m,x] g[m,h] to bf16 by design (unit roundoff 2^-9), so
each element is allowed 2^-9 sum_m |c g p| on top -- from the number format, not from the kernels' output.
Measured e32 on the CPU (largest over the elements of each output; `of top`: relative to |ref|max; ratio: 4 e32 / first term):
  case                                                   output     e32        of top     first term   ratio
  tk bf16 M 100 X 33 H 48 Y 32 | 64 | 128                out        1.7e-07 | 2.5e-07 | 2.2e-07  (2e-07)   1.0e-04 .. 1.1e-04   0.006 .. 0.009
  tk f32  M 100 X 33 H 48 Y 32 | 64 | 128                out        2.4e-07 | 2.5e-07 | 4.1e-07  (4e-07)   1.0e-04 .. 1.1e-04   0.009 .. 0.016
  t2s / t2a bf16 (1025, 65, 128, 128)                    out        3.2e-07    2.7e-07    1.2e-04      0.011
  t3 f32 spread (1025, 81, 128, 128)                     out        2.3e+01    3.6e-07    1.3e+02      0.73
  backward bf16 (1025, 16, 128, 128)                     d_child    3.0e-06    5.4e-07    5.5e-04      0.022
                                                         d_w        6.1e-05    1.7e-06    3.7e-03      0.067
                                                         d_parent   1.2e-06    4.3e-07    2.7e-04      0.017
  backward bf16 (100, 48, 64, 128)                       d_child    4.7e-07    1.9e-07    2.5e-04      0.008
                                                         d_w        6.6e-06    4.5e-07    1.5e-03      0.018
                                                         d_parent   4.9e-07    3.3e-07    1.5e-04      0.013
  backward f32 (100, 48, 64, 128)                        d_child    7.2e-07    2.9e-07    2.5e-04      0.012
                                                         d_w        6.1e-06    4.2e-07    1.5e-03      0.017
                                                         d_parent   4.1e-07    2.7e-07    1.5e-04      0.011
  backward f32 spread (1025, 128, 128, 128)              d_child    4.0e-03    3.1e-07    2.6e-02      0.62
                                                         d_w        4.3e-01    6.1e-07    1.4e+00      1.22
                                                         d_parent   3.7e-03    3.1e-07    2.4e-02      0.62
The first term decides wherever e32 is used.  On d_w of the float32 backward on the magnitude-spread inputs 4 e32 would be 1.22 x the first
term (the sequential float32 oracle itself is 6.1e-7 of |ref|max away from float64 there: 1025 terms over 2^24 of magnitudes); that case is
one of those held to the first term alone, 2e-6 of |ref|max.
"""
import functools

import numpy as np
import pytest
import torch

from test_arc_paths import (BF16, CASES, ERR_SHAPE, F32, ORACLE_MAX_M, ROUNDING, case_id, derive, exact_inputs, input_key, oracle_reference, resolve_m,
                            rounding_inputs)

pytestmark = pytest.mark.gpu

NAN = float("nan")
G = 64                    # guard elements on each side of every buffer
STALE = 3e38              # prefill of the region an output is written to
OUT_NAMES = dict(c="d_child", w="d_w", p="d_parent")


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from vlgae_amd import _C
    return _C.lib()   # must load: the product has no fallback


@functools.lru_cache(maxsize=1)
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def same_bits(a, b):
    bits = {torch.float32: torch.int32, torch.bfloat16: torch.int16}[a.dtype]
    return torch.equal(a.view(bits), b.view(bits))


# ---------------------------------------------------------------------------------------------------------------- guarded buffers
def guarded_operand(vals, dtype):
    """(whole buffer, the operand inside it, a copy of the whole buffer)"""
    t = torch.from_numpy(np.ascontiguousarray(vals)).reshape(-1)
    flat = torch.full((t.numel() + 2 * G,), NAN, dtype=dtype, device=dev())
    inner = flat[G:G + t.numel()]
    inner.copy_(t.to(dtype))
    assert inner.data_ptr() % 16 == 0 and torch.equal(inner.double().cpu(), t)      # the values are exact in the operand type
    return flat, inner, flat.clone()


def guarded_region(n, fill):
    flat = torch.full((n + 2 * G,), NAN, dtype=torch.float32, device=dev())
    inner = flat[G:G + n]
    inner.fill_(fill)
    assert inner.data_ptr() % 256 == 0
    return flat, inner


def guards_intact(flat, n):
    return bool(torch.isnan(flat[:G]).all()) and bool(torch.isnan(flat[G + n:]).all())


def out_shapes(c, M):
    if c.op == "fwd":
        return dict(out=(M, c.H))
    return {OUT_NAMES[o]: s for o, s in (("c", (M, c.X)), ("w", (c.X, c.H, c.Y)), ("p", (M, c.Y))) if o in c.want}


def operands(c, inputs):
    fdt = torch.bfloat16 if c.dt == "bf16" else torch.float32
    child, parent, w, g = inputs
    ops = dict(child=guarded_operand(child, fdt), w=guarded_operand(w, fdt), parent=guarded_operand(parent, fdt))
    if c.op == "bwd":
        ops["g"] = guarded_operand(g, torch.bfloat16 if c.entry == "g16" else torch.float32)
    return ops


def call(lib, c, M, ops, ws_fill, entry=None, g=None):
    """one call into fresh guarded outputs and a fresh guarded workspace; returns (rc, {name: (flat, inner)})"""
    from vlgae_amd import _C
    entry = entry or c.entry
    code = F32 if c.dt == "f32" else BF16
    outs = {name: guarded_region(int(np.prod(s)), STALE) for name, s in out_shapes(c, M).items()}
    ptr = lambda k: _C.ptr(ops[k][1])
    st = _C.stream_of(ops["child"][1])
    if c.op == "fwd":
        need = lib.vlg_trilinear_workspace(M, c.X, c.H, c.Y, code) if entry == "ws" else 0
    else:
        need = lib.vlg_trilinear_backward_workspace(M, c.X, c.H, c.Y, code)
    assert need % 4 == 0
    ws = guarded_region(need // 4, ws_fill) if need else None
    if c.op == "fwd" and entry == "nows":
        rc = lib.vlg_trilinear(ptr("child"), ptr("w"), ptr("parent"), M, c.X, c.H, c.Y, code, _C.ptr(outs["out"][1]), st)
    elif c.op == "fwd":
        rc = lib.vlg_trilinear_ws(ptr("child"), ptr("w"), ptr("parent"), M, c.X, c.H, c.Y, code, _C.ptr(ws[1]) if ws else None, need, _C.ptr(outs["out"][1]), st)
    else:
        gop = g if g is not None else ops["g"]
        o = lambda name: _C.ptr(outs[name][1]) if name in outs else None
        rc = lib.vlg_trilinear_backward_g(ptr("child"), ptr("w"), ptr("parent"), _C.ptr(gop[1]), BF16 if gop[1].dtype == torch.bfloat16 else F32, M, c.X, c.H, c.Y,
                                          code, _C.ptr(ws[1]), need, o("d_child"), o("d_w"), o("d_parent"), st)
    torch.cuda.synchronize()
    tag = case_id(c)
    for name, (flat, inner) in outs.items():
        assert guards_intact(flat, inner.numel()), f"{tag}: a guard element of {name} was written"
    assert ws is None or guards_intact(ws[0], need // 4), f"{tag}: a guard element of the workspace was written"
    return rc, outs


def check_operands(tag, ops, extra=()):
    for name, (flat, _, before) in list(ops.items()) + list(extra):
        assert same_bits(flat, before), f"{tag}: operand {name} or its guard changed"


# ---------------------------------------------------------------------------------------------------------------- references
def device_reference(inputs, want):
    """float64 torch on the device in row chunks of 2048: {name: float64 tensor}"""
    child, parent, w, g = (torch.from_numpy(a).to(dev()) for a in inputs)
    M = child.shape[0]
    if want == "":
        out = torch.empty(M, w.shape[1], dtype=torch.float64, device=dev())
        for m0 in range(0, M, 2048):
            out[m0:m0 + 2048] = torch.einsum("mhy,my->mh", torch.einsum("mx,xhy->mhy", child[m0:m0 + 2048], w), parent[m0:m0 + 2048])
        return dict(out=out)
    d_child, d_parent, d_w = torch.empty_like(child), torch.empty_like(parent), torch.zeros_like(w)
    for m0 in range(0, M, 2048):
        c_, p_, w_ = child[m0:m0 + 2048].clone().requires_grad_(True), parent[m0:m0 + 2048].clone().requires_grad_(True), w.clone().requires_grad_(True)
        t = torch.einsum("mhy,my->mh", torch.einsum("mx,xhy->mhy", c_, w_), p_)
        gc, gw, gp = torch.autograd.grad(t, [c_, w_, p_], g[m0:m0 + 2048])
        d_child[m0:m0 + 2048], d_parent[m0:m0 + 2048] = gc, gp
        d_w += gw
    return dict(d_child=d_child, d_w=d_w, d_parent=d_parent)


def reference64(inputs, want):
    """{name: float64 tensor on the device}: the C oracle up to M = 4096, the device above"""
    if inputs[0].shape[0] > ORACLE_MAX_M:
        return device_reference(inputs, want)
    import oracle
    oracle.build()
    return {k: torch.from_numpy(v).to(dev()) for k, v in oracle_reference(oracle, inputs, want, np.float64).items()}


@functools.lru_cache(maxsize=12)     # the cases of one shape (subsets, entries, dtypes: the exact inputs do not depend on the type) follow each other
def exact_reference(key, bwd):
    return {k: v.float() for k, v in reference64(exact_inputs(key), "cwp" if bwd else "").items()}


def check_exact(tag, name, got, want):
    got, want = got.reshape(want.shape), want.contiguous()
    bad = got.view(torch.int32) != want.view(torch.int32)
    if bool(bad.any()):
        at = tuple(int(i) for i in bad.nonzero()[0])
        rows = sorted({int(i) for i in bad.nonzero()[:, 0][:4096].tolist()})
        raise AssertionError(f"{tag}: {name} differs from the float64 reference in {int(bad.sum())} of {bad.numel()} elements ({int(torch.isnan(got).sum())} NaN, "
                             f"{int((got == STALE).sum())} never written); first at {at}: got {float(got[at])!r}, want {float(want[at])!r}; first index in {rows[:12]} .. {rows[-1]}")


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_exact_operands_every_route(lib, c):
    """Every case of the table: the restated route under the device's CU count is the one the id names; every requested output equals float32
    of the float64 reference bit for bit; guards stay NaN, nothing is left unwritten, no stale workspace element reaches an output, operands
    are untouched, a second call (workspace prefilled with zeros instead of NaN) gives the same bits.  A bf16 cotangent gives the bits of the
    float32 cotangent.  Where d_child is refused (X not a multiple of 16 up to 128) the call returns VLG_ERR_SHAPE with its message."""
    tag = case_id(c)
    assert derive(c, cus()) == c.claim, (tag, cus(), derive(c, cus()))
    M = resolve_m(c, cus())
    key = input_key(c, cus())
    print(f"[arc] {tag}: M = {M}, {cus()} CUs")
    ops = operands(c, exact_inputs(key))
    if c.claim.startswith("err"):
        rc, _ = call(lib, c, M, ops, NAN)
        assert rc == ERR_SHAPE and f"trilinear_backward: X={c.X} must be a multiple of 16 and <= 128".encode() in lib.vlg_last_error(), (rc, lib.vlg_last_error())
        check_operands(tag, ops)
        return
    ref = exact_reference(key, c.op == "bwd")
    rc, first = call(lib, c, M, ops, NAN)
    assert rc == 0, (tag, rc, lib.vlg_last_error())
    for name, (_, inner) in first.items():
        check_exact(tag, name, inner, ref[name])
    rc, again = call(lib, c, M, ops, 0.0)
    assert rc == 0
    for name in first:
        assert same_bits(first[name][0], again[name][0]), f"{tag}: {name} differs between two calls"
    extra = []
    if c.entry == "g16":      # the float32-cotangent entry on the same (bf16-exact) cotangent: the same bits
        g32 = guarded_operand(exact_inputs(key)[3], torch.float32)
        rc, other = call(lib, c, M, ops, NAN, g=g32)
        assert rc == 0
        for name in first:
            assert same_bits(first[name][0], other[name][0]), f"{tag}: {name} differs between the bf16 and the float32 cotangent"
        extra = [("g32", g32)]
    check_operands(tag, ops, extra)


@pytest.mark.parametrize("c", ROUNDING, ids=[case_id(c) for c in ROUNDING])
def test_rounding_data(lib, c):
    """One case per kernel image on rounding inputs: |got - ref64| <= max(tol max(1, |ref|max), 4 e32) (+ 2^-9 sum_m |c g p| per element for d_w
    of the bf16 images); the fp16-parts images: tol = 2e-6 and every row of the row-wise results within 1e-5 of its own largest entry."""
    tag = case_id(c)
    assert derive(c, cus()) == c.claim, (tag, cus(), derive(c, cus()))
    M = resolve_m(c, cus())
    inputs = rounding_inputs(c, cus())
    ref = reference64(inputs, "cwp" if c.op == "bwd" else "")
    r32 = None
    if M <= ORACLE_MAX_M and (c.op == "fwd" or M * c.X * c.H * c.Y <= 5e8):
        import oracle
        r32 = oracle_reference(oracle, inputs, "cwp" if c.op == "bwd" else "", np.float32)
    ops = operands(c, inputs)
    rc, outs = call(lib, c, M, ops, NAN)
    assert rc == 0, (tag, rc, lib.vlg_last_error())
    spread = c.side == "spread"
    tol = 2e-6 if spread else 1e-4
    for name, (_, inner) in outs.items():
        r = ref[name]
        got = inner.reshape(r.shape).double()
        top = float(r.abs().max())
        e32 = float((torch.from_numpy(r32[name].astype(np.float64)).to(dev()) - r).abs().max()) if r32 is not None else 0.0
        first = tol * (top if spread else max(1.0, top))
        bound = torch.full_like(r, max(first, 4 * e32))
        if c.dt == "bf16" and name == "d_w":
            ch, pa, _, g = (torch.from_numpy(np.abs(a)).to(dev()) for a in inputs)
            bound = bound + 2.0 ** -9 * torch.einsum("mx,mh,my->xhy", ch, g, pa)
        err = (got - r).abs()
        print(f"[arc] rounding {tag} {name}: err {float(err.max()):.3e} ({float(err.max()) / top:.3e} of |ref|max {top:.3e}), e32 {e32:.3e} ({e32 / top:.3e}), "
              f"first term {first:.3e}, largest allowed {float(bound.max()):.3e}, err / allowed {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (tag, name, float(err.max()), float((err / bound).max()))
        if spread and name != "d_w":
            rel = float((err.amax(1) / r.abs().amax(1).clamp_min(1e-300)).max())
            print(f"[arc] rounding {tag} {name}: row-wise {rel:.3e}")
            assert rel <= 1e-5, (tag, name, rel)
    check_operands(tag, ops)
