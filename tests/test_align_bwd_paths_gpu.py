"""vlg_bilinear_align_backward (vlgae_amd/csrc/vlg_align.hip) at every route, kernel image and split plan, through the C ABI, against the
float64 oracle.  The case table, the restated dispatch (plan) and the inputs come from tests/test_align_bwd_paths.py, which pins each case
to the routes, images, split plans and boundary numbers its id and claim name:

  route      kernel                                   boundaries the table sits on
  concat2    align_bwd_split2_kernel<MT, CW, NT, NF>  V = 4 .. 48 beside 3, 5, 52; Q around 16 and 48, 96; A = 1, 2, 3 (lone last pair), 15 .. 19
                                                      (split, even opb, second block odd / even); the clamped look-ahead tile at an 8-byte
                                                      offset; B = 1, 63 | 64 | 65 (NF, mirrored wave set), 1024 | 1025 (unsplit)
  split_kc   align_bwd_split(_f32)_kernel<true, ..>   every (NKC, MT x CW, NF, bf16 | f32) with both k_quads branches where reachable; rows and
  split_kn   align_bwd_split(_f32)_kernel<false, ..>  contraction 1 .. 96 around 16, 32, 48, 64; O = 1, 2, 3, 15 | 16 | 17; fixn 1, 2, 63 | 64 | 65,
                                                      512 | 513 (f32), 1024 | 1025 (bf16)
  generic    align_bwd_kernel<In, NCT, NS>            every (dt, NCT, NS); K to 193 (nck 1, 2, 3); M to 97 (idle waves, gx 1 -> 2); 1 .. 5 iterations
                                                      per block; O = 31 | 32 | 33; gx fixn = 767 | 768

Exact operands.  Every product and every partial sum in any order is exact in float32 on the g2 / x2 data sets (the CPU file asserts the
conditions per case, and that the float32 sequential oracle equals the float64 one), so every output must EQUAL float32 of the float64
oracle.  The comparison is by value: the sign of a zero is not part of the contract (a masked row may be -0.0); NaN never matches.
Cotangent positions a mask removes carry finite poison of 2^20 and more, so a leaked term is an error of 2^17 or more.

Guards.  The C ABI is called directly so that the test owns every buffer.  Cotangent, features (NaN bands) and masks (zero bands) sit
between 64-element bands and are compared with a copy after the call.  Outputs sit between NaN bands and are prefilled with NaN: a skipped
zeroing before the two-addend atomics stays NaN.  The workspace is exactly the queried bytes between NaN bands, prefilled with bf16 NaN:
a scratch position read but never written (transposed padding past K, the 96 pad columns of featC, the lo array) reaches the output as
NaN, and the bands must be untouched.  Every call is repeated into fresh buffers with a fresh NaN workspace (same bits); every fourth
case a third time with the workspace prefilled with a large finite pattern.

Rounding set.  One case per route x dtype on normal(0, 0.5) data, both masks random.  Generic images (exact float32 products):
|got - ref64| <= max(2e-5 max(1, |ref|max), 4 e32), e32 the float32 oracle's own largest error against float64 on the same inputs.
Split-term images drop terms by design (two cotangent terms kept; g_lo x_lo dropped for float32 features; below 2^-16 per product by
the header): every element is bound by 2^-16 S + 4 e32, S the same masked contraction of |g| |x| in float64.  Measured on an MI355X
(largest err / bound over the elements of each output):
  case (B 4, A 5)             side       route     err       e32       err / bound
  bf16 d128 Q82 V36           grad_txt   concat2   4.6e-05   6.2e-06   0.108
                              grad_vis   split_kn  4.9e-05   9.2e-06   0.075
  bf16 d128 Q82 V37           grad_txt   split_kc  3.5e-05   6.4e-06   0.090
                              grad_vis   split_kn  4.7e-05   9.8e-06   0.070
  f32  d128 Q82 V36           grad_txt   split_kc  6.8e-05   5.9e-06   0.168
                              grad_vis   split_kn  7.5e-05   1.1e-05   0.111
  bf16 d128 Q100 V36          both       generic   1.2e-05   1.3e-05   0.033
  f32  d128 Q100 V36          both       generic   1.1e-05   1.1e-05   0.029
  bf16 d64  Q82 V36           both       generic   8.4e-06   9.4e-06   0.026
  f32  d32  Q82 V36           both       generic   8.6e-06   9.5e-06   0.030
so the split-term images use a tenth to a sixth of their bound and the generic ones err no more than the float32 oracle itself.
Masked rows are zero by value.

Wall time of this file on an MI355X: 6 s for the 657 tests (644 exact cases; 9 ms a case, oracle included).
"""
import functools

import numpy as np
import pytest
import torch

from test_align_bwd_paths import ALIGNMENT, CASES, PYTHON, ROUNDING, case_id, derive, exact_inputs, input_key, plan, rounding_inputs

pytestmark = pytest.mark.gpu

NAN = float("nan")
G = 64                        # guard elements on each side of every buffer
WS_NAN = 0x7FC1               # bf16 NaN: the workspace prefill, as the 16-bit words the kernels read
WS_OTHER = 0x4F00             # 2^31 as bf16: the other pattern
SIDES = (("t", "grad_txt"), ("v", "grad_vis"))


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from vlgae_amd import _C
    return _C.lib()   # must load: the product has no fallback


def shapes(c):
    return dict(t=(c.B, c.Q, c.d), v=(c.A, c.V, c.d))


# ---------------------------------------------------------------------------------------------------------------- guarded buffers
def guarded_operand(vals, dtype, shift=0):
    """(whole buffer, the operand inside it, a copy of the whole buffer): NaN bands for floats, zero bands for masks; `shift` elements move
    the operand inside its allocation"""
    if vals is None:
        return None, None, None
    t = torch.from_numpy(np.ascontiguousarray(vals)).reshape(-1)
    flat = torch.full((t.numel() + 2 * G + 8,), 0 if dtype == torch.uint8 else NAN, dtype=dtype, device=dev())
    inner = flat[G + shift:G + shift + t.numel()]
    inner.copy_(t.to(dtype))
    assert (inner.data_ptr() - shift * flat.element_size()) % 16 == 0
    return flat, inner, flat.clone()


def guarded_outputs(c):
    """{side: (whole buffer, written region)}, everything NaN"""
    out = {}
    for k in c.want:
        n = int(np.prod(shapes(c)[k]))
        flat = torch.full((n + 2 * G,), NAN, dtype=torch.float32, device=dev())
        out[k] = (flat, flat[G:G + n])
        assert out[k][1].data_ptr() % 128 == 0
    return out


def guarded_workspace(nbytes, fill):
    """(whole buffer, the queried bytes inside it) as 16-bit words"""
    assert nbytes % 2 == 0
    flat = torch.full((nbytes // 2 + 2 * G,), fill, dtype=torch.int16, device=dev())
    return flat, flat[G:G + nbytes // 2]


def same_bits(a, b):
    bits = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}[a.dtype]
    return torch.equal(a.view(bits), b.view(bits))


def operands(c, inputs, g_shift=0):
    fdt = torch.bfloat16 if c.dt == "bf16" else torch.float32
    g, txt, vis, tmask, vmask = inputs
    ops = [guarded_operand(g, torch.float32, g_shift), guarded_operand(txt, fdt), guarded_operand(vis, fdt), guarded_operand(tmask, torch.uint8),
           guarded_operand(vmask, torch.uint8)]
    for (_, inner, _), vals in zip(ops[:3], (g, txt, vis)):       # nothing was rounded on the way in
        assert torch.equal(inner.double().cpu(), torch.from_numpy(vals).reshape(-1))
    return ops


def call(lib, c, ops, bufs, ws_fill=WS_NAN):
    """one call of the C ABI on guarded buffers; the workspace guards are checked here"""
    from vlgae_amd import _C
    in_dtype = _C.BF16 if c.dt == "bf16" else _C.F32
    nbytes = lib.vlg_bilinear_align_backward_workspace(c.B, c.A, c.Q, c.V, c.d, in_dtype)
    assert nbytes == plan(c.dt, c.d, c.B, c.A, c.Q, c.V)["ws_bytes"]
    ws_flat, ws = guarded_workspace(nbytes, ws_fill) if nbytes else (None, None)
    p = lambda k: _C.ptr(bufs[k][1]) if k in bufs else None
    rc = lib.vlg_bilinear_align_backward(_C.ptr(ops[0][1]), _C.ptr(ops[1][1]), _C.ptr(ops[2][1]), _C.ptr(ops[3][1]), _C.ptr(ops[4][1]), c.B, c.A, c.Q, c.V,
                                         c.d, in_dtype, _C.ptr(ws), nbytes, p("t"), p("v"), _C.stream_of(ops[0][1]))
    _C.check(rc, "bilinear_align_backward")
    torch.cuda.synchronize()
    if ws_flat is not None:
        assert bool((ws_flat[:G] == ws_fill).all()) and bool((ws_flat[G + nbytes // 2:] == ws_fill).all()), f"{case_id(c)}: a word outside the queried workspace was written"


def check_exact(tag, c, bufs, ref):
    """the written regions equal float32(float64 oracle) by value; every guard element is still NaN"""
    for k, name in SIDES:
        if k not in bufs:
            continue
        flat, inner = bufs[k]
        got, want = inner.cpu().numpy().reshape(shapes(c)[k]), ref[k]
        bad = ~(got == want)
        if bad.any():
            at = tuple(int(i) for i in np.argwhere(bad)[0])
            err = np.abs(np.where(np.isnan(got), 0, got).astype(np.float64) - want)[bad]
            raise AssertionError(f"{tag}: {name} differs from the float64 oracle in {int(bad.sum())} of {bad.size} elements ({int(np.isnan(got).sum())} NaN); "
                                 f"first at (fixed, row, column) = {at}: got {got[at]!r}, want {want[at]!r}; |err| {err.min():.3e} .. {err.max():.3e}; "
                                 f"fixed indices {sorted({int(i[0]) for i in np.argwhere(bad)})[:12]}, rows {sorted({int(i[1]) for i in np.argwhere(bad)})[:12]}")
        assert int(torch.isnan(flat).sum()) == 2 * G, f"{tag}: a guard element of {name} was written"


def check_operands(tag, ops):
    for flat, _, before in ops:
        assert flat is None or same_bits(flat, before), f"{tag}: an operand or its guard changed"


@functools.lru_cache(maxsize=4)     # the cases of one shape (outputs alone and together, cotangent offsets) follow each other
def exact_reference(key):
    import oracle
    oracle.build()
    inputs = exact_inputs(key)
    rt, rv = oracle.bilinear_align_backward(*inputs, np.float64)
    return inputs, dict(t=rt.astype(np.float32), v=rv.astype(np.float32))


def describe(c):
    d = derive(c)
    keys = ("image", "k_quads", "grid", "split", "opb", "blocks", "lds", "zeroed", "nck", "gx", "idle", "iters_mod3", "lone")
    return {"routes": d["routes"], "ws_bytes": d["ws_bytes"], **{p + k: d[p + k] for p in ("t_", "v_") for k in keys if p + k in d}}


def run_exact(lib, c, g_shift=0, third=False):
    tag = case_id(c) + (f" [cotangent at float offset {g_shift}]" if g_shift else "")
    print(f"[align-bwd] {tag}: {describe(c)}")
    assert derive(c)["routes"] == c.claim["routes"]      # (test_align_bwd_paths.py says which cases moved)
    inputs, ref = exact_reference(input_key(c))
    ops = operands(c, inputs, g_shift)
    first = guarded_outputs(c)
    call(lib, c, ops, first)
    check_exact(tag, c, first, ref)
    for fill in (WS_NAN,) + ((WS_OTHER,) if third else ()):
        again = guarded_outputs(c)
        call(lib, c, ops, again, fill)
        for k in first:
            assert same_bits(first[k][0], again[k][0]), f"{tag}: {dict(SIDES)[k]} differs between two calls (workspace prefill {fill:#x})"
    check_operands(tag, ops)
    return first


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("i", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_exact_operands_every_route(lib, i):
    """Every case of the table (tests/test_align_bwd_paths.py names the route, image and boundary of each id): every requested gradient
    equals float32 of the float64 oracle, guards stay NaN, nothing is left unwritten, operands are untouched, the workspace is not
    overrun, a second call gives the same bits; a gradient asked for alone has the bits it has when both are asked for."""
    c = CASES[i]
    first = run_exact(lib, c, third=i % 4 == 0)
    if c.want != "tv":
        both = c._replace(want="tv", claim=dict(routes=derive(c._replace(want="tv"))["routes"]))
        pair = run_exact(lib, both)
        assert same_bits(first[c.want][0], pair[c.want][0]), f"{case_id(c)}: the gradient alone differs from the same gradient beside the other"


@pytest.mark.parametrize("c", ALIGNMENT, ids=[case_id(c) for c in ALIGNMENT])
def test_cotangent_at_float_offsets(lib, c):
    """The Python wrapper passes any contiguous float32 tensor, so a slice with a storage offset is only 4-byte aligned, and ld_g4 says that
    is enough: grad_out at float offsets 1, 2, 3 inside a larger allocation gives the bits of offset 0 (k_quads branch of split_kc,
    and concat2)."""
    assert derive(c)["t_k_quads"] is True
    base = run_exact(lib, c)
    for shift in (1, 2, 3):
        moved = run_exact(lib, c, g_shift=shift)
        for k in base:
            assert same_bits(base[k][0], moved[k][0]), (case_id(c), shift, k)


def masked_abs_contraction(oracle_mod, inputs):
    g, txt, vis, tmask, vmask = inputs
    return oracle_mod.bilinear_align_backward(np.abs(g), np.abs(txt), np.abs(vis), tmask, vmask, np.float64)


@pytest.mark.parametrize("c", ROUNDING, ids=[case_id(c) for c in ROUNDING])
def test_rounding_data(lib, oracle_mod, c):
    """normal(0, 0.5) data.  Generic images: |got - ref64| <= max(2e-5 max(1, |ref|max), 4 e32).  Split-term images: every element within
    2^-16 S + 4 e32, S the masked contraction of |g| |x| (see the file's docstring).  Masked rows are zero by value."""
    assert derive(c)["routes"] == c.claim["routes"]
    inputs = rounding_inputs(input_key(c))
    r32 = oracle_mod.bilinear_align_backward(*inputs, np.float32)
    r64 = oracle_mod.bilinear_align_backward(*inputs, np.float64)
    S = masked_abs_contraction(oracle_mod, inputs)
    ops = operands(c, inputs)
    bufs = guarded_outputs(c)
    call(lib, c, ops, bufs)
    P = plan(c.dt, c.d, c.B, c.A, c.Q, c.V)
    for (k, name), side, ref32, ref, s_abs, rowmask in zip(SIDES, ("txt", "vis"), r32, r64, S, (inputs[3], inputs[4])):
        flat, inner = bufs[k]
        got = inner.cpu().numpy().reshape(shapes(c)[k])
        dead = rowmask == 0
        assert dead.any() and (~dead).any() and not got[dead].any() and not np.isnan(got).any(), f"{case_id(c)}: masked rows of {name}"
        e32 = float(np.abs(ref32.astype(np.float64) - ref).max())
        err = np.abs(got.astype(np.float64) - ref)
        top = float(np.abs(ref).max())
        if P[side]["route"] == "generic":
            bound = np.full(ref.shape, max(2e-5 * max(1.0, top), 4 * e32))
        else:
            bound = 2.0 ** -16 * s_abs + 4 * e32
        ratio = float((err / np.maximum(bound, 1e-300))[~dead].max())
        print(f"[align-bwd] rounding {case_id(c)} {name} ({P[side]['route']}): err {err.max():.3e}, max|ref| {top:.3e}, e32 {e32:.3e}, "
              f"smallest bound {bound[~dead].min():.3e}, largest err / bound {ratio:.3e}")
        assert (err <= bound).all(), (case_id(c), name, float(err.max()), ratio)
        assert int(torch.isnan(flat).sum()) == 2 * G
    check_operands(case_id(c), ops)


@pytest.mark.parametrize("c", PYTHON, ids=[case_id(c) for c in PYTHON])
def test_python_layer_returns_the_bits_of_the_direct_call(lib, c):
    """align.bilinear_align_backward and autograd through align.gather_logit return the bits of the direct call (bf16 leaves: that value
    cast); want_txt = False / want_vis = False return None."""
    from vlgae_amd import align
    inputs, ref = exact_reference(input_key(c))
    direct = run_exact(lib, c)
    d_t, d_v = direct["t"][1].reshape(shapes(c)["t"]), direct["v"][1].reshape(shapes(c)["v"])
    fdt = torch.bfloat16 if c.dt == "bf16" else torch.float32
    g, txt, vis = (torch.from_numpy(x).to(dev(), dt) for x, dt in zip(inputs[:3], (torch.float32, fdt, fdt)))
    tm, vm = (None if m is None else torch.from_numpy(m).to(dev()).bool() for m in inputs[3:])
    p_t, p_v = align.bilinear_align_backward(g, txt, vis, tm, vm)
    assert same_bits(p_t.contiguous(), d_t) and same_bits(p_v.contiguous(), d_v)
    only_t, none_v = align.bilinear_align_backward(g, txt, vis, tm, vm, want_vis=False)
    none_t, only_v = align.bilinear_align_backward(g, txt, vis, tm, vm, want_txt=False)
    assert none_v is None and none_t is None and same_bits(only_t.contiguous(), d_t) and same_bits(only_v.contiguous(), d_v)
    assert align.bilinear_align_backward(g, txt, vis, tm, vm, want_txt=False, want_vis=False) == (None, None)
    a, b = txt.clone().requires_grad_(True), vis.clone().requires_grad_(True)
    out = align.gather_logit(None, (b, vm, None), (a, tm, None), None).rename(None)
    ga, gb = torch.autograd.grad(out, [a, b], g)
    assert ga.dtype == fdt and gb.dtype == fdt
    assert same_bits(ga.contiguous(), d_t.to(fdt)) and same_bits(gb.contiguous(), d_v.to(fdt))
    a2 = txt.clone().requires_grad_(True)
    out = align.gather_logit(None, (vis, vm, None), (a2, tm, None), None).rename(None)
    (ga2,) = torch.autograd.grad(out, [a2], g)
    assert same_bits(ga2.contiguous(), d_t.to(fdt))
