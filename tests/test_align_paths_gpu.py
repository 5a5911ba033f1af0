"""vlg_bilinear_align (vlgae_amd/csrc/vlg_align.hip) at every dispatch route and tile boundary, through the C ABI, against the float64
oracle.  The case table, the restated dispatch and the inputs come from tests/test_align_paths.py, which pins each case to the routes and
launch-shape numbers its id names:

  route        kernel                                  boundaries the table sits on
  shared_max   align_max_kernel<6>                     V <= 48; Q around 96; a_per_block 3 | 8 + tail 4 | 10 x 31 + tail 1; B = 1, 8, 9 (mirrored wave);
                                                       row tiles / images without a masked element next to masked ones
  shared_full  align_full_kernel                       V in {4, 40, 44}; all eight copy-out shifts sh, also by moving out_full in 16-byte steps;
                                                       Q = 97 at V = 44; the same a_per_block / B cases
  tile48       align_mfma_kernel<TILE, RTB 3>          V = 1 .. 48 around the 16-region tiles; Q around 48; a_per_wave 1 .. 16
  direct       align_mfma_kernel<DIRECT>               V = 49, 50, 53, 96, 97, 193: maxima carried across region groups; Q around 96 | 48; a_per_wave 1 .. 16
  diag_only    align_mfma_kernel<TILE, RTB 3>, apw < 0 alone and behind shared_max / direct; grid 1 -> 2 at V = 192 | 193, the cap of 16 at V = 3073
  tile_full    align_mfma_kernel<TILE>                 vector copy-out at last-group widths 4, 28, 44, 48 (idle lanes), scalar at V = 50; the running mv[]
                                                       row across groups; Q around 96 | 48; a_per_wave 1 .. 16
  stream_maxq  align_mfma_kernel<no tile>              max_q alone: the fold over query passes into out_maxQ; a_per_wave 1 .. 16
  generic      align_kernel                            d = 1, 16, 40, 100; Q, V in {63, 64, 65}; A in {7, 8, 9}; caption tile reused or reloaded

Exact operands.  Features are integers in [-8, 8] divided by 8 (exact in bf16): every product is a multiple of 1 / 64 and every partial
sum at most 128 in magnitude, so every output of every route must EQUAL float32 of the float64 oracle bit for bit -- no tolerance (the CPU
file asserts that the float32 oracle equals the float64 one on the same inputs).

Guards.  The C ABI is called directly so that the test owns every buffer.  Each operand and each output sits between two NaN bands of 64
elements (masks: between bands of zeros); the region an output is to be written to is prefilled with +3e38, NOT NaN: out_maxQ is read back
and folded across query passes with fmaxf, which drops a NaN, so a first pass that failed to write would vanish behind a NaN prefill and
shows as 3e38 here.  A missing write leaves 3e38, a stray write removes a NaN from a band, and the operands with their bands are compared
with a copy taken before the call.  Every call is repeated into fresh buffers (same bits).

Rounding set.  One case per route x image on normal(0, 0.5) features (bf16-rounded for the bf16 images), both masks random:
|got - ref64| <= max(2e-5 max(1, |ref|max), 4 e32) over the unmasked entries, where 2e-5 is the project's rule for float32 accumulation
over d <= 128 (test_bilinear_align_config_size) and e32 the float32 sequential oracle's own error against float64 on the same inputs;
masked entries equal neg_inf exactly.  Measured e32 (largest over the outputs of the case):
  image        shared_max  shared_full  tile48   direct   tile_full  stream_maxq  (diag_only rides with shared_max / tile48 / direct)
  (bf16, 128)  2.1e-06     1.7e-06      -        1.8e-06  2.0e-06    1.8e-06
  (bf16, 64)   -           -            7.5e-07  7.2e-07  8.3e-07    7.2e-07
  (f32, 128)   -           -            3.7e-06  3.5e-06  4.1e-06    3.5e-06
  (f32, 64)    -           -            2.5e-06  2.6e-06  2.6e-06    2.6e-06
  generic, d = 100: bf16 8.8e-07, f32 3.4e-06
so 4 e32 <= 1.7e-5 stays below 2e-5 max(1, |ref|max) (|ref|max is 7.5 .. 12.2 here) and the first term decides.
"""
import functools

import numpy as np
import pytest
import torch

from test_align_paths import CASES, ROUNDING, case_id, derive, exact_inputs, input_key, oracle_outputs, rounding_inputs

pytestmark = pytest.mark.gpu

NAN = float("nan")
G = 64                    # guard elements on each side of every buffer
STALE = 3e38              # prefill of the region an output is written to
NAMES = dict(f="full", v="maxV", q="maxQ", d="diag")
AXES = dict(f="(b, a, q, v)", v="(b, a, q)", q="(b, a, v)", d="(b, q, v)")


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from vlgae_amd import _C
    return _C.lib()   # must load: the product has no fallback


def shapes(c):
    return dict(f=(c.B, c.A, c.Q, c.V), v=(c.B, c.A, c.Q), q=(c.B, c.A, c.V), d=(c.B, c.Q, c.V))


# ---------------------------------------------------------------------------------------------------------------- guarded buffers
def guarded_operand(vals, dtype):
    """(whole buffer, the operand inside it, a copy of the whole buffer): NaN bands for features, zero bands for masks"""
    if vals is None:
        return None, None, None
    t = torch.from_numpy(np.ascontiguousarray(vals)).reshape(-1)
    flat = torch.full((t.numel() + 2 * G,), 0 if dtype == torch.uint8 else NAN, dtype=dtype, device=dev())
    inner = flat[G:G + t.numel()]
    inner.copy_(t.to(dtype))
    assert inner.data_ptr() % 16 == 0
    return flat, inner, flat.clone()


def guarded_outputs(c, shift=0):
    """{key: (whole buffer, written region)}; `shift` floats move the written region inside its allocation"""
    out = {}
    for k in c.outs:
        n = int(np.prod(shapes(c)[k]))
        flat = torch.full((n + 2 * G + 32,), NAN, dtype=torch.float32, device=dev())
        inner = flat[G + shift:G + shift + n]
        inner.fill_(STALE)
        assert inner.data_ptr() % 128 == 4 * shift
        out[k] = (flat, inner)
    return out


def same_bits(a, b):
    bits = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}[a.dtype]
    return torch.equal(a.view(bits), b.view(bits))


def operands(c, inputs):
    fdt = torch.bfloat16 if c.dt == "bf16" else torch.float32
    txt, vis, tmask, vmask = inputs
    ops = [guarded_operand(txt, fdt), guarded_operand(vis, fdt), guarded_operand(tmask, torch.uint8), guarded_operand(vmask, torch.uint8)]
    assert torch.equal(ops[0][1].double().cpu(), torch.from_numpy(txt).reshape(-1)) and torch.equal(ops[1][1].double().cpu(), torch.from_numpy(vis).reshape(-1))
    return ops


def call(lib, c, ops, bufs):
    from vlgae_amd import _C
    p = lambda k: _C.ptr(bufs[k][1]) if k in bufs else None
    rc = lib.vlg_bilinear_align(_C.ptr(ops[0][1]), _C.ptr(ops[1][1]), _C.ptr(ops[2][1]), _C.ptr(ops[3][1]), c.B, c.A, c.Q, c.V, c.d,
                                _C.BF16 if c.dt == "bf16" else _C.F32, c.neg_inf, p("f"), p("v"), p("q"), p("d"), _C.stream_of(ops[0][1]))
    _C.check(rc, "bilinear_align")
    torch.cuda.synchronize()


def check_exact(tag, c, bufs, ref):
    """the written regions equal float32(float64 oracle) bit for bit; every guard element is still NaN"""
    for k, (flat, inner) in bufs.items():
        got, want = inner.cpu().numpy().reshape(shapes(c)[k]), ref[NAMES[k]]
        bad = got.view(np.int32) != want.view(np.int32)
        if bad.any():
            at = tuple(int(i) for i in np.argwhere(bad)[0])
            raise AssertionError(f"{tag}: {NAMES[k]} differs from the float64 oracle in {int(bad.sum())} of {bad.size} elements ({int(np.isnan(got).sum())} NaN, "
                                 f"{int((got == np.float32(STALE)).sum())} never written); first at {AXES[k]} = {at}: got {got[at]!r}, want {want[at]!r}; "
                                 f"all of them at second-last index {sorted({int(i[-2]) for i in np.argwhere(bad)})[:12]} / last index {sorted({int(i[-1]) for i in np.argwhere(bad)})[:12]}")
        assert int(torch.isnan(flat).sum()) == flat.numel() - inner.numel(), f"{tag}: a guard element of {NAMES[k]} was written"


def check_operands(tag, ops):
    for flat, _, before in ops:
        assert flat is None or same_bits(flat, before), f"{tag}: an operand or its guard changed"


@functools.lru_cache(maxsize=8)     # the cases of one shape (the subsets of the outputs) follow each other in the table
def exact_reference(key, neg_inf):
    import oracle
    oracle.build()
    inputs = exact_inputs(key)
    ref = oracle_outputs(oracle, inputs, np.float64, neg_inf)
    return inputs, {k: None if v is None else v.astype(np.float32) for k, v in ref.items()}


def run_exact(lib, c, shift=0):
    tag = case_id(c) + (f" [out_full moved by {4 * shift} bytes]" if shift else "")
    print(f"[align] {tag}: {derive(c)}")
    assert derive(c)["routes"] == c.claim["routes"]      # (test_align_paths.py says which cases moved)
    inputs, ref = exact_reference(input_key(c), c.neg_inf)
    ops = operands(c, inputs)
    first = guarded_outputs(c, shift)
    call(lib, c, ops, first)
    check_exact(tag, c, first, ref)
    again = guarded_outputs(c, shift)
    call(lib, c, ops, again)
    for k in first:
        assert same_bits(first[k][0], again[k][0]), f"{tag}: {NAMES[k]} differs between two calls"
    check_operands(tag, ops)


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_exact_operands_every_route(lib, c):
    """Every case of the table (tests/test_align_paths.py names the route and boundary of each id): every requested output equals
    float32 of the float64 oracle bit for bit, guards stay NaN, nothing is left unwritten, operands are untouched, a second call gives the
    same bits."""
    run_exact(lib, c)


SHIFTED = next(c for c in CASES if c.group == "sf" and c.claim["sh"] == frozenset(range(8)))


@pytest.mark.parametrize("k", range(1, 8))
def test_shared_full_output_at_16_byte_offsets(lib, k):
    """align_full_kernel's copy-out starts each store instruction at a 128-byte line: sh = (dst >> 4) & 7.  out_full at byte offsets 16 k
    inside a larger allocation moves every chunk's sh by k (multiples of 16 only: the vector stores assume that much)."""
    run_exact(lib, SHIFTED, shift=4 * k)


@pytest.mark.parametrize("c", ROUNDING, ids=[case_id(c) for c in ROUNDING])
def test_rounding_data(lib, oracle_mod, c):
    """normal(0, 0.5) features: |got - ref64| <= max(2e-5 max(1, |ref|max), 4 e32) over the unmasked entries of each output, masked
    entries equal neg_inf exactly (see the file's docstring for e32)."""
    assert derive(c)["routes"] == c.claim["routes"]
    inputs = rounding_inputs(input_key(c))
    r32, r64 = (oracle_outputs(oracle_mod, inputs, t, c.neg_inf) for t in (np.float32, np.float64))
    ops = operands(c, inputs)
    bufs = guarded_outputs(c)
    call(lib, c, ops, bufs)
    fill = np.float32(c.neg_inf)
    for k, (flat, inner) in bufs.items():
        got, ref = inner.cpu().numpy().reshape(shapes(c)[k]), r64[NAMES[k]]
        kept = ref != c.neg_inf
        assert kept.any() and (~kept).any() and np.array_equal(got[~kept], np.full(int((~kept).sum()), fill)), f"{case_id(c)}: masked entries of {NAMES[k]}"
        e32 = float(np.abs(r32[NAMES[k]][kept].astype(np.float64) - ref[kept]).max())
        err, top = float(np.abs(got[kept].astype(np.float64) - ref[kept]).max()), float(np.abs(ref[kept]).max())
        bound = max(2e-5 * max(1.0, top), 4 * e32)
        print(f"[align] rounding {case_id(c)} {NAMES[k]}: err {err:.3e}, max|ref| {top:.3e}, e32 {e32:.3e}, bound {bound:.3e}")
        assert err <= bound, (case_id(c), NAMES[k], err, bound)
        assert int(torch.isnan(flat).sum()) == flat.numel() - inner.numel()
    check_operands(case_id(c), ops)
