"""The attention fuse (vlgae_amd/csrc/vlg_attn.hip) at every route, key-split plan and tile boundary, through the C ABI (vlg_attn_fuse,
vlg_attn_fuse_backward), against the float64 oracle (oracle.cpu_oracle.attn_fuse / attn_fuse_backward).  The case table, the restated
dispatch and the inputs come from tests/test_attn_paths.py, which pins every row to the route its id names; here the three size queries of
the library are compared with the restatement again before a row runs, so a row never silently runs another kernel.

Every row runs on two input sets: `random` (normal(0, 0.4) features, as the rest of the suite) and `planted` (a word with score 16 on each
boundary key of the row -- V - 1, 0, chunk and step ends, 16 t - 1 | 16 t --, assigned differently in every sentence, vis_mid rows of small
integers that differ between neighbouring keys and sentences).  The oracle's attention map must give every planted word at least 0.9 of its
weight on its key: a dropped, duplicated or misplaced boundary key, or a row read from the neighbouring sentence, is then wrong by O(1) in
`out` and d_vis_mid.  The forward runs once, the adjoint with float32 gradients and, for bf16 features, bf16 gradients; on the key-split
route with the forward's records handed over (`saved`) and recomputed (saved = NULL): the same bits.  bf16 gradients must equal the float32
ones cast afterwards bit for bit (d_gamma, d_beta identical).  key_chunk = 0 rows above 256 keys run again with the restated CK as an
explicit key_chunk: the same bits.

Tolerances (the suite's): |out - ref| <= 1e-4, attention map 2e-5, float32-feature gradients 1e-4 max(1, |g|max); bf16 features (the oracle
sees the bf16 values): out 1e-4, d_gamma / d_beta 1e-4 max(1, |g|max), the four feature gradients 1e-2 max(1, |g|max) in either gradient
type -- the adjoint's matrix-core operands (dy, P, dS) are single bf16 values by design, and the float32-typed results must cast to exactly the
bf16-typed ones, so both carry that rounding.

Guards.  Every operand, every output, `saved` and both workspaces sit between NaN bands of 64 elements, outputs and workspaces prefilled
with NaN: after every call the bands are intact, the operands unchanged and no output holds a NaN -- which a read of unwritten P^T / dS^T
padding (words past L, keys past V inside a written tile), of an unwritten chunk record or of an unwritten dy^T / txt^T row would leave.

Streaming-softmax numerics: see test_attn_paths.py (numerics_inputs, stream32); allowed max(project tolerance, 8 x the float32
restatement's own error against float64 on the same inputs), every output finite.

Independence, bit for bit, on every route family: sentence b of a batch of 3 equals the same sentence run alone (explicit key_chunk on the
split route, so the plan does not move with B) in `out` and the four feature gradients; out[:, :16], d_enc_x[:, :16], d_txt[:, 1:17] at
L = 17 equal the L = 16 run on the truncated operands.  No legitimate dependence: a wavefront reads its own sentence and word tile only, and
the merge of chunk records is per (sentence, word tile) in chunk order.
"""
import functools

import numpy as np
import pytest
import torch

from test_attn_paths import (BF16, CASES, DTS, F32, FAMILIES, GRAD_NAMES, NUMERICS, NUMERICS_SHAPES, attn_split, case_id, derive, family, forward, fwd_desc,
                             inputs, numerics_inputs, oracle_reference, saved_bytes, stream32, workspace_bwd, workspace_fwd)

pytestmark = pytest.mark.gpu

NAN = float("nan")
G = 64                    # guard elements on each side of every buffer
EPS = 1e-5
TDT = dict(f32=torch.float32, bf16=torch.bfloat16)
CODE = dict(f32=F32, bf16=BF16)


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from vlgae_amd import _C
    return _C.lib()   # must load: the product has no fallback


def same_bits(a, b):
    bits = {torch.float32: torch.int32, torch.bfloat16: torch.int16}[a.dtype]
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(bits), b.contiguous().view(bits))


# ---------------------------------------------------------------------------------------------------------------- guarded buffers
class Buf:
    """`shape` elements of `dtype` between two NaN bands; filled from `vals` (which must be exact in the type) or with NaN"""

    def __init__(self, shape, dtype, vals=None):
        n = int(np.prod(shape))
        self.n, self.flat = n, torch.full((n + 2 * G,), NAN, dtype=dtype, device=dev())
        self.t = self.flat[G:G + n].view(*shape)
        assert self.t.data_ptr() % 16 == 0
        if vals is not None:
            src = torch.from_numpy(np.ascontiguousarray(vals))
            self.t.copy_(src.to(dtype))
            assert torch.equal(self.t.double().cpu(), src.double())
        self.before = self.flat.clone() if vals is not None else None

    def ptr(self):
        from vlgae_amd import _C
        return _C.ptr(self.t)

    def guards_intact(self):
        return bool(torch.isnan(self.flat[:G]).all()) and bool(torch.isnan(self.flat[G + self.n:]).all())

    def unchanged(self):
        bits = {torch.float32: torch.int32, torch.bfloat16: torch.int16}[self.flat.dtype]
        return torch.equal(self.flat.view(bits), self.before.view(bits))


def finish(tag, rc):
    """wait for the call; a HIP error (not one of the library's own codes) ends the session: nothing more is started on a device that faulted"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{tag}: {e}", 3)
    if 0 < rc < 0x1000:
        pytest.exit(f"{tag}: HIP error {rc}", 3)


def operands(x, dt):
    f = TDT[dt]
    return dict(vis=Buf(x.vis.shape, f, x.vis), txt=Buf(x.txt.shape, f, x.txt), mid=Buf(x.mid.shape, f, x.mid), enc=Buf(x.enc.shape, f, x.enc),
                gamma=Buf(x.gamma.shape, torch.float32, x.gamma), beta=Buf(x.beta.shape, torch.float32, x.beta), dout=Buf(x.dout.shape, torch.float32, x.dout))


def check_after(tag, ops, outs):
    for name, b in ops.items():
        assert b.unchanged(), f"{tag}: operand {name} or its guard changed"
    for name, b in outs.items():
        assert b.guards_intact(), f"{tag}: a guard element of {name} was written"


def run_forward(lib, tag, ops, dt, ck=0, attmap=False, save=True):
    """vlg_attn_fuse into fresh NaN-filled guarded buffers: dict(out, att | None, saved | None)"""
    from vlgae_amd import _C
    B, V, d = ops["vis"].t.shape
    L, h = ops["txt"].t.shape[1] - 1, ops["mid"].t.shape[2]
    # (the size queries do not see d: only the key-split route, as restated, is given a workspace and a place for its merged records)
    split = fwd_desc(forward(dt, B, L, V, d, h, ck, attmap)).startswith("split")
    need = lib.vlg_attn_fuse_workspace(B, L, V, h, ck) if split else 0
    sbytes = lib.vlg_attn_fuse_saved_bytes(B, L, V, h, ck) if split else 0
    assert (need > 0) == split and (need, sbytes) == ((workspace_fwd(B, L, V, h, ck), saved_bytes(B, L, V, h, ck)) if split else (0, 0)), tag
    out = Buf((B, L, h), torch.float32)
    att = Buf((B, L, V), torch.float32) if attmap else None
    ws = Buf((need // 4,), torch.float32) if need else None
    saved = Buf((sbytes // 4,), torch.float32) if sbytes and save else None
    p = lambda b: b.ptr() if b is not None else None
    rc = lib.vlg_attn_fuse(ops["vis"].ptr(), ops["txt"].ptr(), ops["mid"].ptr(), ops["enc"].ptr(), ops["gamma"].ptr(), ops["beta"].ptr(), B, L, V, d, h,
                           CODE[dt], EPS, ck, p(ws), need, p(saved), p(att), out.ptr(), _C.stream_of(out.t))
    finish(tag, rc)
    assert rc == 0, (tag, rc, lib.vlg_last_error())
    bufs = {k: b for k, b in dict(out=out, att=att, ws=ws, saved=saved).items() if b is not None}
    check_after(tag + " forward", ops, bufs)
    for k in ("out", "att", "saved"):
        if k in bufs:
            assert not bool(torch.isnan(bufs[k].t).any()), f"{tag}: forward left NaN in {k}"
    return dict(out=out.t, att=att.t if att else None, saved=saved)


def run_backward(lib, tag, ops, dt, gdt, ck=0, saved=None, dout=None, ld=None):
    """vlg_attn_fuse_backward into fresh NaN-filled guarded buffers: {name: tensor}.  dout / ld: a cotangent tensor read through strides"""
    from vlgae_amd import _C
    B, V, d = ops["vis"].t.shape
    L, h = ops["txt"].t.shape[1] - 1, ops["mid"].t.shape[2]
    need = lib.vlg_attn_fuse_backward_workspace(B, L, V, d, h, CODE[gdt], ck)
    assert need == workspace_bwd(B, L, V, d, h, gdt, ck) and need % 4 == 0, tag
    g = TDT[gdt]
    outs = dict(d_vis=Buf((B, V, d), g), d_txt=Buf((B, L + 1, d), g), d_vis_mid=Buf((B, V, h), g), d_enc_x=Buf((B, L, h), g),
                d_gamma=Buf((h,), torch.float32), d_beta=Buf((h,), torch.float32))
    ws = Buf((need // 4,), torch.float32)
    dptr, (ldb, ldl) = (ops["dout"].ptr(), (L * h, h)) if dout is None else (_C.ptr(dout), ld)
    rc = lib.vlg_attn_fuse_backward(ops["vis"].ptr(), ops["txt"].ptr(), ops["mid"].ptr(), ops["enc"].ptr(), ops["gamma"].ptr(), dptr, ldb, ldl, B, L, V, d, h,
                                    CODE[dt], EPS, ck, CODE[gdt], saved.ptr() if saved is not None else None, ws.ptr(), need,
                                    *(outs[n].ptr() for n in GRAD_NAMES), _C.stream_of(ws.t))
    finish(tag, rc)
    assert rc == 0, (tag, rc, lib.vlg_last_error())
    check_after(tag + " adjoint", ops, dict(outs, ws=ws))
    for n in GRAD_NAMES:
        assert not bool(torch.isnan(outs[n].t).any()), f"{tag}: adjoint (g{gdt}) left NaN in {n}: {int(torch.isnan(outs[n].t).sum())} of {outs[n].n}"
    return {n: outs[n].t for n in GRAD_NAMES}


# ---------------------------------------------------------------------------------------------------------------- comparisons
def err_of(got, want):
    return float((got.double().cpu() - torch.from_numpy(np.ascontiguousarray(want))).abs().max())


def check_forward(tag, res, ref, x, out_tol=1e-4):
    e = err_of(res["out"], ref["out"])
    print(f"[attn] {tag}: out err {e:.2e}")
    assert e <= out_tol, (tag, "out", e)
    if res["att"] is not None:
        ea = err_of(res["att"], ref["att"])
        print(f"[attn] {tag}: attention map err {ea:.2e}")
        assert ea <= 2e-5, (tag, "att", ea)


def grad_tol(dt, name, want, floor=None):
    tol = (1e-2 if dt == "bf16" and name in GRAD_NAMES[:4] else 1e-4) * max(1.0, float(np.abs(want).max()))
    return max(tol, floor) if floor is not None else tol


def check_grads(tag, dt, grads, ref, floors=None):
    for n in GRAD_NAMES:
        e, tol = err_of(grads[n], ref[n]), grad_tol(dt, n, ref[n], None if floors is None else floors[n])
        print(f"[attn] {tag}: {n} err {e:.2e} (allowed {tol:.2e}, |ref|max {np.abs(ref[n]).max():.2e})")
        assert e <= tol, (tag, n, e, tol)
    assert not bool(grads["d_txt"][:, 0].any()), f"{tag}: the root slot's gradient is not zero"


def check_same(tag, a, b, names=GRAD_NAMES):
    for n in names:
        assert same_bits(a[n], b[n]), f"{tag}: {n} differs ({int((a[n] != b[n]).sum())} elements)"


def check_cast(tag, g32, g16):
    for n in GRAD_NAMES[:4]:
        assert same_bits(g32[n].bfloat16(), g16[n]), f"{tag}: bf16 {n} is not the float32 one cast"
    check_same(tag, g32, g16, GRAD_NAMES[4:])


def all_grads(lib, tag, ops, dt, ck, saved):
    """the adjoint in every gradient type, with the forward's records handed over and recomputed: {gdt: grads}"""
    res = {}
    for gdt in ("f32", "bf16") if dt == "bf16" else ("f32",):
        res[gdt] = run_backward(lib, f"{tag} g{gdt}", ops, dt, gdt, ck, saved)
        if saved is not None:
            check_same(f"{tag} g{gdt} saved vs recomputed", res[gdt], run_backward(lib, f"{tag} g{gdt} saved=NULL", ops, dt, gdt, ck, None))
    if "bf16" in res:
        check_cast(tag, res["f32"], res["bf16"])
    return res


@functools.lru_cache(maxsize=4)
def _reference(oracle_mod, key, kind):
    return oracle_reference(oracle_mod, inputs(CASES[key], kind))


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("kind", ["random", "planted"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_every_route(lib, oracle_mod, i, kind):
    """Every row of the table, on random and on planted inputs: forward and adjoint against the float64 oracle inside NaN guards (module
    docstring)."""
    c = CASES[i]
    tag = f"{case_id(c)} {kind}"
    assert derive(c) == (c.fwd, c.bwd), tag
    x, ref = inputs(c, kind), _reference(oracle_mod, i, kind)
    for b, w, k in x.plant:
        assert ref["att"][b, w, k] >= 0.9, (tag, b, w, k, ref["att"][b, w, k])
    ops = operands(x, c.dt)
    fwd = run_forward(lib, tag, ops, c.dt, c.ck, c.attmap)
    sp = attn_split(c.B, c.L, c.V, c.ck)
    assert (fwd["saved"] is not None) == (c.fwd.startswith("split")), tag
    check_forward(tag, fwd, ref, x)
    if c.fwd.startswith("split"):      # without `saved` the merged records go to the workspace: the same bits
        assert same_bits(fwd["out"], run_forward(lib, tag + " unsaved", ops, c.dt, c.ck, save=False)["out"]), tag
    if c.bwd == "nobwd":
        return
    grads = all_grads(lib, tag, ops, c.dt, c.ck, fwd["saved"])
    for gdt, g in grads.items():
        check_grads(f"{tag} g{gdt}", c.dt, g, ref)
    if c.ck == 0 and c.V > 256:      # the automatic plan against the same plan asked for by key_chunk
        assert sp == attn_split(c.B, c.L, c.V, sp.CK)
        again = run_forward(lib, tag + " explicit", ops, c.dt, sp.CK, False)
        assert same_bits(fwd["out"], again["out"]), f"{tag}: out differs between key_chunk = 0 and key_chunk = {sp.CK}"
        for gdt, g in all_grads(lib, tag + " explicit", ops, c.dt, sp.CK, again["saved"]).items():
            check_same(f"{tag} g{gdt} automatic vs explicit", grads[gdt], g)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("V,ck", NUMERICS_SHAPES)
@pytest.mark.parametrize("name", NUMERICS)
def test_streaming_softmax_numerics(lib, oracle_mod, name, V, ck, dt):
    """Rising and falling step maxima, a dominated chunk set, +-256 offsets: finite everywhere, and within max(project tolerance, 8 x the
    float32 restatement's own error) of the float64 oracle."""
    x = numerics_inputs(name, dt, V)
    B, L = x.vis.shape[0], x.txt.shape[1] - 1
    sp = attn_split(B, L, V, ck)
    assert (sp.NC == 1) == (ck >= V)
    tag = f"numerics {name} V{V} ck{ck} {dt}"
    ref = oracle_reference(oracle_mod, x)
    s32 = stream32(x, sp.CK)
    e32 = {k: float(np.abs(s32[k] - ref[k]).max()) for k in s32}
    ops = operands(x, dt)
    fwd = run_forward(lib, tag, ops, dt, ck)
    assert bool(torch.isfinite(fwd["out"]).all()), tag
    print(f"[attn] {tag}: e32 " + " ".join(f"{k} {v:.1e}" for k, v in e32.items()))
    check_forward(tag, fwd, ref, x, max(1e-4, 8 * e32["out"]))
    for gdt, g in all_grads(lib, tag, ops, dt, ck, fwd["saved"]).items():
        assert all(bool(torch.isfinite(g[n]).all()) for n in GRAD_NAMES), tag
        check_grads(f"{tag} g{gdt}", dt, g, ref, {n: 8 * e32[n] for n in GRAD_NAMES})


def _sub(x, b=None, L=None):
    """sentence b alone, or the first L words"""
    if b is not None:
        return x._replace(vis=x.vis[b:b + 1], txt=x.txt[b:b + 1], mid=x.mid[b:b + 1], enc=x.enc[b:b + 1], dout=x.dout[b:b + 1], plant=())
    return x._replace(txt=x.txt[:, :L + 1], enc=x.enc[:, :L], dout=x.dout[:, :L], plant=())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", [n for n, _ in FAMILIES] + ["generic"])
def test_sentences_and_word_tiles_are_independent(lib, name, dt):
    """Bit for bit: a sentence inside a batch of 3 against the same sentence alone; the first 16 words at L = 17 against the L = 16 run."""
    if name == "generic":
        c = [r for r in CASES if r.dt == dt and r.side == "d24-V300"][0]
    else:
        c = family(name, dt)
    c = c._replace(B=3)
    x = inputs(c, "random")
    run = lambda y, tag: (lambda ops: (lambda f: (f, all_grads(lib, tag, ops, dt, c.ck, f["saved"]) if c.bwd != "nobwd" else {}))(run_forward(lib, tag, ops, dt, c.ck)))(operands(y, dt))
    tag = f"independence {name} {dt}"
    whole_f, whole_g = run(x, tag + " batch")
    for b in range(3):
        f, g = run(_sub(x, b=b), f"{tag} sentence {b}")
        assert same_bits(whole_f["out"][b:b + 1], f["out"]), f"{tag}: out of sentence {b} depends on the batch"
        for gdt in g:
            for n in GRAD_NAMES[:4]:
                assert same_bits(whole_g[gdt][n][b:b + 1], g[gdt][n]), f"{tag}: {n} (g{gdt}) of sentence {b} depends on the batch"
    assert c.L == 17
    f, g = run(_sub(x, L=16), tag + " L16")
    assert same_bits(whole_f["out"][:, :16], f["out"]), f"{tag}: out[:, :16] depends on the 17th word"
    for gdt in g:
        assert same_bits(whole_g[gdt]["d_enc_x"][:, :16], g[gdt]["d_enc_x"]), f"{tag}: d_enc_x[:, :16] (g{gdt}) depends on the 17th word"
        assert same_bits(whole_g[gdt]["d_txt"][:, 1:17], g[gdt]["d_txt"][:, 1:17]), f"{tag}: d_txt[:, 1:17] (g{gdt}) depends on the 17th word"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", [n for n, _ in FAMILIES])
def test_cotangent_read_in_place_through_strides(lib, name, dt):
    """dout as a [B, L, h] view with row stride h + 4 and batch stride (L + 3)(h + 4) inside a NaN-filled buffer, and broadcast over the words
    (stride 0 over L) and over the batch (stride 0 over B): the same bits as the contiguous copy of the same values."""
    c = family(name, dt)
    x = inputs(c, "random")
    B, L, h = c.B, c.L, c.h
    tag = f"strides {name} {dt}"
    forms = {"padded": (x.dout, ((L + 3) * (h + 4), h + 4)), "over-words": (np.broadcast_to(x.dout[:, :1], x.dout.shape), (h + 4, 0)),
             "over-batch": (np.broadcast_to(x.dout[:1], x.dout.shape), (0, h + 4))}
    for form, (vals, (ldb, ldl)) in forms.items():
        y = x._replace(dout=np.ascontiguousarray(vals))
        ops = operands(y, dt)
        saved = run_forward(lib, tag, ops, dt, c.ck)["saved"]
        flat = torch.full((G + B * (L + 3) * (h + 4) + G,), NAN, dtype=torch.float32, device=dev())
        view = torch.as_strided(flat, (B, L, h), (ldb, ldl, 1), G)
        rows = torch.from_numpy(y.dout).float().to(dev())
        if form == "padded":
            view.copy_(rows)
        elif form == "over-words":
            torch.as_strided(flat, (B, h), (ldb, 1), G).copy_(rows[:, 0])
        else:
            torch.as_strided(flat, (L, h), (ldl, 1), G).copy_(rows[0])
        assert torch.equal(view, rows) and view.data_ptr() % 16 == 0
        before = flat.clone()
        for gdt in ("f32", "bf16") if dt == "bf16" else ("f32",):
            want = run_backward(lib, f"{tag} {form} contiguous g{gdt}", ops, dt, gdt, c.ck, saved)
            got = run_backward(lib, f"{tag} {form} g{gdt}", ops, dt, gdt, c.ck, saved, dout=view, ld=(ldb, ldl))
            check_same(f"{tag} {form} g{gdt}", want, got)
        assert torch.equal(flat.view(torch.int32), before.view(torch.int32))
