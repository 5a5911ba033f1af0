"""CPU: the dispatch of the attention fuse (vlgae_amd/csrc/vlg_attn.hip: vlg_attn_fuse, vlg_attn_fuse_backward) restated in Python, pinned to
the library through its three size queries, an LDS bound over every launch of the restated plan, the host-side error returns, and the case
table of tests/test_attn_paths_gpu.py with the route every case claims.

(dtype, B, L, V, d, h, key_chunk, attention map or not, gradient type) become launches:

  forward    gen      attn_fuse_kernel<dt>                    the attention map is asked for, d % 16, h % 16 or h > 256.  QC words per block:
                                                              min(L, 32) halved until 4 (32 max(d + 1, h) + QC (d + V + h + 3)) <= 150 KiB
                                                              (VLG_ERR_SHAPE "exceed the LDS budget" when QC = 1 does not fit); above 60 KiB the
                                                              launch raises the kernel's dynamic-LDS attribute first
             mfma     attn_fuse_mfma_kernel<dt, T>            NC = 1.  T = 4 above 48 keys (64-key steps), else ceil(V / 16).  Tile body: f32; bf16
                                                              with T <= 3 widens on load (fp32 MFMAs); bf16 with T = 4 is the streaming tile
             split    attn_fuse_split_kernel<dt> (T = 4) +    NC > 1: AttnSplit.  key_chunk > 0: CK = 64 ceil(key_chunk / 64); V <= 256: one pass;
                      attn_merge_records_kernel +             else the cost model rounds(B WT NC / 1024) x per x 2 + B WT NC x 0.008 over per =
                      attn_fuse_combine_kernel<dt>            1 .. ceil(V / 64) steps per chunk, ties to the larger per (which can be one pass)
  adjoint    one      attn_fuse_bwd_words_kernel<dt, g, T, FTM>   NC = 1;  FTM = 16 above 128 features, else 8
             split    [split + merge unless `saved`] + attn_bwd_combine_kernel<dt, g> + attn_bwd_sweep_kernel<dt, FTM> + attn_bwd_dtxt_kernel<g>;
                      sweep bodies: f32 (FTM 8 | 16), bf16 streaming (FTM = 8), bf16 non-streaming (d > 128)
             then     attn_bwd_regions_bf16_kernel<g, FTM> (bf16 features; bf16 P^T / dS^T scratch [b][word tile][Vp][16]) or
                      attn_fuse_bwd_regions_kernel<f32, f32, FTM> (float32 scratch [b][Vp][Lp]), and attn_fuse_bwd_affine_kernel over B WT rows

CASES: every id names group, dtype, shape, key_chunk, the claimed forward and adjoint descriptors (mfma.<dt>.T<T>, split.<dt>.CK<CK>.NC<NC>,
gen.QC<QC>; bwd.one.<dt>.T<T>.FTM<FTM>, bwd.split.f32.FTM<FTM>, bwd.split.bf16.stream | d256; `nobwd` where the adjoint does not take the shape
or the row is about the attention map) and the side of the boundary the row sits on.  The GPU file runs every row on two input sets
(inputs(): `random`, the suite's normal(0, 0.4) features, and `planted`, below) and the adjoint with float32 and, for bf16 features, bf16
gradients.  Pair counts B NC of the split grid: 1 cannot occur on this route (NC > 1); the rows hold 2, 3, 7, 8, 9.

Planted peaks (inputs(c, "planted")).  boundary_keys(): V - 1, 0, CK - 1, CK, the first key of the last chunk, 63, 64, 16 t - 1 and 16 t for
t <= T, the first key of the last 64-key step (the first d of them).  Key k_j of sentence b is vis[b, k_j] = 4 e_((j + b) mod J); every other key
row holds integers in [-4, 4] / 64; planted word i (the last word, the first word of the last tile, the first word of every tile, then the
words in order until every key has one) is txt = 4 e_((i mod J + b) mod J): score 16 on its key, 0 on the other planted keys, at most
0.25 d' on the rest (d' <= 1 non-zero coordinate), so its softmax weight on its key is >= 1 / (1 + V e^-15.75) > 0.9997 at V = 1369;
test_planted_words_sit_on_their_keys asserts >= 0.9 in float64 for every row.  vis_mid[b, v, c] = ((v + 1)(2 c + 1) mod 11 - 5 +
(b + 1) c^2 mod 3 - 1) / 4, of order 1 as features are (float32 rounding in dS = P (dP - D) grows with |vis_mid| h): rows of neighbouring
keys and of neighbouring sentences differ by more than a constant (which the LayerNorm would remove), so a dropped, duplicated or
misplaced boundary key, or a row of the next sentence, moves `out` of
the planted word and d_vis_mid of the key by O(1).  All planted values are exact in bf16.

Streaming-softmax numerics (numerics_inputs): scores 8 (k // 64) + (k % 64) / 8 (a ragged last step still tops the step before; x the word's
scale 1 or 3 / 4, + at most 0.25 from four small coordinates) with either sign -- the step maximum rises, or falls, at every 64-key step,
by more than 100 over 1369 keys: later chunks merge with exp(-large) = 0 --, one 64-key chunk lifted by 128, or every score offset by +-256.
The magnitude sits in txt (128, 96, 256), not in vis (<= 1.32): bf16 features enter the adjoint's products with dS as single bf16 values by
design, so d_txt = dS . vis carries up to 2^-9 sum_k |dS_k| |vis_k|, and the suite's 1e-2 max(1, |g|max) presumes key features of order 1.
stream32() restates the streaming computation in float32 numpy (float32 scores,
64-key steps, chunk records merged in chunk order, float32 adjoint from the merged statistics); the GPU file allows max(project
tolerance, 8 x its error against the float64 oracle).  Measured on the CPU (largest over the elements; B = 2, L = 17, d = h = 32;
every key_chunk of NUMERICS_SHAPES within 2 x these figures; d_beta is exact):
  case       V      out       d_vis (|ref|max)     d_txt     d_vis_mid  d_enc_x   d_gamma
  rise       300    3.7e-07   3.3e-05 (2.8e+02)    8.3e-08   7.3e-08    1.5e-07   2.4e-06
  fall       300    5.6e-07   6.7e-05 (2.3e+02)    2.8e-08   9.5e-08    2.1e-07   2.0e-06
  dominated  300    6.2e-07   1.1e-04 (9.4e+02)    1.6e-07   1.4e-07    1.8e-07   1.3e-06
  plus256    300    3.5e-07   1.2e-04 (6.5e+02)    2.4e-07   8.7e-08    1.7e-07   1.3e-06
  minus256   300    5.4e-07   1.2e-04 (7.8e+02)    3.1e-07   9.8e-08    1.6e-07   1.7e-06
  rise       1369   4.2e-07   3.7e-05 (2.6e+02)    3.4e-07   6.4e-08    1.3e-07   1.3e-06
  fall       1369   5.2e-07   3.6e-05 (3.5e+02)    5.6e-08   8.4e-08    1.4e-07   1.5e-06
  dominated  1369   3.5e-07   1.2e-04 (8.5e+02)    1.3e-07   7.1e-08    1.4e-07   9.6e-07
  plus256    1369   4.4e-07   1.3e-04 (6.3e+02)    3.1e-07   1.0e-07    1.5e-07   2.1e-06
  minus256   1369   3.6e-07   7.9e-05 (4.3e+02)    2.8e-07   9.4e-08    1.4e-07   2.2e-06
8 x these stay below the project tolerance (1e-4 for out, 1e-4 max(1, |g|max) for the gradients) in every case, so it decides.
"""
import collections
import ctypes
import functools
import itertools
import os
import re
import zlib

import numpy as np
import pytest

from conftest import ROOT

# ---------------------------------------------------------------------------------------------------------------- the restatement
F32, BF16 = 0, 1
ERR_SHAPE, ERR_DTYPE, ERR_ARG, ERR_WORKSPACE = 0x1001, 0x1002, 0x1003, 0x1004
LDS_LIMIT = 160 * 1024
GEN_LDS_RULE, GEN_ATTR_ABOVE = 150 * 1024, 60 * 1024
K_FT, MAX_CT, MAX_FT = 32, 16, 16
STAGE_BYTES = 2 * 32 * 160
SWEEP_BYTES = 64 * 288


def cdiv(a, b):
    return (a + b - 1) // b


def rec_floats(h):
    return (h >> 4) * 256 + 32


Split = collections.namedtuple("Split", "WT CK NC")


@functools.lru_cache(maxsize=None)
def attn_split(B, L, V, key_chunk):
    """AttnSplit"""
    WT, tiles = cdiv(L, 16), cdiv(V, 64)
    if key_chunk > 0:
        per = cdiv(key_chunk, 64)
    elif V <= 256:
        per = tiles
    else:
        waves, best, per = B * WT, 1e30, tiles
        for cand in range(1, tiles + 1):
            w = waves * cdiv(tiles, cand)
            cost = float(cdiv(w, 1024)) * cand * 2.0 + float(w) * 0.008
            if cost < best - 1e-9 or (cost < best + 1e-9 and cand > per):
                best, per = cost, cand
    per = max(min(per, tiles), 1)
    return Split(WT, 64 * per, cdiv(tiles, per))


def workspace_fwd(B, L, V, h, key_chunk):
    """vlg_attn_fuse_workspace"""
    if B < 1 or L < 1 or V < 1 or h < 16:
        return 0
    sp = attn_split(B, L, V, key_chunk)
    return 4 * (B * sp.WT * sp.NC + B * sp.WT) * rec_floats(h) if sp.NC > 1 else 0


def saved_bytes(B, L, V, h, key_chunk):
    """vlg_attn_fuse_saved_bytes"""
    if B < 1 or L < 1 or V < 1 or h < 16:
        return 0
    sp = attn_split(B, L, V, key_chunk)
    return 4 * B * sp.WT * rec_floats(h) if sp.NC > 1 else 0


def tiles_of(V):
    return 4 if V > 48 else cdiv(V, 16)


def bwd_plan(B, L, V, d, h, gdt, key_chunk):
    """AttnBwdPlan: the carves in floats, in the order the launcher lays them out, and the byte count"""
    sp = attn_split(B, L, V, key_chunk)
    WT, T = cdiv(L, 16), tiles_of(V)
    Vp, Lp = cdiv(V, 16 * T) * 16 * T, 16 * WT
    per = max(rec_floats(h), (d >> 4) * 256)
    p = dict(sp=sp, WT=WT, T=T, Vp=Vp, Lp=Lp, pt=B * Vp * Lp, part=B * WT * 2 * h,
             rec=B * WT * sp.NC * per + B * WT * rec_floats(h) if sp.NC > 1 else 0, stats=B * WT * 48 if sp.NC > 1 else 0,
             dy=(B * L * h + 63) & ~63 if gdt == "bf16" else 0, tr=(B * (h + d) * Lp + 1) // 2)
    p["bytes"] = 4 * (2 * p["pt"] + p["part"] + p["rec"] + p["stats"] + p["dy"] + p["tr"])
    return p


def workspace_bwd(B, L, V, d, h, gdt, key_chunk):
    """vlg_attn_fuse_backward_workspace"""
    if B < 1 or L < 1 or V < 1 or d < 16 or h < 16:
        return 0
    return bwd_plan(B, L, V, d, h, gdt, key_chunk)["bytes"]


def generic_plan(L, V, d, h):
    """(QC, LDS bytes) of attn_fuse_kernel; QC = 0 where one word per block does not fit"""
    tile_f, per_q = K_FT * max(d + 1, h), (d + 1) + V + h + 2
    QC = min(L, 32)
    while QC > 1 and 4 * (tile_f + per_q * QC) > GEN_LDS_RULE:
        QC >>= 1
    lds = 4 * (tile_f + per_q * QC)
    return (QC, lds) if lds <= GEN_LDS_RULE else (0, lds)


def generic_v(QC, d, h, fits=GEN_LDS_RULE):
    """the largest V at which QC words per block ask for at most `fits` bytes"""
    return (fits // 4 - K_FT * max(d + 1, h)) // QC - (d + h + 3)


def _split_launches(dt, B, sp, h):
    pairs = B * sp.NC
    return [dict(k="attn_fuse_split_kernel", dt=dt, CK=sp.CK, NC=sp.NC, pairs=pairs, grid_x=cdiv(pairs, 8) * 8, lds=STAGE_BYTES),
            dict(k="attn_merge_records_kernel", lds=0)]


def forward(dt, B, L, V, d, h, key_chunk=0, attmap=False):
    """vlg_attn_fuse past its argument checks: the launches, or (code, message fragment)"""
    if B < 0 or L < 1 or V < 1 or d < 1 or h < 1:
        return ERR_SHAPE, "bad shape"
    if B == 0:
        return []
    if B > 65535:
        return ERR_SHAPE, "exceeds grid.y"
    if not attmap and d % 16 == 0 and h % 16 == 0 and h <= 16 * MAX_CT and V * h * 4 < 1 << 31:
        sp = attn_split(B, L, V, key_chunk)
        if sp.NC > 1:
            return _split_launches(dt, B, sp, h) + [dict(k="attn_fuse_combine_kernel", dt=dt, lds=4 * 16 * (h + 4))]
        T = tiles_of(V)
        return [dict(k="attn_fuse_mfma_kernel", dt=dt, T=T, body="f32" if dt == "f32" else ("stream" if T == 4 else "widen"), steps=cdiv(V, 16 * T),
                     lds=STAGE_BYTES + 4 * 16 * (h + 4))]
    QC, lds = generic_plan(L, V, d, h)
    if QC == 0:
        return ERR_SHAPE, "exceed the LDS budget"
    return [dict(k="attn_fuse_kernel", dt=dt, QC=QC, lds=lds, attr=lds > GEN_ATTR_ABOVE, blocks=cdiv(L, QC), halved=QC < min(L, 32))]


def backward(dt, gdt, B, L, V, d, h, key_chunk=0, saved=False):
    """vlg_attn_fuse_backward past its argument checks (B >= 1): the launches, or (code, message fragment)"""
    if B < 0 or L < 1 or V < 1 or d < 1 or h < 1:
        return ERR_SHAPE, "bad shape"
    if d % 16 or h % 16 or d > 16 * MAX_FT or h > 16 * MAX_CT:
        return ERR_SHAPE, "multiples of 16"
    if max(V, L) * max(d, h) * 4 >= 1 << 31:
        return ERR_SHAPE, "exceed 2 GiB"
    if B > 65535:
        return ERR_SHAPE, "exceeds grid.y"
    if gdt == "bf16" and dt != "bf16":
        return ERR_DTYPE, "grad_dtype"
    p = bwd_plan(B, L, V, d, h, gdt, key_chunk)
    sp, FTM, gsz = p["sp"], 16 if d > 128 else 8, 2 if gdt == "bf16" else 4
    if sp.NC > 1:
        body = f"f32.FTM{FTM}" if dt == "f32" else ("stream" if FTM == 8 else "d256")
        Ls = ([] if saved else _split_launches(dt, B, sp, h)) + \
            [dict(k="attn_bwd_combine_kernel", dt=dt, g=gdt, lds=4 * 32 * (h + 4)),
             dict(k="attn_bwd_sweep_kernel", dt=dt, FTM=FTM, body=body, pairs=B * sp.NC, lds=max(SWEEP_BYTES + 4096, STAGE_BYTES)),
             dict(k="attn_bwd_dtxt_kernel", g=gdt, lds=0)]
    else:
        Ls = [dict(k="attn_fuse_bwd_words_kernel", dt=dt, g=gdt, T=p["T"], FTM=FTM, lds=STAGE_BYTES + 4 * 32 * (h + 4))]
    if dt == "bf16":
        Ls.append(dict(k="attn_bwd_regions_bf16_kernel", g=gdt, FTM=FTM, lds=16 * (max(h, d) + 8) * gsz))
    else:
        Ls.append(dict(k="attn_fuse_bwd_regions_kernel", FTM=FTM, lds=0))
    return Ls + [dict(k="attn_fuse_bwd_affine_kernel", R=B * p["WT"], lds=4 * 1024)]


def image_of(l):
    k = l["k"]
    if k == "attn_fuse_mfma_kernel":
        return f"attn_fuse_mfma_kernel<{l['dt']}, {l['T']}>"
    if k == "attn_fuse_bwd_words_kernel":
        return f"attn_fuse_bwd_words_kernel<{l['dt']}, g{l['g']}, {l['T']}, {l['FTM']}>"
    if k == "attn_bwd_combine_kernel":
        return f"attn_bwd_combine_kernel<{l['dt']}, g{l['g']}>"
    if k == "attn_bwd_sweep_kernel":
        return f"attn_bwd_sweep_kernel<{l['dt']}, {l['FTM']}>"
    if k == "attn_bwd_dtxt_kernel":
        return f"attn_bwd_dtxt_kernel<g{l['g']}>"
    if k == "attn_bwd_regions_bf16_kernel":
        return f"attn_bwd_regions_bf16_kernel<g{l['g']}, {l['FTM']}>"
    if k == "attn_fuse_bwd_regions_kernel":
        return f"attn_fuse_bwd_regions_kernel<f32, gf32, {l['FTM']}>"
    if k in ("attn_fuse_kernel", "attn_fuse_split_kernel", "attn_fuse_combine_kernel"):
        return f"{k}<{l['dt']}>"
    return k


DG = (("f32", "f32"), ("bf16", "f32"), ("bf16", "bf16"))      # (features, gradients) the library builds
IMAGES = [f"{k}<{dt}>" for k in ("attn_fuse_kernel", "attn_fuse_split_kernel", "attn_fuse_combine_kernel") for dt in ("f32", "bf16")] + \
    [f"attn_fuse_mfma_kernel<{dt}, {T}>" for dt in ("f32", "bf16") for T in (1, 2, 3, 4)] + ["attn_merge_records_kernel", "attn_fuse_bwd_affine_kernel"] + \
    [f"attn_fuse_bwd_words_kernel<{dt}, g{g}, {T}, {F}>" for dt, g in DG for T in (1, 2, 3, 4) for F in (8, 16)] + \
    [f"attn_bwd_combine_kernel<{dt}, g{g}>" for dt, g in DG] + [f"attn_bwd_sweep_kernel<{dt}, {F}>" for dt in ("f32", "bf16") for F in (8, 16)] + \
    [f"attn_bwd_dtxt_kernel<g{g}>" for g in ("f32", "bf16")] + [f"attn_bwd_regions_bf16_kernel<g{g}, {F}>" for g in ("f32", "bf16") for F in (8, 16)] + \
    [f"attn_fuse_bwd_regions_kernel<f32, gf32, {F}>" for F in (8, 16)]


def fwd_desc(Ls):
    if isinstance(Ls, tuple):
        return f"err{Ls[0]:x}"
    l = Ls[0]
    if l["k"] == "attn_fuse_kernel":
        return f"gen.QC{l['QC']}"
    if l["k"] == "attn_fuse_mfma_kernel":
        return f"mfma.{l['dt']}.T{l['T']}"
    return f"split.{l['dt']}.CK{l['CK']}.NC{l['NC']}"


def bwd_desc(Ls):
    if isinstance(Ls, tuple):
        return "nobwd"
    for l in Ls:
        if l["k"] == "attn_fuse_bwd_words_kernel":
            return f"bwd.one.{l['dt']}.T{l['T']}.FTM{l['FTM']}"
        if l["k"] == "attn_bwd_sweep_kernel":
            return f"bwd.split.{l['dt']}.{l['body'] if l['dt'] == 'bf16' else l['body'][4:]}"


# ---------------------------------------------------------------------------------------------------------------- the case table
Case = collections.namedtuple("Case", "group dt B L V d h ck attmap fwd bwd side")
CASES = []
DTS = ("f32", "bf16")


def case_id(c):
    return f"{c.group}-{c.dt}-B{c.B}-L{c.L}-V{c.V}-d{c.d}-h{c.h}-ck{c.ck}{'-att' if c.attmap else ''}-{c.fwd}-{c.bwd}-{c.side}"


def derive(c):
    """(forward descriptor, adjoint descriptor) of a row under the restatement"""
    f = fwd_desc(forward(c.dt, c.B, c.L, c.V, c.d, c.h, c.ck, c.attmap))
    return f, ("nobwd" if c.attmap else bwd_desc(backward(c.dt, "f32", c.B, c.L, c.V, c.d, c.h, c.ck)))


def launches(c):
    """[(call, launches)] of a row: the forward, and the adjoint per gradient type, with and without the saved records"""
    out = [("fwd", forward(c.dt, c.B, c.L, c.V, c.d, c.h, c.ck, c.attmap))]
    if c.bwd != "nobwd":
        for g in ("f32", "bf16") if c.dt == "bf16" else ("f32",):
            for saved in (False, True):
                out.append((f"bwd g{g}{' saved' if saved else ''}", backward(c.dt, g, c.B, c.L, c.V, c.d, c.h, c.ck, saved)))
    return [(call, L) for call, L in out if isinstance(L, list)]


def _bwd_name(dt, V, d, split):
    FTM = 16 if d > 128 else 8
    if not split:
        return f"bwd.one.{dt}.T{tiles_of(V)}.FTM{FTM}"
    return f"bwd.split.f32.FTM{FTM}" if dt == "f32" else f"bwd.split.bf16.{'stream' if FTM == 8 else 'd256'}"


def one(group, dt, V, side, B=2, L=17, d=32, h=32, ck=0):
    CASES.append(Case(group, dt, B, L, V, d, h, ck, False, f"mfma.{dt}.T{tiles_of(V)}", _bwd_name(dt, V, d, False), side))


def split(group, dt, V, ck, CK, NC, side, B=2, L=17, d=32, h=32):
    CASES.append(Case(group, dt, B, L, V, d, h, ck, False, f"split.{dt}.CK{CK}.NC{NC}", _bwd_name(dt, V, d, True), side))


def gen(group, dt, V, QC, side, B=2, L=17, d=32, h=32, attmap=False):
    CASES.append(Case(group, dt, B, L, V, d, h, 0, attmap, f"gen.QC{QC}", "nobwd", side))


MFMA_V = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 255, 256)
WORD_L = (1, 15, 16, 17, 31, 32, 33)
FEAT_D = (16, 32, 48, 112, 128, 144, 160, 256)
CHAN_H = (16, 48, 64, 80, 240, 256)
AFFINE_ROWS = {1: (1, 1), 15: (3, 80), 16: (2, 128), 17: (1, 272), 33: (3, 176)}       # B WT: (B, L)
GEN_HALVE_V = generic_v(32, 32, 32) + 1              # d = h = 32: the first V at which 32 words per block do not fit (1101)
GEN_ATTR_V = generic_v(8, 32, 32, GEN_ATTR_ABOVE)    # d = h = 32, L = 8: the last V whose request stays at 60 KiB (1721)
AUTO_PLANS = {(70, 40, 321): (128, 3), (86, 40, 257): (192, 2), (64, 40, 1369): (320, 5), (1024, 16, 257): (320, 1), (2, 17, 300): (64, 5),
              (2, 40, 1369): (64, 22), (256, 40, 1369): (1408, 1)}      # (B, L, V): (CK, NC) of key_chunk = 0

for dt in DTS:
    for V in MFMA_V:          # T = ceil(V / 16) up to 48 keys, 64-key steps above: one key and 63 keys in the last step
        one("T", dt, V, f"V{V}-steps{cdiv(V, 16 * tiles_of(V))}-last{(V - 1) % (16 * tiles_of(V)) + 1}")
    for V in (16, 32, 48, 64):      # every T with sixteen feature tiles in the adjoint
        one("Tftm16", dt, V, f"V{V}", d=144)
    for V in (36, 130):
        for L in WORD_L:
            one("words", dt, V, f"L{L}-wt{cdiv(L, 16)}", L=L)
        for h in CHAN_H:
            one("chan", dt, V, f"h{h}-ct{h // 16}", h=h)
    for d in FEAT_D:
        one("feat", dt, 36, f"d{d}-tail{d % 32}" if d < 128 else f"d{d}-second{d - 128}", d=d)
    for d in (16, 48, 112):       # the streaming bf16 tile with a short first chunk
        one("feat", dt, 130, f"d{d}-tail{d % 32}-streamed", d=d)
    one("feat", dt, 130, "d160-second32-streamed", d=160)
    # key-split, explicit key_chunk: V on both sides of a chunk end
    for CK in (64, 128, 192):
        for V, side in ((2 * CK - 1, "lastkeyofchunk"), (2 * CK, "wholechunks"), (2 * CK + 1, "onekeychunk")):
            split("ck", dt, V, CK, CK, cdiv(V, CK), f"{side}-pairs{2 * cdiv(V, CK)}")
    split("ck", dt, 161, 100, 128, 2, "keychunk100-roundedup-pairs4")
    for B, V, side in ((1, 128, "pairs2-pad6"), (1, 129, "pairs3-pad5"), (1, 448, "pairs7-pad1"), (2, 256, "pairs8-pad0"), (3, 129, "pairs9-pad7")):
        split("pairs", dt, V, 64, 64, cdiv(V, 64), side, B=B)
    for d in (16, 32, 48, 112, 128, 144, 256):      # the sweep bodies: streaming (d <= 128) and d > 128
        split("feat", dt, 300, 64, 64, 5, f"d{d}", d=d)
    for h in CHAN_H:
        split("chan", dt, 300, 64, 64, 5, f"h{h}-ct{h // 16}", h=h)
    for L in WORD_L:
        split("words", dt, 300, 128, 128, 3, f"L{L}-wt{cdiv(L, 16)}", L=L)
    # key_chunk = 0 on both sides of 256 keys, and the automatic plans
    one("auto", dt, 256, "V256-onepass-ws0")
    for (B, L, V), (CK, NC) in AUTO_PLANS.items():
        if (B, V) == (256, 1369):
            continue      # (pinned by test_automatic_plans; 14 M scores per pass are not a quick case)
        if NC > 1:
            split("auto", dt, V, 0, CK, NC, f"plan-per{CK // 64}", B=B, L=L)
        else:
            one("auto", dt, V, "plan-onepass-above256", B=B, L=L)
    split("auto", dt, 257, 0, 64, 5, "V257-NC5")
    # the shipped layout (V = 1369, d = 128, h = 256) under the two plans the benchmark's batches get, asked for by key_chunk at B = 2
    split("shipped", dt, 1369, 320, 320, 5, "planofB64", L=40, d=128, h=256)
    one("shipped", dt, 1369, "planofB256-22steps", L=40, d=128, h=256, ck=1408)
    # the affine reduction's 16 row groups
    for rows, (B, L) in AFFINE_ROWS.items():
        one("affine", dt, 36, f"rows{rows}", B=B, L=L)
    split("affine", dt, 129, 64, 64, 3, "rows17", B=1, L=272)
    # the generic route
    gen("gen", dt, 36, 17, "attmap", attmap=True)
    gen("gen", dt, 36, 17, "d24", d=24)
    gen("gen", dt, 36, 17, "h72", h=72)
    gen("gen", dt, 36, 17, "h272", h=272)
    gen("gen", dt, 300, 17, "d24-V300", d=24)
    gen("gen", dt, GEN_HALVE_V - 1, 32, "L33-lastVofQC32", L=33, attmap=True)
    gen("gen", dt, GEN_HALVE_V, 16, "L33-halved", L=33, attmap=True)
    gen("gen", dt, GEN_HALVE_V, 16, "L64-halved", L=64, attmap=True)
    gen("gen", dt, GEN_HALVE_V, 13, "L13-nothalved", L=13, attmap=True)
    # (2268 keys: the softmax sum and the output sum of attn_fuse_kernel run over 71 key tiles)
    gen("gen", dt, generic_v(16, 32, 32) + 1, 8, "L33-halvedtwice", L=33, attmap=True)
    gen("gen", dt, GEN_ATTR_V, 8, "L8-lds61440-noattribute", L=8, attmap=True)
    gen("gen", dt, GEN_ATTR_V + 1, 8, "L8-lds61472-attribute", L=8, attmap=True)


# rows the other tests of the GPU file run on: one per route family
FAMILIES = [("mfma-widen", dict(V=36, ck=0)), ("mfma-stream", dict(V=130, ck=0)), ("split", dict(V=300, ck=64)), ("split-d256", dict(V=300, ck=64, d=144))]
LDS_ERROR_SHAPE = dict(B=1, L=1, V=40000, d=24, h=16)      # one word per block asks for 4 (800 + 40043) = 163372 bytes


# ---------------------------------------------------------------------------------------------------------------- inputs
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def bf16_round(a):
    """float64 values of the nearest bf16 (ties to even)"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def to_type(a, dt):
    return bf16_round(a) if dt == "bf16" else np.asarray(a, dtype=np.float32).astype(np.float64)


def plan_of(c):
    """(T, CK, NC) the keys of a row stream through (generic route: one pass, T from V)"""
    if c.fwd.startswith("split"):
        sp = attn_split(c.B, c.L, c.V, c.ck)
        return 4, sp.CK, sp.NC
    return tiles_of(c.V), 64 * cdiv(c.V, 64), 1


def boundary_keys(V, T, CK, NC, d):
    ks = [V - 1, 0]
    if NC > 1:
        ks += [CK - 1, CK, (NC - 1) * CK]
    ks += [63, 64]
    for t in range(1, T + 1):
        ks += [16 * t - 1, 16 * t]
    ks.append((cdiv(V, 64) - 1) * 64)
    out = []
    for k in ks:
        if 0 <= k < V and k not in out:
            out.append(k)
    return out[:d]


def planted_words(L, J):
    WT = cdiv(L, 16)
    order = [L - 1, 16 * (WT - 1)] + [16 * t for t in range(WT)] + list(range(L))
    out = []
    for w in order:
        if w not in out:
            out.append(w)
    return out[:min(L, max(J, WT + 1))]


Inputs = collections.namedtuple("Inputs", "vis txt mid enc gamma beta dout plant")


@functools.lru_cache(maxsize=6)
def _inputs(dt, B, L, V, d, h, T, CK, NC, kind):
    rng = _rng(kind, B, L, V, d, h)
    vis, txt = rng.standard_normal((B, V, d)) * 0.4, rng.standard_normal((B, L + 1, d)) * 0.4
    mid, enc = rng.standard_normal((B, V, h)), rng.standard_normal((B, L, h))
    gamma, beta, dout = rng.random(h) + 0.5, rng.standard_normal(h), rng.standard_normal((B, L, h))
    plant = []
    if kind == "planted":
        keys = boundary_keys(V, T, CK, NC, d)
        J, words = len(keys), planted_words(L, len(keys))
        vis = rng.integers(-4, 5, (B, V, d)) / 64.0
        ch = np.arange(h)[None, None, :]
        mid = (((np.arange(V)[None, :, None] + 1) * (2 * ch + 1)) % 11 - 5 + ((np.arange(B)[:, None, None] + 1) * ch * ch) % 3 - 1) / 4.0
        for b in range(B):
            for j, k in enumerate(keys):
                vis[b, k] = 0.0
                vis[b, k, (j + b) % J] = 4.0
            for i, w in enumerate(words):
                txt[b, 1 + w] = 0.0
                txt[b, 1 + w, (i % J + b) % J] = 4.0
                plant.append((b, w, keys[i % J]))
    vis, txt, mid, enc = (to_type(a, dt) for a in (vis, txt, mid, enc))
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    return Inputs(vis, txt, mid, enc, f32(gamma), f32(beta), f32(dout), tuple(plant))


def inputs(c, kind):
    """the float64 values of a row's operands, exact in the row's type: kind `random` or `planted`"""
    return _inputs(c.dt, c.B, c.L, c.V, c.d, c.h, *plan_of(c), kind)


NUMERICS = ("rise", "fall", "dominated", "plus256", "minus256")
NUMERICS_SHAPES = ((300, 64), (300, 128), (1369, 64), (1369, 320), (1369, 0), (300, 300))      # (V, key_chunk); 128, 320: two and five steps per chunk (the
# running maximum rescales inside attn_fuse_split_kernel and the sweep); 0: the automatic plan (CK = 64 at this batch); key_chunk >= V: the one-pass T = 4 route


@functools.lru_cache(maxsize=4)
def numerics_inputs(name, dt, V, B=2, L=17, d=32, h=32):
    rng = _rng("numerics", name, V)
    k = np.arange(V)
    vis = np.zeros((B, V, d))
    vis[:, :, 0], vis[:, :, 1] = (0.0 if name == "dominated" else (k // 64) / 16.0), (k % 64) / 1024.0
    vis[:, :, 4:8] = rng.integers(-4, 5, (B, V, 4)) / 64.0
    txt = np.zeros((B, L + 1, d))
    sign = -1.0 if name in ("fall", "minus256") else 1.0
    scale = np.where(np.arange(L) % 2 == 0, 128.0, 96.0)
    txt[:, 1:, 0] = txt[:, 1:, 1] = sign * scale
    txt[:, 1:, 4:8] = rng.integers(-4, 5, (B, L, 4)) / 4.0
    txt[:, 0] = 1.0
    if name in ("plus256", "minus256"):
        vis[:, :, 2], txt[:, 1:, 2] = 1.0, sign * 256.0
    if name == "dominated":
        vis[:, 64:128, 3], txt[:, 1:, 3] = 0.5, 256.0
    mid, enc = rng.integers(-8, 9, (B, V, h)) / 4.0, rng.integers(-8, 9, (B, L, h)) / 4.0
    gamma, beta, dout = rng.integers(2, 7, h) / 4.0, rng.integers(-4, 5, h) / 4.0, rng.integers(-8, 9, (B, L, h)) / 8.0
    for a in (vis, txt, mid, enc):
        assert np.array_equal(bf16_round(a), a)
    return Inputs(vis, txt, mid, enc, gamma, beta, dout, ())


GRAD_NAMES = ("d_vis", "d_txt", "d_vis_mid", "d_enc_x", "d_gamma", "d_beta")


def oracle_reference(oracle, x):
    """float64: dict(att, out, d_vis, d_txt, d_vis_mid, d_enc_x, d_gamma, d_beta)"""
    att, out = oracle.attn_fuse(x.vis, x.txt, x.mid, x.enc, x.gamma, x.beta, 1e-5, np.float64)
    grads = oracle.attn_fuse_backward(x.vis, x.txt, x.mid, x.enc, x.gamma, x.dout, 1e-5, np.float64)
    return dict(att=att, out=out, **dict(zip(GRAD_NAMES, grads)))


def stream32(x, CK, eps=1e-5):
    """The streaming computation restated in float32 numpy: float32 scores, 64-key steps inside chunks of CK keys with a running maximum and
    rescales, chunk records (max, sum, unnormalised Y) merged in chunk order, LayerNorm, and the adjoint from the merged statistics.
    Returns the same dict as oracle_reference (without att)."""
    f = np.float32
    vis, txt, mid, enc, gamma, beta, dout = (np.asarray(a, dtype=f) for a in x[:7])
    B, V, d = vis.shape
    L, h = txt.shape[1] - 1, mid.shape[2]
    S = np.einsum("bld,bvd->blv", txt[:, 1:], vis).astype(f)
    recs = []
    for c0 in range(0, V, CK):
        m_run, z_run, Y = np.full((B, L), -np.inf, f), np.zeros((B, L), f), np.zeros((B, L, h), f)
        for v0 in range(c0, min(V, c0 + CK), 64):
            s = S[:, :, v0:min(V, c0 + CK, v0 + 64)]
            m = np.maximum(m_run, s.max(-1))
            r = np.exp(m_run - m).astype(f)
            p = np.exp(s - m[..., None]).astype(f)
            z_run = (z_run * r + p.sum(-1, dtype=f)).astype(f)
            Y = (Y * r[..., None] + np.einsum("blv,bvh->blh", p, mid[:, v0:v0 + p.shape[2]])).astype(f)
            m_run = m
        recs.append((m_run, z_run, Y))
    m = functools.reduce(np.maximum, [r[0] for r in recs])
    z, Y = np.zeros((B, L), f), np.zeros((B, L, h), f)
    for mc, zc, Yc in recs:
        w = np.exp(mc - m).astype(f)
        z, Y = (z + w * zc).astype(f), (Y + w[..., None] * Yc).astype(f)
    M = (Y / z[..., None]).astype(f)
    y = enc + M
    mean = y.mean(-1, keepdims=True, dtype=f)
    rstd = (1 / np.sqrt(((y - mean) ** 2).mean(-1, keepdims=True, dtype=f) + f(eps))).astype(f)
    yh = (y - mean) * rstd
    res = dict(out=yh * gamma + beta, d_beta=dout.sum((0, 1), dtype=f), d_gamma=(dout * yh).sum((0, 1), dtype=f))
    dyh = dout * gamma
    dy = (rstd * (dyh - dyh.mean(-1, keepdims=True, dtype=f) - yh * (dyh * yh).mean(-1, keepdims=True, dtype=f))).astype(f)
    P = (np.exp(S - m[..., None]) / z[..., None]).astype(f)
    dP = np.einsum("blh,bvh->blv", dy, mid).astype(f)
    dS = (P * (dP - (dy * M).sum(-1, keepdims=True, dtype=f))).astype(f)
    d_txt = np.zeros_like(txt)
    d_txt[:, 1:] = np.einsum("blv,bvd->bld", dS, vis)
    res.update(d_vis=np.einsum("blv,bld->bvd", dS, txt[:, 1:]), d_txt=d_txt, d_vis_mid=np.einsum("blv,blh->bvh", P, dy), d_enc_x=dy)
    return {k: np.asarray(v, dtype=np.float64) for k, v in res.items()}


def numerics_error(oracle, name, V, ck):
    """{output: largest |stream32 - float64 oracle|}, and the oracle's results"""
    x = numerics_inputs(name, "f32", V)
    CK = attn_split(x.vis.shape[0], x.txt.shape[1] - 1, V, ck).CK
    ref, got = oracle_reference(oracle, x), stream32(x, CK)
    return {k: float(np.abs(got[k] - ref[k]).max()) for k in got}, ref


# ---------------------------------------------------------------------------------------------------------------- tests
SWEEP_B = (1, 2, 3, 15, 64, 70, 86, 256, 1024)
SWEEP_L = (1, 16, 17, 40, 272)
SWEEP_V = (1, 16, 17, 48, 49, 64, 65, 255, 256, 257, 300, 320, 321, 1369, 2000)
SWEEP_DH = ((32, 32), (128, 256), (144, 80), (16, 16))
SWEEP_CK = (0, 1, 64, 100, 128, 192, 320, 5000)


def sweep_shapes():
    s = set(itertools.product(SWEEP_B, SWEEP_L, SWEEP_V, SWEEP_DH[:2], (0,))) | set(itertools.product(SWEEP_B[:4], SWEEP_L[:4], SWEEP_V, SWEEP_DH, SWEEP_CK))
    for V in (257, 320, 321, 1369):      # every (B, L) with B WT around 1024 / NC: where the cost model's round count steps
        for nc in range(1, cdiv(V, 64) + 1):
            for waves in range(max(1, 1024 // nc - 2), 1024 // nc + 3):
                s.add((waves, 16, V, (32, 32), 0))
                for WT in (2, 3):
                    if waves % WT == 0:
                        s.add((waves // WT, 16 * WT - 5, V, (32, 32), 0))
    return s | {(c.B, c.L, c.V, (c.d, c.h), c.ck) for c in CASES}


@pytest.fixture(scope="module")
def lib():
    from vlgae_amd.build import build_library
    build_library()            # hipcc cross-compiles for gfx950 without a GPU
    from vlgae_amd import _C
    return _C.lib()


def test_constants_read_from_the_source():
    s = open(os.path.join(ROOT, "vlgae_amd", "csrc", "vlg_attn.hip")).read()
    one = lambda pat: (lambda f: f[0] if len(f) == 1 else pytest.fail(f"{pat}: {f}"))(re.findall(pat, s))
    assert int(one(r"constexpr int kFT = (\d+);")) == K_FT and int(one(r"constexpr int kAttnMaxCT = (\d+);")) == MAX_CT
    assert int(one(r"constexpr int kAttnMaxFT = (\d+);")) == MAX_FT
    assert int(one(r"constexpr int kStagePitch = (\d+);")) * 64 == STAGE_BYTES and one(r"constexpr int kStageBytes = (.*?);") == "2 * 32 * kStagePitch"
    assert int(one(r"constexpr int kSweepPitch = (\d+);")) * 64 == SWEEP_BYTES and one(r"constexpr int kSweepBytes = (.*?);") == "64 * kSweepPitch"
    assert one(r"sizeof\(float\) \* \(tile_f \+ per_q \* QC\) > (\d+) \* 1024\) QC >>= 1;") == "150"
    # the generic kernel goes through vlg::launch like every other, whose one threshold for raising the dynamic-LDS limit is the HIP default:
    # the 60 KiB the restatement still marks (GEN_ATTR_ABOVE) lies below it, so both rows about it launch without the attribute call
    launch_h = open(os.path.join(ROOT, "vlgae_amd", "csrc", "vlg_launch.h")).read()
    assert re.findall(r"constexpr size_t kDefaultDynamicLds = (\d+) \* 1024;", launch_h) == ["64"] and len(re.findall(r"if \(lds > kDefaultDynamicLds\) \{", launch_h)) == 1
    assert len(re.findall(r'launch\("attn_fuse_kernel", attn_fuse_kernel<INV>, dim3\(\(L \+ QC - 1\) / QC, B\), dim3\(kAlignThreads\), lds, s,', s)) == 1
    assert GEN_ATTR_ABOVE < 64 * 1024 and "hipFuncSetAttribute" not in s
    assert one(r"cost = \(double\)\(\(w \+ 1023\) / 1024\) \* cand \* ([\d.]+) \+ \(double\)w \* ([\d.]+);") == ("2.0", "0.008")
    assert one(r"return \(size_t\)\(h >> 4\) \* (\d+) \+ (\d+); \}") == ("256", "32")
    assert one(r"T = V > (\d+) \? 4 : \(V \+ 15\) / 16;") == "48" and one(r"switch \(V > (\d+) \? 4 : \(V \+ 15\) / 16\)") == "48"
    assert one(r"else if \(V <= (\d+)\) per = tiles;") == "256"


def test_size_queries_reproduce_the_restated_plan(lib):
    """vlg_attn_fuse_workspace, vlg_attn_fuse_saved_bytes and vlg_attn_fuse_backward_workspace (both gradient types) over the sweep and every
    row of the case table; NC read back from the forward workspace equals the restated NC."""
    shapes = sorted(sweep_shapes())
    assert len(shapes) >= 2000
    wrong = []
    for B, L, V, (d, h), ck in shapes:
        got = (lib.vlg_attn_fuse_workspace(B, L, V, h, ck), lib.vlg_attn_fuse_saved_bytes(B, L, V, h, ck),
               lib.vlg_attn_fuse_backward_workspace(B, L, V, d, h, F32, ck), lib.vlg_attn_fuse_backward_workspace(B, L, V, d, h, BF16, ck))
        want = (workspace_fwd(B, L, V, h, ck), saved_bytes(B, L, V, h, ck), workspace_bwd(B, L, V, d, h, "f32", ck), workspace_bwd(B, L, V, d, h, "bf16", ck))
        sp = attn_split(B, L, V, ck)
        nc = got[0] // (4 * rec_floats(h) * B * sp.WT) - 1 if got[0] else 1
        if got != want or nc != sp.NC or (got[0] and got[0] % (4 * rec_floats(h) * B * sp.WT)):
            wrong.append(((B, L, V, d, h, ck), got, want, nc, sp))
    assert not wrong, (len(wrong), wrong[:10])
    for args in ((0, 17, 36, 32, 0), (2, 0, 36, 32, 0), (2, 17, 0, 32, 0), (2, 17, 300, 15, 64)):
        assert lib.vlg_attn_fuse_workspace(*args) == 0 == workspace_fwd(*args) and lib.vlg_attn_fuse_saved_bytes(*args) == 0 == saved_bytes(*args)
    assert lib.vlg_attn_fuse_backward_workspace(2, 17, 36, 15, 32, F32, 0) == 0 == workspace_bwd(2, 17, 36, 15, 32, "f32", 0)


def test_automatic_plans():
    """key_chunk = 0: one pass up to 256 keys; above, the cost model's plan -- the plans the benchmark runs (B = 64 and B = 256 at L = 40,
    V = 1369) and the rows of the table with more than one 64-key step per chunk, or a single pass above 256 keys."""
    for (B, L, V), (CK, NC) in AUTO_PLANS.items():
        sp = attn_split(B, L, V, 0)
        assert (sp.CK, sp.NC) == (CK, NC), ((B, L, V), sp)
    assert attn_split(2, 17, 256, 0) == Split(2, 256, 1) and workspace_fwd(2, 17, 256, 32, 0) == 0 and attn_split(2, 17, 257, 0) == Split(2, 64, 5)
    # (86, 40, 257): the last chunk holds two steps, the second a single key
    assert 257 - 192 == 65
    # 1024 waves at 5 steps: per = 5 costs 1 x 5 x 2 + 8.192, per = 1 costs 5 x 1 x 2 + 40.96: a single pass above 256 keys
    assert attn_split(1024, 16, 257, 0).NC == 1 and attn_split(1, 16, 257, 0).CK == 64
    # explicit key_chunk: rounded up to 64-key steps, clamped to the sentence
    assert attn_split(2, 17, 161, 100) == Split(2, 128, 2) and attn_split(2, 17, 161, 5000) == Split(2, 192, 1) and attn_split(2, 17, 161, 1) == Split(2, 64, 3)


def lds_violations():
    bad = []
    for B, L, V, (d, h), ck in sorted(sweep_shapes()):
        for dt in DTS:
            calls = [("fwd", forward(dt, B, L, V, d, h, ck)), ("fwd att", forward(dt, B, L, V, d, h, ck, True)), ("fwd d+8", forward(dt, B, L, V, d + 8, h, ck))]
            calls += [(f"bwd g{g}", backward(dt, g, B, L, V, d, h, ck)) for g in DTS]
            for call, Ls in calls:
                for l in Ls if isinstance(Ls, list) else []:
                    if l["lds"] > LDS_LIMIT or (l["k"] == "attn_fuse_kernel" and l["lds"] > GEN_LDS_RULE):
                        bad.append((call, dt, B, L, V, d, h, ck, image_of(l), l["lds"]))
    return bad


def test_every_launch_fits_the_lds(lib):
    """No launch of the restated plan asks for more than 160 KiB of LDS, and the generic kernel keeps to its own 150 KiB; where even one word
    per block does not fit, vlg_attn_fuse returns VLG_ERR_SHAPE before any launch."""
    bad = lds_violations()
    assert not bad, "launches asking for too much LDS:\n  " + "\n  ".join(map(str, bad[:20]))
    # the largest requests of the matrix-core kernels are at h = 256
    assert max(l["lds"] for g in DTS for l in backward("bf16", g, 2, 17, 300, 256, 256, 64)) == max(SWEEP_BYTES + 4096, 4 * 32 * 260) == 33280
    assert forward("f32", 2, 17, 36, 32, 256)[0]["lds"] == STAGE_BYTES + 64 * 260
    s = LDS_ERROR_SHAPE
    assert generic_plan(s["L"], s["V"], s["d"], s["h"]) == (0, 163372) and forward("f32", **s) == (ERR_SHAPE, "exceed the LDS budget")
    assert generic_plan(1, generic_v(1, 24, 16), 24, 16)[0] == 1 and generic_plan(1, generic_v(1, 24, 16) + 1, 24, 16)[0] == 0
    one_ = ctypes.c_void_p(64)      # refused before any launch: never dereferenced
    for code in (F32, BF16):
        rc = lib.vlg_attn_fuse(one_, one_, one_, one_, one_, one_, s["B"], s["L"], s["V"], s["d"], s["h"], code, 1e-5, 0, None, 0, None, None, one_, None)
        assert rc == ERR_SHAPE and b"exceed the LDS budget" in lib.vlg_last_error(), (rc, lib.vlg_last_error())
        rc = lib.vlg_attn_fuse(one_, one_, one_, one_, one_, one_, 1, 1, 40000, 32, 32, code, 1e-5, 0, None, 0, None, one_, one_, None)      # with the map
        assert rc == ERR_SHAPE and b"exceed the LDS budget" in lib.vlg_last_error()
    # QC of the rows about the halving, and the 60 KiB attribute
    assert GEN_HALVE_V == 1101 and generic_plan(33, 1100, 32, 32) == (32, 153600) and generic_plan(33, 1101, 32, 32)[0] == 16 and generic_plan(13, 1101, 32, 32)[0] == 13
    assert GEN_ATTR_V == 1721 and generic_plan(8, 1721, 32, 32) == (8, 61440) and generic_plan(8, 1722, 32, 32) == (8, 61472)


def test_cases_are_on_the_route_their_id_names():
    moved = [f"{case_id(c)}: restated {derive(c)}" for c in CASES if derive(c) != (c.fwd, c.bwd)]
    assert not moved, "cases that left the route they were written for:\n  " + "\n  ".join(moved)
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    for c in CASES:
        for call, Ls in launches(c):
            for l in Ls:
                assert l["lds"] <= LDS_LIMIT, (case_id(c), call)
        assert c.B * c.L * c.V * (c.d + c.h) <= 3e8, case_id(c)      # the float64 oracle stays well under a second per pass
        if c.fwd.startswith("split") and c.ck:
            assert attn_split(1, c.L, c.V, c.ck) == attn_split(3, c.L, c.V, c.ck)      # an explicit key_chunk: the plan does not move with B


def _with(pred):
    return [c for c in CASES if pred(c)]


def test_every_image_and_boundary_has_a_case():
    ran = collections.defaultdict(list)
    for c in CASES:
        for _, Ls in launches(c):
            for l in Ls:
                ran[image_of(l)].append(case_id(c))
    assert set(ran) == set(IMAGES), (sorted(set(IMAGES) - set(ran)), sorted(set(ran) - set(IMAGES)))
    for dt in DTS:
        rows = _with(lambda c: c.dt == dt)
        g = lambda name: [c for c in rows if c.group == name]
        assert {c.V for c in g("T")} == set(MFMA_V) and {c.fwd for c in g("T")} == {f"mfma.{dt}.T{T}" for T in (1, 2, 3, 4)}
        assert {c.bwd for c in g("T") + g("Tftm16")} == {f"bwd.one.{dt}.T{T}.FTM{F}" for T in (1, 2, 3, 4) for F in (8, 16)}
        assert {(c.V - 1) % 64 + 1 for c in g("T") if c.V > 64} >= {1, 63, 64}      # keys in the last streamed step
        for V in (36, 130):
            assert {c.L for c in g("words") if c.V == V and c.ck == 0} == set(WORD_L) and {c.h for c in g("chan") if c.V == V} == set(CHAN_H)
        assert {c.L for c in g("words") if c.ck} == set(WORD_L) and {c.h for c in g("chan") if c.ck} == set(CHAN_H)
        assert {c.d for c in g("feat") if c.V == 36} == set(FEAT_D) and {c.d for c in g("feat") if c.V == 130} >= {16, 48, 112}
        assert {c.d for c in g("feat") if c.ck} >= {16, 48, 112, 128, 144, 256}
        assert {c.bwd for c in rows if c.fwd.startswith("split")} == ({"bwd.split.f32.FTM8", "bwd.split.f32.FTM16"} if dt == "f32" else {"bwd.split.bf16.stream", "bwd.split.bf16.d256"})
        for CK in (64, 128, 192):
            assert {c.V for c in g("ck") if c.ck == CK} == {2 * CK - 1, 2 * CK, 2 * CK + 1}
        assert {c.B * plan_of(c)[2] for c in g("pairs")} == {2, 3, 7, 8, 9}
        auto = g("auto")
        assert {(c.B, c.L, c.V) for c in auto} == {(2, 17, 256), (2, 17, 257)} | (set(AUTO_PLANS) - {(256, 40, 1369)})
        assert any(c.V > 256 and c.fwd.startswith("mfma") for c in auto) and {plan_of(c)[1] // 64 for c in auto if c.fwd.startswith("split")} == {1, 2, 3, 5}
        assert {(c.fwd, c.d, c.h) for c in g("shipped")} == {(f"split.{dt}.CK320.NC5", 128, 256), (f"mfma.{dt}.T4", 128, 256)}
        assert {c.B * cdiv(c.L, 16) for c in g("affine") if c.ck == 0} == {1, 15, 16, 17, 33} and any(c.ck for c in g("affine"))
        gen_ = g("gen")
        assert {c.side for c in gen_} >= {"attmap", "d24", "h72", "h272"} and {c.fwd for c in gen_} == {"gen.QC8", "gen.QC13", "gen.QC16", "gen.QC17", "gen.QC32"}
        L_ = lambda c: forward(c.dt, c.B, c.L, c.V, c.d, c.h, c.ck, c.attmap)[0]
        assert {(c.L, L_(c)["halved"]) for c in gen_ if c.V == GEN_HALVE_V} == {(33, True), (64, True), (13, False)}
        assert {(L_(c)["lds"], L_(c)["attr"]) for c in gen_ if c.L == 8} == {(61440, False), (61472, True)}
    for name, _ in FAMILIES:
        assert family(name, "bf16") in CASES and family(name, "f32") in CASES


def family(name, dt):
    kw = dict(FAMILIES)[name]
    want = dict(dict(B=2, L=17, d=32, h=32, attmap=False), **kw)
    rows = [c for c in CASES if c.dt == dt and all(getattr(c, k) == v for k, v in want.items())]
    assert rows, (name, dt)
    return rows[0]


def test_planted_words_sit_on_their_keys():
    """Every planted word of every row puts at least 0.9 of its softmax weight on its key (float64 softmax of the row's own operands); every
    planted value is exact in bf16; neighbouring sentences assign different directions to the same key."""
    low = 1.0
    for c in CASES:
        if c.B * c.V * c.d > 4e6 and c.dt == "bf16":
            continue      # (the same operands as the float32 row: the planted values are exact in both types)
        x = inputs(c, "planted")
        T, CK, NC = plan_of(c)
        keys = boundary_keys(c.V, T, CK, NC, c.d)
        assert c.V - 1 in keys and 0 in keys and len(keys) <= c.d and (NC == 1 or {CK - 1, CK, (NC - 1) * CK} <= set(keys) or c.d < 8)
        words = {w for b, w, k in x.plant if b == 0}
        assert c.L - 1 in words and 16 * (cdiv(c.L, 16) - 1) in words and {16 * t for t in range(cdiv(c.L, 16))} <= words
        assert c.L < len(keys) or {k for b, w, k in x.plant if b == 0} == set(keys)
        for a in (x.vis, x.mid):
            assert np.array_equal(bf16_round(a), a)
        for b, w, k in x.plant:
            s = x.vis[b] @ x.txt[b, 1 + w]
            p = np.exp(s - s.max())
            wgt = p[k] / p.sum()
            low = min(low, wgt)
            assert s[k] == 16.0 and wgt >= 0.9, (case_id(c), b, w, k, wgt)
            assert np.array_equal(bf16_round(x.txt[b, 1 + w]), x.txt[b, 1 + w])
        if c.B > 1 and len(keys) > 1:
            assert not np.array_equal(x.vis[0, keys[0]], x.vis[1, keys[0]])
    print(f"[attn] smallest planted weight over the table: {low:.6f}")
    assert low >= 0.999


def _word_out(x, b, w, vis_b, mid_b, keep=None):
    """float64 `out` row of word w of sentence b over the given key rows (keep: a mask over the keys)"""
    s = vis_b @ x.txt[b, 1 + w]
    p = np.exp(s - s.max()) * (1.0 if keep is None else keep)
    y = x.enc[b, w] + (p / p.sum()) @ mid_b
    return (y - y.mean()) / np.sqrt(y.var() + 1e-5) * x.gamma + x.beta


def test_planted_inputs_expose_a_boundary_key():
    """What the planted set is for, in float64 on the CPU: dropping a planted word's boundary key, reading the key before it in its place, or
    reading that key's rows from the next sentence moves the word's `out` row by far more than the 1e-4 the GPU file allows -- and on the
    random set of the same shape at V = 1369 the first of these stays below the bf16 gradient tolerance of 1e-2, which is the gap."""
    least = 1e30
    for c in [family(n, "f32") for n, _ in FAMILIES] + [r for r in CASES if r.dt == "f32" and r.group in ("ck", "auto", "pairs")]:
        x = inputs(c, "planted")
        for b, w, k in x.plant:
            want = _word_out(x, b, w, x.vis[b], x.mid[b])
            drop = _word_out(x, b, w, x.vis[b], x.mid[b], keep=np.arange(c.V) != k)
            moves = [np.abs(drop - want).max()]
            if k > 0:
                vis_b, mid_b = x.vis[b].copy(), x.mid[b].copy()
                vis_b[k], mid_b[k] = vis_b[k - 1], mid_b[k - 1]
                moves.append(np.abs(_word_out(x, b, w, vis_b, mid_b) - want).max())
            if c.B > 1:
                nb = b + 1 if b + 1 < c.B else b - 1
                moves.append(np.abs(_word_out(x, b, w, x.vis[nb], x.mid[nb]) - want).max())
            least = min(least, *moves)
            assert min(moves) >= 0.05, (case_id(c), b, w, k, moves)
    c = [r for r in CASES if r.dt == "f32" and r.group == "shipped" and r.fwd.startswith("split")][0]
    x = inputs(c, "random")
    most = max(np.abs(_word_out(x, b, w, x.vis[b], x.mid[b], keep=np.arange(c.V) != k) - _word_out(x, b, w, x.vis[b], x.mid[b])).max()
               for b in range(c.B) for w in (0, c.L - 1) for k in (0, 319, 320, c.V - 1))
    print(f"[attn] a dropped boundary key moves out by >= {least:.3f} on every planted word; on random features at V = 1369 by <= {most:.1e}")
    assert most < 1e-2 < 0.05 <= least


@pytest.mark.parametrize("V,ck", NUMERICS_SHAPES)
def test_numerics_inputs_stress_the_streaming_softmax(oracle_mod, V, ck):
    """The five score patterns do what their names say (from the float64 scores), and the float32 restatement of the streaming computation
    stays finite and close to the float64 oracle: the figures of the table in the module docstring."""
    for name in NUMERICS:
        x = numerics_inputs(name, "f32", V)
        S = np.einsum("bld,bvd->blv", x.txt[:, 1:], x.vis)
        steps = np.stack([S[:, :, v0:v0 + 64].max(-1) for v0 in range(0, V, 64)], -1)
        if name in ("rise", "plus256"):
            assert (np.diff(steps, axis=-1) > 0.5).all()
        if name in ("fall", "minus256"):
            assert (np.diff(steps, axis=-1) < -0.5).all() and steps[..., 0].min() - steps[..., -1].max() > (100 if V > 1000 else 4)
        if name == "dominated":
            assert (steps[..., 1] - np.delete(steps, 1, -1).max(-1) > 100).all()
        if name == "plus256":
            assert S.min() >= 128 and np.float32(S.max()) > 89      # exp overflows without the max subtraction
        if name == "minus256":
            assert S.max() <= -128 and np.float32(S.max()) < -104
        err, ref = numerics_error(oracle_mod, name, V, ck)
        print(f"[attn] numerics {name:<10} V {V:<5} ck {ck:<4} " + " ".join(f"{k} {err[k]:.1e} (|ref| {np.abs(ref[k]).max():.1e})" for k in ("out",) + GRAD_NAMES))
        for k, e in err.items():
            assert np.isfinite(e) and e <= 1e-4 * max(1.0, np.abs(ref[k]).max()), (name, k, e)


def test_host_error_returns(lib):
    """Every refusal that comes before the first HIP call: its code and a word of vlg_last_error()."""
    one_ = ctypes.c_void_p(64)      # never dereferenced
    fuse, back = lib.vlg_attn_fuse, lib.vlg_attn_fuse_backward
    err = lambda: lib.vlg_last_error()
    ops = [one_] * 6

    def f(B=2, L=17, V=36, d=32, h=32, code=F32, ck=0, ws=None, nws=0, saved=None, att=None, out=one_, ops=ops):
        return fuse(*ops, B, L, V, d, h, code, 1e-5, ck, ws, nws, saved, att, out, None)

    def b(B=2, L=17, V=36, d=32, h=32, code=F32, ck=0, g=F32, ldb=None, ldl=None, ws=one_, nws=1 << 40, outs=None, ops=ops):
        ldb, ldl = L * h if ldb is None else ldb, h if ldl is None else ldl
        return back(*ops, ldb, ldl, B, L, V, d, h, code, 1e-5, ck, g, None, ws, nws, *(outs or [one_] * 6), None)

    for kw in (dict(B=-1), dict(L=0), dict(V=0), dict(d=0), dict(h=0)):
        assert f(**kw) == ERR_SHAPE and b"bad shape" in err() and forward("f32", **dict(dict(B=2, L=17, V=36, d=32, h=32), **kw))[0] == ERR_SHAPE
        assert b(**kw) == ERR_SHAPE and (b"bad shape" in err() or b"multiples of 16" in err())
    assert f(B=0, ops=[None] * 6, out=None) == 0      # nothing to do
    for k in range(6):
        assert f(ops=[None if i == k else one_ for i in range(6)]) == ERR_ARG and b"null buffer" in err()
        assert b(ops=[None if i == k else one_ for i in range(6)]) == ERR_ARG and b"null buffer" in err()
    assert f(out=None) == ERR_ARG and b"null buffer" in err()
    for k in range(4):
        assert b(outs=[None if i == k else one_ for i in range(6)]) == ERR_ARG and b"null buffer" in err()
    for k in (4, 5):      # d_gamma, d_beta
        assert b(outs=[None if i == k else one_ for i in range(6)]) == ERR_ARG and b"null output" in err()
    assert f(B=65536) == ERR_SHAPE and b"exceeds grid.y" in err() and forward("f32", 65536, 17, 36, 32, 32)[0] == ERR_SHAPE
    assert b(B=65536) == ERR_SHAPE and b"exceeds grid.y" in err()
    assert f(B=65535, V=300, ck=64, ws=one_, nws=0) == ERR_WORKSPACE      # (B = 65535 itself passes the check)
    for bad in (2, -1, 7):
        assert f(code=bad) == ERR_DTYPE and b"in_dtype" in err() and b(code=bad) == ERR_DTYPE and b"in_dtype" in err()
    # the forward split route's workspace
    for code in (F32, BF16):
        need = lib.vlg_attn_fuse_workspace(2, 17, 300, 32, 64)
        assert need == workspace_fwd(2, 17, 300, 32, 64) > 0
        assert f(V=300, ck=64, code=code, ws=one_, nws=need - 1) == ERR_WORKSPACE and b"workspace" in err()
        assert f(V=300, ck=64, code=code, ws=None, nws=need) == ERR_WORKSPACE and b"workspace" in err()
        for g in (F32, BF16) if code == BF16 else (F32,):
            for V, ck in ((36, 0), (300, 64)):
                need = lib.vlg_attn_fuse_backward_workspace(2, 17, V, 32, 32, g, ck)
                assert need == workspace_bwd(2, 17, V, 32, 32, "bf16" if g else "f32", ck) > 0
                assert b(V=V, ck=ck, code=code, g=g, nws=need - 1) == ERR_WORKSPACE and b"workspace" in err()
                assert b(V=V, ck=ck, code=code, g=g, ws=None, nws=need) == ERR_WORKSPACE
    # the adjoint's shapes
    for kw in (dict(d=24), dict(h=24), dict(d=272), dict(h=272)):
        assert b(**kw) == ERR_SHAPE and b"multiples of 16 and <= 256" in err() and backward("f32", "f32", 2, 17, 36, kw.get("d", 32), kw.get("h", 32))[0] == ERR_SHAPE
    for ldb, ldl in ((-4, 32), (17 * 32, -32), (17 * 32 + 2, 32), (17 * 32, 34), (1, 32)):
        assert b(ldb=ldb, ldl=ldl) == ERR_SHAPE and b"dout strides" in err()
    assert b(code=F32, g=BF16) == ERR_DTYPE and b"grad_dtype" in err() and backward("f32", "bf16", 2, 17, 36, 32, 32)[0] == ERR_DTYPE
    assert b(code=BF16, g=2) == ERR_DTYPE and b"grad_dtype" in err()


if __name__ == "__main__":      # the coverage list: kernel image -> rows
    ran = collections.defaultdict(list)
    for c in CASES:
        for _, Ls in launches(c):
            for l in Ls:
                ran[image_of(l)].append(case_id(c))
    for image in IMAGES:
        print(f"{image}: {len(ran[image])} rows, e.g. {ran[image][:1]}")
    print(len(CASES), "rows")
