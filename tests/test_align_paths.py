"""CPU: the dispatch of vlg_bilinear_align (vlgae_amd/csrc/vlg_align.hip) restated in Python, its constants read back from the sources,
and the case table of tests/test_align_paths_gpu.py with the class every case claims.

vlg_bilinear_align turns (dtype, d, B, A, Q, V, which outputs) into one or two launches.  The routes, and what each branches on:

  route        kernel                                    taken when                                          passes      launch shape
  shared_max   align_max_kernel<6>                       bf16, d 128, no full, max_v or max_q, V <= 48       Q / 96      a_per_block, ceil(B / 8) wave rows
  shared_full  align_full_kernel                         bf16, d 128, full alone, V <= 44, V % 4 == 0        Q / 96      a_per_block; copy-out shifted by sh
  tile48       align_mfma_kernel<TILE, RTB 3>            d 64 | 128, no full, a maximum with max_v or diag,  Q / 48      a_per_wave
                                                         V <= 48 (bf16 d 128 goes to shared_max instead)
  direct       align_mfma_kernel<DIRECT>                 as tile48 with V > 48: maxima in registers across   Q / 96|48   a_per_wave, n_grp = ceil(V / 48)
                                                         the region groups; diag comes from diag_only
  diag_only    align_mfma_kernel<TILE, RTB 3>, apw < 0   diag alone, or behind shared_max / direct           Q / 48      grid min(ceil(n_grp / 4), 16)
  tile_full    align_mfma_kernel<TILE>                   full with anything else, or where shared_full       Q / 96|48   a_per_wave, n_grp; running mv[] row;
                                                         does not apply                                                  vector (V % 4 == 0) or scalar copy-out
  stream_maxq  align_mfma_kernel<no tile>                max_q alone, outside shared_max                     Q / 96|48   a_per_wave, n_grp
  generic      align_kernel                              d not in {64, 128}                                  Q / 64      8 images per block, 64 x 64 tiles

(passes: 96 rows for bf16 and 48 for float32 where two are given.)  Images: (bf16, 128), (bf16, 64), (f32, 128), (f32, 64); tile48 is
unreachable for (bf16, 128) because shared_max holds exactly its conditions -- test_every_reachable_class_has_a_case shows it from the
restatement.

CASES holds the smallest shapes at which each class exists; every row states the routes and launch-shape numbers it claims,
test_cases_are_in_the_class_their_name_claims re-derives them, and a change of a constant fails here before it moves a GPU case off its
boundary unnoticed.  The groups of the table and the boundary each sits on:

  sub    all 15 subsets of {full, max_v, max_q, diag} x the four images x V = 8 (V % 4 == 0 <= 44), 46 (45..48), 50 (> 48); masks cycle
  q      Q = 1, 15, 16, 17, QB - 1, QB, QB + 1, 2 QB + 1 per route (QB the route's pass size): the max_q fold across query passes
  v      V = 1, 15, 16, 17, 47, 48, 49, 96, 97 per image on the maxima routes, tile_full and stream_maxq: the 16-region tiles and the 48-region group
  cpy    tile_full copy-out: last-group widths 4, 28, 44, 48 alone and behind a full group (vector, idle lanes past rps rows), V = 50 (scalar)
  sf     shared_full: V = 4, 40, 44; Q V / 4 odd (all eight sh residues); Q = 97 at V = 44 (a full 96-row pass and a one-row pass)
  dg     the diagonal launch's grid: V = 192 | 193 (1 -> 2), V = 3073 (the cap of 16)
  apw    a_per_wave 1, 2, 4, 8, 16 with idle waves behind the last image and (apw > 1) a wave cut short by A
  apb    a_per_block of the shared-tile kernels: A < 8, block 8 + tail 4, block 10 x 31 with tail 1; B = 1, 8, 9 (the mirrored wave)
  gen    generic: d = 1, 16, 40, 100; Q, V in {63, 64, 65}; A in {7, 8, 9}; the caption tile reused across images (Q <= 64)
  msk    per route x image: both masks random, tmask only, vmask only, `edges` (below); neg_inf = -1000 once per route

`edges` masks, all at once (Q % 16 != 0, V % 16 != 0, Q > 16, B = A = 4): caption 0 / image 0 lose their first and last row / region (the
clamped duplicates of the last one must stay masked), caption 1 / image 1 are masked whole, caption 2 keeps its first 16-row tile whole and
loses rows of the later one, caption 3 / image 2 are kept whole (next to masked neighbours: the wave-uniform "nothing masked here" ballots
of align_max_kernel / align_full_kernel take both sides within one launch), image 3 loses every third region.
"""
import collections
import ctypes
import itertools
import os
import re
import zlib

import numpy as np
import pytest

from conftest import ROOT

# ---------------------------------------------------------------------------------------------------------------- the restatement
K_CTB = 3                      # kCTB: 16-region column tiles per LDS tile pass / region group
VB = K_CTB * 16                # regions per group; the tile48 / direct boundary
K_AM_ROWS = 48                 # kAMRows: regions of a shared image tile; the shared_max bound on V
K_AM_WAVES = 8                 # kAMWaves: captions (wavefronts) per workgroup of the shared-tile kernels
RTB = {"bf16": 6, "f32": 3}    # MfmaCfg::RTB: 16-row tiles per query pass
RTB_TILE48 = 3                 # the RTBV argument of the tile48 / diag_only instantiations
AM_RT = 6                      # align_max_kernel<6>
AF_RT = 6                      # VLG_AF_RT
SHARED_FULL_MAX_V = 44
APW_MIN_BLOCK_ROWS = 512       # the a_per_wave loop halves while ceil(A / (4 apw)) B is below this
APW_START = ((2048, 16), (64, 8))    # A >= 2048 ? 16 : A >= 64 ? 8 : 1
APB_WGS, APB_MIN = 256, 8      # a_per_block = clamp(ceil(A ceil(B / 8) / 256), 8, A)
DIAG_GRID_CAP = 16
K_QT = K_VT = 64               # generic tiles
GENERIC_APB = 8
LDS_BUDGET = 160 * 1024
VLG_ERR_SHAPE = 0x1001
IMAGES = (("bf16", 128), ("bf16", 64), ("f32", 128), ("f32", 64))


def cdiv(a, b):
    return (a + b - 1) // b


def a_per_wave(A, B):
    apw = next((w for lo, w in APW_START if A >= lo), 1)
    while apw > 1 and cdiv(A, 4 * apw) * B < APW_MIN_BLOCK_ROWS:
        apw >>= 1
    return apw


def a_per_block(A, B):
    return min(max(cdiv(A * cdiv(B, K_AM_WAVES), APB_WGS), APB_MIN), A)


def generic_lds(d, Q, V):
    return 4 * ((K_QT + K_VT) * (d + 1) + K_QT * (K_VT + 1) + Q + V)


def _mfma(route, img, B, A, Q, V, rtb, diag_only=False):
    n_grp, QB = cdiv(V, VB), rtb * 16
    L = dict(route=route, image=img, QB=QB, passes=cdiv(Q, QB), n_grp=n_grp)
    if diag_only:
        L.update(grid_x=max(1, min(cdiv(n_grp, 4), DIAG_GRID_CAP)), grid_y=B)
        return L
    apw = a_per_wave(A, B)
    gx = cdiv(A, 4 * apw)
    waves = [max(0, min(apw, A - w * apw)) for w in range(4 * gx)]      # n_img of every wave of a caption's blocks
    L.update(apw=apw, grid_x=gx, grid_y=B, cut=sum(0 < n < apw for n in waves), idle=sum(n == 0 for n in waves))
    if route == "tile_full":
        last = V - (n_grp - 1) * VB
        L.update(last_width=last, copy="vector" if V % 4 == 0 else "scalar")      # ((vn & 3) == 0 && (V & 3) == 0); full groups are 48 wide
        if V % 4 == 0:
            L.update(idle_lanes=64 - (64 // (last // 4)) * (last // 4))
    return L


def _shared(route, B, A, Q, V, rt):
    apb = a_per_block(A, B)
    gx, gy = cdiv(A, apb), cdiv(B, K_AM_WAVES)
    L = dict(route=route, image=("bf16", 128), QB=rt * 16, passes=cdiv(Q, rt * 16), n_grp=1, apb=apb, grid_x=gx, grid_y=gy,
             tail=A - (gx - 1) * apb, mirrored=gy * K_AM_WAVES - B)
    if route == "shared_full":     # sh = (dst >> 4) & 7 of every (b, a, pass) chunk, base offset 0
        L["sh"] = frozenset(((((b * A + a) * Q + q0) * V * 4) >> 4) & 7 for b in range(B) for a in range(A) for q0 in range(0, Q, rt * 16))
    return L


def dispatch(dt, d, B, A, Q, V, outs):
    """the launches of vlg_bilinear_align(outs = a string over f v q d), or the refusal it returns first"""
    full, mv, mq, dg = ("f" in outs), ("v" in outs), ("q" in outs), ("d" in outs)
    assert outs and B >= 1 and A >= 1 and Q >= 1 and V >= 1 and d >= 1
    if dg and A != B:
        return VLG_ERR_SHAPE
    img = (dt, d)
    diag = lambda: _mfma("diag_only", img, B, A, Q, V, RTB_TILE48, True)
    if img == ("bf16", 128) and not full and (mv or mq) and V <= K_AM_ROWS:
        return [_shared("shared_max", B, A, Q, V, AM_RT)] + ([diag()] if dg else [])
    if img == ("bf16", 128) and full and not (mv or mq or dg) and V <= SHARED_FULL_MAX_V and V % 4 == 0:
        return [_shared("shared_full", B, A, Q, V, AF_RT)]
    if d in (64, 128):
        tile = full or dg or mv
        if tile and not full:
            if (mv or mq) and V <= VB:
                return [_mfma("tile48", img, B, A, Q, V, RTB_TILE48)]
            return ([_mfma("direct", img, B, A, Q, V, RTB[dt])] if mv or mq else []) + ([diag()] if dg else [])
        return [_mfma("tile_full" if tile else "stream_maxq", img, B, A, Q, V, RTB[dt])]
    lds = generic_lds(d, Q, V)
    if lds > LDS_BUDGET:
        return VLG_ERR_SHAPE
    gx = cdiv(A, GENERIC_APB)
    return [dict(route="generic", image=(dt, "generic"), QB=K_QT, passes=cdiv(Q, K_QT), vtiles=cdiv(V, K_VT), apb=GENERIC_APB, grid_x=gx, grid_y=B,
                 tail=A - (gx - 1) * GENERIC_APB, reuse=Q <= K_QT and min(A, GENERIC_APB) > 1, big_lds=lds > 64 * 1024)]


def derive(c):
    """what a case's claim is compared with: the routes in launch order, the first launch's numbers, the diagonal launch's grid"""
    L = dispatch(c.dt, c.d, c.B, c.A, c.Q, c.V, c.outs)
    out = dict(routes="+".join(l["route"] for l in L))
    out.update({k: v for k, v in L[0].items() if k != "route"})
    for l in L:
        if l["route"] == "diag_only":
            out["dgrid"] = l["grid_x"]
    return out


# ---------------------------------------------------------------------------------------------------------------- inputs
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def make_masks(mask, B, A, Q, V, rng):
    if mask == "none":
        return None, None
    if mask == "edges":
        assert B >= 4 and A >= 4 and Q > 16 and Q % 16 and V % 16 and V >= 4
        t, v = np.ones((B, Q), np.uint8), np.ones((A, V), np.uint8)
        t[0, 0] = t[0, Q - 1] = 0
        t[1, :] = 0
        t[2, 16::2] = 0
        t[2, Q - 1] = 0
        v[0, 0] = v[0, V - 1] = 0
        v[1, :] = 0
        v[3, ::3] = 0
        return t, v
    t, v = (rng.random((B, Q)) < 0.8).astype(np.uint8), (rng.random((A, V)) < 0.8).astype(np.uint8)
    return dict(both=(t, v), t=(t, None), v=(None, v))[mask]


def input_key(c):
    return (c.dt, c.d, c.B, c.A, c.Q, c.V, c.mask)


def exact_inputs(key):
    """txt [B,Q,d], vis [A,V,d] as float64 holding integers in [-8, 8] / 8 (exact in bf16): every product is a multiple of 1 / 64 and
    every partial sum at most d <= 128 in magnitude, so any order of float32 accumulation is exact"""
    dt, d, B, A, Q, V, mask = key
    rng = _rng("exact", *key)
    txt, vis = rng.integers(-8, 9, (B, Q, d)) / 8.0, rng.integers(-8, 9, (A, V, d)) / 8.0
    return (txt, vis) + make_masks(mask, B, A, Q, V, rng)


def rounding_inputs(key):
    """normal(0, 0.5) features as float64, rounded to bf16 for the bf16 images"""
    import torch
    dt, d, B, A, Q, V, mask = key
    rng = _rng("rounding", *key)
    txt, vis = rng.normal(0, 0.5, (B, Q, d)), rng.normal(0, 0.5, (A, V, d))
    if dt == "bf16":
        txt, vis = (torch.from_numpy(x).float().bfloat16().double().numpy() for x in (txt, vis))
    else:
        txt, vis = (x.astype(np.float32).astype(np.float64) for x in (txt, vis))
    return (txt, vis) + make_masks(mask, B, A, Q, V, rng)


def oracle_outputs(oracle, inputs, dtype, neg_inf):
    txt, vis, tmask, vmask = inputs
    diag = txt.shape[0] == vis.shape[0]
    return oracle.bilinear_align(txt, vis, tmask, vmask, dtype, neg_inf, True, True, True, diag)


# ---------------------------------------------------------------------------------------------------------------- the case table
Case = collections.namedtuple("Case", "group dt d B A Q V outs mask neg_inf claim")
CASES = []


def add(group, dt, d, B, A, Q, V, outs, mask="none", neg_inf=-1e20, **claim):
    CASES.append(Case(group, dt, d, B, A, Q, V, outs, mask, neg_inf, claim))


def case_id(c):
    return f"{c.group}_{c.dt}_d{c.d}_B{c.B}_A{c.A}_Q{c.Q}_V{c.V}_{c.outs}_{c.mask}" + ("" if c.neg_inf == -1e20 else "_ni1000") + "_" + c.claim["routes"]


SUBSETS = ["".join(s) for n in range(1, 5) for s in itertools.combinations("fvqd", n)]
WIDTHS = (8, 46, 50)        # V % 4 == 0 <= 44; 45..48; > 48
MASKS = ("none", "both", "t", "v")
# routes per width class; every subset with `f` and something else is tile_full everywhere
SUB_GENERAL = {"f": ("tile_full",) * 3, "v": ("tile48", "tile48", "direct"), "q": ("stream_maxq",) * 3, "d": ("diag_only",) * 3,
               "vq": ("tile48", "tile48", "direct"), "vd": ("tile48", "tile48", "direct+diag_only"), "qd": ("tile48", "tile48", "direct+diag_only"),
               "vqd": ("tile48", "tile48", "direct+diag_only")}
SUB_BF16_128 = {"f": ("shared_full", "tile_full", "tile_full"), "v": ("shared_max", "shared_max", "direct"),
                "q": ("shared_max", "shared_max", "stream_maxq"), "d": ("diag_only",) * 3, "vq": ("shared_max", "shared_max", "direct"),
                "vd": ("shared_max+diag_only", "shared_max+diag_only", "direct+diag_only"),
                "qd": ("shared_max+diag_only", "shared_max+diag_only", "direct+diag_only"),
                "vqd": ("shared_max+diag_only", "shared_max+diag_only", "direct+diag_only")}
for dt, d in IMAGES:
    for wi, V in enumerate(WIDTHS):
        for si, outs in enumerate(SUBSETS):
            table = SUB_BF16_128 if (dt, d) == ("bf16", 128) else SUB_GENERAL
            add("sub", dt, d, 3, 3, 5, V, outs, MASKS[(si + wi) % 4], routes=table.get(outs, ("tile_full",) * 3)[wi])

# Q on both sides of the pass size, per route; pass size written per row
QROWS = [("bf16", 128, 5, "vq", "shared_max", 96), ("bf16", 128, 4, "f", "shared_full", 96), ("bf16", 64, 5, "vq", "tile48", 48),
         ("f32", 64, 5, "vq", "tile48", 48), ("bf16", 64, 50, "vq", "direct", 96), ("f32", 64, 50, "vq", "direct", 48),
         ("bf16", 64, 5, "d", "diag_only", 48), ("bf16", 64, 5, "fvq", "tile_full", 96), ("f32", 64, 5, "fvq", "tile_full", 48),
         ("bf16", 64, 5, "q", "stream_maxq", 96), ("f32", 64, 5, "q", "stream_maxq", 48)]
for dt, d, V, outs, routes, QB in QROWS:
    for Q in (1, 15, 16, 17, QB - 1, QB, QB + 1, 2 * QB + 1):
        add("q", dt, d, 2, 2, Q, V, outs, routes=routes, QB=QB, passes=(Q + QB - 1) // QB)

# V across the 16-region tiles and the 48-region group, per image: {V: groups}
VGROUPS = {1: 1, 15: 1, 16: 1, 17: 1, 47: 1, 48: 1, 49: 2, 96: 2, 97: 3}
for dt, d in IMAGES:
    for V, ng in VGROUPS.items():
        small = "shared_max+diag_only" if (dt, d) == ("bf16", 128) else "tile48"
        routes = small if V <= 48 else "direct+diag_only"
        add("v", dt, d, 2, 2, 3, V, "vqd", routes=routes, n_grp=ng, **(dict(dgrid=1) if "diag_only" in routes else {}))
        add("v", dt, d, 2, 2, 3, V, "fvq", routes="tile_full", n_grp=ng)
        add("v", dt, d, 2, 2, 3, V, "q", routes="shared_max" if V <= 48 and (dt, d) == ("bf16", 128) else "stream_maxq",
            n_grp=1 if V <= 48 and (dt, d) == ("bf16", 128) else ng)

# tile_full copy-out: {V: (groups, last width, lanes idle in a vector step or None for the scalar loop)}; Q = 21 is several steps of 2 rps rows
COPY = {4: (1, 4, 0), 28: (1, 28, 1), 44: (1, 44, 9), 48: (1, 48, 4), 50: (2, 2, None), 52: (2, 4, 0), 76: (2, 28, 1), 92: (2, 44, 9), 96: (2, 48, 4)}
for dt in ("bf16", "f32"):
    for V, (ng, last, idle_lanes) in COPY.items():
        extra = dict(copy="scalar") if idle_lanes is None else dict(copy="vector", idle_lanes=idle_lanes)
        add("cpy", dt, 64, 2, 2, 21, V, "fd", routes="tile_full", n_grp=ng, last_width=last, **extra)

# shared_full
ALL8 = frozenset(range(8))
add("sf", "bf16", 128, 3, 3, 5, 4, "f", routes="shared_full", sh=ALL8, passes=1)                      # chunks of 5 pieces: 5 k mod 8 over 9 pairs
add("sf", "bf16", 128, 2, 2, 7, 40, "f", routes="shared_full", sh=frozenset({0, 6, 4, 2}), passes=1)   # 70 pieces per pair
add("sf", "bf16", 128, 2, 2, 97, 44, "f", routes="shared_full", sh=frozenset({0, 3, 6, 1}), passes=2)  # 1067 pieces per pair, 1056 per full pass
add("sf", "bf16", 128, 2, 2, 96, 44, "f", routes="shared_full", sh=frozenset({0}), passes=1)

# the diagonal launch's grid
for dt in ("bf16", "f32"):
    for V, ng, grid in ((192, 4, 1), (193, 5, 2), (3073, 65, 16)):
        add("dg", dt, 64, 2, 2, 3, V, "d", routes="diag_only", n_grp=ng, dgrid=grid)
add("dg", "bf16", 64, 2, 2, 3, 193, "vqd", routes="direct+diag_only", n_grp=5, dgrid=2)
add("dg", "bf16", 128, 2, 2, 3, 193, "qd", routes="direct+diag_only", n_grp=5, dgrid=2)

# a_per_wave: (apw, B, A, waves cut short by A, idle waves).  A = 70 is a whole number of 2-image waves, so apw 2 also runs at A = 69.
APW = [(1, 3, 70, 0, 2), (2, 57, 70, 0, 1), (2, 57, 69, 1, 1), (4, 103, 70, 1, 2), (8, 171, 70, 1, 3), (16, 16, 2050, 1, 3)]
for dt in ("bf16", "f32"):
    for apw, B, A, cut, idle in APW:
        Q = 3 if B * A < 8000 else 2
        for V, outs, routes in ((3, "vq", "tile48"), (50, "vq", "direct"), (3, "fvq", "tile_full"), (3, "q", "stream_maxq")):
            add("apw", dt, 64, B, A, Q, V, outs, routes=routes, apw=apw, cut=cut, idle=idle)

# a_per_block of the shared-tile kernels: (B, A, block, blocks, tail, mirrored waves)
APB = [(1, 3, 3, 1, 3, 7), (8, 20, 8, 3, 4, 0), (9, 20, 8, 3, 4, 7), (57, 301, 10, 31, 1, 7)]
for B, A, apb, blocks, tail, mirrored in APB:
    add("apb", "bf16", 128, B, A, 3, 5, "vq", routes="shared_max", apb=apb, grid_x=blocks, tail=tail, mirrored=mirrored)
    add("apb", "bf16", 128, B, A, 3, 4, "f", routes="shared_full", apb=apb, grid_x=blocks, tail=tail, mirrored=mirrored)

# generic
for dt in ("bf16", "f32"):
    for d in (1, 16, 40, 100):
        add("gen", dt, d, 3, 3, 5, 6, "fvqd", MASKS[d % 4], routes="generic", big_lds=d == 100, reuse=True)
for i, (Q, V) in enumerate(itertools.product((63, 64, 65), repeat=2)):
    add("gen", ("bf16", "f32")[i % 2], 16, 2, 2, Q, V, "fvqd", routes="generic", passes=1 + (Q > 64), vtiles=1 + (V > 64), reuse=Q <= 64)
for A, blocks, tail in ((7, 1, 7), (8, 1, 8), (9, 2, 1)):
    add("gen", "f32", 40, 2, A, 5, 6, "fvq", "both", routes="generic", grid_x=blocks, tail=tail, reuse=True)
    add("gen", "bf16", 40, 2, A, 65, 6, "fvq", routes="generic", grid_x=blocks, tail=tail, reuse=False, passes=2)

# masks per route x image (B = A = 4, Q = 21 = 16 + 5; V = 13 | 12 | 53: V % 16 != 0), neg_inf = -1000 once per route
MASKED = [("bf16", 128, 13, "vqd", "shared_max+diag_only"), ("bf16", 128, 12, "f", "shared_full")]
MASKED += [(dt, d, 13, "vqd", "tile48") for dt, d in IMAGES[1:]]
MASKED += [(dt, d, 53, "vqd", "direct+diag_only") for dt, d in IMAGES]
MASKED += [(dt, d, V, "fvqd", "tile_full") for dt, d in IMAGES for V in (13, 53)]
MASKED += [(dt, d, 53, "q", "stream_maxq") for dt, d in IMAGES]
MASKED += [(dt, 40, 13, "fvqd", "generic") for dt in ("bf16", "f32")]
_seen = set()
for dt, d, V, outs, routes in MASKED:
    for mask in ("both", "t", "v", "edges"):
        add("msk", dt, d, 4, 4, 21, V, outs, mask, routes=routes)
    if routes not in _seen:
        _seen.add(routes)
        add("msk", dt, d, 4, 4, 21, V, outs, "edges", -1000.0, routes=routes)
    else:
        add("msk", dt, d, 4, 4, 21, V, outs, "none", routes=routes)

# the rounding set: one case per route x image on normal(0, 0.5) features (generic: d = 100, where the sequential float32 sum is longest)
ROUNDING = []
for dt, d in IMAGES:
    small = [("vqd", 13, "shared_max+diag_only"), ("f", 12, "shared_full")] if (dt, d) == ("bf16", 128) else [("vqd", 13, "tile48")]
    for outs, V, routes in small + [("vqd", 53, "direct+diag_only"), ("fvqd", 53, "tile_full"), ("q", 53, "stream_maxq")]:
        ROUNDING.append(Case("rnd", dt, d, 4, 4, 21, V, outs, "both", -1e20, dict(routes=routes)))
ROUNDING += [Case("rnd", dt, 100, 4, 4, 21, 13, "fvqd", "both", -1e20, dict(routes="generic")) for dt in ("bf16", "f32")]


def routes_of(c):
    return c.claim["routes"].split("+")


def mask_features(tmask, vmask, Q, V):
    """what the `edges` masks must hold"""
    f = set()
    if tmask is not None and vmask is not None:
        f |= {"last_row"} if (tmask[:, Q - 1] == 0).any() and Q % 16 else set()
        f |= {"last_region"} if (vmask[:, V - 1] == 0).any() and V % 16 else set()
        f |= {"first_row"} if (tmask[:, 0] == 0).any() else set()
        f |= {"first_region"} if (vmask[:, 0] == 0).any() else set()
        f |= {"whole_caption"} if (tmask.sum(1) == 0).any() else set()
        f |= {"whole_image"} if (vmask.sum(1) == 0).any() else set()
        f |= {"clean_first_tile"} if any(t[:16].all() and not t[16:].all() and t[16:].any() for t in tmask) else set()
        f |= {"clean_caption"} if tmask.all(1).any() else set()
        f |= {"clean_image_beside_masked"} if any(vmask[a].all() and 0 < vmask[a + 1].sum() < V for a in range(len(vmask) - 1)) else set()
    return f


EDGE_FEATURES = {"last_row", "last_region", "first_row", "first_region", "whole_caption", "whole_image", "clean_first_tile", "clean_caption",
                 "clean_image_beside_masked"}


# ---------------------------------------------------------------------------------------------------------------- tests
def _src(name):
    return open(os.path.join(ROOT, "vlgae_amd", "csrc", name)).read()


def test_constants_read_from_the_sources():
    """Every constant of the restatement, found in the sources by regex and equal to the restatement's."""
    s, m = _src("vlg_align.hip"), _src("vlg_mfma.h")

    def num(pattern, text=s):
        found = re.findall(pattern, text)
        assert len(found) == 1, (pattern, found)
        return found[0] if isinstance(found[0], tuple) else int(found[0])

    assert num(r"constexpr int kCTB = (\d+);") == K_CTB
    assert num(r"constexpr int kQT = (\d+);") == K_QT and num(r"constexpr int kVT = (\d+);") == K_VT
    assert num(r"kAMWaves = (\d+),") == K_AM_WAVES and num(r"kAMRows = (\d+),") == K_AM_ROWS
    assert num(r"struct MfmaCfg<false> \{[^}]*?RTB = (\d+)", m) == RTB["bf16"] and num(r"struct MfmaCfg<true> \{[^}]*?RTB = (\d+)", m) == RTB["f32"]
    assert num(r"#define VLG_AF_RT (\d+)") == AF_RT
    assert num(r"align_max_kernel<(\d+)>, grid") == AM_RT
    # the shared_full bound and divisibility, the shared_max and tile48 bounds (as expressions of the constants above)
    assert tuple(map(int, num(r"!out_maxV && !out_maxQ && !out_diag && V <= (\d+) && V % (\d+) == 0\)"))) == (SHARED_FULL_MAX_V, 4)
    assert len(re.findall(r"!f32in && d == 128 && !out_full && \(out_maxV \|\| out_maxQ\) && V <= kAMRows\)", s)) == 1
    assert len(re.findall(r"if \(\(out_maxV \|\| out_maxQ\) && V <= kCTB \* 16\)", s)) == 1 and VB == K_CTB * 16
    assert SHARED_FULL_MAX_V * 4 * K_AM_WAVES * AF_RT * 16 + 2 * K_AM_ROWS * 256 + 2 * K_AM_ROWS <= LDS_BUDGET      # why 44: the output blocks beside the image tiles
    # tile48 and both diagonal launches are the RTB-3 tile instantiation; direct / tile_full / stream_maxq take MfmaCfg::RTB
    assert set(re.findall(r"launch_align_mfma<(?:F32|false), (?:KCHV|4), true, false, (\d+)>", s)) == {str(RTB_TILE48)} and \
        len(re.findall(r"launch_align_mfma<(?:F32|false), (?:KCHV|4), true, false, \d+>", s)) == 3
    assert len(re.findall(r"launch_align_mfma<F32, KCHV, false, false, MfmaCfg<F32>::RTB, true>", s)) == 1
    # a_per_wave
    assert tuple(map(int, num(r"A >= (\d+) \? (\d+) : A >= (\d+) \? (\d+) : 1;"))) == APW_START[0] + APW_START[1]
    assert num(r"\(4 \* a_per_wave\)\) \* B < (\d+)\) a_per_wave >>= 1;") == APW_MIN_BLOCK_ROWS
    # a_per_block of both shared-tile launchers
    assert re.findall(r"int a_per_block = \(int\)\(\(\(long\)A \* by \+ (\d+)\) / (\d+)\);", s) == [(str(APB_WGS - 1), str(APB_WGS))] * 3      # align_full, align_max, and the arg-max launcher
    assert len(re.findall(r"if \(a_per_block < 8\) a_per_block = 8;", s)) == 1 and len(re.findall(r"if \(a_per_block < \(8 \+ ng - 1\) / ng\)", s)) == 2 and len(re.findall(r"const int ng = ARGS \? \(V \+ kAMRows - 1\) / kAMRows : 1;", s)) == 1
    assert len(re.findall(r"const int by = \(B \+ kAMWaves - 1\) / kAMWaves;", s)) == 3
    # the diagonal launch's grid
    assert tuple(map(int, num(r"std::min\(\(n_grp \+ 3\) / (\d+), (\d+)\)\)"))) == (4, DIAG_GRID_CAP)
    # generic
    assert num(r"int a_per_block = (\d+);") == GENERIC_APB and num(r"if \(lds > (\d+) \* 1024\) return set_error\(VLG_ERR_SHAPE") * 1024 == LDS_BUDGET
    assert len(re.findall(r"\(size_t\)\(kQT \+ kVT\) \* \(d \+ 1\) \+ \(size_t\)kQT \* \(kVT \+ 1\) \+ Q \+ V\)", s)) == 1
    # the copy-out shift and its vector condition
    assert len(re.findall(r"const int sh = \(int\)\(\(reinterpret_cast<uintptr_t>\(dst4\) >> 4\) & 7\);", s)) == 1
    assert len(re.findall(r"if \(\(vn & 3\) == 0 && \(V & 3\) == 0\)", s)) == 1


def test_cases_are_in_the_class_their_name_claims():
    """Every case of the GPU file: the restated dispatch gives the routes and every launch-shape number the table claims."""
    moved = []
    for c in CASES + ROUNDING:
        got = derive(c)
        wrong = {k: (got.get(k), v) for k, v in c.claim.items() if got.get(k) != v}
        if wrong:
            moved.append(f"{case_id(c)}: (restated, claimed) {wrong}")
        assert c.B * c.A * c.Q * c.V * c.d <= 2.2e8, case_id(c)
    assert not moved, "cases that left the path they were written for:\n  " + "\n  ".join(moved)
    assert len({case_id(c) for c in CASES}) == len(CASES) and len({case_id(c) for c in ROUNDING}) == len(ROUNDING)


def _have(**want):
    """cases whose fields / claims equal `want` (routes: contained in the launch list)"""
    def ok(c):
        for k, v in want.items():
            if k == "route":
                if v not in routes_of(c):
                    return False
            elif k == "image":
                if (c.dt, c.d) != v:
                    return False
            elif (getattr(c, k) if k in Case._fields else c.claim.get(k)) != v:
                return False
        return True
    return [c for c in CASES if ok(c)]


def test_every_reachable_class_has_a_case():
    """Coverage, from the claims (which the test above ties to the restatement)."""
    mfma_routes = ("tile48", "direct", "diag_only", "tile_full", "stream_maxq")
    reachable = {("shared_max", ("bf16", 128)), ("shared_full", ("bf16", 128))} | {(r, im) for r in mfma_routes for im in IMAGES}
    reachable.discard(("tile48", ("bf16", 128)))
    # ... and nothing else: the restatement over every subset, image and a sweep of V never gives tile48 for (bf16, 128)
    seen = set()
    for (dt, d), outs, V in itertools.product(IMAGES, SUBSETS, range(1, 100)):
        seen |= {(l["route"], l["image"]) for l in dispatch(dt, d, 3, 3, 5, V, outs)}
    assert seen == reachable
    for route, image in sorted(reachable):
        assert _have(route=route, image=image), (route, image)
        assert [c for c in ROUNDING if route in routes_of(c) and (c.dt, c.d) == image], (route, image)
        for mask in ("none", "both", "t", "v", "edges"):
            assert _have(route=route, image=image, mask=mask), (route, image, mask)
    for dt in ("bf16", "f32"):
        for mask in ("none", "both", "t", "v", "edges"):
            assert _have(route="generic", dt=dt, mask=mask), (dt, mask)
        assert [c for c in ROUNDING if c.claim["routes"] == "generic" and c.dt == dt and c.d == 100]
    for route in ("shared_max", "shared_full", "generic") + mfma_routes:
        assert _have(route=route, neg_inf=-1000.0, mask="edges"), route
    # the 15 subsets at three widths per image, A == B
    for image in IMAGES:
        for V in WIDTHS:
            assert {c.outs for c in _have(group="sub", image=image, V=V) if c.A == c.B} == set(SUBSETS) and len(SUBSETS) == 15
    assert WIDTHS[0] % 4 == 0 and WIDTHS[0] <= SHARED_FULL_MAX_V < WIDTHS[1] <= VB < WIDTHS[2]
    # Q on both sides of the pass size, per route
    for route, QB in (("shared_max", 96), ("shared_full", 96), ("tile48", 48), ("direct", 96), ("direct", 48), ("diag_only", 48), ("tile_full", 96),
                      ("tile_full", 48), ("stream_maxq", 96), ("stream_maxq", 48)):
        assert {c.Q for c in _have(group="q", route=route, QB=QB)} == {1, 15, 16, 17, QB - 1, QB, QB + 1, 2 * QB + 1}, (route, QB)
        assert max(c.claim["passes"] for c in _have(group="q", route=route, QB=QB)) == 3
    assert {c.Q for c in _have(route="generic")} >= {63, 64, 65}
    # V
    for image in IMAGES:
        for outs in ("vqd", "fvq", "q"):
            assert {c.V for c in _have(group="v", image=image, outs=outs)} == {1, 15, 16, 17, 47, 48, 49, 96, 97}
    for dt in ("bf16", "f32"):
        cp = _have(group="cpy", dt=dt, route="tile_full")
        assert {c.claim["last_width"] for c in cp if c.claim["n_grp"] == 1 and c.claim["copy"] == "vector"} == {4, 28, 44, 48}
        assert {c.claim["last_width"] for c in cp if c.claim["n_grp"] == 2 and c.claim["copy"] == "vector"} == {4, 28, 44, 48}
        assert {c.V for c in cp if c.claim["copy"] == "scalar"} == {50} and {c.V for c in cp} >= {50, 52}
        assert {c.claim.get("idle_lanes") for c in cp} >= {0, 1, 4, 9} and all("d" in c.outs and c.Q > 2 * 9 for c in cp)
    # shared_full
    sf = _have(group="sf")
    assert {c.V for c in sf} == {4, 40, 44} and any(c.claim["sh"] == ALL8 and (c.Q * c.V // 4) % 2 for c in sf)
    assert any((c.Q, c.V, c.claim["passes"]) == (97, 44, 2) for c in sf)
    # the diagonal launch's grid
    for dt in ("bf16", "f32"):
        assert {(c.V, c.claim["dgrid"]) for c in _have(group="dg", dt=dt, outs="d")} == {(192, 1), (193, 2), (3073, 16)}
    assert all((c.B, c.A, c.Q, c.d) == (2, 2, 3, 64) for c in _have(group="dg", outs="d"))
    # a_per_wave: every value on the four routes, idle waves behind the last image, a wave cut short wherever apw > 1
    for dt in ("bf16", "f32"):
        for route in ("tile48", "direct", "tile_full", "stream_maxq"):
            for apw in (1, 2, 4, 8, 16):
                got = _have(group="apw", dt=dt, route=route, apw=apw)
                assert got and all(c.claim["idle"] > 0 for c in got) and (apw == 1 or any(c.claim["cut"] == 1 for c in got)), (dt, route, apw)
                assert all(c.V in (3, 50) and c.Q in (2, 3) for c in got)
    assert {(c.claim["apw"], c.B, c.A) for c in _have(group="apw")} >= {(1, 3, 70), (2, 57, 70), (4, 103, 70), (8, 171, 70), (16, 16, 2050)}
    # a_per_block
    for route in ("shared_max", "shared_full"):
        got = _have(group="apb", route=route)
        assert any(c.A < 8 and c.claim["apb"] == c.A for c in got) and any((c.A, c.claim["apb"], c.claim["tail"]) == (20, 8, 4) for c in got)
        assert any((c.B, c.A, c.claim["apb"], c.claim["grid_x"], c.claim["tail"]) == (57, 301, 10, 31, 1) for c in got) and {c.B for c in got} >= {1, 8, 9}
    # generic
    gen = _have(route="generic")
    assert {(c.dt, c.d) for c in gen} >= set(itertools.product(("bf16", "f32"), (1, 16, 40, 100)))
    assert {(c.Q, c.V) for c in gen} >= set(itertools.product((63, 64, 65), repeat=2)) and {c.A for c in gen} >= {7, 8, 9}
    assert any(c.claim.get("reuse") is True and c.A > 1 for c in gen) and any(c.claim.get("reuse") is False and c.A > 1 for c in gen)
    # the edges masks hold what their name says
    for c in _have(mask="edges"):
        assert c.Q % 16 and c.V % 16 and c.Q > 16
        _, _, t, v = exact_inputs(input_key(c))
        assert mask_features(t, v, c.Q, c.V) == EDGE_FEATURES, case_id(c)


def test_restatement_fails_when_a_constant_moves(monkeypatch):
    """The table is tied to the constants: with kAMRows 48 -> 64 in the restatement, cases leave their class."""
    import sys
    me = sys.modules[__name__]
    monkeypatch.setattr(me, "K_AM_ROWS", 64)
    assert any(derive(c)["routes"] != c.claim["routes"] for c in CASES)
    with pytest.raises(AssertionError):
        test_constants_read_from_the_sources()


def test_a_per_wave_pairs_rederived():
    """The (B, A) pairs of the a_per_wave cases, from the loop: start value by A, halved while ceil(A / (4 apw)) B < 512."""
    assert [a_per_wave(A, B) for _, B, A, _, _ in APW] == [w for w, *_ in APW]
    assert a_per_wave(70, 56) == 1 and a_per_wave(70, 102) == 2 and a_per_wave(70, 170) == 4 and a_per_wave(2050, 15) == 8     # one caption fewer: the next value down
    assert a_per_wave(63, 4096) == 1 and a_per_wave(64, 4096) == 8 and a_per_wave(2047, 4096) == 8 and a_per_wave(2048, 4096) == 16
    assert [a_per_block(A, B) for B, A, *_ in APB] == [b for _, _, b, *_ in APB]


def test_exact_inputs_make_the_float32_oracle_equal_the_float64_oracle(oracle_mod):
    """On every case's inputs the float32 oracle (sequential sums) equals the float64 oracle in all four outputs: the sums are exact, so
    the GPU file may ask for equality with float32(float64 oracle) whatever the order of accumulation."""
    done = set()
    for c in CASES:
        key = input_key(c) + (c.neg_inf,)
        if key in done:
            continue
        done.add(key)
        inputs = exact_inputs(input_key(c))
        r32, r64 = (oracle_outputs(oracle_mod, inputs, t, c.neg_inf) for t in (np.float32, np.float64))
        for name in ("full", "maxV", "maxQ", "diag"):
            if r64[name] is not None:
                assert np.array_equal(r32[name], r64[name].astype(np.float32)), (case_id(c), name)
        kept = r64["full"][r64["full"] != c.neg_inf]
        assert np.abs(kept).max(initial=0) <= c.d and np.array_equal(kept * 64, np.round(kept * 64))


@pytest.fixture(scope="module")
def lib():
    from vlgae_amd.build import build_library
    build_library()            # hipcc cross-compiles for gfx950 without a GPU
    from vlgae_amd import _C
    return _C.lib()


def test_host_refusals(lib):
    """d = 300 exceeds the generic kernel's LDS budget; diag with A != B: VLG_ERR_SHAPE before any launch, on every image."""
    # Refused before any launch, so the pointer is never used.  Where a GPU is present it is a real buffer large enough for every operand
    # and output of these shapes, so that a host check weakened later fails an assertion here instead of launching on a made-up address.
    import torch
    if torch.cuda.is_available():
        held = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
        one = ctypes.c_void_p(held.data_ptr())
    else:
        one = ctypes.c_void_p(64)
    for in_dtype, dt in ((0, "f32"), (1, "bf16")):
        assert dispatch(dt, 300, 1, 1, 1, 1, "f") == VLG_ERR_SHAPE and isinstance(dispatch(dt, 250, 1, 1, 1, 1, "f"), list)
        assert lib.vlg_bilinear_align(one, one, None, None, 1, 1, 1, 1, 300, in_dtype, -1e20, one, None, None, None, None) == VLG_ERR_SHAPE
        assert b"LDS tile budget" in lib.vlg_last_error()
        for d in (128, 64, 40):
            for outs in ((None, None, None, one), (one, one, one, one), (None, one, None, one)):
                assert dispatch(dt, d, 2, 3, 4, 5, "d") == VLG_ERR_SHAPE
                assert lib.vlg_bilinear_align(one, one, None, None, 2, 3, 4, 5, d, in_dtype, -1e20, *outs, None) == VLG_ERR_SHAPE
                assert b"A == B" in lib.vlg_last_error()
