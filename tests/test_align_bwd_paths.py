"""CPU: the dispatch of vlg_bilinear_align_backward (vlgae_amd/csrc/vlg_align.hip) restated in Python, its constants read back from the
sources, and the case table of tests/test_align_bwd_paths_gpu.py with the class every case claims.

vlg_bilinear_align_backward turns (dtype, d, B, A, Q, V, which gradients) into one launch chain per wanted side.  Both sides are the same
loop over a cotangent g [B,A,Q,V] with different strides:

  side      output        fixed index   outer O   rows M   contraction K   masks (row, contraction)
  caption   grad_txt      b (fixn = B)  A         Q        V               tmask, vmask
  image     grad_vis      a (fixn = A)  B         V        Q               vmask, tmask

  route      kernel                                      taken when                                         kernel image
  concat2    align_bwd_concat_transpose_kernel +         caption side, bf16, d 128, Q <= 96, V % 4 == 0,    (MT, CW, NF)
             align_bwd_split2_kernel                     4 <= V <= 48: two images per step
  split_kc   align_bwd_transpose_kernel +                caption side, d 128, Q <= 96, V <= 96 otherwise    (KC, NKC, MT, CW, NF, f32feat)
             align_bwd_split(_f32)_kernel<KCONTIG>
  split_kn   the same, <!KCONTIG>                        image side, d 128, Q <= 96, V <= 96                (KN, NKC, MT, CW, NF, f32feat)
  generic    align_bwd_kernel<In, NCT, NS>               d 32 | 64; d 128 with Q > 96 or V > 96             (dt, NCT = d / 16, NS)

NKC = ceil(K / 32); MT x CW = 3 x 2 for M <= 48 and 6 x 1 above; NF = 2 (two fixed indices per workgroup) for bf16 features and fixn >= 64
where launch_bwd_split's NFV rule allows it; NS from the ladder 6 | 9 | 12 | 21 | 24 over ceil(K / 4).  Every route may split its outer range
over two workgroups whose partial sums meet by atomicAdd in an output zeroed first: the split routes when 2 fixn <= 1024 nf and O >= 16,
the generic one when gx fixn < 768 and O >= 32.  That is 30 generic + 33 split + 4 concat2 = 67 reachable kernel images;
test_every_reachable_image_has_a_case enumerates them from the restatement and shows which template arguments the dispatch never forms.

CASES holds the smallest shapes at which each class exists; every row states the routes, images, split plans and boundary numbers it
claims, and test_cases_are_in_the_class_their_name_claims re-derives them from plan().  The groups:

  sp     split-term path, bf16 and float32 features: rows M and contraction K in 1, 15, 16, 17, 31, 32 | 33, 48 | 49, 64 | 65, 95, 96 | 97 on
         both sides; both k_quads branches of the caption side at every NKC it reaches; 97 falls to generic on both sides
  o      outer count O = 1, 2, 3 (a prologue with nothing behind it), 15 | 16 | 17 (split 1 -> 2, opb 9 + 8)
  fx     fixed indices 1, 2, 63 | 64 | 65 (NF = 2 begins; at 65 a mirrored wave set that stores nothing) on every NF = 2 image
  big    the unsplit plan: fixn 512 | 513 (float32), 1024 | 1025 (bf16, NF = 2) at O = 16, Q = V = 1 .. 4, either side
  cc     concat2: V = 4, 8, 20, 32, 36, 44, 48 beside 3, 5, 52; Q = 1, 16, 17, 48 | 49, 96; A = 1, 2, 3, 15 .. 19 (lone last pair, even
         opb, second block odd / even); A even with V % 8 == 4 (the clamped look-ahead tile at an 8-byte offset); B = 1, 63 | 64 | 65
  gn     generic: every (dt, NCT, NS); K = 1, 24 | 25, 36 | 37, 48 | 49, 84 | 85, 96 | 97, 192 | 193; M = 1, 16, 17, 48, 64 | 65, 97;
         1 .. 5 iterations per block; O = 31 | 32 | 33; gx fixn = 767 | 768 at O = 32
  mk     per route x dtype: masks none, t, v, both, edges
  x2     the float32-feature split images on the x2 data set (below)

Exact operands.  g2: features are integers in [-R, R] / 8 (R <= 8), the cotangent odd integers of 9 .. gb <= 11 significant bits, (gb, R)
chosen per case so that terms 2^gb R < 2^24 (terms = max(A V, B Q), everything in units of 1 / 8): every product and every partial sum
in any order is exact in float32, the second bf16 term of every cotangent element is non-zero and the third is zero.  x2 (float32 split
images): features odd integers of 9 bits / 512 (hi and lo bf16 parts both non-zero), the cotangent integers of at most 8 significant bits
(g_lo = 0, so the dropped g_lo x_lo is exactly zero and g_hi x_lo is exercised).  Cotangent positions a mask removes carry finite poison:
+-2^20 where only vmask removes them, distinct values above 2^21 where tmask does.
"""
import collections
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_align_paths import EDGE_FEATURES, _rng, cdiv, make_masks, mask_features

# ---------------------------------------------------------------------------------------------------------------- the restatement
SPLIT_MAX_M, SPLIT_MAX_K, SPLIT_D = 96, 96, 128     # bwd_split_ok
CONCAT_SPAN, CONCAT_PAD = 96, 96                    # bwd_concat_ok: 2 K <= 96; bwd_concat_pitch: O K + 96 rounded up to 8
K_NT = 2                                            # kNT: bf16 terms of the cotangent
K_CW3 = 2                                           # kCW3: column groups of the three-row-tile images
MT3_ROWS = 48                                       # M <= 48: MT 3 x CW kCW3; above: MT 6 x CW 1
NS_LADDER = (6, 9, 12, 21, 24)
GEN_SPLIT_WGS, GEN_SPLIT_O = 768, 16                # generic: gx fixn < 768 and O / 2 >= 16
SPLIT_FIX, SPLIT_O = 1024, 16                       # split routes: 2 fixn <= 1024 nf and O >= 16
NF_MIN = 64                                         # two fixed indices per workgroup from fixn >= 64 (bf16 features)
K_BWD_THREADS = 256
LDS_BUDGET = 160 * 1024
VLG_F32, VLG_BF16 = 0, 1
DTYPES = ("bf16", "f32")


def nfv(kc, nkc, mt):
    """launch_bwd_split: the two-index form where it fits the registers of a 12-wave block"""
    return 1 if nkc == 3 and (mt == 6 or kc) else 2


def split_ok(d, M, K):
    return d == SPLIT_D and M <= SPLIT_MAX_M and K <= SPLIT_MAX_K


def concat_ok(K):
    return K % 4 == 0 and K >= 4 and 2 * K <= CONCAT_SPAN


def concat_pitch(O, K):
    return (O * K + CONCAT_PAD + 7) // 8 * 8


def _blocks(O, split, opb):
    return [(y * opb, min(O, (y + 1) * opb)) for y in range(split)]


def _mt(M):
    return (3, K_CW3) if M <= MT3_ROWS else (6, 1)


def split_side(kc, dt, fixn, O, M, K, sr, sk):
    f32 = dt == "f32"
    Kp = cdiv(K, 32) * 32
    nkc = Kp // 32
    nf = 2 if not f32 and fixn >= NF_MIN else 1
    split = 2 if fixn * 2 <= SPLIT_FIX * nf and O >= SPLIT_O else 1
    opb = cdiv(O, split)
    mt, cw = _mt(M)
    nfe = nfv(kc, nkc, mt) if nf == 2 else 1
    quads = (K % 4 == 0 and K >= 4) if kc else None
    gx = cdiv(fixn, nfe)
    last = ((K - 4 if quads else K - 1) + (3 if quads else 0)) if kc else (K - 1) * sk
    return dict(route="split_kc" if kc else "split_kn", image=("KC" if kc else "KN", nkc, mt, cw, nfe, f32), k_quads=quads, grid=(gx, split),
                threads=64 * mt * cw * nfe, split=split, opb=opb, blocks=_blocks(O, split, opb), lds=(4 if f32 else 2) * 128 * (Kp * 2 + 32),
                zeroed=split > 1, fixn=fixn, O=O, M=M, K=K, nkc=nkc, mt=mt, nf=nfe, mirrored=gx * nfe - fixn,
                goff_max=4 * ((M - 1) * sr + last), step2=0)


def concat_side(B, A, Q, V):
    nf = 2 if B >= NF_MIN else 1
    split = 2 if B * 2 <= SPLIT_FIX * nf and A >= SPLIT_O else 1
    opb = (cdiv(A, split) + 1) & ~1
    mt, cw = _mt(Q)
    gx = cdiv(B, nf)
    blocks = _blocks(A, split, opb)
    return dict(route="concat2", image=(mt, cw, nf), k_quads=True, grid=(gx, split), threads=384 * nf, split=split, opb=opb, blocks=blocks,
                lds=2 * 128 * (CONCAT_SPAN * 2 + 32), zeroed=split > 1, fixn=B, O=A, M=Q, K=V, nkc=3, mt=mt, nf=nf, mirrored=gx * nf - B,
                lone=[(o1 - o0) % 2 == 1 for o0, o1 in blocks], goff_max=4 * ((Q - 1) * V + V - 1), step2=4 * Q * V if A > 1 else 0,
                step2_zero_at_end=A % 2 == 1,                    # the last step of the range holds pair A - 1 alone: o + 1 == O
                tile8=((A - 1) * V * 2) % 16 == 8,               # the look-ahead tile clamped to pair A - 1 starts 8 bytes off a 16-byte line
                straddle=(V // 32) != ((2 * V - 1) // 32))      # the second pair's positions cross a 32-position chunk


def generic_side(dt, d, fixn, O, M, K):
    steps = cdiv(K, 4)
    ns = next((n for n in NS_LADDER[:-1] if steps <= n), NS_LADDER[-1])
    tiles = cdiv(M, 16)
    gx = cdiv(tiles, 4)
    split = 2 if gx * fixn < GEN_SPLIT_WGS and O // 2 >= GEN_SPLIT_O else 1
    opb = cdiv(O, split)
    nck = cdiv(K, ns * 4)
    blocks = _blocks(O, split, opb)
    iters = [(o1 - o0) * nck for o0, o1 in blocks]
    return dict(route="generic", image=(dt, d // 16, ns), k_quads=None, grid=(gx, fixn, split), threads=K_BWD_THREADS, split=split, opb=opb,
                blocks=blocks, lds=2 * ns * 4 * (d + 16) * (4 if dt == "f32" else 2), zeroed=split > 1, fixn=fixn, O=O, M=M, K=K, ns=ns, nck=nck,
                gx=gx, idle=gx * 4 - tiles, iters=iters, iters_mod3=[i % 3 for i in iters], goff_max=0, step2=0)


def plan(dt, d, B, A, Q, V, want_txt=True, want_vis=True):
    """what vlg_bilinear_align_backward launches per wanted side, and how it carves the workspace (bytes)"""
    assert dt in DTYPES and d in (32, 64, 128) and min(B, A, Q, V) >= 1 and (want_txt or want_vis)
    fast = split_ok(d, Q, V)
    assert fast == split_ok(d, V, Q)           # one condition decides both sides
    f32 = dt == "f32"
    concat = fast and concat_ok(V) and not f32
    P = dict(txt=None, vis=None)
    if want_txt:
        P["txt"] = concat_side(B, A, Q, V) if concat else split_side(True, dt, B, A, Q, V, V, 1) if fast else generic_side(dt, d, B, A, Q, V)
    if want_vis:
        P["vis"] = split_side(False, dt, A, B, V, Q, 1, V) if fast else generic_side(dt, d, A, B, V, Q)
    ws, off = [], 0
    if fast:
        Vp, Qp = cdiv(V, 32) * 32, cdiv(Q, 32) * 32
        parts = ("hi", "lo") if f32 else ("hi",)
        for name, n in ([("featC", 128 * concat_pitch(A, V))] if concat else [("visT_" + p, A * 128 * Vp) for p in parts]) + \
                [("txtT_" + p, B * 128 * Qp) for p in parts]:
            ws.append((name, off, 2 * n))
            off += 2 * n
    P["ws"], P["ws_bytes"] = ws, off
    return P


# ---------------------------------------------------------------------------------------------------------------- the case table
Case = collections.namedtuple("Case", "group dt d B A Q V mask want data claim")
CASES = []
MASKS = ("none", "both", "t", "v")


def add(group, dt, d, B, A, Q, V, mask="none", want="tv", data="g2", **claim):
    CASES.append(Case(group, dt, d, B, A, Q, V, mask, want, data, claim))


def derive(c):
    """what a case's claim is compared with: every number of plan() per wanted side, t_* for the caption side and v_* for the image side"""
    P = plan(c.dt, c.d, c.B, c.A, c.Q, c.V, "t" in c.want, "v" in c.want)
    out = dict(routes="+".join(P[s]["route"] for s in ("txt", "vis") if P[s]), ws_bytes=P["ws_bytes"])
    for pre, s in (("t_", "txt"), ("v_", "vis")):
        if P[s]:
            out.update({pre + k: v for k, v in P[s].items()})
    return out


def case_id(c):
    return f"{c.group}_{c.dt}_d{c.d}_B{c.B}_A{c.A}_Q{c.Q}_V{c.V}_{c.want}_{c.mask}_{c.data}_{c.claim['routes']}"


def input_key(c):
    return (c.dt, c.d, c.B, c.A, c.Q, c.V, c.mask, c.data)


def fast_routes(dt, V):
    return ("concat2" if dt == "bf16" and concat_ok(V) else "split_kc") + "+split_kn"


NKC_OF = {1: 1, 3: 1, 15: 1, 16: 1, 17: 1, 31: 1, 32: 1, 33: 2, 40: 2, 48: 2, 49: 2, 52: 2, 64: 2, 65: 3, 95: 3, 96: 3}     # ceil(K / 32)
MT_OF = {k: 3 if k <= 48 else 6 for k in NKC_OF}
SWEEP = (1, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 95, 96)
n = 0
for dt in DTYPES:
    # rows and contraction length of both sides: Q sweeps against V = 3 (words), 40 (quads / concat2), 49, 52, 96 (quads), and V against the same Q
    pairs = [(q, v) for q in SWEEP for v in (3, 40, 49, 52, 96)] + [(q, v) for v in SWEEP for q in (3, 40, 49, 96)]
    for Q, V in sorted(set(pairs)):
        n += 1
        cl = dict(routes=fast_routes(dt, V), v_nkc=NKC_OF[Q], v_mt=MT_OF[V], t_mt=MT_OF[Q], t_split=1, v_split=1)
        if "split_kc" in cl["routes"]:
            cl.update(t_nkc=NKC_OF[V], t_k_quads=V % 4 == 0 and V >= 4)
        add("sp", dt, 128, 2, 2, Q, V, MASKS[n % 4], **cl)
    # 97 rows or positions: both sides leave the split-term path together
    for Q, V in ((97, 3), (3, 97), (96, 97), (97, 96), (97, 40)):
        add("sp", dt, 128, 2, 2, Q, V, routes="generic+generic", ws_bytes=0)

# outer count: (O, split, opb, blocks) for the split routes; B = A = O puts both sides on the boundary
OUTER = {1: (1, 1, [(0, 1)]), 2: (1, 2, [(0, 2)]), 3: (1, 3, [(0, 3)]), 15: (1, 15, [(0, 15)]), 16: (2, 8, [(0, 8), (8, 16)]), 17: (2, 9, [(0, 9), (9, 17)])}
for dt in DTYPES:
    for O, (split, opb, blocks) in OUTER.items():
        for Q, V in ((5, 3), (50, 70), (33, 96)):
            add("o", dt, 128, O, O, Q, V, MASKS[(O + Q) % 4], routes="split_kc+split_kn", t_split=split, t_opb=opb, t_blocks=blocks, v_split=split,
                v_opb=opb, v_blocks=blocks, t_zeroed=split == 2, v_zeroed=split == 2)

# fixed indices: NF = 2 from 64 on; 65 leaves one wave set mirroring index 64, which must store nothing.  Every NF = 2 image:
# caption side (B >= 64) NKC 1 | 2 x MT 3 | 6; image side (A >= 64) NKC 1 | 2 x MT 3 | 6 and NKC 3 x MT 3; NKC 3 elsewhere keeps NF = 1
FX = [(20, 5), (60, 5), (20, 37), (60, 37), (90, 5), (20, 70), (60, 70), (90, 70), (90, 90), (5, 90), (60, 90), (20, 52), (60, 64)]      # (the last two: quads)
for Q, V in FX:
    for fixn, nfe_if, mirrored in ((63, 1, 0), (64, 2, 0), (65, 2, 1)):
        if fixn != 65 and (Q, V) not in ((20, 5), (60, 37), (90, 70), (90, 5)):
            continue
        t_nf = nfe_if if nfv(True, cdiv(V, 32), MT_OF.get(Q, 3 if Q <= 48 else 6)) == 2 else 1
        v_nf = nfe_if if nfv(False, cdiv(Q, 32), 3 if V <= 48 else 6) == 2 else 1
        add("fx", "bf16", 128, fixn, 2, Q, V, MASKS[(Q + fixn) % 4], routes="split_kc+split_kn", t_nf=t_nf, t_mirrored=mirrored if t_nf == 2 else 0, v_nf=1,
            t_split=1)
        add("fx", "bf16", 128, 2, fixn, Q, V, MASKS[(V + fixn) % 4], routes="split_kc+split_kn", v_nf=v_nf, v_mirrored=mirrored if v_nf == 2 else 0, t_nf=1,
            v_split=1)
for fixn in (1, 2, 63, 64, 65):      # fixn = 1, 2 (one workgroup or two); float32 features never take the two-index form
    add("fx", "f32", 128, fixn, 3, 20, 37, "both", routes="split_kc+split_kn", t_nf=1, v_nf=1, t_grid=(fixn, 1))
    add("fx", "bf16", 128, fixn, 17, 20, 37, "both", routes="split_kc+split_kn", t_nf=2 if fixn >= 64 else 1, t_split=2, t_opb=9, t_blocks=[(0, 9), (9, 17)])
add("fx", "bf16", 128, 1, 1, 1, 1, routes="split_kc+split_kn", t_grid=(1, 1), v_grid=(1, 1))
add("fx", "f32", 128, 1, 1, 1, 1, routes="split_kc+split_kn", t_grid=(1, 1), v_grid=(1, 1))

# the unsplit plan at large fixn, O = 16: (dt, fixn, split)
BIG = [("f32", 512, 2), ("f32", 513, 1), ("bf16", 1024, 2), ("bf16", 1025, 1)]
for dt, fixn, split in BIG:
    for s in (1, 2, 3, 4):
        t_routes = fast_routes(dt, s)
        add("big", dt, 128, fixn, 16, s, s, MASKS[s % 4], routes=t_routes, t_split=split, t_opb=16 // split, t_zeroed=split == 2, v_split=2,
            **(dict(t_nf=2) if dt == "bf16" and s < 4 else {}))
        add("big", dt, 128, 16, fixn, s, s, MASKS[(s + 1) % 4], routes=t_routes, v_split=split, v_opb=16 // split, v_zeroed=split == 2, t_split=2,
            **(dict(v_nf=2) if dt == "bf16" else {}))

# concat2
for V in (4, 8, 20, 32, 36, 44, 48, 3, 5, 52):
    for Q in (17, 49):
        inside = V % 4 == 0 and 4 <= V <= 48
        add("cc", "bf16", 128, 2, 3, Q, V, MASKS[(V + Q) % 4], routes=("concat2" if inside else "split_kc") + "+split_kn",
            **(dict(t_image=(3 if Q <= 48 else 6, 2 if Q <= 48 else 1, 1), t_straddle=V in (20, 36, 44, 48), t_lone=[True], t_step2_zero_at_end=True) if inside else {}))
for Q in (1, 16, 48, 96):      # (17 and 49 are in the V rows above)
    for V in (20, 36):
        add("cc", "bf16", 128, 2, 3, Q, V, MASKS[Q % 4], routes="concat2+split_kn", t_mt=3 if Q <= 48 else 6)
# A: (split, opb, blocks, lone per block)
CC_A = {1: (1, 2, [(0, 1)], [True]), 2: (1, 2, [(0, 2)], [False]), 3: (1, 4, [(0, 3)], [True]), 15: (1, 16, [(0, 15)], [True]),
        16: (2, 8, [(0, 8), (8, 16)], [False, False]), 17: (2, 10, [(0, 10), (10, 17)], [False, True]), 18: (2, 10, [(0, 10), (10, 18)], [False, False]),
        19: (2, 10, [(0, 10), (10, 19)], [False, True])}
for A, (split, opb, blocks, lone) in CC_A.items():
    for V in (20, 8):
        add("cc", "bf16", 128, 2, A, 5, V, MASKS[A % 4], routes="concat2+split_kn", t_split=split, t_opb=opb, t_blocks=blocks, t_lone=lone,
            t_step2_zero_at_end=A % 2 == 1, t_tile8=V == 20 and A % 2 == 0, t_step2=0 if A == 1 else 4 * 5 * V)
for B, nf, mirrored in ((1, 1, 0), (63, 1, 0), (64, 2, 0), (65, 2, 1)):
    for A, Q in ((3, 5), (17, 50)):
        add("cc", "bf16", 128, B, A, Q, 20, MASKS[(B + A) % 4], routes="concat2+split_kn", t_image=(3 if Q <= 48 else 6, 2 if Q <= 48 else 1, nf),
            t_mirrored=mirrored, t_split=2 if A == 17 else 1)

# generic: ns by K, nck
NS_OF = {1: (6, 1), 24: (6, 1), 25: (9, 1), 36: (9, 1), 37: (12, 1), 48: (12, 1), 49: (21, 1), 84: (21, 1), 85: (24, 1), 96: (24, 1), 97: (24, 2), 192: (24, 2),
         193: (24, 3)}
n = 0
for dt in DTYPES:
    for d in (32, 64, 128):
        for K, (ns, nck) in NS_OF.items():
            n += 1
            far, near = (97, 97) if d == 128 else (17, 3)
            add("gn", dt, d, 2, 2, far, K, MASKS[n % 4], routes="generic+generic", t_image=(dt, d // 16, ns), t_nck=nck, ws_bytes=0)
            if (n + d // 32) % 2:      # the image side's contraction: every other (dt, d, K)
                add("gn", dt, d, 2, 2, K, near, MASKS[(n + 1) % 4], routes="generic+generic", v_image=(dt, d // 16, ns), v_nck=nck, ws_bytes=0)
# M: (gx, idle waves)
GEN_M = {1: (1, 3), 16: (1, 3), 17: (1, 2), 48: (1, 1), 64: (1, 0), 65: (2, 3), 97: (2, 1)}
for i, (M, (gx, idle)) in enumerate(GEN_M.items()):
    add("gn", DTYPES[i % 2], 64, 2, 2, M, 5, MASKS[i % 4], routes="generic+generic", t_gx=gx, t_idle=idle)
    add("gn", DTYPES[(i + 1) % 2], 64, 2, 2, 5, M, MASKS[(i + 1) % 4], routes="generic+generic", v_gx=gx, v_idle=idle)
# iterations per block 1 .. 5 (one chunk per outer index), then 2 x 2 and 5 x 1 with two chunks
for O in (1, 2, 3, 4, 5):
    add("gn", DTYPES[O % 2], 32, O, O, 5, 7, MASKS[O % 4], routes="generic+generic", t_iters=[O], v_iters=[O], t_iters_mod3=[O % 3])
add("gn", "f32", 64, 2, 2, 5, 97, routes="generic+generic", t_iters=[4], t_nck=2)
add("gn", "bf16", 64, 1, 1, 5, 97, routes="generic+generic", t_iters=[2], t_nck=2)
for O, split, opb, iters in ((31, 1, 31, [31]), (32, 2, 16, [16, 16]), (33, 2, 17, [17, 16])):
    for dt in DTYPES:
        add("gn", dt, 64, O, O, 3, 3, MASKS[O % 4], routes="generic+generic", t_split=split, t_opb=opb, t_iters=iters, v_split=split, t_zeroed=split == 2)
for fixn, split in ((767, 2), (768, 1)):
    add("gn", "bf16", 32, fixn, 32, 2, 2, "both", routes="generic+generic", t_split=split, v_split=2, t_grid=(1, fixn, split))
    add("gn", "f32", 32, 32, fixn, 2, 2, "both", routes="generic+generic", v_split=split, t_split=2, v_grid=(1, fixn, split))

# masks per route x dtype (B = A = 4, Q = 21 = 16 + 5, V % 16 != 0), every mask kind; outputs alone and together
MASKED = [("bf16", 128, 21, 12, "concat2+split_kn"), ("bf16", 128, 21, 13, "split_kc+split_kn"), ("bf16", 128, 21, 52, "split_kc+split_kn"),
          ("f32", 128, 21, 12, "split_kc+split_kn"), ("f32", 128, 21, 13, "split_kc+split_kn"), ("bf16", 64, 21, 13, "generic+generic"),
          ("f32", 64, 21, 13, "generic+generic"), ("bf16", 128, 21, 101, "generic+generic"), ("f32", 128, 21, 101, "generic+generic")]
for dt, d, Q, V, routes in MASKED:
    for mask in ("none", "both", "t", "v", "edges"):
        add("mk", dt, d, 4, 4, Q, V, mask, routes=routes)
    add("mk", dt, d, 4, 4, Q, V, "both", "t", routes=routes.split("+")[0])
    add("mk", dt, d, 4, 4, Q, V, "both", "v", routes=routes.split("+")[1])
# ... and across a split (two-addend atomics into a zeroed output) with edges masks
for dt in DTYPES:
    for V in (12, 13):
        add("mk", dt, 128, 17, 17, 21, V, "edges", routes=fast_routes(dt, V), t_split=2, v_split=2)
    add("mk", dt, 64, 33, 33, 21, 13, "edges", routes="generic+generic", t_split=2, v_split=2)

# x2 on the float32 split images: every (side, NKC, MT), both k_quads branches
for Q, V in [(q, v) for q in (5, 70) for v in (3, 4, 50, 52, 90, 96)] + [(40, 3), (40, 50), (96, 96)]:
    add("x2", "f32", 128, 2, 3, Q, V, MASKS[(Q + V) % 4], data="x2", routes="split_kc+split_kn", t_k_quads=V % 4 == 0)
add("x2", "f32", 128, 17, 17, 21, 13, "edges", data="x2", routes="split_kc+split_kn", t_split=2, v_split=2)
add("x2", "f32", 128, 513, 16, 2, 2, "both", data="x2", routes="split_kc+split_kn", t_split=1, v_split=2)

# cotangent at float offsets 1, 2, 3 inside a larger allocation: one k_quads case of split_kc and one of concat2
ALIGNMENT = [Case("al", "f32", 128, 3, 3, 21, 12, "both", "tv", "g2", dict(routes="split_kc+split_kn", t_k_quads=True)),
             Case("al", "bf16", 128, 3, 3, 21, 52, "both", "tv", "g2", dict(routes="split_kc+split_kn", t_k_quads=True)),
             Case("al", "bf16", 128, 3, 3, 21, 20, "both", "tv", "g2", dict(routes="concat2+split_kn"))]

# the rounding set: one case per route x dtype on normal(0, 0.5) data, both masks random
ROUNDING = [Case("rnd", "bf16", 128, 4, 5, 82, 36, "both", "tv", "rnd", dict(routes="concat2+split_kn")),
            Case("rnd", "bf16", 128, 4, 5, 82, 37, "both", "tv", "rnd", dict(routes="split_kc+split_kn")),
            Case("rnd", "f32", 128, 4, 5, 82, 36, "both", "tv", "rnd", dict(routes="split_kc+split_kn")),
            Case("rnd", "bf16", 128, 4, 5, 100, 36, "both", "tv", "rnd", dict(routes="generic+generic")),
            Case("rnd", "f32", 128, 4, 5, 100, 36, "both", "tv", "rnd", dict(routes="generic+generic")),
            Case("rnd", "bf16", 64, 4, 5, 82, 36, "both", "tv", "rnd", dict(routes="generic+generic")),
            Case("rnd", "f32", 32, 4, 5, 82, 36, "both", "tv", "rnd", dict(routes="generic+generic"))]

# the Python layer: one case per route
PYTHON = [c for c in ALIGNMENT[1:]] + [Case("py", "f32", 64, 3, 3, 21, 13, "both", "tv", "g2", dict(routes="generic+generic"))]


# ---------------------------------------------------------------------------------------------------------------- inputs
G2_CHOICES = ((11, 8), (10, 8), (9, 8), (9, 4), (9, 2), (9, 1))      # (significant bits of the cotangent, feature range R) in order of preference
X2_BITS = 9                                                            # feature integers of the x2 set: 9 significant bits


def data_params(key):
    """(gb, R | xb): the widest ranges with terms 2^gb R < 2^24, terms = max(A V, B Q); every magnitude bound is a power of two at or above
    what bf16 rounding of a term can reach, so the bound holds for the kernels' partial sums over t0, t1, hi and lo parts as well"""
    dt, d, B, A, Q, V, mask, data = key
    terms = max(A * V, B * Q)
    if data == "g2":
        return next((gb, R) for gb, R in G2_CHOICES if terms * 2 ** gb * R < 2 ** 24)
    gb = min(8, int(math.floor(math.log2((2 ** 24 - 1) / (terms * 2 ** X2_BITS)))))
    assert gb >= 1, "x2 does not fit this shape"
    return gb, X2_BITS


def backward_masks(mask, B, A, Q, V, rng):
    return make_masks(mask, B, A, Q, V, rng)


def poison(g, tmask, vmask, rng):
    """finite poison at the cotangent positions a mask removes: +-2^20 where vmask alone does, distinct values above 2^21 where tmask does"""
    B, A, Q, V = g.shape
    if vmask is not None:
        dead = np.broadcast_to((vmask == 0)[None, :, None, :], g.shape)
        g[dead] = (rng.integers(0, 2, g.shape) * 2 - 1)[dead] * 2.0 ** 20
    if tmask is not None:
        dead = np.broadcast_to((tmask == 0)[:, None, :, None], g.shape)
        distinct = 2.0 ** 21 + 4096.0 * (np.arange(g.size).reshape(g.shape) % 251)
        g[dead] = ((rng.integers(0, 2, g.shape) * 2 - 1) * distinct)[dead]
    return g


def exact_inputs(key):
    """(g [B,A,Q,V], txt [B,Q,d], vis [A,V,d], tmask, vmask) as float64 (masks uint8 or None)"""
    dt, d, B, A, Q, V, mask, data = key
    rng = _rng("bwd-exact", *key)
    gb, xr = data_params(key)
    sign = lambda shape: rng.integers(0, 2, shape) * 2.0 - 1.0
    if data == "g2":
        txt, vis = rng.integers(-xr, xr + 1, (B, Q, d)) / 8.0, rng.integers(-xr, xr + 1, (A, V, d)) / 8.0
        g = sign((B, A, Q, V)) * (rng.integers(128, 2 ** (gb - 1), (B, A, Q, V)) * 2 + 1)            # odd, 257 .. 2^gb - 1
    else:
        assert data == "x2" and dt == "f32"
        txt = sign((B, Q, d)) * (rng.integers(128, 256, (B, Q, d)) * 2 + 1) / 512.0                  # odd, 257 .. 511: nine bits
        vis = sign((A, V, d)) * (rng.integers(128, 256, (A, V, d)) * 2 + 1) / 512.0
        g = sign((B, A, Q, V)) * rng.integers(1, 2 ** gb, (B, A, Q, V))
    tmask, vmask = backward_masks(mask, B, A, Q, V, rng)
    return poison(g, tmask, vmask, rng), txt, vis, tmask, vmask


def rounding_inputs(key):
    import torch
    dt, d, B, A, Q, V, mask, data = key
    rng = _rng("bwd-rounding", *key)
    g, txt, vis = rng.normal(0, 0.5, (B, A, Q, V)), rng.normal(0, 0.5, (B, Q, d)), rng.normal(0, 0.5, (A, V, d))
    g = g.astype(np.float32).astype(np.float64)
    if dt == "bf16":
        txt, vis = (torch.from_numpy(x).float().bfloat16().double().numpy() for x in (txt, vis))
    else:
        txt, vis = (x.astype(np.float32).astype(np.float64) for x in (txt, vis))
    return (g, txt, vis) + backward_masks(mask, B, A, Q, V, rng)


def bf16_terms(x):
    """x (float64, exact in float32) as its successive bf16 terms t0, t1, t2 (round to nearest even, as the kernels' casts)"""
    import torch
    v, out = torch.from_numpy(np.ascontiguousarray(x)).float(), []
    for _ in range(3):
        h = v.bfloat16().float()
        out.append(h.double().numpy())
        v = v - h
    return out


# ---------------------------------------------------------------------------------------------------------------- tests
def _src():
    return open(os.path.join(ROOT, "vlgae_amd", "csrc", "vlg_align.hip")).read()


def test_constants_read_from_the_sources():
    """Every constant of the restatement, found in vlg_align.hip by regex and equal to the restatement's."""
    s = _src()

    def num(pattern):
        found = re.findall(pattern, s)
        assert len(found) == 1, (pattern, found)
        return tuple(map(int, found[0])) if isinstance(found[0], tuple) else int(found[0])

    def once(pattern):
        assert len(re.findall(pattern, s)) == 1, pattern

    assert num(r"\(in_dtype == VLG_BF16 \|\| in_dtype == VLG_F32\) && d == (\d+) && M <= (\d+) && K <= (\d+);") == (SPLIT_D, SPLIT_MAX_M, SPLIT_MAX_K)
    assert num(r"static bool bwd_concat_ok\(int K\) \{ return \(K & 3\) == 0 && K >= 4 && 2 \* K <= (\d+); \}") == CONCAT_SPAN
    assert num(r"static size_t bwd_concat_pitch\(int O, int K\) \{ return \(\(size_t\)O \* K \+ (\d+) \+ 7\) / 8 \* 8; \}") == CONCAT_PAD
    assert num(r"constexpr int kNT = (\d+);") == K_NT and num(r"constexpr int kCW3 = (\d+);") == K_CW3
    assert num(r"constexpr int kBwdThreads = (\d+);") == K_BWD_THREADS
    assert num(r"const int ns = steps <= (\d+) \? (\d+) : steps <= (\d+) \? (\d+) : steps <= (\d+) \? (\d+) : steps <= (\d+) \? (\d+) : (\d+);") == \
        tuple(x for n_ in NS_LADDER[:-1] for x in (n_, n_)) + NS_LADDER[-1:]
    once(r"const int steps = \(K \+ 3\) / 4;")
    for n_ in NS_LADDER:      # every rung of the ladder has its instantiation
        once(r"ns == %d \? VLG_BWD3\(INV, NCTV, %d\)" % (n_, n_) if n_ != NS_LADDER[-1] else r": VLG_BWD3\(INV, NCTV, %d\)\)" % n_)
    assert num(r"if \(\(long\)gx \* fixn < (\d+) && O / 2 >= (\d+)\) split = 2;") == (GEN_SPLIT_WGS, GEN_SPLIT_O)
    assert num(r"if \(\(long\)fixn \* 2 <= (\d+) \* nf && O >= (\d+)\) split = 2;") == (SPLIT_FIX, SPLIT_O)
    assert num(r"int split = \(\(long\)B \* 2 <= (\d+) \* nf && A >= (\d+)\) \? 2 : 1;") == (SPLIT_FIX, SPLIT_O)
    assert num(r"const int nf = \(!f32feat && fixn >= (\d+)\) \? 2 : 1;") == NF_MIN and num(r"const int nf = B >= (\d+) \? 2 : 1;") == NF_MIN
    once(r"constexpr int NFV = \(NKCV == 3 && \(MTV == 6 \|\| KC\)\) \? 1 : 2;")
    once(r"const int nfe = nf == 2 \? NFV : 1;")
    assert num(r"\(M <= (\d+) \? VLG_BS\(KC, NKCV, 3, kCW3\) : VLG_BS\(KC, NKCV, 6, 1\)\)") == MT3_ROWS
    assert num(r"Q <= (\d+) \? \(nf == 2 \? VLG_BS2K\(3, 2, 2\) : VLG_BS2K\(3, 2, 1\)\) : \(nf == 2 \? VLG_BS2K\(6, 1, 2\) : VLG_BS2K\(6, 1, 1\)\)") == MT3_ROWS
    once(r"\(nkc == 1 \? VLG_BS2\(KC, 1\) : nkc == 2 \? VLG_BS2\(KC, 2\) : VLG_BS2\(KC, 3\)\)")
    # launch shapes, LDS and the outer ranges
    once(r"dim3\(\(fixn \+ nfe - 1\) / nfe, split\), dim3\(64 \* MTV \* CWV \* nfe\)")
    once(r"dim3\(\(B \+ NFV - 1\) / NFV, split\), dim3\(384 \* NFV\)")
    once(r"const size_t lds = \(f32feat \? 4 : 2\) \* \(size_t\)128 \* \(Kp \* 2 \+ 32\);")
    once(r"const size_t lds = 2 \* \(size_t\)128 \* \(96 \* 2 \+ 32\);")
    once(r"const size_t lds = 2 \* \(size_t\)ns \* 4 \* \(d \+ 16\) \* esz;")
    once(r"const int tiles = \(M \+ 15\) / 16, gx = \(tiles \+ 3\) / 4;")
    once(r"const int opb = \(\(A \+ split - 1\) / split \+ 1\) & ~1;")
    assert len(re.findall(r"const int opb = \(O \+ split - 1\) / split;", s)) == 2
    once(r"const bool k_quads = \(K & 3\) == 0 && K >= 4;")
    once(r"const bool concat = bwd_split_ok\(in_dtype, d, Q, V\) && bwd_concat_ok\(V\) && !f32feat;")
    # the three lines of the mutation check are where the restatement says they are
    once(r"for \(int t = 0; t < \(part == 0 \? NT : 1\); \+\+t\)")
    once(r"float v = kk < K \|\| \(kk < 2 \* K && second\) \? graw\[kc\]\[j\] : 0\.f;")
    # the header states the finite-cotangent contract
    h = open(os.path.join(ROOT, "include", "vlgae_amd.h")).read()
    assert len(re.findall(r"grad_out must be finite", h)) == 1


def test_cases_are_in_the_class_their_name_claims():
    """Every case of the GPU file: plan() gives the routes, images, split plans and boundary numbers the table claims."""
    moved = []
    for c in CASES + ALIGNMENT + ROUNDING + PYTHON:
        got = derive(c)
        wrong = {k: (got.get(k), v) for k, v in c.claim.items() if got.get(k) != v}
        if wrong:
            moved.append(f"{case_id(c)}: (restated, claimed) {wrong}")
        assert c.B * c.A * c.Q * c.V <= 1.3e6 and c.B * c.A * c.Q * c.V * c.d <= 1.7e8, case_id(c)       # a few seconds at most, oracle included
    assert not moved, "cases that left the path they were written for:\n  " + "\n  ".join(moved)
    assert len({case_id(c) for c in CASES}) == len(CASES)


def _sides(cases=None):
    """(case, side name, side plan) of every wanted side of every case"""
    for c in CASES if cases is None else cases:
        P = plan(c.dt, c.d, c.B, c.A, c.Q, c.V, "t" in c.want, "v" in c.want)
        for s in ("txt", "vis"):
            if P[s]:
                yield c, s, P[s]


GRID_QV = (1, 3, 4, 5, 8, 20, 24, 25, 32, 33, 36, 37, 48, 49, 52, 64, 65, 84, 85, 96, 97, 193)
GRID_BA = ((2, 2), (64, 2), (2, 64), (64, 64), (1025, 16), (16, 1025))


def reachable_images():
    seen = set()
    for dt in DTYPES:
        for d in (32, 64, 128):
            for B, A in GRID_BA:
                for Q in GRID_QV:
                    for V in GRID_QV:
                        P = plan(dt, d, B, A, Q, V)
                        seen |= {(P[s]["route"], P[s]["image"], P[s]["k_quads"]) for s in ("txt", "vis")}
    return seen


def test_every_reachable_image_has_a_case():
    """Coverage.  The restatement enumerates the reachable (route, image, k_quads branch) set over a shape grid; every member has a case,
    and the template arguments the dispatch never forms are shown absent from the enumeration, not skipped by hand."""
    reach = reachable_images()
    images = {(r, im) for r, im, _ in reach}
    assert len(images) == 67 and len({im for r, im in images if r == "generic"}) == 30 and len({im for r, im in images if r == "concat2"}) == 4
    # what the dispatch cannot reach: NF = 2 with three chunks on six row tiles or on the caption side; NF = 2 with float32 features;
    # the quad branch of the caption side with bf16 features and one chunk (V <= 32, V % 4 == 0 is concat2)
    split_images = {im for r, im in images if r.startswith("split")}
    every = {(s, nkc, mt, K_CW3 if mt == 3 else 1, nf, f32) for s in ("KC", "KN") for nkc in (1, 2, 3) for mt in (3, 6) for nf in (1, 2) for f32 in (False, True)}
    assert split_images <= every
    assert every - split_images == {im for im in every if im[4] == 2 and (im[5] or (im[1] == 3 and (im[2] == 6 or im[0] == "KC")))}
    assert {(im, kq) for r, im, kq in reach if r == "split_kc" and im[1] == 1 and not im[5]} == \
        {(("KC", 1, mt, K_CW3 if mt == 3 else 1, nf, False), False) for mt in (3, 6) for nf in (1, 2)}
    assert {kq for r, im, kq in reach if r == "split_kc" and im[5]} == {True, False}
    have = {(s["route"], s["image"], s["k_quads"]) for _, _, s in _sides()}
    assert have <= reach or not (have - reach), sorted(have - reach)
    assert not (reach - have), "reachable images without a case:\n  " + "\n  ".join(map(str, sorted(reach - have, key=str)))
    # float32 split images: each runs g2 and x2, on both k_quads branches
    f32_split = {k for k in reach if k[0].startswith("split") and k[1][5]}
    for data in ("g2", "x2"):
        got = {(s["route"], s["image"], s["k_quads"]) for _, _, s in _sides([c for c in CASES if c.data == data])}
        assert not (f32_split - got), (data, sorted(f32_split - got, key=str))
    # every route x dtype: every mask kind, each output alone, a rounding case, an edges case across a split
    for route, dts in (("concat2", ("bf16",)), ("split_kc", DTYPES), ("split_kn", DTYPES), ("generic", DTYPES)):
        for dt in dts:
            mine = [(c, s) for c, _, s in _sides() if s["route"] == route and c.dt == dt]
            assert {c.mask for c, _ in mine} >= {"none", "both", "t", "v", "edges"}, (route, dt)
            assert {c.want for c, _ in mine} >= {"tv", "v" if route == "split_kn" else "t"} or route == "generic", (route, dt)
            assert any(c.mask == "edges" and s["split"] == 2 for c, s in mine), (route, dt)
            assert any(s["route"] == route and c.dt == dt for c, _, s in _sides(ROUNDING)), (route, dt)
        assert any(s["route"] == route for c, _, s in _sides(PYTHON)), route
    assert {c.want for c in CASES if c.claim["routes"] == "generic"} >= {"t"} and {c.want for c in CASES if c.claim["routes"] == "generic"}
    # the boundaries named in the file's docstring, from the plans of the cases
    sp = [(c, n_, s) for c, n_, s in _sides() if s["route"] in ("split_kc", "split_kn")]
    for dt in DTYPES:
        assert {s["M"] for c, _, s in sp if c.dt == dt} >= {1, 15, 16, 17, 48, 49, 95, 96}
        for route in ("split_kc", "split_kn"):
            want_k = {1, 31, 33, 65, 95} | ({32, 64, 96} if route == "split_kn" or dt == "f32" else {64, 96})
            assert {s["K"] for c, _, s in sp if c.dt == dt and s["route"] == route} >= want_k, (dt, route)
            assert {s["O"] for c, _, s in sp if c.dt == dt and s["route"] == route} >= {1, 2, 3, 15, 16, 17}
            assert any(s["O"] == 17 and s["blocks"] == [(0, 9), (9, 17)] for c, _, s in sp if c.dt == dt and s["route"] == route)
        assert {s["fixn"] for c, _, s in sp if c.dt == dt} >= {1, 2, 63, 64, 65}
    assert any(c.Q == 97 and c.d == 128 for c in CASES) and any(c.V == 97 and c.d == 128 for c in CASES)
    assert {(s["fixn"], s["split"]) for c, _, s in sp if c.dt == "f32" and s["O"] == 16 and c.group == "big"} >= {(512, 2), (513, 1)}
    assert {(s["fixn"], s["split"], s["nf"]) for c, _, s in sp if c.dt == "bf16" and s["O"] == 16 and c.group == "big"} >= {(1024, 2, 2), (1025, 1, 2)}
    assert any(s["mirrored"] == 1 and s["nf"] == 2 for c, _, s in sp if s["route"] == "split_kc") and any(s["mirrored"] == 1 for c, _, s in sp if s["route"] == "split_kn")
    cc = [(c, s) for c, _, s in _sides() if s["route"] == "concat2"]
    assert {s["K"] for c, s in cc} >= {4, 8, 20, 32, 36, 44, 48} and {c.V for c in CASES if c.group == "cc"} >= {3, 5, 52}
    assert {s["M"] for c, s in cc} >= {1, 16, 17, 48, 49, 96} and {s["O"] for c, s in cc} >= {1, 2, 3, 15, 16, 17, 18, 19}
    assert {s["fixn"] for c, s in cc} >= {1, 63, 64, 65, 1024, 1025} and {(s["fixn"], s["split"]) for c, s in cc if s["O"] == 16} >= {(1024, 2), (1025, 1)}
    assert any(s["tile8"] and s["O"] % 2 == 0 and s["K"] % 8 == 4 for c, s in cc) and any(s["straddle"] for c, s in cc)
    assert {tuple(s["lone"]) for c, s in cc} >= {(True,), (False,), (False, False), (False, True)} and all(s["opb"] % 2 == 0 for c, s in cc)
    assert any(s["step2"] == 0 for c, s in cc) and any(s["mirrored"] == 1 for c, s in cc)
    gn = [(c, s) for c, _, s in _sides() if s["route"] == "generic"]
    assert {s["K"] for c, s in gn} >= set(NS_OF) and {s["M"] for c, s in gn} >= set(GEN_M)
    assert {i for c, s in gn for i in s["iters"]} >= {1, 2, 3, 4, 5} and {s["nck"] for c, s in gn} >= {1, 2, 3}
    assert {(s["O"], s["split"]) for c, s in gn} >= {(31, 1), (32, 2), (33, 2)}
    assert {(s["gx"] * s["fixn"], s["split"]) for c, s in gn if s["O"] == 32} >= {(767, 2), (768, 1)}
    assert {s["idle"] for c, s in gn} >= {0, 1, 2, 3} and {s["gx"] for c, s in gn} >= {1, 2}
    # the edges masks hold what their name says
    for c in CASES:
        if c.mask == "edges":
            _, _, _, t, v = exact_inputs(input_key(c))
            assert mask_features(t, v, c.Q, c.V) == EDGE_FEATURES, case_id(c)


def test_restatement_fails_when_a_constant_moves(monkeypatch):
    """The table is tied to the constants: with the row bound of the three-tile images 48 -> 64, or NF = 2 from 65 on, in the restatement, cases leave their class."""
    import sys
    me = sys.modules[__name__]
    monkeypatch.setattr(me, "MT3_ROWS", 64)
    assert any(derive(c).get("t_mt") != c.claim.get("t_mt", derive(c).get("t_mt")) for c in CASES)
    with pytest.raises(AssertionError):
        test_constants_read_from_the_sources()
    monkeypatch.setattr(me, "MT3_ROWS", 48)
    monkeypatch.setattr(me, "NF_MIN", 65)
    with pytest.raises(AssertionError):
        test_cases_are_in_the_class_their_name_claims()


@pytest.fixture(scope="module")
def lib():
    from vlgae_amd.build import build_library
    build_library()            # hipcc cross-compiles for gfx950 without a GPU
    from vlgae_amd import _C
    return _C.lib()


def test_workspace_layout_sums_to_the_query(lib):
    """plan()'s workspace carving (visT / featC then txtT, hi then lo) is contiguous and ends at vlg_bilinear_align_backward_workspace, for
    every case and for a grid around every boundary of the fast path; the query needs no GPU."""
    shapes = {(c.dt, c.d, c.B, c.A, c.Q, c.V) for c in CASES + ALIGNMENT + ROUNDING + PYTHON}
    for dt in DTYPES:
        for d in (32, 64, 128):
            for B, A in ((1, 1), (3, 2), (2, 17), (65, 3)):
                for Q in (1, 31, 32, 33, 64, 65, 95, 96, 97):
                    for V in (1, 3, 4, 5, 8, 31, 32, 33, 44, 47, 48, 49, 52, 64, 65, 95, 96, 97):
                        shapes.add((dt, d, B, A, Q, V))
    for dt, d, B, A, Q, V in sorted(shapes):
        P = plan(dt, d, B, A, Q, V)
        end = 0
        for name, off, ext in P["ws"]:
            assert off == end and ext > 0 and off % 16 == 0, (dt, d, B, A, Q, V, name)       # uint4 loads: every array starts on 16 bytes
            end = off + ext
        assert end == P["ws_bytes"] == lib.vlg_bilinear_align_backward_workspace(B, A, Q, V, d, VLG_BF16 if dt == "bf16" else VLG_F32), (dt, d, B, A, Q, V)
        names = [nm for nm, _, _ in P["ws"]]
        fast = d == 128 and Q <= 96 and V <= 96
        assert names == ([] if not fast else (["featC", "txtT_hi"] if dt == "bf16" and concat_ok(V) else ["visT_hi", "txtT_hi"]) if dt == "bf16" else
                         ["visT_hi", "visT_lo", "txtT_hi", "txtT_lo"])
    assert lib.vlg_bilinear_align_backward_workspace(0, 1, 1, 1, 128, 1) == 0 and lib.vlg_bilinear_align_backward_workspace(2, 2, 5, 5, 128, 7) == 0


def test_lds_and_offsets_fit():
    """Every launch's LDS is at most 160 KiB; every 32-bit byte offset the split kernels form (goff, step2, and their sum plus the 16 bytes
    of a quad load) is below 2^32 and inside one (fixed, outer) pair's cotangent block or the next one's."""
    for c, name, s in _sides(CASES + ALIGNMENT + ROUNDING + PYTHON):
        assert 0 < s["lds"] <= LDS_BUDGET, (case_id(c), name)
        assert s["threads"] <= 1024 and all(0 < x <= 65535 for x in s["grid"][1:]) and s["grid"][0] > 0
        assert s["goff_max"] + s["step2"] + 16 < 2 ** 32
        if s["route"] != "generic":
            assert s["goff_max"] + 4 <= 4 * c.Q * c.V, (case_id(c), name)      # the last word read lies in the pair's [Q, V] block
        assert all(o0 < o1 for o0, o1 in s["blocks"]) and s["blocks"][0][0] == 0 and s["blocks"][-1][1] == s["O"]
        assert all(a[1] == b[0] for a, b in zip(s["blocks"], s["blocks"][1:])) and len(s["blocks"]) <= 2      # two addends: order-free
    for O in range(SPLIT_O, 200):       # no split plan has an empty second block, also with concat2's even opb
        assert all(o0 < o1 for o0, o1 in _blocks(O, 2, cdiv(O, 2))) and all(o0 < o1 for o0, o1 in _blocks(O, 2, (cdiv(O, 2) + 1) & ~1))


def test_exact_inputs_make_the_float32_oracle_equal_the_float64_oracle(oracle_mod):
    """The exactness conditions of the data, per case: terms x max|g| x max|x| / quantum < 2^24; the float32 sequential oracle equals the
    float64 one bit for bit; g2: the second bf16 term of the cotangent is non-zero (on every element: they are odd with more than eight bits)
    and the third is zero; x2: both bf16 parts of every feature are non-zero, the cotangent has no second term."""
    done, threads = set(), oracle_mod.max_threads()
    oracle_mod.set_threads(min(threads, 8))       # the shapes are small: more threads than that only wait for each other
    for c in CASES + ALIGNMENT + PYTHON:
        key = input_key(c)
        if key in done:
            continue
        done.add(key)
        g, txt, vis, tmask, vmask = exact_inputs(key)
        keep = np.ones(g.shape, bool)
        if tmask is not None:
            keep &= (tmask != 0)[:, None, :, None]
        if vmask is not None:
            keep &= (vmask != 0)[None, :, None, :]
        assert np.isfinite(g).all() and np.array_equal(g.astype(np.float32).astype(np.float64), g)
        gb, xr = data_params(key)
        terms = max(c.A * c.V, c.B * c.Q)
        live = g[keep]
        if c.data == "g2":
            gmax, xmax = 2.0 ** gb, float(xr)                                    # in units of 1 and 1 / 8
            assert np.abs(live).max(initial=0) < gmax and max(np.abs(txt).max(), np.abs(vis).max()) * 8 <= xmax
            assert np.array_equal(txt * 8, np.round(txt * 8)) and np.array_equal(vis * 8, np.round(vis * 8))
            t0, t1, t2 = bf16_terms(live)
            assert (t1 != 0).mean() >= 0.5 if live.size else True
            assert not t2.any() and np.array_equal(t0 + t1, live) and np.abs(t0).max(initial=0) <= gmax
        else:
            gmax, xmax = 2.0 ** gb, 2.0 ** xr                                    # in units of 1 and 1 / 512
            assert np.abs(live).max(initial=0) < gmax
            t0, t1, _ = bf16_terms(live)
            assert not t1.any()
            for x in (txt, vis):
                hi, lo, rest = bf16_terms(x)
                assert hi.all() and lo.all() and not rest.any() and np.abs(hi * 512).max() <= xmax
        assert terms * gmax * xmax < 2 ** 24, case_id(c)
        poisoned = g[~keep]
        assert poisoned.size == 0 or np.abs(poisoned).min() >= 2.0 ** 20
        r32 = oracle_mod.bilinear_align_backward(g, txt, vis, tmask, vmask, np.float32)
        r64 = oracle_mod.bilinear_align_backward(g, txt, vis, tmask, vmask, np.float64)
        for a, b in zip(r32, r64):
            assert np.array_equal(a, b.astype(np.float32)) and np.isfinite(b).all(), case_id(c)
            assert np.abs(b).max() < 2 ** 24 / (8 if c.data == "g2" else 512)
    oracle_mod.set_threads(threads)


def test_mutations_reasoned_through_the_restatement():
    """Three one-line mutations of the kernels, as far as the restatement can tell (run on the GPU once, on scratch builds: the first two
    fail every g2 case of the split-term routes, 447 tests; the third passes all):
    kNT 2 -> 1 and `part == 0 ? NT : 1` -> `1` drop the second cotangent term of every product on part 0: on g2 every live cotangent element
    has a non-zero second term, so every split-term case with a live element changes by at least min|t1| / 8 per product -- no rounding.
    Dropping `&& second` in align_bwd_split2_kernel changes NOTHING the output can show: a block ends on a lone pair only at o + 1 == O
    (opb is even), where positions K .. 2 K - 1 of the tile are the zero pad columns of featC (bwd_concat_pitch's 96), and the cotangent
    re-read there (step2 == 0) is finite.  The select and the pad guard the same positions twice."""
    for c, _, s in _sides():
        if s["route"] == "concat2":
            assert s["opb"] % 2 == 0
            for (o0, o1), lone in zip(s["blocks"], s["lone"]):
                assert not lone or o1 == s["O"]                                   # the lone pair is the range's last: pair o + 1 does not exist
                assert concat_pitch(s["O"], s["K"]) >= s["O"] * s["K"] + s["K"]   # ... and its columns are pad
    g2_split = [c for c, _, s in _sides() if s["route"] != "generic" and c.data == "g2"]
    assert len(g2_split) > 100
