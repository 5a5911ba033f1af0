"""CPU: the dispatch of the arc encoder's trilinear contraction (vlgae_amd/csrc/vlg_arc.hip) restated in Python, pinned to the library
through its two workspace queries, an LDS bound over every launch of the restated plan, the host-side error returns, and the case table
of tests/test_arc_paths_gpu.py with the route every case claims.

vlg_trilinear / vlg_trilinear_ws / vlg_trilinear_backward[_g] turn (dtype, M, X, H, Y, workspace or not, which gradients) into launches:

  route          kernel(s)                                   taken when
  tk             tri_kernel<dt, KCH, RT>                     everything else.  KCH = Y / 32 (bf16) or Y / 16 (f32); xs = 2 ranges of x (atomics
                                                             into a zeroed out, grid padded to ceil(n_rb / 4) * 8 blocks) when X >= 32, else 1;
                                                             RT (16-row tiles per block) from a cost model over the CU count: 4 | 6 for bf16,
                                                             3 | 4 for f32, the second where it saves a round of blocks
  t2s / t2a      tri2_kernel + tri2_reduce_kernel (slabs) /  bf16, H = Y = 128, M >= 1024, 2 <= X <= 256.  With a workspace: xs = tri2_splits slabs
  t2d            tri2_kernel into `out` (two-range atomics   added in a fixed order (t2s), or one range stored directly (t2d, xs = 1: only the
                 or one range)                               backward gets there).  Without one: two ranges by atomicAdd (t2a) while
                                                             ceil(X / 2) <= 96, else tk
  t3             tri_split_rows_kernel x 2 + tri3_kernel     f32, H = Y = 128, M >= 1024, 2 <= X <= 256, with a workspace (without: tk)
                 (+ tri2_reduce_kernel when xs > 1)
  backward       d_child = dispatch(parent, wA, g, M, Y, X, H), d_parent = dispatch(child, wB, g, M, X, Y, H) on permuted weight copies
                 (tri_permute2_kernel when both are asked for and X, Y are multiples of 16 up to 128, else tri_permute_kernel mode 0 / 1);
                 d_w: dw2 = tri_dw2_kernel + tri_dw2_reduce_kernel (bf16, H = Y = 128, X even, M >= 1024; S row chunks, a trailing one may be
                 empty), else dw = three tri_transpose_kernel + tri_dw_kernel (rows padded to Mp).  float32 at X = H = Y = 128, M >= 1024 runs on
                 fp16 parts: tri_permute2_kernel, tri_split_rows_kernel, tri3_kernel, tri_absmax3_kernel + tri_dw3_kernel + tri_dw2_reduce_kernel

The LDS request of tri2_kernel is 65536 + 1024 ceil(X / xs) bytes: tri2_splits raises xs until ceil(X / xs) <= 96, and the atomic two-range form
is used only while ceil(X / 2) <= 96 (test_every_launch_fits_the_lds names the shapes that asked for more before that rule).

CASES: every id names group, entry, dtype, shape, the requested gradients, the claimed route descriptors (tk.<dt>.k<KCH>.r<RT>.xs<xs>.rb<n_rb>,
t2s|t2a|t2d.xs<xs>.rb<n_rb>, t3.xs<xs>.rb<n_rb>, dw2|dw3.S<S>.e<empty chunks>, dw.<dt>.Mp<Mp>) and the side of the boundary the row sits on.
Rows that target an RT take M from rt_run(): the first run of M that selects that RT at the row's xs under the given CU count ("lo" / "hi"
are its ends), so the GPU file reaches the named image on whatever count the device reports; their descriptors leave n_rb out.

Exact inputs (exact_inputs): child, parent, w and g are integers in [-4, 4] divided by 4.  Every two-factor product has at most 5 significant
bits (bf16(c * g) of tri_dw_kernel / tri_dw2_kernel is exact), every fp16 split has a zero lo part, every term is a multiple of 1 / 64 of
magnitude <= 1, and X * Y <= 32768, M < 262144 keep every partial sum in any order below 2^24 units: every output of every route must equal
float32 of the float64 reference bit for bit.  test_exact_inputs_are_exact asserts the bound from the shapes and, where the C oracle is
affordable, that its float32 results equal its float64 ones.
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
K_TRI2_ROWS = K_TRI3_ROWS = 256
TRI2_LDS_W = 2 * 128 * 128 * 2          # two weight planes of 128 x 128 bf16
TRI2_MAX_XPER = (LDS_LIMIT - TRI2_LDS_W) // (4 * K_TRI2_ROWS)     # 96: x values per workgroup whose float32 factors fit behind the planes
TRI3_MAX_XPER = 80
K_DW2_STAGE, K_DW2_XB, K_DW2_PITCH = 64, 2, 288
K_DW3_STAGE, K_DW3_XB, K_DW3_PITCH, K_DW3_MAX_BLOCKS = 32, 2, 288, 64
K_DW_SPLIT, K_DW_HT, K_DW_YT = 4, 4, 8
RT_CAND = {"bf16": (4, 6), "f32": (3, 4)}
RT_STREAM = {"bf16": 34.0, "f32": 1.5}
KW = {"bf16": 32, "f32": 16}
DEFAULT_CUS = 256


def cdiv(a, b):
    return (a + b - 1) // b


def up(b):
    return (b + 255) & ~255


def tri2_applies(M, X, H, Y, f32):
    return not f32 and H == 128 and Y == 128 and M >= 1024 and 2 <= X <= 256


def tri2_splits(M, X, guard=True):
    n_rb = cdiv(M, K_TRI2_ROWS)
    xs = min(max((256 + n_rb // 2) // n_rb, 1), 8)
    while xs > 1 and X // xs < 8:
        xs -= 1
    while guard and cdiv(X, xs) > TRI2_MAX_XPER:
        xs += 1
    return xs


def tri2_part_bytes(M, X, guard=True):
    xs = tri2_splits(M, X, guard)
    return 4 * xs * M * 128 if xs > 1 else 0


def tri3_applies(M, X, H, Y):
    return H == 128 and Y == 128 and M >= 1024 and 2 <= X <= 256


def tri3_splits(M, X, guard=True):
    xs = tri2_splits(M, X, guard)
    while cdiv(X, xs) > TRI3_MAX_XPER:
        xs += 1
    return xs


def tri3_part_bytes(M, X, guard=True):
    xs = tri3_splits(M, X, guard)
    return 4 * xs * M * 128 if xs > 1 else 0


def tri3_carve(rows):
    return 2 * up(rows * 128 * 2) + up(rows * 4)


def tri3_fwd_bytes(M, X, guard=True):
    return tri3_carve(X * 128) + tri3_carve(M) + up(tri3_part_bytes(M, X, guard))


def dw2_applies(M, X, H, Y, f32):
    return not f32 and H == 128 and Y == 128 and X % K_DW2_XB == 0 and M >= 1024


def dw2_splits(M, X):
    S = 8
    while S > 1 and ((X // K_DW2_XB) * (S // 2) >= 256 or cdiv(M, S) < 4 * K_DW2_STAGE):
        S //= 2
    return S


def dw3_applies(M, X, H, Y):
    return H == 128 and Y == 128 and X == 128 and M >= 1024


def dw3_splits(M, X):
    S = 8
    while S > 1 and ((X // K_DW3_XB) * (S // 2) >= 256 or cdiv(M, S) < 8 * K_DW3_STAGE):
        S //= 2
    return S


def pick_rt(dt, M, xs, cus):
    """launch_tri's rows per block: the first candidate unless the second needs fewer rounds of blocks by enough"""
    best = best_cost = None
    for rt in RT_CAND[dt]:
        cost = cdiv(cdiv(M, 16 * rt) * xs, cus) * (rt + RT_STREAM[dt])
        if best is None or cost < best_cost:
            best, best_cost = rt, cost
    return best


@functools.lru_cache(maxsize=None)
def rt_run(dt, rt, xs, cus):
    """(smallest, largest) M of the first run of row counts at which launch_tri picks `rt` with `xs` ranges on `cus` CUs"""
    lo = next((M for M in range(1, 1 << 17) if pick_rt(dt, M, xs, cus) == rt), None)
    assert lo is not None, f"no M below 2^17 selects RT = {rt} for {dt} at xs = {xs} on {cus} CUs"
    hi = lo
    while hi + 1 < (1 << 17) and pick_rt(dt, hi + 1, xs, cus) == rt:
        hi += 1
    return lo, hi


def workspace_fwd(dt, M, X, H, Y, guard=True):
    """vlg_trilinear_workspace"""
    if M < 1 or X < 1 or H < 1 or Y < 1:
        return 0
    if dt == "f32":
        return tri3_fwd_bytes(M, X, guard) if tri3_applies(M, X, H, Y) else 0
    return tri2_part_bytes(M, X, guard) if tri2_applies(M, X, H, Y, False) else 0


def bwd_plan(dt, M, X, H, Y, guard=True):
    """TriBwdPlan: offsets and bytes of the backward's scratch"""
    f32 = dt == "f32"
    esz = 4 if f32 else 2
    Mp = cdiv(M, KW[dt]) * KW[dt]
    wbytes = up(X * H * Y * esz)
    p = dict(Mp=Mp, off_wA=0, off_wB=wbytes, off_gB=2 * wbytes)
    p["off_cT"] = p["off_gB"] + up(M * H * esz)
    p["off_gT"] = p["off_cT"] + up(X * Mp * esz)
    p["off_pT"] = p["off_gT"] + up(H * Mp * esz)
    p["off_part"] = p["off_pT"] + up(Y * Mp * esz)
    pb = 4 * dw2_splits(M, X) * X * H * Y if dw2_applies(M, X, H, Y, f32) else 0
    if tri2_applies(M, Y, X, H, f32):
        pb = max(pb, tri2_part_bytes(M, Y, guard))
    if tri2_applies(M, X, Y, H, f32):
        pb = max(pb, tri2_part_bytes(M, X, guard))
    p["bytes"] = p["off_part"] + up(pb)
    if f32 and tri3_applies(M, X, H, Y) and dw3_applies(M, X, H, Y):
        off = p["off_gB"] + tri3_carve(Y * X) + tri3_carve(X * Y) + tri3_carve(M) + up(4 * 3 * K_DW3_MAX_BLOCKS)
        pb3 = max(4 * dw3_splits(M, X) * X * H * Y, tri3_part_bytes(M, Y, guard), tri3_part_bytes(M, X, guard))
        p["bytes"] = max(p["bytes"], off + up(pb3))
    return p


def workspace_bwd(dt, M, X, H, Y, guard=True):
    """vlg_trilinear_backward_workspace"""
    if M < 1 or X < 1 or H < 1 or Y < 1:
        return 0
    return bwd_plan(dt, M, X, H, Y, guard)["bytes"]


def check_dims(M, X, H, Y):
    if M < 0 or X < 1 or H < 1 or Y < 1 or H % 16 or H > 128 or X > 256:
        return ERR_SHAPE
    return 0


def _tri(dt, M, X, H, Y, cus):
    xs = 2 if X >= 32 else 1
    rt = pick_rt(dt, M, xs, cus)
    rows, n_rb = 16 * rt, cdiv(M, 16 * rt)
    blocks = cdiv(n_rb, 4) * 8 if xs == 2 else n_rb
    return [dict(k="tri_kernel", image=(dt, Y // KW[dt], rt), xs=xs, n_rb=n_rb, blocks=blocks, exited=blocks - n_rb * xs, lds=4 * rows * cdiv(X, xs),
                 ragged=M % rows != 0, n_ht=H // 16)]


def _tri2(M, X, part, guard):
    xs = tri2_splits(M, X, guard) if part else 2
    n_rb = cdiv(M, K_TRI2_ROWS)
    form = "a" if not part else ("d" if xs == 1 else "s")
    L = [dict(k="tri2_kernel", form=form, xs=xs, n_rb=n_rb, blocks=n_rb * xs, lds=TRI2_LDS_W + 4 * K_TRI2_ROWS * cdiv(X, xs), ragged=M % K_TRI2_ROWS != 0,
              ragged_x=X % xs != 0)]
    return L + ([dict(k="tri2_reduce_kernel", S=xs)] if form == "s" else [])


def _tri3(M, X, guard):
    xs = tri3_splits(M, X, guard)
    n_rb = cdiv(M, K_TRI3_ROWS)
    L = [dict(k="tri3_kernel", xs=xs, n_rb=n_rb, blocks=n_rb * xs, lds=4 * 64 * 128 * 2 + 4 * (2 * 64 + K_TRI3_ROWS * cdiv(X, xs)), ragged=M % K_TRI3_ROWS != 0)]
    return L + ([dict(k="tri2_reduce_kernel", S=xs)] if xs > 1 else [])


def dispatch_tri(dt, M, X, H, Y, part, cus, guard=True):
    """dispatch_tri: launches, or the error code"""
    if dt == "f32":
        if part and tri3_applies(M, X, H, Y):
            return [dict(k="tri_split_rows_kernel", rows=X * 128), dict(k="tri_split_rows_kernel", rows=M)] + _tri3(M, X, guard)
    elif tri2_applies(M, X, H, Y, False) and (part or not guard or cdiv(X, 2) <= TRI2_MAX_XPER):
        return _tri2(M, X, part, guard)
    if Y not in (32, 64, 128):
        return ERR_SHAPE
    return _tri(dt, M, X, H, Y, cus)


def forward(dt, M, X, H, Y, entry, cus=DEFAULT_CUS, guard=True):
    """vlg_trilinear (entry nows), vlg_trilinear_ws with its workspace (ws) or with ws = NULL (wsnull)"""
    rc = check_dims(M, X, H, Y)
    if rc or M == 0:
        return rc or []
    part = entry == "ws" and workspace_fwd(dt, M, X, H, Y, guard) > 0
    return dispatch_tri(dt, M, X, H, Y, part, cus, guard)


def backward(dt, M, X, H, Y, want, g16=False, cus=DEFAULT_CUS, guard=True):
    """vlg_trilinear_backward_g: [(role, launch)] in launch order, or (code, message fragment).  `want` is a string over c (d_child), w, p."""
    f32 = dt == "f32"
    rc = check_dims(M, X, H, Y)
    if rc:
        return rc, "trilinear_backward"
    if g16 and f32:
        return ERR_DTYPE, "a bf16 cotangent needs bf16 features"
    if Y not in (32, 64, 128):
        return ERR_SHAPE, f"trilinear_backward: Y={Y} (supported: 32, 64, 128)"
    if H not in (32, 64, 128):
        return ERR_SHAPE, f"trilinear_backward: H={H} (supported: 32, 64, 128)"
    dc, dw, dp = "c" in want, "w" in want, "p" in want
    L = []
    if f32 and tri3_applies(M, X, H, Y) and dw3_applies(M, X, H, Y):
        if dc or dp:
            L += [("prep", dict(k="tri_permute2_kernel", T="f32")), ("prep", dict(k="tri_split_rows_kernel", rows=M))]
        if dc:
            L += [("dc", dict(k="tri_split_rows_kernel", rows=Y * X))] + [("dc", l) for l in _tri3(M, Y, guard)]
        if dp:
            L += [("dp", dict(k="tri_split_rows_kernel", rows=X * Y))] + [("dp", l) for l in _tri3(M, X, guard)]
        if dw:
            S = dw3_splits(M, X)
            KC = cdiv(cdiv(M, S), K_DW3_STAGE) * K_DW3_STAGE
            L += [("dw", dict(k="tri_absmax3_kernel")),
                  ("dw", dict(k="tri_dw3_kernel", S=S, KC=KC, blocks=(X // K_DW3_XB) * S, lds=2 * 2 * (K_DW3_XB + 1) * K_DW3_STAGE * K_DW3_PITCH,
                              empty=sum(s * KC >= M for s in range(S)))), ("dw", dict(k="tri_dw2_reduce_kernel", S=S))]
        return L
    if not f32 and not g16:
        L.append(("prep", dict(k="tri_cast_bf16_kernel")))
    permuted = dc and dp and H <= 128 and X % 16 == 0 and X <= 128 and Y % 16 == 0 and Y <= 128
    if permuted:
        L.append(("prep", dict(k="tri_permute2_kernel", T=dt)))
    for on, role, mode, (x_, h_) in ((dc, "dc", 0, (Y, X)), (dp, "dp", 1, (X, Y))):
        if not on:
            continue
        if h_ % 16 or h_ > 128:
            return ERR_SHAPE, f"trilinear_backward: {'XY'[mode]}={h_} must be a multiple of 16 and <= 128"
        if not permuted:
            L.append((role, dict(k="tri_permute_kernel", mode=mode, T=dt)))
        r = dispatch_tri(dt, M, x_, h_, H, not f32, cus, guard)
        assert isinstance(r, list)      # (its contracted dimension is H, checked above)
        L += [(role, l) for l in r]
    if dw and dw2_applies(M, X, H, Y, f32):
        S = dw2_splits(M, X)
        KC = cdiv(cdiv(M, S), K_DW2_STAGE) * K_DW2_STAGE
        L += [("dw", dict(k="tri_dw2_kernel", S=S, KC=KC, blocks=(X // K_DW2_XB) * S, lds=2 * (K_DW2_XB + 1) * K_DW2_STAGE * K_DW2_PITCH,
                          empty=sum(s * KC >= M for s in range(S)))), ("dw", dict(k="tri_dw2_reduce_kernel", S=S))]
    elif dw:
        Mp = bwd_plan(dt, M, X, H, Y, guard)["Mp"]
        L += [("dw", dict(k="tri_transpose_kernel", cast=False, T=dt)), ("dw", dict(k="tri_transpose_kernel", cast=not (not f32 and g16), T=dt)),
              ("dw", dict(k="tri_transpose_kernel", cast=False, T=dt)),
              ("dw", dict(k="tri_dw_kernel", T=dt, Mp=Mp, pad=Mp - M, blocks=X * cdiv(H // 16, K_DW_HT), lds=4 * 4 * (K_DW_SPLIT - 1) * K_DW_HT * K_DW_YT * 64))]
    return L


def image_of(l):
    """the kernel image a launch runs, as the coverage list names it"""
    k = l["k"]
    if k == "tri_kernel":
        return "tri_kernel<%s, %d, %d>" % l["image"]
    if k == "tri2_kernel":
        return "tri2_kernel[%s]" % dict(s="slab", a="atomic", d="direct")[l["form"]]
    if k == "tri_permute_kernel":
        return f"tri_permute_kernel<{l['T']}>[mode {l['mode']}]"
    if k == "tri_permute2_kernel":
        return f"tri_permute2_kernel<{l['T']}>"
    if k == "tri_transpose_kernel":
        return f"tri_transpose_kernel<{l['T']}, {'cast' if l['cast'] else 'no cast'}>"
    if k == "tri_dw_kernel":
        return f"tri_dw_kernel<{l['T']}>"
    return k


IMAGES = ["tri_kernel<%s, %d, %d>" % (dt, Y // KW[dt], rt) for dt in ("bf16", "f32") for Y in (32, 64, 128) for rt in RT_CAND[dt]] + \
    ["tri2_kernel[slab]", "tri2_kernel[atomic]", "tri2_kernel[direct]", "tri2_reduce_kernel", "tri_split_rows_kernel", "tri3_kernel", "tri_absmax3_kernel",
     "tri_dw3_kernel", "tri_permute_kernel<bf16>[mode 0]", "tri_permute_kernel<bf16>[mode 1]", "tri_permute_kernel<f32>[mode 0]",
     "tri_permute_kernel<f32>[mode 1]", "tri_permute2_kernel<bf16>", "tri_permute2_kernel<f32>", "tri_transpose_kernel<bf16, cast>",
     "tri_transpose_kernel<bf16, no cast>", "tri_transpose_kernel<f32, cast>", "tri_transpose_kernel<f32, no cast>", "tri_cast_bf16_kernel",
     "tri_dw_kernel<bf16>", "tri_dw_kernel<f32>", "tri_dw2_kernel", "tri_dw2_reduce_kernel"]


def desc(l, rb=True):
    """the route descriptor of a main launch, as the case ids spell it"""
    k = l["k"]
    if k == "tri_kernel":
        s = "tk.%s.k%d.r%d.xs%d" % (l["image"] + (l["xs"],))
    elif k == "tri2_kernel":
        s = f"t2{l['form']}.xs{l['xs']}"
    elif k == "tri3_kernel":
        s = f"t3.xs{l['xs']}"
    elif k in ("tri_dw2_kernel", "tri_dw3_kernel"):
        return f"{k[4:7]}.S{l['S']}.e{l['empty']}"
    elif k == "tri_dw_kernel":
        return f"dw.{l['T']}.Mp{l['Mp']}"
    else:
        return None
    return s + (f".rb{l['n_rb']}" if rb else "")


# ---------------------------------------------------------------------------------------------------------------- the case table
# op fwd: entry nows | ws | wsnull, want "";  op bwd: entry g32 | g16 (the cotangent's type), want over c w p.
# M: an int, or "lo" / "hi": the ends of rt_run(dt, RT of the claim, xs of the claim, CUs).
Case = collections.namedtuple("Case", "group op dt M X H Y entry want claim side")
CASES, ROUNDING = [], []


def _rt_of(claim):
    m = re.match(r"tk\.(bf16|f32)\.k\d+\.r(\d+)\.xs(\d+)", claim)
    return int(m.group(2)), int(m.group(3))


def resolve_m(c, cus=DEFAULT_CUS):
    if isinstance(c.M, int):
        return c.M
    rt, xs = _rt_of(c.claim)
    return rt_run(c.dt, rt, xs, cus)[0 if c.M == "lo" else 1]


def case_id(c):
    return f"{c.group}-{c.entry}-{c.dt}-M{c.M}-X{c.X}-H{c.H}-Y{c.Y}" + (f"-{c.want}" if c.want else "") + f"-{c.claim}-{c.side}"


def fwd(group, dt, M, X, H, Y, entry, claim, side, table=None):
    (CASES if table is None else table).append(Case(group, "fwd", dt, M, X, H, Y, entry, "", claim, side))


def bwd(group, dt, M, X, H, Y, want, claim, side, entry="g32", table=None):
    (CASES if table is None else table).append(Case(group, "bwd", dt, M, X, H, Y, entry, want, claim, side))


def derive(c, cus=DEFAULT_CUS):
    """what a case's claim is compared with: the descriptors of the main launches, or err<code>"""
    M = resolve_m(c, cus)
    if c.op == "fwd":
        L = forward(c.dt, M, c.X, c.H, c.Y, c.entry, cus)
        return f"err{L:x}" if isinstance(L, int) else "+".join(d for d in (desc(l, isinstance(c.M, int)) for l in L) if d)
    L = backward(c.dt, M, c.X, c.H, c.Y, c.want, c.entry == "g16", cus)
    if isinstance(L, tuple):
        return f"err{L[0]:x}"
    out = []
    for role in ("dc", "dw", "dp"):
        d = [desc(l) for r, l in L if r == role and desc(l)]
        if d:
            out.append(f"{role}={d[0]}")
    perm = [image_of(l) for _, l in L if l["k"].startswith("tri_permute")]
    return ",".join(out) + ("," + "+".join("p2" if "permute2" in p else "pm" + p[-2] for p in perm) if perm else "")


def launches(c, cus=DEFAULT_CUS):
    M = resolve_m(c, cus)
    if c.op == "fwd":
        L = forward(c.dt, M, c.X, c.H, c.Y, c.entry, cus)
        return [] if isinstance(L, int) else L
    L = backward(c.dt, M, c.X, c.H, c.Y, c.want, c.entry == "g16", cus)
    return [] if isinstance(L, tuple) else [l for _, l in L]


BASE_RT = {"bf16": 4, "f32": 3}
ALT_RT = {"bf16": 6, "f32": 4}
KCH = lambda dt, Y: Y // KW[dt]

# ---- tri_kernel, forward through vlg_trilinear (H = 32 unless the row is about H: not H = Y = 128, so bf16 never leaves for tri2_kernel)
for dt in ("bf16", "f32"):
    rt, rows = BASE_RT[dt], 16 * BASE_RT[dt]
    for Y in (32, 64, 128):
        for X in (1, 16, 31, 32, 33, 256):      # the xs switch at X = 32; X = 256: the largest cT
            xs = 2 if X >= 32 else 1
            fwd("tk", dt, 100, X, 32, Y, "nows", f"tk.{dt}.k{KCH(dt, Y)}.r{rt}.xs{xs}.rb{cdiv(100, rows)}", f"xs{'2' if X >= 32 else '1'}side")
        for xs, X in ((1, 16), (2, 32)):        # the other RT: both ends of the run of M that selects it
            for end in ("lo", "hi"):
                fwd("tk", dt, end, X, 32, Y, "nows", f"tk.{dt}.k{KCH(dt, Y)}.r{ALT_RT[dt]}.xs{xs}", f"rt{ALT_RT[dt]}{end}")
        fwd("tk", dt, "lo", 256, 32, Y, "nows", f"tk.{dt}.k{KCH(dt, Y)}.r{ALT_RT[dt]}.xs2", f"rt{ALT_RT[dt]}lo-maxcT")
        for X in (1, 31, 33):                   # x ranges of odd length: the last pass of the weight ring is partial at either ring depth
            fwd("tk", dt, "lo", X, 32, Y, "nows", f"tk.{dt}.k{KCH(dt, Y)}.r{ALT_RT[dt]}.xs{2 if X >= 32 else 1}", f"rt{ALT_RT[dt]}lo-oddrange")
    for xs, X in ((1, 16), (2, 32)):
        for M, side in ((1, "onerow"), (rows, "1block"), (rows + 1, "1block+1row"), (4 * rows, "4blocks-nopad"), (4 * rows + 1, "5blocks-padded")):
            fwd("tk", dt, M, X, 32, 64, "nows", f"tk.{dt}.k{KCH(dt, 64)}.r{rt}.xs{xs}.rb{cdiv(M, rows)}", side)
    for H in (16, 48, 80, 96, 112, 128):        # waves whose h-tile is at or past n_ht load clamped rows and store nothing
        fwd("tk", dt, 100, 32, H, 64, "nows", f"tk.{dt}.k{KCH(dt, 64)}.r{rt}.xs2.rb{cdiv(100, rows)}", f"nht{H // 16}")

# ---- tri2_kernel (bf16, H = Y = 128) with a workspace; xs: 8 where X / 8 >= 8, down to 1 (no workspace asked for: the atomic form) below X = 16
T2_SMALL = {2: "t2a.xs2", 15: "t2a.xs2", 16: "t2s.xs2", 17: "t2s.xs2", 64: "t2s.xs8", 65: "t2s.xs8", 128: "t2s.xs8", 193: "t2s.xs8", 256: "t2s.xs8"}
for M in (1024, 1025, 1280, 1281):
    for X, route in T2_SMALL.items():
        fwd("t2", "bf16", M, X, 128, 128, "ws", f"{route}.rb{cdiv(M, 256)}", ("raggedrows" if M % 256 else "wholerows") + ("-raggedx" if X % int(route[-1]) else ""))
fwd("t2", "bf16", 10496, 128, 128, 128, "ws", "t2s.xs6.rb41", "configsize")
fwd("t2", "bf16", 18945, 256, 128, 128, "ws", "t2s.xs3.rb75", "xper86")
fwd("t2", "bf16", 26113, 193, 128, 128, "ws", "t2s.xs3.rb103", "afterfix-xper97to65")
fwd("t2", "bf16", 43521, 128, 128, 128, "ws", "t2s.xs2.rb171", "afterfix-xper128to64")
fwd("t2", "bf16", 1023, 128, 128, 128, "ws", "tk.bf16.k4.r4.xs2.rb16", "below1024")
for entry in ("nows", "wsnull"):
    for X, side in ((17, "raggedx"), (128, "even"), (192, "lds163840")):
        fwd("t2", "bf16", 1025, X, 128, 128, entry, "t2a.xs2.rb5", side)
    for X in (193, 256):
        fwd("t2", "bf16", 1025, X, 128, 128, entry, "tk.bf16.k4.r4.xs2.rb17", "afterfix-xper>96")

# ---- tri3_kernel (float32, H = Y = 128) with a workspace; without one the same shapes are tri_kernel<f32>
T3_SMALL = {2: 1, 17: 2, 80: 8, 81: 8, 128: 8, 161: 8, 256: 8}
for M in (1024, 1025):
    for X, xs in T3_SMALL.items():
        fwd("t3", "f32", M, X, 128, 128, "ws", f"t3.xs{xs}.rb{cdiv(M, 256)}", "raggedrows" if M % 256 else "wholerows")
fwd("t3", "f32", 18945, 256, 128, 128, "ws", "t3.xs4.rb75", "splits3to4")
fwd("t3", "f32", 43521, 128, 128, 128, "ws", "t3.xs2.rb171", "xper64")
for X in T3_SMALL:
    fwd("t3", "f32", 1025, X, 128, 128, "nows", f"tk.f32.k8.r3.xs{2 if X >= 32 else 1}.rb22", "noworkspace")
fwd("t3", "f32", 18945, 256, 128, 128, "nows", "tk.f32.k8.r4.xs2.rb297", "noworkspace")
fwd("t3", "f32", 43521, 128, 128, 128, "nows", "tk.f32.k8.r4.xs2.rb681", "noworkspace")

# ---- the backward, all three outputs
for M, xs in ((1024, 8), (1025, 8), (2047, 8), (2048, 8), (2049, 8), (10496, 6)):
    rb = cdiv(M, 256)
    bwd("bw", "bf16", M, 128, 128, 128, "cwp", f"dc=t2s.xs{xs}.rb{rb},dw=dw2.S4.e0,dp=t2s.xs{xs}.rb{rb},p2", "raggedrows" if M % 256 else "wholerows")
bwd("bw", "bf16", 43521, 128, 128, 128, "cwp", "dc=t2s.xs2.rb171,dw=dw2.S4.e0,dp=t2s.xs2.rb171,p2", "afterfix-xper128to64")
bwd("bw", "bf16", 2049, 64, 128, 128, "cwp", "dc=tk.bf16.k4.r4.xs2.rb33,dw=dw2.S8.e1,dp=t2s.xs8.rb9,p2", "emptychunk7")
for M, X in ((2049, 2), (1025, 256)):      # d_child needs X % 16 == 0, X <= 128: an error for all three, the other two alone are right
    bwd("bw", "bf16", M, X, 128, 128, "cwp", "err1001", "dchild-refused")
bwd("bw", "bf16", 2049, 2, 128, 128, "w", "dw=dw2.S8.e1", "emptychunk7")
bwd("bw", "bf16", 2049, 2, 128, 128, "p", "dp=t2d.xs1.rb9,pm1", "onerange")
bwd("bw", "bf16", 2049, 2, 128, 128, "wp", "dw=dw2.S8.e1,dp=t2d.xs1.rb9,pm1", "onerange")
bwd("bw", "bf16", 1025, 256, 128, 128, "w", "dw=dw2.S2.e0", "S2")      # (128 pairs of x: S = 2 at any M)
bwd("bw", "bf16", 1025, 256, 128, 128, "p", "dp=t2s.xs8.rb5,pm1", "xper32")
bwd("bw", "bf16", 1025, 256, 128, 128, "wp", "dw=dw2.S2.e0,dp=t2s.xs8.rb5,pm1", "S2")
for M in (1024, 1025, 2049):
    rb = cdiv(M, 256)
    bwd("bw", "f32", M, 128, 128, 128, "cwp", f"dc=t3.xs8.rb{rb},dw=dw3.S4.e0,dp=t3.xs8.rb{rb},p2", "fp16parts")
bwd("bw", "f32", 1023, 128, 128, 128, "cwp", "dc=tk.f32.k8.r3.xs2.rb22,dw=dw.f32.Mp1024,dp=tk.f32.k8.r3.xs2.rb22,p2", "below1024")
for dt in ("bf16", "f32"):
    for X, H, Y in ((16, 32, 32), (48, 64, 128), (128, 128, 64), (32, 32, 128)):
        for M in (1, 31, 32, 33, 1000):
            Mp, rb = cdiv(M, KW[dt]) * KW[dt], cdiv(M, 16 * BASE_RT[dt])
            tk = lambda x_, y_: f"tk.{dt}.k{KCH(dt, y_)}.r{BASE_RT[dt]}.xs{2 if x_ >= 32 else 1}.rb{rb}"
            bwd("dw", dt, M, X, H, Y, "cwp", f"dc={tk(Y, H)},dw=dw.{dt}.Mp{Mp},dp={tk(X, H)},p2", f"pad{Mp - M}")

# ---- the backward with a subset of the outputs: tri2 / dw2, generic bf16, generic float32, fp16 parts
SUBSETS = ["".join(s) for n in (1, 2, 3) for s in itertools.combinations("cwp", n)]
SUB_ROUTES = {("bf16", 1025, 128): dict(c="dc=t2s.xs8.rb5", w="dw=dw2.S4.e0", p="dp=t2s.xs8.rb5"),
              ("bf16", 100, 48): dict(c="dc=tk.bf16.k2.r4.xs2.rb2", w="dw=dw.bf16.Mp128", p="dp=tk.bf16.k2.r4.xs2.rb2"),
              ("f32", 100, 48): dict(c="dc=tk.f32.k4.r3.xs2.rb3", w="dw=dw.f32.Mp112", p="dp=tk.f32.k4.r3.xs2.rb3"),
              ("f32", 1025, 128): dict(c="dc=t3.xs8.rb5", w="dw=dw3.S4.e0", p="dp=t3.xs8.rb5")}
for (dt, M, X), routes in SUB_ROUTES.items():
    H, Y = (128, 128) if X == 128 else (64, 128)
    for want in SUBSETS:
        fp16 = (dt, X) == ("f32", 128)
        perm = ("p2" if "c" in want and "p" in want else "+".join(f"pm{'cp'.index(o)}" for o in want if o in "cp")) if not fp16 else ("p2" if want != "w" else "")
        bwd("sub", dt, M, X, H, Y, want, ",".join(routes[o] for o in want) + ("," + perm if perm else ""), "subset")
for X, dp in ((1, "dp=tk.bf16.k4.r4.xs1.rb17"), (5, "dp=t2d.xs1.rb5")):      # odd X: d_w leaves tri_dw2_kernel for tri_dw_kernel
    bwd("sub", "bf16", 1025, X, 128, 128, "w", "dw=dw.bf16.Mp1056", "oddX")
    bwd("sub", "bf16", 1025, X, 128, 128, "wp", f"dw=dw.bf16.Mp1056,{dp},pm1", "oddX")

# ---- the bf16 cotangent entry: g used in place, transposed without the cast
bwd("g16", "bf16", 1025, 128, 128, 128, "cwp", "dc=t2s.xs8.rb5,dw=dw2.S4.e0,dp=t2s.xs8.rb5,p2", "ginplace", entry="g16")
bwd("g16", "bf16", 100, 48, 64, 128, "cwp", "dc=tk.bf16.k2.r4.xs2.rb2,dw=dw.bf16.Mp128,dp=tk.bf16.k2.r4.xs2.rb2,p2", "nocast", entry="g16")

# ---- the rounding set: one case per kernel image (the fp16-parts images on magnitude-spread inputs)
for dt in ("bf16", "f32"):
    for Y in (32, 64, 128):
        fwd("rnd", dt, 100, 33, 48, Y, "nows", f"tk.{dt}.k{KCH(dt, Y)}.r{BASE_RT[dt]}.xs2.rb{cdiv(100, 16 * BASE_RT[dt])}", "normal", table=ROUNDING)
        fwd("rnd", dt, "lo", 33, 48, Y, "nows", f"tk.{dt}.k{KCH(dt, Y)}.r{ALT_RT[dt]}.xs2", "normal", table=ROUNDING)
fwd("rnd", "bf16", 1025, 65, 128, 128, "ws", "t2s.xs8.rb5", "normal", table=ROUNDING)
fwd("rnd", "bf16", 1025, 65, 128, 128, "nows", "t2a.xs2.rb5", "normal", table=ROUNDING)
fwd("rnd", "f32", 1025, 81, 128, 128, "ws", "t3.xs8.rb5", "spread", table=ROUNDING)
bwd("rnd", "bf16", 1025, 16, 128, 128, "cwp", "dc=tk.bf16.k4.r4.xs2.rb17,dw=dw2.S4.e0,dp=t2s.xs2.rb5,p2", "normal", table=ROUNDING)      # (X = 16: tri_dw2_kernel at an eighth of the oracle's cost)
bwd("rnd", "bf16", 100, 48, 64, 128, "cwp", "dc=tk.bf16.k2.r4.xs2.rb2,dw=dw.bf16.Mp128,dp=tk.bf16.k2.r4.xs2.rb2,p2", "normal", table=ROUNDING)
bwd("rnd", "f32", 100, 48, 64, 128, "cwp", "dc=tk.f32.k4.r3.xs2.rb3,dw=dw.f32.Mp112,dp=tk.f32.k4.r3.xs2.rb3,p2", "normal", table=ROUNDING)
bwd("rnd", "f32", 1025, 128, 128, 128, "cwp", "dc=t3.xs8.rb5,dw=dw3.S4.e0,dp=t3.xs8.rb5,p2", "spread", table=ROUNDING)

ORACLE_MAX_M = 4096      # the C oracle is the reference up to here; above it float64 torch on the device, in row chunks


# ---------------------------------------------------------------------------------------------------------------- inputs
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def input_key(c, cus=DEFAULT_CUS):
    return (resolve_m(c, cus), c.X, c.H, c.Y)


@functools.lru_cache(maxsize=4)
def exact_inputs(key):
    """child [M,X], parent [M,Y], w [X,H,Y], g [M,H] as float64 holding integers in [-4, 4] / 4 (exact in bf16 and fp16)"""
    M, X, H, Y = key
    rng = _rng("exact", *key)
    return tuple(rng.integers(-4, 5, s) / 4.0 for s in ((M, X), (M, Y), (X, H, Y), (M, H)))


def exact_bound_holds(M, X, H, Y):
    """every sum of either pass, in units of 1 / 64, stays below 2^24: float32 accumulation in any order is exact"""
    return X * Y <= 32768 and H * Y <= 32768 and X * H <= 32768 and M < 262144 and 64 * max(X * Y, H * Y, X * H, M) <= 1 << 24


def rounding_inputs(c, cus=DEFAULT_CUS):
    """normal(0, 0.5) features, w / sqrt(X Y), rounded to the operand type (the cotangent too: it is bf16 in the product); `spread`: the
    magnitude-spread inputs of test_arc_trilinear_float32_on_fp16_parts (rows over 2^24, weight rows over 2^12, cotangent rows over 2^20)"""
    import torch
    M, X, H, Y = key = input_key(c, cus)
    rng = _rng("rounding", c.side, *key)
    child, parent, w, g = rng.normal(0, 0.5, (M, X)), rng.normal(0, 0.5, (M, Y)), rng.normal(0, 1, (X, H, Y)) / np.sqrt(X * Y), rng.normal(0, 1, (M, H))
    if c.side == "spread":
        rows = np.exp2(rng.integers(-12, 13, (M, 1)).astype(np.float64))
        child, parent = child * rows, parent * rows[::-1]
        w = w * np.exp2(rng.integers(-6, 7, (X, H, 1)).astype(np.float64))
        g = g * 1e-4 * np.exp2(rng.integers(-10, 11, (M, 1)).astype(np.float64))
    if c.dt == "bf16":
        return tuple(torch.from_numpy(a).float().bfloat16().double().numpy() for a in (child, parent, w, g))
    return tuple(a.astype(np.float32).astype(np.float64) for a in (child, parent, w, g))


def oracle_reference(oracle, inputs, want, dtype):
    """{out | d_child, d_w, d_parent: array} from the C oracle"""
    child, parent, w, g = inputs
    if want == "":
        return dict(out=oracle.arc_encoder(child, parent, w, None, None, dtype))
    d_child, d_parent, d_w, _, _ = oracle.arc_encoder_backward(child, parent, w, None, g, dtype)
    return dict(d_child=d_child, d_w=d_w, d_parent=d_parent)


# ---------------------------------------------------------------------------------------------------------------- tests
SWEEP_M = (1, 1023, 1024, 1025, 2047, 2048, 2049, 10496, 18945, 26112, 26113, 43520, 43521, 100000)
SWEEP_X = (1, 2, 15, 16, 17, 64, 65, 128, 192, 193, 256)
SWEEP_HY = ((128, 128), (64, 128), (128, 64), (32, 32), (48, 64))


@pytest.fixture(scope="module")
def lib():
    from vlgae_amd.build import build_library
    build_library()            # hipcc cross-compiles for gfx950 without a GPU
    from vlgae_amd import _C
    return _C.lib()


def _src():
    return open(os.path.join(ROOT, "vlgae_amd", "csrc", "vlg_arc.hip")).read()


def source_bounds_tri2():
    """whether the source bounds tri2_kernel's x range at all: without that rule the pin below holds for guard=False and the LDS test fails"""
    return "kTri2MaxXPer" in _src()


def test_constants_read_from_the_source():
    s = _src()
    one = lambda pat: (lambda f: f[0] if len(f) == 1 else pytest.fail(f"{pat}: {f}"))(re.findall(pat, s))
    assert tuple(map(int, one(r"constexpr int kTri2Threads = (\d+), kTri2Rows = (\d+);"))) == (512, K_TRI2_ROWS)
    assert tuple(map(int, one(r"constexpr int kTri3Threads = (\d+), kTri3Rows = (\d+);"))) == (512, K_TRI3_ROWS)
    assert int(one(r"constexpr int kTri2MaxXPer = (\d+);")) == TRI2_MAX_XPER == 96 and TRI2_LDS_W + 4 * K_TRI2_ROWS * TRI2_MAX_XPER == LDS_LIMIT
    assert int(one(r"while \(\(X \+ xs - 1\) / xs > (\d+)\) \+\+xs;")) == TRI3_MAX_XPER
    assert tuple(map(int, one(r"kDw2Threads = \d+, kDw2Stage = (\d+), kDw2XB = (\d+);"))) == (K_DW2_STAGE, K_DW2_XB)
    assert tuple(map(int, one(r"kDw3Threads = \d+, kDw3Stage = (\d+), kDw3XB = (\d+), kDw3MaxBlocks = (\d+);"))) == (K_DW3_STAGE, K_DW3_XB, K_DW3_MAX_BLOCKS)
    assert one(r"const int cand\[3\] = \{F32IN \? (\d) : (\d), F32IN \? (\d) : (\d), F32IN \? \d : \d\};") == ("3", "4", "4", "6")
    assert one(r"const float stream = F32IN \? ([\d.]+)f : ([\d.]+)f;") == ("1.5", "34.")
    assert one(r"const int xs = X >= (\d+) \? 2 : 1;") == "32"


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_workspace_queries_reproduce_the_restated_plan(lib, dt):
    """Both workspace entry points over the sweep and over every case: the restated carving gives the library's byte counts."""
    code = F32 if dt == "f32" else BF16
    shapes = {(M, X, H, Y) for M in SWEEP_M for X in SWEEP_X for H, Y in SWEEP_HY} | {input_key(c) for c in CASES + ROUNDING if c.dt == dt}
    wrong = []
    for M, X, H, Y in sorted(shapes):
        got = (lib.vlg_trilinear_workspace(M, X, H, Y, code), lib.vlg_trilinear_backward_workspace(M, X, H, Y, code))
        want = (workspace_fwd(dt, M, X, H, Y, source_bounds_tri2()), workspace_bwd(dt, M, X, H, Y, source_bounds_tri2()))
        if got != want:
            wrong.append(((M, X, H, Y), got, want))
    assert not wrong, wrong[:10]
    assert lib.vlg_trilinear_workspace(0, 128, 128, 128, code) == 0 and lib.vlg_trilinear_backward_workspace(0, 128, 128, 128, code) == 0


def lds_violations(guard=True, cus=DEFAULT_CUS):
    """(call, dtype, M, X, H, Y, kernel, bytes) of every launch of the restated plan over the sweep that asks for more LDS than a workgroup has"""
    bad = []
    for dt, M, X, (H, Y) in itertools.product(("bf16", "f32"), SWEEP_M, SWEEP_X, SWEEP_HY):
        if check_dims(M, X, H, Y):
            continue
        calls = [(e, forward(dt, M, X, H, Y, e, cus, guard)) for e in ("ws", "nows")]
        for want in ("c", "w", "p"):
            L = backward(dt, M, X, H, Y, want, False, cus, guard)
            calls.append(("bwd " + want, [] if isinstance(L, tuple) else [l for _, l in L]))
        for call, L in calls:
            for l in (L if isinstance(L, list) else []):
                if l.get("lds", 0) > LDS_LIMIT:
                    bad.append((call, dt, M, X, H, Y, image_of(l), l["lds"]))
    return bad


def test_every_launch_fits_the_lds():
    """No launch of the restated plan, with or without a workspace, forward or backward, asks for more than the 163840 bytes of LDS a workgroup
    can have.  Without the bound on the x range of tri2_kernel (guard=False restates the plan before it) the same sweep names: bf16 with a
    workspace at M >= 43521, X = 128 in the backward (one range of 128: 196608 bytes) and at M in 26113 .. 43520, X = 193 (two ranges of 97:
    164864), and without a workspace at any M >= 1024 with X = 193 .. 256 (164864 .. 196608)."""
    bad = lds_violations(guard=source_bounds_tri2())
    assert not bad, "launches asking for more than %d bytes of LDS:\n  " % LDS_LIMIT + "\n  ".join(map(str, bad))
    before = lds_violations(guard=False)
    rows = {(b[0], b[2], b[3], b[7]) for b in before}
    assert {b[6] for b in before} == {"tri2_kernel[direct]", "tri2_kernel[slab]", "tri2_kernel[atomic]"}
    assert not any(b[1] == "f32" or b[2] < 1024 or b[3] <= TRI2_MAX_XPER or b[4:6] != (128, 128) for b in before)
    assert {("ws", 26113, 193, 164864), ("ws", 43520, 193, 164864)} <= rows and not any(b[2] == 26112 and b[0] != "nows" for b in before)
    assert all({("nows", M, 193, 164864), ("nows", M, 256, 196608)} <= rows for M in SWEEP_M if M >= 1024)
    assert {(call, M, 128, 196608) for call in ("bwd c", "bwd p") for M in (43521, 100000)} <= rows and not any(b[2] == 43520 and b[3] == 128 for b in before)
    # the plan of every shape that fitted before is unchanged
    for M, X in itertools.product(range(1024, 60000, 251), range(2, 257)):
        if TRI2_LDS_W + 4 * K_TRI2_ROWS * cdiv(X, tri2_splits(M, X, False)) <= LDS_LIMIT:
            assert tri2_splits(M, X) == tri2_splits(M, X, False)
        assert tri3_splits(M, X) == tri3_splits(M, X, False)


def test_cases_are_on_the_route_their_id_names():
    moved = [f"{case_id(c)}: restated {derive(c)}" for c in CASES + ROUNDING if derive(c) != c.claim]
    assert not moved, "cases that left the route they were written for:\n  " + "\n  ".join(moved)
    ids = [case_id(c) for c in CASES + ROUNDING]
    assert len(set(ids)) == len(ids)
    for c in CASES + ROUNDING:
        M, X, H, Y = input_key(c)
        assert exact_bound_holds(M, X, H, Y) and M <= 43521, case_id(c)
        for l in launches(c):
            assert l.get("lds", 0) <= LDS_LIMIT, case_id(c)
    # rows that target an RT: the ends of the run, at 256 CUs, and the run moves with the CU count
    assert rt_run("bf16", 6, 2, 256) == (8193, 12288) and rt_run("bf16", 6, 1, 256) == (16385, 24576)
    assert rt_run("f32", 4, 2, 256) == (6145, 8192) and rt_run("f32", 4, 1, 256) == (12289, 16384) and pick_rt("f32", 12289, 2, 256) == 4
    assert rt_run("bf16", 6, 2, 304) != rt_run("bf16", 6, 2, 256)
    for cus in (64, 228, 256, 304):
        for c in CASES + ROUNDING:
            if not isinstance(c.M, int):
                assert derive(c, cus) == c.claim, (case_id(c), cus)


def _with(pred):
    return [c for c in CASES if pred(c)]


def test_every_image_and_boundary_has_a_case():
    ran = collections.defaultdict(list)
    for c in CASES:
        for l in launches(c):
            ran[image_of(l)].append(case_id(c))
    assert set(ran) == set(IMAGES), (sorted(set(IMAGES) - set(ran)), sorted(set(ran) - set(IMAGES)))
    rnd = {image_of(l) for c in ROUNDING for l in launches(c)}
    assert rnd >= {i for i in IMAGES if i.startswith("tri_kernel<")} | {"tri2_kernel[slab]", "tri2_kernel[atomic]", "tri3_kernel", "tri_dw3_kernel", "tri_dw2_kernel",
                                                                         "tri_dw_kernel<bf16>", "tri_dw_kernel<f32>"}
    first = lambda c: launches(c)[0]
    for dt in ("bf16", "f32"):
        rows = 16 * BASE_RT[dt]
        tk = _with(lambda c: c.group == "tk" and c.dt == dt)
        for Y in (32, 64, 128):
            for rt in RT_CAND[dt]:
                assert {c.X for c in tk if first(c)["image"] == (dt, Y // KW[dt], rt)} >= {1, 16, 31, 32, 33, 256}
        assert {c.M for c in tk if isinstance(c.M, int)} >= {1, rows, rows + 1, 4 * rows, 4 * rows + 1}
        assert any(first(c)["exited"] == 6 and first(c)["n_rb"] == 5 for c in tk) and any(first(c)["exited"] == 0 and first(c)["n_rb"] == 4 and first(c)["xs"] == 2 for c in tk)
        assert {c.H for c in tk if c.X == 32 and c.M == 100} >= {16, 48, 80, 96, 112, 128}
        dw = _with(lambda c: c.group == "dw" and c.dt == dt)
        assert {(c.X, c.H, c.Y) for c in dw} == {(16, 32, 32), (48, 64, 128), (128, 128, 64), (32, 32, 128)} and {c.M for c in dw} == {1, 31, 32, 33, 1000}
    t2 = _with(lambda c: c.group == "t2")
    assert {(c.M, c.X) for c in t2 if c.entry == "ws"} >= set(itertools.product((1024, 1025, 1280, 1281), (2, 15, 16, 17, 64, 65, 128, 193, 256))) | \
        {(10496, 128), (18945, 256), (26113, 193), (43521, 128), (1023, 128)}
    for entry in ("nows", "wsnull"):
        assert {c.X for c in t2 if c.entry == entry and c.M == 1025} == {17, 128, 192, 193, 256}
    assert any(first(c)["lds"] == LDS_LIMIT for c in t2)
    t3 = _with(lambda c: c.group == "t3")
    assert {(c.M, c.X) for c in t3 if c.entry == "ws"} == set(itertools.product((1024, 1025), (2, 17, 80, 81, 128, 161, 256))) | {(18945, 256), (43521, 128)}
    assert {(c.M, c.X) for c in t3 if c.entry == "nows"} >= {(18945, 256), (43521, 128)}
    bw = _with(lambda c: c.group == "bw")
    assert {c.M for c in bw if c.dt == "bf16" and c.X == 128 and c.want == "cwp"} >= {1024, 1025, 2047, 2048, 2049, 10496}
    assert {(c.X, c.want) for c in bw if c.dt == "bf16" and c.X != 128} == {(64, "cwp")} | set(itertools.product((2, 256), ("cwp", "w", "p", "wp")))
    assert {l["S"] for c in bw for l in launches(c) if l["k"] == "tri_dw2_kernel"} == {2, 4, 8} and any(l.get("empty") == 1 for c in bw for l in launches(c))
    assert {c.M for c in bw if c.dt == "f32"} == {1023, 1024, 1025, 2049}
    sub = _with(lambda c: c.group == "sub")
    for key in SUB_ROUTES:
        assert {c.want for c in sub if (c.dt, c.M, c.X) == key} == set(SUBSETS) and len(SUBSETS) == 7
    assert {(c.X, c.want) for c in sub if c.X in (1, 5)} == set(itertools.product((1, 5), ("w", "wp")))
    assert {c.X for c in _with(lambda c: c.entry == "g16")} == {128, 48}


def test_exact_inputs_are_exact(oracle_mod):
    """The bound from the shapes for every case; and on the cases the C oracle handles cheaply, its float32 results (sequential sums) equal
    its float64 results: the sums are exact in any order."""
    for c in CASES:
        assert exact_bound_holds(*input_key(c)), case_id(c)
    child, parent, w, g = exact_inputs((33, 48, 64, 128))
    for a in (child, parent, w, g):
        assert np.array_equal(a * 4, np.round(a * 4)) and np.abs(a).max() == 1.0
    prod = np.unique(np.outer(np.arange(-4, 5), np.arange(-4, 5)))
    assert all(len(bin(abs(int(v))).rstrip("0")) - 2 <= 5 for v in prod if v)      # at most 5 significant bits
    done = set()
    for c in CASES:
        M, X, H, Y = key = input_key(c)
        if M * X * H * Y > 3e7 or key in done:
            continue
        done.add(key)
        r32, r64 = (dict(oracle_reference(oracle_mod, exact_inputs(key), "", t), **oracle_reference(oracle_mod, exact_inputs(key), "cwp", t))
                    for t in (np.float32, np.float64))
        for name in r64:
            assert np.array_equal(r32[name], r64[name].astype(np.float32)), (key, name)
            assert np.array_equal(r64[name] * 64, np.round(r64[name] * 64)) and np.abs(r64[name]).max() * 64 < 1 << 24
    assert len(done) >= 20


def test_host_error_returns(lib):
    """check_dims, the dtype checks, the backward's H / Y lists, a short workspace and a NULL operand are refused before any launch; M = 0 is
    a success that touches nothing."""
    import torch
    if torch.cuda.is_available():       # refused before any launch: where a GPU is present the pointer is a real buffer large enough anyway
        held = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda:0")
        one = ctypes.c_void_p(held.data_ptr())
    else:
        one = ctypes.c_void_p(64)
    tri, tws, bwd_, bwg = lib.vlg_trilinear, lib.vlg_trilinear_ws, lib.vlg_trilinear_backward, lib.vlg_trilinear_backward_g
    big = 1 << 20
    for code in (F32, BF16):
        dt = "f32" if code == F32 else "bf16"
        for X, H, msg in ((257, 32, b"X=257 > 256"), (32, 0, b"bad shape"), (32, 24, b"H=24 must be a multiple of 16"), (32, 144, b"H=144 must be a multiple of 16")):
            assert forward(dt, 10, X, H, 32, "nows") == ERR_SHAPE and backward(dt, 10, X, H, 32, "cwp")[0] == ERR_SHAPE
            assert tri(one, one, one, 10, X, H, 32, code, one, None) == ERR_SHAPE and msg in lib.vlg_last_error()
            assert tws(one, one, one, 10, X, H, 32, code, one, big, one, None) == ERR_SHAPE and msg in lib.vlg_last_error()
            assert bwd_(one, one, one, one, 10, X, H, 32, code, one, big, one, one, one, None) == ERR_SHAPE and msg in lib.vlg_last_error()
        assert backward(dt, 10, 32, 48, 32, "cwp") == (ERR_SHAPE, "trilinear_backward: H=48 (supported: 32, 64, 128)")
        assert bwd_(one, one, one, one, 10, 32, 48, 32, code, one, big, one, one, one, None) == ERR_SHAPE and b"H=48 (supported" in lib.vlg_last_error()
        assert backward(dt, 10, 32, 32, 96, "cwp") == (ERR_SHAPE, "trilinear_backward: Y=96 (supported: 32, 64, 128)")
        assert bwd_(one, one, one, one, 10, 32, 32, 96, code, one, big, one, one, one, None) == ERR_SHAPE and b"Y=96 (supported" in lib.vlg_last_error()
        assert forward(dt, 10, 32, 32, 96, "nows") == ERR_SHAPE
        assert tri(one, one, one, 10, 32, 32, 96, code, one, None) == ERR_SHAPE and b"contracted dimension 96" in lib.vlg_last_error()
        need = lib.vlg_trilinear_backward_workspace(100, 32, 64, 32, code)
        assert need == workspace_bwd(dt, 100, 32, 64, 32) > 0
        assert bwd_(one, one, one, one, 100, 32, 64, 32, code, one, need - 1, one, one, one, None) == ERR_WORKSPACE and b"workspace" in lib.vlg_last_error()
        assert bwd_(one, one, one, one, 100, 32, 64, 32, code, None, need, one, one, one, None) == ERR_WORKSPACE
        for k in range(4):      # a NULL operand
            ops = [None if i == k else one for i in range(4)]
            assert bwd_(*ops, 100, 32, 64, 32, code, one, need, one, one, one, None) == ERR_ARG and b"null buffer" in lib.vlg_last_error()
            if k < 3:
                assert tri(*ops[:3], 10, 32, 32, 32, code, one, None) == ERR_ARG and tws(*ops[:3], 10, 32, 32, 32, code, one, big, one, None) == ERR_ARG
        assert tri(one, one, one, 10, 32, 32, 32, code, None, None) == ERR_ARG and tws(one, one, one, 10, 32, 32, 32, code, one, big, None, None) == ERR_ARG
        # M = 0: nothing to do (d_w NULL here: with it the call zeroes d_w on the device); M < 0
        assert tri(None, None, None, 0, 32, 32, 32, code, None, None) == 0 and tws(None, None, None, 0, 32, 32, 32, code, None, 0, None, None) == 0
        assert bwd_(None, None, None, None, 0, 32, 32, 32, code, None, 0, None, None, None, None) == 0
        assert tri(one, one, one, -1, 32, 32, 32, code, one, None) == ERR_SHAPE and b"bad shape" in lib.vlg_last_error()
        assert bwd_(one, one, one, one, -1, 32, 32, 32, code, one, big, one, one, one, None) == ERR_SHAPE
    for bad in (2, -1, 7):
        assert tri(one, one, one, 10, 32, 32, 32, bad, one, None) == ERR_DTYPE and tws(one, one, one, 10, 32, 32, 32, bad, one, big, one, None) == ERR_DTYPE
        assert bwd_(one, one, one, one, 10, 32, 32, 32, bad, one, big, one, one, one, None) == ERR_DTYPE and b"in_dtype" in lib.vlg_last_error()
    # a bf16 cotangent needs bf16 features; a cotangent type that is neither
    assert backward("f32", 10, 32, 32, 32, "cwp", g16=True)[0] == ERR_DTYPE
    assert bwg(one, one, one, one, BF16, 10, 32, 32, 32, F32, one, big, one, one, one, None) == ERR_DTYPE and b"a bf16 cotangent needs bf16 features" in lib.vlg_last_error()
    assert bwg(one, one, one, one, 2, 10, 32, 32, 32, BF16, one, big, one, one, one, None) == ERR_DTYPE


if __name__ == "__main__":      # the coverage list: kernel image -> case ids
    ran = collections.defaultdict(list)
    for c in CASES + ROUNDING:
        for l in launches(c):
            ran[image_of(l)].append(case_id(c))
    for image in IMAGES:
        print(f"{image}: {len(ran[image])} cases, e.g. {ran[image][:2]}")
    print(len(CASES), "exact cases,", len(ROUNDING), "rounding cases")
