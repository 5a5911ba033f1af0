#!/usr/bin/env python3
"""Per-width timeline of the headline DMV1o launch (fused inside + outside, short image, B = 256, L = 40, bf16).

Builds the stamped library variant (tools/build_variant.sh NAME -DVLG_STAMP=2: per-width stamps only, see DevX::wstamp) unless
--lib names one, runs the headline launch a few times, and prints for every width of each pass, as the median over the first
16 sentences (workgroups) of the last launch, in s_memtime cycles:
  G, T          lanes per span and split points per lane (the schedule of vlg_dp_core.h: make_sched / group_log2 for the inside
                pass, the group table bw_group / bw_terms for the outside pass)
  live          wavefronts per direction that hold a span of that width (the others skip the body: kSkipDeadWaves)
  body_max      slowest wavefront: previous barrier's release -> its body's end
  body_min      fastest wavefront (a dead one when live < 4)
  skew          last body end - first body end
  bar           barrier: last body end -> release
  width         release -> release
and each wavefront's SIMD (HW_ID bits 5:4).  Usage:  python tools/time_dp_widths.py [--lib PATH] [--name stamp] [-D...]
Extra -D arguments go to the variant build (e.g. -DVLG_MIRROR_RIGHT=0 for the unmirrored placement)."""
import argparse
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW, KBLOCKS = 64, 16
KWORDS = 2 * KW * 2 * 8 + 8
M32 = 1 << 32   # the stamps are the low 32 bits of s_memtime


def group_log2(spans, w, cap):
    lg = 0
    while lg < 6 and (1 << lg) < w and spans * (2 << lg) <= cap:
        lg += 1
    return lg


BW_TABLE = (4, 8, 10, 12, 16, 32, 64)   # vlg_dp_core.h: bw_group -- the outside pass's lane groups in the short image


def bw_group(spans, w, waves=4):
    """vlg_dp_core.h: bw_piece_of -- the largest entry with spans <= waves (64 / G) and (G < 2 w or G the first entry)"""
    G = BW_TABLE[0]
    for g in BW_TABLE[1:]:
        if spans <= waves * (64 // g) and g < 2 * w:
            G = g
    return G


def bw_terms(G, Ne_max=41, waves=4):
    """vlg_dp_core.h: bw_terms -- the terms per lane the piece's single body runs at every width"""
    return max([-(-w // G) for ne in range(2, Ne_max + 1) for w in range(1, ne) if bw_group(ne - w, w, waves) == G] or [1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="an already-built stamped variant")
    ap.add_argument("--name", default="stamp")
    ap.add_argument("--launches", type=int, default=20)
    args, defs = ap.parse_known_args()
    lib_path = args.lib
    if lib_path is None:
        out = subprocess.run(["bash", os.path.join(ROOT, "tools", "build_variant.sh"), args.name, "-DVLG_STAMP=2", *defs],
                             check=True, capture_output=True, text=True, cwd=ROOT).stdout.split()
        lib_path = os.path.join(ROOT, out[-1])
    lib_path = os.path.abspath(lib_path)
    os.environ["VLGAE_AMD_LIB"] = lib_path
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from vlgae_amd import _C
    import vlgae_amd.torch_struct as ts
    from bench import synth

    B, L = 256, 40
    N = L + 1
    dev = torch.device("cuda:0")
    lib = _C.lib()
    dec, attach, root = synth(B, L, 1000, dev, torch.float32)
    md, ma = (t.to(torch.bfloat16).contiguous() for t in ts.DMV1o.merge(dec, attach, root))
    lengths = torch.full((B,), L, dtype=torch.long, device=dev)
    logZ = torch.empty(B, dtype=torch.float32, device=dev)
    gdec = torch.zeros((B, N, 2, 2, 2), dtype=torch.float32, device=dev)
    gatt = torch.zeros((B, N, N, 2), dtype=torch.float32, device=dev)
    ws_bytes = lib.vlg_workspace_bytes(_C.OP_DMV1O_INSIDE_OUTSIDE, B, N, 0)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = [_C.ptr(x) for x in (md, ma, lengths, logZ, gdec, gatt, ws)]
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(args.launches):
        ev0.record()
        _C.check(lib.vlg_dmv1o_inside_outside(p[0], p[1], p[2], B, N, _C.BF16, 0, None, p[3], p[4], p[5], p[6], ws_bytes, sp),
                 "dmv1o_inside_outside")
        ev1.record()
        torch.cuda.synchronize()
        times.append(ev0.elapsed_time(ev1) * 1e3)
    handle = ctypes.CDLL(lib_path)
    if not hasattr(handle, "vlg_dp_stamps"):   # an unstamped library: the launches alone (e.g. under a counter pass)
        print(f"# {os.path.basename(lib_path)}: launch {np.median(times):.1f} us (median of {len(times)}); no stamps in this build")
        return
    buf = (ctypes.c_uint * (KBLOCKS * KWORDS))()
    fn = handle.vlg_dp_stamps
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t]
    if fn(buf, KBLOCKS * KWORDS) != KWORDS:
        raise SystemExit("vlg_dp_stamps failed")
    a = np.frombuffer(buf, dtype=np.uint32).reshape(KBLOCKS, KWORDS).astype(np.int64)
    st = a[:, :-8].reshape(KBLOCKS, 2, KW, 2, 8)   # [block][pass][w][body end | release][wave]
    hw = a[:, -8:]
    simd = (hw >> 4) & 3
    print(f"# {os.path.basename(lib_path)}: B={B} L={L} bf16, launch {np.median(times):.1f} us (median of {len(times)}, stamped build)")
    print(f"# SIMD of waves 0-7, first 4 workgroups: {[list(map(int, s)) for s in simd[:4]]}")
    Ne = N
    for pas, name in ((0, "inside"), (1, "outside")):
        ws_ = list(range(1, Ne)) if pas == 0 else list(range(Ne - 1, 0, -1))
        print(f"## {name} pass (cycles; median over {KBLOCKS} workgroups)")
        print(f"{'w':>3} {'G':>3} {'T':>2} {'live':>4} {'body_max':>8} {'body_min':>8} {'skew':>6} {'bar':>6} {'width':>6}")
        tot = {"width": 0, "body_max": 0, "bar": 0, "skew": 0}
        for w in ws_:
            prev = w - 1 if pas == 0 else w + 1
            rel_prev = st[:, pas, prev, 1, :].max(axis=1)   # (prev = 0 / Ne: the pass-start stamp)
            end = st[:, pas, w, 0, :]
            rel = st[:, pas, w, 1, :].max(axis=1)
            body = (end - rel_prev[:, None]) % M32
            cap = 256
            if pas == 1:      # outside: groups from the table, 64 // G of them per wavefront, the piece's terms at every width
                G = bw_group(Ne - w, w)
                T = bw_terms(G)
                live = min(4, -(-(Ne - w) // (64 // G)))
            else:             # inside: make_sched, the widths 1 and 2 as one closed piece of one lane per span
                lg = 0 if w <= 2 else group_log2(Ne - w, w, cap)
                G = 1 << lg
                T = (w + G - 1) >> lg
                live = min(4, -(-((Ne - w) * G) // 64))
            row = {"body_max": np.median(body.max(axis=1)), "body_min": np.median(body.min(axis=1)),
                   "skew": np.median((end.max(axis=1) - end.min(axis=1)) % M32), "bar": np.median((rel - end.max(axis=1)) % M32),
                   "width": np.median((rel - rel_prev) % M32)}
            for k in tot:
                tot[k] += row[k]
            print(f"{w:>3} {G:>3} {T:>2} {live:>4} {row['body_max']:>8.0f} {row['body_min']:>8.0f} {row['skew']:>6.0f} "
                  f"{row['bar']:>6.0f} {row['width']:>6.0f}")
        print(f"sum  width {tot['width']:.0f}  body_max {tot['body_max']:.0f}  skew {tot['skew']:.0f}  barrier {tot['bar']:.0f}")
    # outside the passes (dmv_run's stamps, one row of 8 floats per wavefront in the last rows of grad_dec: slowest wavefront of a
    # workgroup, median over the same workgroups): the load stage, the section between the passes, the count write-out
    torch.cuda.synchronize()
    rows = gdec.view(B, N, 8)[:KBLOCKS, N - 8:, :].flip(1).cpu().numpy()   # [block][wave][word]
    stage, mid, out, passes = (float(np.median(rows[:, :, k].max(axis=1))) for k in (5, 6, 7, 4))
    print("## outside the passes (cycles; slowest wavefront, median over the workgroups)")
    print(f"load stage {stage:.0f}  between the passes {mid:.0f}  count write-out {out:.0f}  (inside start -> outside end {passes:.0f})")
    # the write-out's four sections (short image since round 13; the rows below the first eight; an older build leaves zeros there)
    split = gdec.view(B, N, 8)[:KBLOCKS, N - 16:N - 8, :4].flip(1).cpu().numpy()   # [block][wave][entry | attach | STOP | GO]
    if split.any():
        b_, a_, s_, g_ = (float(np.median(split[:, :, k].max(axis=1))) for k in range(4))
        print(f"write-out sections: entry {b_:.0f}  attach counts {a_:.0f}  STOP counts {s_:.0f}  GO row sums {g_:.0f}")
        print("# entry: from the outside pass's last barrier to the write-out's first stamp -- the wavefronts' skew behind that barrier, the")
        print("#   decode mode's clear + barrier (not in this launch: heads == null), and whatever the compiler moved above the stamp.  The")
        print("#   stamps order nothing: a section's reads may be issued in the section before it, so only the sum is exact.")
        print("# load stage: since round 13 stamped at KERNEL ENTRY -- it now includes the kernarg and lengths[b] loads, the range check, the")
        print("#   chart carve and this diagnostic build's own stamp-table clear + barrier, none of which an earlier build's figure")
        print("#   (stamped at dmv_run's entry, behind all of them) contains: the new figure is an upper bound of the like-for-like one.")


if __name__ == "__main__":
    main()
