#!/usr/bin/env python3
"""Instruction mix of the short fused DMV1o kernel, per barrier-to-barrier interval of its gfx950 ISA.

    python tools/dp_body_mix.py [--unit 001] [--kernel SUBSTRING] [--asm FILE] [--min-block 8]

Compiles one structured-DP translation unit (vlg_dp_inst.hip, --unit = family / semiring / input digits, default 001 = DMV1o
merged potentials / Log / bf16) for the device only, to assembly, with the flags vlgae_amd.build uses -- or reads an assembly
file already made that way (--asm) -- and walks the text of one kernel (default: dmv1o_kernel<Log, kModeShort, fused, BF16In>).
The text is cut at every s_barrier; for each interval, and for each basic block of at least --min-block instructions inside it,
the instructions are counted by class.  Opcodes are sorted by prefix only:

    int     vector integer / address arithmetic (every v_ opcode not named below)
    mov     v_mov_*, v_accvgpr_*
    sel     v_cndmask_*
    cmp     v_cmp_*, v_cmpx_*
    fp      vector floating point (v_ opcodes with _f16 / _f32 / _f64 / _bf16 in the name, DPP forms included)
    trans   v_exp_*, v_log_*, v_rcp_*, v_rsq_*, v_sqrt_*, v_sin_*, v_cos_*
    xlane   v_permlane*, v_readlane / v_readfirstlane / v_writelane
    lds     ds_*
    vmem    global_*, flat_*, buffer_*, scratch_*
    scalar  s_* other than the waits
    wait    s_waitcnt*, s_nop, s_barrier

A width loop of the DP has one barrier, so an interval holds the tail of one segment's loop, the prologue of the next segment and
that segment's width bodies (one per split-point count T, each a chain of basic blocks); `loop` marks a block that a later branch
jumps back to.  The inside pass's intervals come first in the text (their butterflies show in `dpp`, the count of DPP-form and
permlane instructions), the outside pass's after them, segments 6 ... 0."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("int", "mov", "sel", "cmp", "fp", "trans", "xlane", "lds", "vmem", "scalar", "wait")
TRANS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")
FLOAT = ("_f16", "_f32", "_f64", "_bf16")


def classify(op):
    if op.startswith(("s_waitcnt", "s_nop", "s_barrier")):
        return "wait"
    if op.startswith("s_"):
        return "scalar"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if op.startswith(("v_mov_", "v_accvgpr_")):
        return "mov"
    if op.startswith("v_cndmask_"):
        return "sel"
    if op.startswith("v_cmp"):
        return "cmp"
    if op.startswith(TRANS):
        return "trans"
    if op.startswith(("v_permlane", "v_readlane", "v_readfirstlane", "v_writelane")):
        return "xlane"
    if any(f in op for f in FLOAT):
        return "fp"
    return "int"


def compile_unit(unit):
    sys.path.insert(0, ROOT)
    from vlgae_amd import build as b
    f, s, i = unit
    flags = [*b.FLAGS, *b.DP_FLAGS, f"-DVLG_INST_FAMILY={f}", f"-DVLG_INST_SR={s}", f"-DVLG_INST_IN={i}"]
    with tempfile.TemporaryDirectory(prefix="dp_body_mix_") as td:
        out = os.path.join(td, "unit.s")
        cmd = [b._hipcc(), f"--offload-arch={b.ARCH}", *flags, "--offload-device-only", "-S", os.path.join(b.CSRC, "vlg_dp_inst.hip"), "-o", out]
        subprocess.run(cmd, check=True)
        return open(out).read().splitlines(), " ".join(cmd[1:-3])


def kernel_text(text, pattern):
    lines, on, name = [], False, None
    for ln in text:
        if not on:
            if re.match(r"^[A-Za-z_][\w$.]*:", ln) and pattern in ln.split(":")[0]:
                on, name = True, ln.split(":")[0]
            continue
        if ln.startswith(".Lfunc_end"):
            break
        lines.append(ln.rstrip("\n"))
    if not on:
        raise SystemExit(f"no kernel whose symbol contains {pattern!r} in the assembly")
    return name, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--unit", default="001")
    ap.add_argument("--kernel", default="dmv1o_kernelILi0ELi4ELb1E", help="substring of the mangled kernel symbol")
    ap.add_argument("--asm", default=None)
    ap.add_argument("--min-block", type=int, default=8)
    a = ap.parse_args()
    if a.asm:
        text, how = open(a.asm).read().splitlines(), f"--asm {os.path.basename(a.asm)}"
    else:
        text, how = compile_unit(a.unit)
    name, lines = kernel_text(text, a.kernel)
    dem = subprocess.run(["c++filt", name], stdout=subprocess.PIPE, text=True).stdout.strip()

    # basic blocks: [label, [opcodes]], cut at labels; intervals: cut behind every s_barrier
    label_re = re.compile(r"^(\.LBB\d+_\d+):")
    branch_re = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")
    order, blocks, intervals, cur = {}, [], [[]], None
    for ln in lines:
        m = label_re.match(ln)
        if m:
            cur = {"label": m.group(1), "ops": [], "loop": False}
            order[cur["label"]] = len(blocks)
            blocks.append(cur)
            intervals[-1].append(cur)
            continue
        s = ln.strip()
        if not s or s.startswith((";", ".", "//")) or not ln.startswith(("\t", " ")):
            continue
        op = s.split()[0]
        if cur is None:
            cur = {"label": "(entry)", "ops": [], "loop": False}
            blocks.append(cur)
            intervals[-1].append(cur)
        cur["ops"].append((op, s))
        if op == "s_barrier":   # the rest of this block belongs to the next interval
            cur = {"label": cur["label"] + "+", "ops": [], "loop": False}
            blocks.append(cur)
            intervals.append([cur])
    for k, b in enumerate(blocks):
        for op, s in b["ops"]:
            m = branch_re.match("\t" + s)
            if m and order.get(m.group(1), len(blocks)) <= k:
                blocks[order[m.group(1)]]["loop"] = True

    def mix(ops):
        c = dict.fromkeys(CLASSES, 0)
        dpp = 0
        for op, _ in ops:
            c[classify(op)] += 1
            dpp += ("_dpp" in op) or op.startswith("v_permlane")
        return c, dpp

    def row(tag, ops, extra=""):
        c, dpp = mix(ops)
        return f"{tag:<22}{len(ops):>6}" + "".join(f"{c[k]:>7}" for k in CLASSES) + f"{dpp:>6}  {extra}"

    total = sum(len(b["ops"]) for b in blocks)
    print(f"# {dem}")
    print(f"# {how}")
    print(f"# {total} instructions, {len(intervals)} barrier-to-barrier intervals; blocks of >= {a.min_block} instructions listed")
    print(f"{'':<22}{'instr':>6}" + "".join(f"{k:>7}" for k in CLASSES) + f"{'dpp':>6}")
    for k, iv in enumerate(intervals):
        ops = [o for b in iv for o in b["ops"]]
        print(row(f"interval {k}", ops, f"{len(iv)} blocks"))
        for b in iv:
            if len(b["ops"]) >= a.min_block:
                print(row("  " + b["label"], b["ops"], "loop" if b["loop"] else ""))
    print(row("kernel", [o for b in blocks for o in b["ops"]]))


if __name__ == "__main__":
    main()
