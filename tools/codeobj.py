"""Register / scratch / LDS figures of every kernel in the built objects, from the gfx950 code-object notes.

    python tools/codeobj.py [pattern]     # kernels whose demangled name contains the pattern
    python tools/codeobj.py --digest [DIR]   # sha256 of every object's gfx950 code object (DIR: another build's objects), to compare builds

For each translation-unit object in vlgae_amd/_lib the gfx950 offload bundle is extracted (llvm-objdump --offloading, in a
temporary directory) and its AMDGPU metadata note (YAML) parsed: vgpr_count, agpr_count, spills, private segment (scratch)
bytes, static LDS bytes, max workgroup size.  tests/test_codeobj.py asserts on the same records."""
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def kernels_of(obj_path):
    """[{name, demangled, vgpr_count, ...}] for one object built by vlgae_amd.build."""
    out = []
    with tempfile.TemporaryDirectory() as td:
        local = os.path.join(td, os.path.basename(obj_path))
        shutil.copy(obj_path, local)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], cwd=td, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
        for co in glob.glob(os.path.join(td, "*gfx950*")):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], stdout=subprocess.PIPE, text=True).stdout
            if "---" not in notes:
                continue
            doc = notes.split("---", 1)[1].split("\n...", 1)[0]
            meta = yaml.safe_load(doc) or {}
            # .text bytes of every kernel: the FUNC symbols of the code object (the kernel descriptor `name.kd` is a separate OBJECT symbol)
            sizes = {}
            for line in subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--symbols", "--wide", co], stdout=subprocess.PIPE, text=True).stdout.splitlines():
                f = line.split()
                if len(f) >= 8 and f[3] == "FUNC":
                    sizes[f[7]] = int(f[2], 0) if not f[2].isdigit() else int(f[2])
            for k in meta.get("amdhsa.kernels", []):
                rec = {key.lstrip("."): val for key, val in k.items() if key != ".args"}
                rec["text_bytes"] = sizes.get(rec.get("name"), 0)
                rec["kernarg"] = [(a.get(".size"), a.get(".offset"), a.get(".value_kind")) for a in k.get(".args", [])]
                out.append(rec)
    if out:
        dem = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in out), stdout=subprocess.PIPE, text=True).stdout.splitlines()
        for k, d in zip(out, dem):
            k["demangled"] = d
    return out


def all_kernels(lib_dir=None):
    res = []
    for obj in sorted(glob.glob(os.path.join(lib_dir or os.path.join(ROOT, "vlgae_amd", "_lib"), "*.o"))):
        for k in kernels_of(obj):
            k["object"] = os.path.basename(obj)
            res.append(k)
    return res


def digests(lib_dir=None):
    """{object name: [sha256 of each gfx950 code object in it]} for a directory of objects built by vlgae_amd.build: two builds whose
    digests agree run the same device code (`python tools/codeobj.py --digest [DIR]`, once per build, and compare the lines)."""
    import hashlib
    res = {}
    for obj in sorted(glob.glob(os.path.join(lib_dir or os.path.join(ROOT, "vlgae_amd", "_lib"), "*.o"))):
        with tempfile.TemporaryDirectory() as td:
            local = os.path.join(td, os.path.basename(obj))
            shutil.copy(obj, local)
            subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], cwd=td, stdout=subprocess.DEVNULL,
                           stderr=subprocess.DEVNULL)
            res[os.path.basename(obj)] = [hashlib.sha256(open(co, "rb").read()).hexdigest() for co in sorted(glob.glob(os.path.join(td, "*gfx950*")))]
    return res


def sections(lib_dir=None, names=(".text", ".rodata")):
    """[(object name, section, sha256 of its bytes)] of every gfx950 code object: what two builds must share to run the same
    instructions on the same constants, whatever else of the code object (symbol order, notes) moved."""
    import hashlib
    res = []
    for obj in sorted(glob.glob(os.path.join(lib_dir or os.path.join(ROOT, "vlgae_amd", "_lib"), "*.o"))):
        with tempfile.TemporaryDirectory() as td:
            local = os.path.join(td, os.path.basename(obj))
            shutil.copy(obj, local)
            subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], cwd=td, stdout=subprocess.DEVNULL,
                           stderr=subprocess.DEVNULL)
            for co in sorted(glob.glob(os.path.join(td, "*gfx950*"))):
                for sec in names:
                    raw = os.path.join(td, "section.bin")
                    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", f"--only-section={sec}", co, raw], check=True)
                    res.append((os.path.basename(obj), sec, hashlib.sha256(open(raw, "rb").read()).hexdigest()))
    return res


if __name__ == "__main__":
    if "--sections" in sys.argv:   # one line per (object, section); diff the output of two builds
        rest = [a for a in sys.argv[1:] if a != "--sections"]
        for name, sec, sha in sections(rest[0] if rest else None):
            print(name, sec, sha[:16])
        sys.exit(0)
    if "--notes" in sys.argv:      # one line per kernel with every figure of its note but the text size; diff the output of two builds
        rest = [a for a in sys.argv[1:] if a != "--notes"]
        for k in all_kernels(rest[0] if rest else None):
            print(k["object"], {key: val for key, val in sorted(k.items()) if key not in ("object", "text_bytes")})
        sys.exit(0)
    if "--digest" in sys.argv:
        rest = [a for a in sys.argv[1:] if a != "--digest"]
        for name, shas in digests(rest[0] if rest else None).items():
            print(name, *shas)
        sys.exit(0)
    pat = sys.argv[1] if len(sys.argv) > 1 else ""
    for k in all_kernels():
        if pat in k.get("demangled", ""):
            print(f'{k["object"]:20s} vgpr {k.get("vgpr_count", -1):3d} agpr {k.get("agpr_count", -1):3d} spill v{k.get("vgpr_spill_count", 0):<3d} s{k.get("sgpr_spill_count", 0):<3d} '
                  f'scratch {k.get("private_segment_fixed_size", 0):4d} text {k.get("text_bytes", 0) / 1024:6.1f}K lds {k.get("group_segment_fixed_size", 0):6d} wg {k.get("max_flat_workgroup_size", 0):4d}  {k.get("demangled", "?")[:120]}')
