"""CPU: the short-sentence code image of the DMV1o kernel bodies, on the host, under ASan + UBSan.

tests/emu/emu_short.cpp is a stand-alone program (its own main): it runs dmv_run<Log, true, kSpansShort> and
dmv_run<Log, true, kSpansGeneral> of vlgae_amd/csrc/vlg_dp_core.h on the same merged potentials with 512 host threads as the lanes
and demands identical bits in logZ and in both count tensors, for every length 1 ... 40 as N = 41 and as N = len + 1 -- every
segment boundary of make_sched, the empty segments included.  The short image's per-segment byte addresses (BwAddr) are plain
host-compilable C++; its unclamped reads need the arena's slack, which must still be zero after every run.  The program is built
with -fsanitize=address,undefined as an ordinary executable, the sanitizer runtimes linked in statically (the program then has no
say in, and no need of, what the environment preloads), and must finish clean; nothing is loaded into Python."""
import os
import subprocess

from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "emu", "_build")
SRC = os.path.join(ROOT, "tests", "emu", "emu_short.cpp")
CORE = os.path.join(ROOT, "vlgae_amd", "csrc", "vlg_dp_core.h")
REPORTS = ("AddressSanitizer", "runtime error:", "LeakSanitizer")


def test_short_image_equals_general_image_bit_for_bit_under_sanitizers():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "emu_short_san")
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in (SRC, CORE)):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-static-libasan", "-static-libubsan", SRC, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=0")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=900)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert not any(tag in r.stdout for tag in REPORTS), r.stdout[-4000:]
    assert "80 sentences, short image vs general image: 0 failures" in r.stdout
