"""CPU: the group-size rule and the lane map of the short image's outside pass (vlg_dp_core.h: bw_sched, bw_piece_of, bw_lane).

tests/emu/sched_short.cpp is a stand-alone program (its own main).  For every Ne = 2 ... 41 and every width it checks that the rule's
group size G, the groups per wavefront and the term count satisfy what the header asserts at compile time (capacity, G non-decreasing
in w, at most two terms per lane and one at G = 64, G TM <= 64, at least one group per wavefront), and that the lane -> (slot, rr) map
covers every (span, split point) of the width exactly once with no group crossing a multiple of 64.  Built as an ordinary executable
with -fsanitize=address,undefined, the sanitizer runtimes linked in statically; nothing is loaded into Python."""
import os
import subprocess

from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "emu", "_build")
SRC = os.path.join(ROOT, "tests", "emu", "sched_short.cpp")
CORE = os.path.join(ROOT, "vlgae_amd", "csrc", "vlg_dp_core.h")
REPORTS = ("AddressSanitizer", "runtime error:", "LeakSanitizer")


def test_outside_pass_group_table_and_lane_map():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "sched_short_san")
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in (SRC, CORE)):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-static-libasan", "-static-libubsan", SRC, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=0")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert not any(tag in r.stdout for tag in REPORTS), r.stdout[-4000:]
    assert "820 widths of 40 sentences: 0 failures" in r.stdout
