"""CPU: the stationary cells of the short image's outside pass (vlg_dp_core.h: dmv_bw_segment_p keeps xa and its adjoint word in
registers over a piece).

tests/emu/plan_short.cpp is a stand-alone program (its own main).  For every tensor width N = 2 ... 41, every sentence Ne <= N, both
directions, every piece of the group table and every lane it checks that the reference index formulas (dmv_bw_addr) address the same
xa cell at every width of a piece and that BwAddr's steps follow them, and it replays the pass on counters: every word a lane holds
in a register has that lane as its only writer inside the piece, and every own-cell read (and the width-0 cells of the count
write-out) finds all contributions in the chart.  Built as an ordinary executable with -fsanitize=address,undefined, the sanitizer
runtimes linked in statically; nothing is loaded into Python."""
import os
import subprocess

from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "emu", "_build")
SRC = os.path.join(ROOT, "tests", "emu", "plan_short.cpp")
CORE = os.path.join(ROOT, "vlgae_amd", "csrc", "vlg_dp_core.h")
REPORTS = ("AddressSanitizer", "runtime error:", "LeakSanitizer")


def test_outside_pass_stationary_cells_have_one_owner_per_piece():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "plan_short_san")
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in (SRC, CORE)):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-static-libasan", "-static-libubsan", SRC, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=0")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert not any(tag in r.stdout for tag in REPORTS), r.stdout[-4000:]
    assert "820 (N, Ne) pairs" in r.stdout and ": 0 failures" in r.stdout
