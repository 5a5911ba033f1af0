"""CPU: the cells the short image holds in registers over a piece since round 12 (vlg_dp_core.h: dmv_bw_dir_p's BwHeld -- the outside
pass's second stationary walk, uu / gCc on the left, vv / gI on the right -- and dmv_fw_piece_p's FwHeld -- the inside pass's
stationary value cells of every term but the last).

tests/emu/hold_short.cpp is a stand-alone program (its own main).  For every tensor width N = 2 ... 41, every sentence Ne <= N, both
directions, every piece and every lane it checks that dmv_bw_addr names the same held addresses at every width of a piece, replays
the outside pass on counters of gCc and gI (one holder per held word and piece; the only other store to a held word is the right
direction's own-cell store at w = r + 1, behind the holder's last add; ga, gi_old, the GO-count rows and the width-0 cells find every
contribution), and for the inside pass that the held cells are written below the piece's first width and that FwAddr::step() leaves
their addresses alone.  Built as an ordinary executable with -fsanitize=address,undefined, the sanitizer runtimes linked in
statically; nothing is loaded into Python."""
import os
import subprocess

from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "emu", "_build")
SRC = os.path.join(ROOT, "tests", "emu", "hold_short.cpp")
CORE = os.path.join(ROOT, "vlgae_amd", "csrc", "vlg_dp_core.h")
REPORTS = ("AddressSanitizer", "runtime error:", "LeakSanitizer")


def test_held_cells_of_both_passes_are_stationary_and_have_one_owner():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "hold_short_san")
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in (SRC, CORE)):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-static-libasan", "-static-libubsan", SRC, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=0")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert not any(tag in r.stdout for tag in REPORTS), r.stdout[-4000:]
    assert "820 (N, Ne) pairs" in r.stdout and ": 0 failures" in r.stdout
    # the replay must have seen held adds and held inside terms at all (an empty sweep would pass everything above)
    counts = r.stdout.rsplit("pairs,", 1)[1]
    assert " 0 held adds" not in counts and " 0 held inside terms" not in counts, counts
