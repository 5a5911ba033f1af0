"""CPU: the short image's load stage since round 13 (vlg_dp_core.h: dmv_stage_request / dmv_stage_write) -- the requests of all N rows
issued without regard to the length, every chart cell stored once by the lane that owns it.

tests/emu/stage_short.cpp is a stand-alone program (its own main).  For every tensor width N = 2 ... 41, every sentence Ne <= N and
the three forms the stage is compiled for (MergedIO on fp32 and bf16 storage, RuleIO) it runs the 512 lanes of the stage one after
the other in forward, reverse and shuffled order and checks that C and I hold in all Ne P cells the bits the general image's stage
leaves there, that each of those cells has exactly one writer -- its owner -- and that no other cell is stored.  The potentials are
allocated at exactly their element counts and the charts at exactly N P cells, with NaN / +-inf / 3e38 at the positions past the
sentence and on attach's diagonal and token ids outside the table past the sentence: a request or a store past a slice is a
sanitizer error, and a poisoned value in a cell is a failure.  Built as an ordinary executable with -fsanitize=address,undefined,
the sanitizer runtimes linked in statically; nothing is loaded into Python.

The count write-out of the same round (dmv_counts_out_short) is run on 512 host threads (it has a barrier and a lane-group
all-reduce) for the same (N, Ne), MergedIO and RuleIO, the Log semiring's dense counts and the Max semiring's tree counts with and
without the head vector, on adjoint charts of exactly N P cells: every output must equal, bit for bit, what dmv_counts_out leaves --
the statements dmv_run executes for the other images (vlg_dp_counts_body.h), compiled from the same text."""
import os
import subprocess

from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "emu", "_build")
SRC = os.path.join(ROOT, "tests", "emu", "stage_short.cpp")
CORE = os.path.join(ROOT, "vlgae_amd", "csrc", "vlg_dp_core.h")
REPORTS = ("AddressSanitizer", "runtime error:", "LeakSanitizer")


def test_stage_cells_equal_the_general_image_and_have_one_writer():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "stage_short_san")
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in (SRC, CORE)):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-static-libasan", "-static-libubsan", SRC, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=0")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=900)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert not any(tag in r.stdout for tag in REPORTS), r.stdout[-4000:]
    assert "820 (N, Ne) pairs, 7380 stage runs, 2460 write-out comparisons" in r.stdout and ": 0 failures" in r.stdout
    # the sweep must have seen cells and stores at all, two stores (C and I) per cell
    cells, stores = (int(r.stdout.rsplit(f" {word}", 1)[0].rsplit(" ", 1)[1]) for word in ("chart cells", "stores"))
    assert cells > 0 and stores == 2 * cells, (cells, stores)
