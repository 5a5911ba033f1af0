"""CPU: the give-up rules of the k-best walks (vlgae_amd/csrc/vlg_dp_kbest.h: kbest_bp_fits, kbest_child_fits, kbest_walk_finish) under
both models' walks.  The emulators fill the charts, overwrite the back-pointer of rank 0 of a sentence's root cell with a value that does
not fit it, and walk: that rank must come back with heads 0 and score NaN, every other rank and sentence as without the damage, and
nothing outside the charts may be touched (the emulators' canaries)."""
import ctypes

import numpy as np
import pytest

import test_dmv_kbest_host as DMV
import test_kbest_host as DEP

N, K, KC = 6, 4, 4
LENGTHS = [N - 1, 3]
W = LENGTHS[0]   # the width of the damaged root cell CR(0, len) of sentence 0
# a back-pointer is r << 8 | p << 4 | q: the children of CR(0, w) are IR(0, 1 + r)[p] and CR(1 + r, w)[q]
PLANTED = {"r = w": W << 8,
           "p = KC": KC << 4,
           "q = KC": KC,
           "rank 1 of a width-0 child": (W - 1) << 8 | 1}   # CR(w, w)[1]


def _run(model, mode, plant):
    if model == "deptree":
        emu = ctypes.CDLL(DEP._build(DEP.os.path.join(DEP.BUILD, "libvlg_emu_kbest.so"), ["-fPIC", "-shared"]))
        arc = DEP.R.potentials(np.random.default_rng(611), (2, N, N))
        pots = [np.ascontiguousarray(arc, np.float32)]
        fn = emu.emu_deptree_kbest_planted
    else:
        emu = ctypes.CDLL(DMV._build(DMV.os.path.join(DMV.BUILD, "libvlg_emu_dmv_kbest.so"), ["-fPIC", "-shared"]))
        dec, attach = DMV.R.potentials(np.random.default_rng(612), 2, N)
        pots = [np.ascontiguousarray(dec, np.float32), np.ascontiguousarray(attach, np.float32)]
        fn = emu.emu_dmv1o_kbest_planted
    ln, pl = np.asarray(LENGTHS, np.int64), np.asarray(plant, np.int32)
    heads = np.full((K, 2, N), -1, np.int64)
    scores, count = np.full((K, 2), np.nan, np.float32), np.full(2, -1, np.int32)
    p = DEP._p
    assert fn(*[p(a) for a in pots], p(ln), 2, N, 0, K, mode, p(pl), p(heads), p(scores), p(count), 8, 1) == 0
    return heads, scores, count, emu.emu_canary_trips()


@pytest.mark.parametrize("what", list(PLANTED))
@pytest.mark.parametrize("mode", (0, 2))
@pytest.mark.parametrize("model", ("deptree", "dmv1o"))
def test_walk_gives_up_on_a_back_pointer_that_does_not_fit(model, mode, what):
    heads0, scores0, count0, trips0 = _run(model, mode, [-1, -1])
    assert list(count0) == [K, K] and not np.isnan(scores0).any() and heads0[:, 0, 1:].min() >= 0
    heads, scores, count, trips = _run(model, mode, [PLANTED[what], -1])
    assert trips == trips0 == 0
    assert not heads[0, 0].any() and np.isnan(scores[0, 0])                     # the damaged rank: heads 0, score NaN
    assert np.array_equal(count, count0)                                        # (the count reads the values, not the pointers)
    assert np.array_equal(heads[1:], heads0[1:]) and np.array_equal(heads[0, 1], heads0[0, 1])
    assert np.array_equal(scores[1:].view(np.uint32), scores0[1:].view(np.uint32)) and scores[0, 1].view(np.uint32) == scores0[0, 1].view(np.uint32)
