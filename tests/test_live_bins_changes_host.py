"""CPU: the ladder of live bins that tests/test_live_bins_changes.py climbs, pinned on the host tables without a device (tests/emu/live_kept_emu.cpp
live_emu_sampled: make_bar_taps of glv_tables.h under a sample_scale / sample_range), and the shape of the kept-extent bookkeeping in the host sources.

The live bins of a GLV_OP_BARS_ONLY batch are the bins its bars sample, in whole 64s.  They move with sample_scale and sample_range, and with the shipped
range they do not move with smooth_factor; 80 bars at phase 0 and bars = n at phase 0.5 sample the same bins.  A change in the tap arithmetic shows here,
not as a GPU test whose growing changes no longer grow."""
import ctypes as C
import os
import subprocess

import pytest

from src_scan import ROOT, function_body, read_host_src, strip_comments

# n -> {(sample_scale, sample_range): live bins}; range 0.9 is the shipped one
LADDER = {
    1024: {(12.0, 0.9): 256, (10.0, 0.9): 256, (9.0, 0.9): 320, (8.0, 0.9): 320, (7.0, 0.9): 384, (6.0, 0.9): 448, (8.0, 0.8): 256},
    4096: {(12.0, 0.9): 832, (10.0, 0.9): 960, (9.0, 0.9): 1088, (8.0, 0.9): 1216, (7.0, 0.9): 1408, (6.0, 0.9): 1600, (8.0, 0.8): 832},
}
# the live share of a row of 4096 bins: three eighths (glv_frame.h LIVE_RBLOCKS) -- beyond it a batch has no live class and glv_batch_live_bins is 0
LIVE_SHARE_4096 = 1536


@pytest.fixture(scope="module")
def liveemu(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "emu", "live_kept_emu.cpp")
    so = str(tmp_path_factory.mktemp("livebins") / "libliveemu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
    L = C.CDLL(so)
    L.live_emu_sampled.argtypes = [C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_float]; L.live_emu_sampled.restype = C.c_uint32
    return L


@pytest.mark.parametrize("n", [1024, 4096])
def test_the_ladder_of_live_bins(liveemu, n):
    """every rung for 80 bars at phase 0 and for bars = n at phase 0.5; smooth_factor 0.0125 / 0.025 / 0.05 leave every rung where it is"""
    for (scale, rng), want in LADDER[n].items():
        for bars, phase in ((80, 0.0), (n, 0.5)):
            for factor in (0.025, 0.0125, 0.05):
                got = liveemu.live_emu_sampled(n, bars, factor, phase, scale, rng)
                assert got == want, (n, scale, rng, bars, phase, factor, got, want)


def test_the_schedules_grow_shrink_and_leave_the_live_share():
    """what the GPU file relies on: the schedule 9, 8, 10, 9, 12, 7, 6 at n = 4096 grows inside one block of n / 8 bins (9 -> 8), shrinks, grows back, and
    ends beyond the live share; 12, 9, 7, 9 at n = 1024 grows twice and stays inside three eighths of the row"""
    r = {s: LADDER[4096][(s, 0.9)] for s in (12.0, 10.0, 9.0, 8.0, 7.0, 6.0)}
    assert r[12.0] < r[10.0] < r[9.0] < r[8.0] < r[7.0] <= LIVE_SHARE_4096 < r[6.0]
    assert r[9.0] // 512 == (r[8.0] - 1) // 512 == 2                      # bins [1024, 1536): the last of the three live blocks
    q = {s: LADDER[1024][(s, 0.9)] for s in (12.0, 9.0, 7.0)}
    assert q[12.0] < q[9.0] < q[7.0] <= 3 * 1024 // 8


def test_one_extent_is_recorded_and_one_check_reads_it():
    """glv_host.h keeps the extent beside ran_live and clears it with it; the process call, the track executor and adopt_streams lower it through one
    function; set_params, both texel tables and their clear ask one predicate; the descriptor reports the extent, not the current live bins; both ring
    track entries put it back with ran_live when a launch fails"""
    host = strip_comments(open(os.path.join(ROOT, "glava_amd", "csrc", "glv_host.h")).read())
    assert "ran_live = false; kept_live = 0;" in function_body(host, r"void rewind_state\(")
    src = strip_comments(read_host_src())
    assert src.count("ran_live_over(") == 4 and src.count("ran_live = true") == 1      # the definition and its three callers: nobody else marks a batch live
    assert "b->ran_live_over(b->live_bins())" in function_body(src, r"\nint run_chain\(")
    assert "b->ran_live_over(tp.kept)" in function_body(src, r"\nint track\(glv_batch\* b,")
    assert "ran_live_over(fit.kept)" in function_body(src, r"\nvoid adopt_streams\(")
    assert "keeps_live(b->live_bins())" in function_body(src, r"\nint glv_batch_set_params\(")
    snap = function_body(src, r"\nstatic int set_snap_texels\(")
    assert snap.count("keeps_live(") == 2 and snap.index("keeps_live(b->live_bins_with(0u))") < snap.index("b->snap = BarTableSet()")
    assert "d->kept_bins = b->kept_bins();" in function_body(src, r"\nvoid stream_desc\(")
    for entry in (r"\nint ring_track\(", r"\nint ring_track_each\("):
        body = function_body(src, entry)
        assert "kept_live = b->kept_live" in body and "b->kept_live = kept_live" in body, entry
