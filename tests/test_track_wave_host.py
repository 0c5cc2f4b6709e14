"""CPU: track mode for the wave module (glv_batch_track_wave_s16) without a device -- the exported symbols and their Python prototypes, the map from
output row to the first frame of its window, and the path's freedom from allocating / synchronising HIP calls."""
import ctypes as C
import os
import re

import pytest

from src_scan import ROOT, TRACK_COMMON, assert_launch_only, function_body, read_csrc, read_host_src, strip_comments


def test_track_wave_symbols_are_exported_and_bound(glvlib):
    L = C.CDLL(glvlib.LIB_PATH)
    for name in ("glv_batch_track_wave_work_bytes", "glv_batch_track_wave_s16"):
        assert hasattr(L, name), name
    lib = glvlib.lib()
    assert lib.glv_batch_track_wave_work_bytes.restype is C.c_uint64
    assert len(lib.glv_batch_track_wave_work_bytes.argtypes) == 5 and len(lib.glv_batch_track_wave_s16.argtypes) == 9
    assert callable(glvlib.Batch.track_wave_work_bytes) and callable(glvlib.Batch.track_wave_s16)
    header = open(os.path.join(ROOT, "include", "glv_spectrum.h")).read()
    assert "glv_batch_track_wave_work_bytes(" in header and "glv_batch_track_wave_s16(" in header
    assert glvlib.lib().glv_abi_version() == 7                                   # added within ABI 7: detected by the symbol


@pytest.mark.parametrize("n", [256, 4096])
def test_every_output_row_starts_where_its_window_does(glvlib, n):
    """row t * streams * 2 + 2 s + c reads the n frames from s * pitch_frames + t * hop on: the helper against a brute-force loop, no row starting
    outside its stream's pitch, the last window ending inside the buffer -- for hops that are no power of two, no multiple of 8, and larger than n"""
    G = glvlib
    for hop in (1, 8, 100, n, n + 8):
        for steps in (1, 2, 11):
            need = n + (steps - 1) * hop
            for pitch in (need, need + 1, need + 3 * hop):
                for streams in (1, 3):
                    rows = G.track_wave_rows(n, hop, pitch, streams, steps)
                    assert len(rows) == steps * streams * 2
                    r = 0
                    for t in range(steps):
                        for s in range(streams):
                            for c in range(2):
                                assert rows[r] == s * pitch + t * hop, (hop, steps, pitch, streams, t, s, c)
                                assert s * pitch <= rows[r] and rows[r] + n <= (s + 1) * pitch           # inside its stream's pitch
                                r += 1
                    assert max(rows) + n <= streams * pitch                                                # the last window ends inside the buffer
                    assert max(rows) + n == (streams - 1) * pitch + need
    for bad in (dict(hop=0), dict(steps=0), dict(pitch_frames=n + 10 * 8 - 1)):
        kw = dict(n=n, hop=8, pitch_frames=n + 10 * 8, streams=2, steps=11)
        kw.update(bad)
        with pytest.raises(ValueError):
            G.track_wave_rows(**kw)


def test_track_wave_path_has_no_allocating_or_synchronising_call():
    src = read_host_src()
    assert_launch_only(src, [r"\nint plan_track_wave\(", r"\nbool pitch_too_short\(", r"\nint track_wave\(glv_batch\* b,", r"\nint plan_wave\(", r"\nint glv_batch_track_wave_s16\(",
                             r"\nuint64_t glv_batch_track_wave_work_bytes\("] + TRACK_COMMON)
    # the rows between the two launches live in the caller's workspace, not in the scratch rows of one update
    body = strip_comments(function_body(src, r"\nint track_wave\(glv_batch\* b,"))
    assert "d_scratch" not in body and "d_work" in body
    # the launchers the path calls launch and nothing else
    misc, bars = read_csrc("glv_misc.hip"), read_csrc("glv_bars.hip")
    for text, sig, kernels in ((misc, r"\nhipError_t launch_wave_track\(", (r"glv_wave_kernel<3, true>", r"glv_wave_kernel<3, false>")),
                               (bars, r"\nhipError_t launch_bars_i8_pcm_track\(", (r"launch_bars_i8_in<I8_PCM_TRACK, true>", r"launch_bars_i8_in<I8_PCM_TRACK, false>"))):
        assert_launch_only(text, [sig])
        body = strip_comments(function_body(text, sig))
        for k in kernels:
            assert re.search(k, body), (sig, k)
