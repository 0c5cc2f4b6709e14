"""CPU: track mode (glv_batch_track_s16) without a device -- the exported symbols and their Python prototypes, the map from window (stream,
step) to (transform launch, row) and its bounds, and the track path's freedom from allocating / synchronising HIP calls."""
import ctypes as C
import os
import re

import pytest

from src_scan import ROOT, TRACK_EXECUTOR, assert_launch_only, function_body, read_csrc, read_host_src, strip_comments


def test_track_symbols_are_exported_and_bound(glvlib):
    L = C.CDLL(glvlib.LIB_PATH)
    for name in ("glv_batch_track_work_bytes", "glv_batch_track_s16"):
        assert hasattr(L, name), name
    lib = glvlib.lib()
    assert lib.glv_batch_track_work_bytes.restype is C.c_uint64
    assert len(lib.glv_batch_track_work_bytes.argtypes) == 5 and len(lib.glv_batch_track_s16.argtypes) == 9
    assert callable(glvlib.Batch.track_work_bytes) and callable(glvlib.Batch.track_s16)
    header = open(os.path.join(ROOT, "include", "glv_spectrum.h")).read()
    assert "glv_batch_track_work_bytes(" in header and "glv_batch_track_s16(" in header


@pytest.mark.parametrize("n", [256, 4096])
def test_every_window_is_one_row_of_one_launch(glvlib, n):
    """window (s, t) starts at s * pitch_frames + t * hop: row k = start / n of launch r = (start % n) / hop, which transforms the K_r back-to-back
    windows starting at r * hop + k * n (include/glv_spectrum.h).  Every window a call reads is a distinct row inside its launch, the row IS that
    window, and no launch's last window ends past the streams * pitch_frames frames of the buffer."""
    G = glvlib
    for hop in (4, n // 16, n // 4, n // 2, n):
        for steps in (1, 2, 11, 2 * (n // hop) + 1):
            need = n + (steps - 1) * hop
            for pitch in (need, need + hop, need + 3 * hop, (need + 5 * n) // hop * hop):
                for streams in (1, 2, 3, 7):
                    K = G.track_residues(n, hop, pitch, streams, steps)
                    assert len(K) == n // hop
                    seen = set()
                    for s in range(streams):
                        for t in range(steps):
                            r, k = G.track_window(n, hop, pitch, s, t)
                            assert 0 <= r < n // hop and 0 <= k < K[r], (hop, steps, pitch, streams, s, t, r, k, K[r])
                            assert r * hop + k * n == s * pitch + t * hop
                            assert (r, k) not in seen
                            seen.add((r, k))
                    for r, k_r in enumerate(K):
                        assert k_r >= 0 and r * hop + k_r * n <= streams * pitch, (hop, steps, pitch, streams, r, k_r)
                        # ... nor past the last window any step reads: a chunk of a longer buffer may end where its last window ends
                        assert r * hop + k_r * n <= (streams - 1) * pitch + need


def test_track_path_has_no_allocating_or_synchronising_call():
    src = read_host_src()
    assert_launch_only(src, [r"\nint plan_track\(", r"\nint glv_batch_track_s16\(", r"\nuint64_t glv_batch_track_work_bytes\("] + TRACK_EXECUTOR)
    # the residue stage holds the only loop of launches on the path: the executor and the other stages have none
    assert "for (" in strip_comments(function_body(src, r"\nint track_residues\("))
    for sig in (r"\nint track\(glv_batch\* b,", r"\nint track_windows\(", r"\nint track_scan\(", r"\nint glv_batch_track_s16\("):
        body = strip_comments(function_body(src, sig))
        assert "for (" not in body and "while (" not in body, sig
    # the launchers the path calls launch and nothing else
    misc = read_csrc("glv_misc.hip")
    assert_launch_only(misc, [r"\nhipError_t launch_track_scan\("])
    body = strip_comments(function_body(misc, r"\nhipError_t launch_track_scan\("))
    assert re.search(r"glv_track_scan_kernel<true>", body) and re.search(r"glv_track_scan_kernel<false>", body)
