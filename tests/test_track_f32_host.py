"""CPU: track mode from float recordings (glv_batch_track_windows_f32, glv_batch_track_wave_f32) without a device -- the exported symbols and their
Python prototypes, the input mode's place in the kernel's enumeration, and the paths' freedom from allocating / synchronising HIP calls (the method
of tests/test_track_windows_host.py and tests/test_track_wave_host.py)."""
import ctypes as C
import os
import re

from src_scan import ROOT, TRACK_COMMON, TRACK_EXECUTOR, assert_launch_only, function_body, read_csrc, read_host_src, strip_comments

ENTRIES = ("glv_batch_track_windows_f32", "glv_batch_track_wave_f32")


def test_track_f32_symbols_are_exported_and_bound(glvlib):
    L = C.CDLL(glvlib.LIB_PATH)
    lib = glvlib.lib()
    header = open(os.path.join(ROOT, "include", "glv_spectrum.h")).read()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert len(getattr(lib, name).argtypes) == 9, name
        assert re.search(r"\nint " + name + r"\(glv_batch\* b, const float\* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps,", header), name
    # sized by the queries of the s16 entries: no query of their own
    assert not hasattr(L, "glv_batch_track_windows_f32_work_bytes") and not hasattr(L, "glv_batch_track_wave_f32_work_bytes")
    assert not hasattr(L, "glv_batch_track_f32")                              # the residue entry has no float twin
    assert callable(glvlib.Batch.track_windows_f32) and callable(glvlib.Batch.track_wave_f32)
    assert lib.glv_abi_version() == 7                                        # added within the ABI: detected by the symbol


def test_the_input_mode_is_appended():
    """IN_F32_TRACK = 6 behind the existing modes, which keep their values (they index the plan cache and are part of the wisdom file's keys)"""
    frame = strip_comments(read_csrc("glv_frame.h"))
    m = re.search(r"enum InMode \{([^}]*)\}", frame)
    names = [tuple(s.strip() for s in item.split("=")) for item in m.group(1).split(",") if item.strip()]
    assert names == [("IN_S16_STEREO", "0"), ("IN_F32_PLANAR", "1"), ("IN_S16_RING", "2"), ("IN_F32_STEREO", "3"), ("IN_F32_RING", "4"),
                     ("IN_S16_TRACK", "5"), ("IN_F32_TRACK", "6")]
    assert re.search(r"kInKinds = 7\b", read_csrc("glv_host.h"))             # ... and the plan cache has a row for it


def test_track_f32_paths_have_no_allocating_or_synchronising_call():
    src = read_host_src()
    assert_launch_only(src, [r"\nint glv_batch_track_windows_f32\(", r"\nint plan_track_windows\(", r"\nuint64_t glv_batch_track_windows_work_bytes\("] + TRACK_EXECUTOR)
    assert_launch_only(src, [r"\nint glv_batch_track_wave_f32\(", r"\nint plan_track_wave\(", r"\nbool pitch_too_short\(", r"\nint track_wave\(glv_batch\* b,", r"\nint plan_wave\(",
                             r"\nuint64_t glv_batch_track_wave_work_bytes\("] + TRACK_COMMON)
    # the float entries add no stage and no loop: they hand the executors the input's type and nothing else
    for name in ENTRIES:
        body = strip_comments(function_body(src, r"\nint " + name + r"\("))
        assert "for (" not in body and "while (" not in body and "glv::launch_" not in body, name
    assert "track(b, tp," in strip_comments(function_body(src, r"\nint glv_batch_track_windows_f32\("))
    assert "track_wave(b, d_pcm, true," in strip_comments(function_body(src, r"\nint glv_batch_track_wave_f32\("))
    # one transform launch, whose mode is the plan's
    body = strip_comments(function_body(src, r"\nint track_windows\("))
    assert body.count("glv::launch_frame(") == 1 and "tp.f32 ? glv::IN_F32_TRACK : glv::IN_S16_TRACK" in body
    # the launcher of the waveform kernel launches and nothing else, in the float kind for float input
    misc = read_csrc("glv_misc.hip")
    assert_launch_only(misc, [r"\nhipError_t launch_wave_track\("])
    body = strip_comments(function_body(misc, r"\nhipError_t launch_wave_track\("))
    for k in (r"glv_wave_kernel<4, true>", r"glv_wave_kernel<4, false>"):
        assert re.search(k, body), k
