"""CPU: track mode at given window starts (glv_batch_track_at_s16 / _f32) without a device -- the exported symbols and their Python prototypes, the
tables of glava_amd.track_starts against a restatement in exact fractions, the clamp's mirror, and the path's freedom from allocating / synchronising
HIP calls (the method of tests/test_track_host.py)."""
import ctypes as C
import os
import re
from fractions import Fraction
from math import floor

import pytest

from glava_amd.track_starts import live_update_starts, renderer_starts
from src_scan import ROOT, TRACK_EXECUTOR, TRACK_COMMON, assert_launch_only, function_body, read_csrc, read_host_src, strip_comments

SYMBOLS = ("glv_batch_track_at_work_bytes", "glv_batch_track_at_s16", "glv_batch_track_at_f32")
RATES = [(22050, 60, 1), (44100, 24, 1), (48000, 60000, 1001), (44100, 60, 1)]


def test_track_at_symbols_are_exported_bound_and_declared(glvlib):
    L = C.CDLL(glvlib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(L, name), name
    lib = glvlib.lib()
    assert lib.glv_batch_track_at_work_bytes.restype is C.c_uint64
    assert len(lib.glv_batch_track_at_work_bytes.argtypes) == 3
    assert len(lib.glv_batch_track_at_s16.argtypes) == 9 and len(lib.glv_batch_track_at_f32.argtypes) == 9
    for meth in ("track_at_work_bytes", "track_at_s16", "track_at_f32"):
        assert callable(getattr(glvlib.Batch, meth)), meth
    header = open(os.path.join(ROOT, "include", "glv_spectrum.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header, name
    assert "min(d_starts[t], pitch_frames - n)" in header                        # the clamp is part of the contract
    assert lib.glv_abi_version() == 7                                            # added within the ABI: detected by the symbol


def test_track_at_refuses_without_a_device(glvlib):
    lib = glvlib.lib()
    assert lib.glv_batch_track_at_work_bytes(None, 1, glvlib.OP_FFT) == 0
    assert lib.glv_batch_track_at_s16(None, None, 0, None, 0, None, None, glvlib.OP_FFT, None) == glvlib.ERR_INVALID
    assert lib.glv_batch_track_at_f32(None, None, 0, None, 0, None, None, glvlib.OP_FFT, None) == glvlib.ERR_INVALID


@pytest.mark.parametrize("rate,num,den", RATES)
def test_renderer_starts_are_the_floor_of_the_exact_position(rate, num, den):
    steps = 4000
    got = renderer_starts(rate, num, den, steps)
    assert got == [floor(Fraction(t) * rate / Fraction(num, den)) for t in range(steps)]
    assert got[0] == 0 and all(b >= a for a, b in zip(got, got[1:]))
    assert all(isinstance(v, int) for v in got)
    if (rate, num, den) == (44100, 60, 1):
        assert got == [t * 735 for t in range(steps)]                            # the uniform hop of the hop entries
    if (rate, num, den) == (22050, 60, 1):
        assert {b - a for a, b in zip(got, got[1:])} == {367, 368}               # 367.5 frames a step, no drift: step 2 k is at 735 k exactly
        assert got[2::2] == [735 * k for k in range(1, steps // 2)]


@pytest.mark.parametrize("update_frames", [16, 256])
@pytest.mark.parametrize("rate,num,den", RATES)
def test_live_update_starts_follow_the_latest_complete_update(rate, num, den, update_frames):
    """brute force: walk the render frames in exact time, count the complete updates each one sees, and open a new step whenever that count moved"""
    frames = 1500
    starts, step_of = live_update_starts(rate, num, den, frames, update_frames)
    want_starts, want_step, seen = [], [], 0
    for j in range(frames):
        t = Fraction(j) * Fraction(den, num)                                      # seconds
        avail = floor(t * rate)                                                   # whole audio frames written by then
        updates = avail // update_frames
        if updates != seen:                                                       # `modified`: a newer update than the one last shown
            want_starts.append(updates * update_frames)
            seen = updates
        want_step.append(len(want_starts) - 1)
    assert starts == want_starts and step_of == want_step
    assert len(step_of) == frames and step_of[0] == -1                            # nothing to show before the first update
    assert all(b > a for a, b in zip(starts, starts[1:]))                         # distinct, forwards
    assert all(s % update_frames == 0 and s >= update_frames for s in starts)
    assert all(0 <= b - a <= 1 for a, b in zip(step_of, step_of[1:]))             # a frame shows its predecessor's step or the next
    if update_frames == 256 and (rate, num, den) == (22050, 60, 1):               # 86 updates against 60 frames a second: advances of 256 or 512
        assert {b - a for a, b in zip(starts, starts[1:])} == {256, 512}


def test_tables_refuse_what_is_not_a_positive_integer():
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            renderer_starts(bad, 60, 1, 4)
        with pytest.raises(ValueError):
            live_update_starts(22050, 60, 1, 4, bad)


def test_the_clamp_mirror(glvlib):
    G = glvlib
    n, pitch = 1024, 5001
    for start, want in ((0, 0), (1, 1), (pitch - n - 1, pitch - n - 1), (pitch - n, pitch - n), (pitch - n + 1, pitch - n), (pitch, pitch - n), (2 ** 32 - 1, pitch - n)):
        assert G.track_at_start(pitch, n, start) == want
        assert G.track_at_start(pitch, n, start) + n <= pitch                     # the window lies inside the recording, whatever the entry
    assert G.track_at_start(n, n, 77) == 0                                        # a recording of one window
    for bad in (dict(pitch_frames=n - 1, n=n, start=0), dict(pitch_frames=pitch, n=n, start=-1), dict(pitch_frames=pitch, n=n, start=2 ** 32)):
        with pytest.raises(ValueError):
            G.track_at_start(**bad)
    # the C twin states the same rule once for the frame kernels and once for the wave kernel
    frame, launch = read_csrc("glv_frame.h"), read_csrc("glv_launch.h")
    assert "entry < w.start_max ? entry : w.start_max" in function_body(frame, r"uint64_t track_window_start\(")
    assert "entry < w.start_max ? entry : w.start_max" in function_body(launch, r"uint64_t wave_window_start\(")
    host = strip_comments(read_host_src())
    assert host.count("start_max = pitch_frames - b->p.n") == 2                    # set where the windows' geometry is, for both kernels


def test_track_at_path_has_no_allocating_or_synchronising_call():
    src = read_host_src()
    assert_launch_only(src, [r"\nint plan_track_at\(", r"\nint track_at\(glv_batch\* b,", r"\nint windows_args\(", r"\nvoid windows_geometry\(", r"\nint plan_track_windows\(",
                             r"\nint plan_track_columns\(", r"\nint plan_track_live\(", r"\nint plan_track_wave\(", r"\nint track_wave\(glv_batch\* b,", r"\nint track_columns\(",
                             r"\nuint64_t glv_batch_track_at_work_bytes\(", r"\nint glv_batch_track_at_s16\(", r"\nint glv_batch_track_at_f32\("] + TRACK_EXECUTOR + TRACK_COMMON)
    plain = strip_comments(src)
    # the entries add no stage of their own: the table's refusals, a plan of the form the batch takes, then the executors of the hop entries
    for name in ("glv_batch_track_at_s16", "glv_batch_track_at_f32"):
        body = function_body(plain, r"\nint " + name + r"\(")
        assert "track_at(b, d_pcm," in body and "glv::launch_" not in body and "for (" not in body, name
    body = function_body(plain, r"\nint track_at\(glv_batch\* b,")
    assert "plan_track_at(" in body and "track(b, tp," in body and "track_wave(b, d_pcm," in body
    assert "glv::launch_" not in body and "for (" not in body and "while (" not in body
    body = function_body(plain, r"\nint plan_track_at\(")
    for form in ("plan_track_live(", "plan_track_columns(", "plan_track_windows("):
        assert form in body, form
    for decided_once in ("tp.state =", "tp.in16 =", "tp.out16 =", "tp.bars =", "check_ops(", "gl_storage == 2", "single_row", "windows_args("):
        assert decided_once not in body, decided_once
    # the hop and pitch rule is written once, and every form that reads windows where they lie asks it
    assert plain.count("int windows_args(") == 1 and plain.count("windows_args(") == 5
    # one scan launch in the host sources, one transform launch of the windows form, no loop in the executors
    assert plain.count("launch_track_scan(") == 1
    assert function_body(plain, r"\nint track_windows\(").count("glv::launch_frame(") == 1
    for sig in (r"\nint track\(glv_batch\* b,", r"\nint track_scan\(", r"\nint track_windows\("):
        body = function_body(plain, sig)
        assert "for (" not in body and "while (" not in body, sig
    # the launchers the path calls launch and nothing else
    assert_launch_only(read_csrc("glv_misc.hip"), [r"\nhipError_t launch_track_scan\(", r"\nhipError_t launch_frame\(", r"\nhipError_t launch_wave_track\("])


def test_every_older_entry_passes_a_null_table():
    """the hop entries never set the table: TrackPlan / TrackWavePlan / WaveWindows default to none, only track_at hands one on, and the transform's
    arguments take the plan's"""
    src = strip_comments(read_host_src())
    assert "const uint32_t* starts = nullptr;" in src                             # TrackPlan
    assert "const uint32_t* starts = nullptr;" in strip_comments(read_csrc("glv_launch.h"))      # WaveWindows
    assert src.count("tp.starts = ") == 1 and "tp.starts = d_starts" in function_body(src, r"\nint track_at\(glv_batch\* b,")
    assert "a.trk.starts = tp.starts;" in function_body(src, r"\nint track_windows\(")
    assert "w.starts = d_starts;" in function_body(src, r"\nint track_wave\(glv_batch\* b,")
    assert "const uint32_t* d_starts = nullptr)" in src                           # track_wave's default
    for name in re.findall(r"\nint (glv_batch_track_[a-z]+_(?:s16|f32)|glv_batch_track_s16)\(", src):
        if name.startswith("glv_batch_track_at_"):
            continue
        body = function_body(src, r"\nint " + name + r"\(")
        assert "starts" not in body and "tp.at" not in body, name
    # the kernels: a null table is t * hop, in the one place each computes a start
    assert "(uint64_t) t * w.hop" in function_body(read_csrc("glv_frame.h"), r"uint64_t track_window_start\(")
    assert "(uint64_t) t * w.hop" in function_body(read_csrc("glv_launch.h"), r"uint64_t wave_window_start\(")
    # ... and the frame kernel reads the table in kinds of its own (IN_S16_TRACK_AT / IN_F32_TRACK_AT, a template constant): the hop kinds' code has no table in it
    tmpl = strip_comments(read_csrc("glv_kernel_tmpl.h"))
    assert tmpl.count("a.trk.starts") == 1 and "if constexpr (TRACK_TABLE) return a.trk.starts[f % a.trk.steps]; else return 0u;" in tmpl
    assert tmpl.count("(uint64_t) t * a.trk.hop") == 1 and tmpl.count("(entry < a.trk.start_max ? entry : a.trk.start_max)") == 1
    body = function_body(src, r"\nint track_windows\(")
    assert "!tp.starts ? hop_mode : tp.f32 ? glv::IN_F32_TRACK_AT : glv::IN_S16_TRACK_AT" in body and "launch_plan(b, a.units, hop_mode," in body
    frame = strip_comments(read_csrc("glv_frame.h"))
    assert "constexpr int IN_S16_TRACK_AT = 7, IN_F32_TRACK_AT = 8;" in frame and "constexpr int kFrameKinds = 9;" in frame
    inst = strip_comments(read_csrc("glv_inst.hip"))
    for kind, part in (("IN_S16_TRACK_AT", "_part5"), ("IN_F32_TRACK_AT", "_part6")):
        assert inst.count(f"launch_log<{kind}, 0>") == 1 and inst.count(f"launch_log<{kind}, 1>") == 1, kind
        assert f"if (in_mode == {kind}) return GLV_CAT(GLV_CAT(launch_frame_, GLV_LOG_NN), {part})" in inst
    assert "glv::kFrameKinds" in function_body(src, r"\nint batch_prepare\(")    # their function attributes are set at creation: a first call can be captured
