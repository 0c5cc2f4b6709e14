"""CPU: track mode with a per-step update rate (glv_batch_track_rates_s16 / _f32) without a device -- the exported symbols and their Python prototypes,
the path's freedom from allocating / synchronising HIP calls (the method of tests/test_track_at_host.py), glava_amd.track_starts.live_session_rates
against a brute-force walk of render.c:2379-2399 written here, and the classification of the GPU file's texel table."""
import ctypes as C
import os

import numpy as np
import pytest

from glava_amd.track_starts import live_session_rates, live_update_starts
from src_scan import ROOT, TRACK_COMMON, TRACK_EXECUTOR, assert_launch_only, function_body, read_csrc, read_host_src, strip_comments
from track_rates_lib import F32, FLOAT_STEP, FLOAT_UR, STEPS, TEXEL_FLOAT_STEPS, TEXEL_INTEGER_D, TEXEL_STEP, TEXEL_UR, classify, step_of

SYMBOLS = ("glv_batch_track_rates_s16", "glv_batch_track_rates_f32")


def test_track_rates_symbols_are_exported_bound_and_declared(glvlib):
    L = C.CDLL(glvlib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(L, name), name
    lib = glvlib.lib()
    assert len(lib.glv_batch_track_rates_s16.argtypes) == 10 and len(lib.glv_batch_track_rates_f32.argtypes) == 10
    for meth in ("track_rates_s16", "track_rates_f32"):
        assert callable(getattr(glvlib.Batch, meth)), meth
    header = open(os.path.join(ROOT, "include", "glv_spectrum.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header, name
    assert "gravity_step * (1.0F / d_ur[t])" in header                           # the expression is part of the contract
    assert lib.glv_abi_version() == 7                                            # added within the ABI: detected by the symbol


def test_track_rates_refuses_without_a_device(glvlib):
    lib = glvlib.lib()
    ops = glvlib.OP_FFT | glvlib.OP_GRAVITY
    assert lib.glv_batch_track_rates_s16(None, None, 0, None, None, 0, None, None, ops, None) == glvlib.ERR_INVALID
    assert lib.glv_batch_track_rates_f32(None, None, 0, None, None, 0, None, None, ops, None) == glvlib.ERR_INVALID


def test_track_rates_path_has_no_allocating_or_synchronising_call():
    src = read_host_src()
    assert_launch_only(src, [r"\nint track_rates\(glv_batch\* b,", r"\nint track_at\(glv_batch\* b,", r"\nint plan_track_at\(", r"\nint windows_args\(", r"\nvoid windows_geometry\(",
                             r"\nint plan_track_windows\(", r"\nint plan_track_columns\(", r"\nint plan_track_live\(", r"\nint track_columns\(",
                             r"\nuint64_t glv_batch_track_at_work_bytes\(", r"\nint glv_batch_track_rates_s16\(", r"\nint glv_batch_track_rates_f32\("] + TRACK_EXECUTOR + TRACK_COMMON)
    plain = strip_comments(src)
    # the entries add no stage: the rate table's refusals, then the table call with the table handed on -- no launch, no loop, no plan of their own
    for name in SYMBOLS:
        body = function_body(plain, r"\nint " + name + r"\(")
        assert "track_rates(b, d_pcm," in body and "glv::launch_" not in body and "for (" not in body, name
    body = function_body(plain, r"\nint track_rates\(glv_batch\* b,")
    assert "track_at(b, d_pcm," in body and "d_ur)" in body
    for absent in ("glv::launch_", "for (", "while (", "plan_track", "TrackPlan", "b->p.ur", "update_gravity_step("):
        assert absent not in body, absent
    for refusal in ("!d_ur", "& 3u", "ops & GLV_OP_WAVE", "!(ops & GLV_OP_GRAVITY)"):
        assert refusal in body, refusal
    # what the table call refuses for the batch's sake is refused in track_chain, which every form's plan runs: gl_storage 2 and a single-row batch (the drop-ins
    # expose no batch to a binding, so the GPU file cannot make one)
    chain = function_body(plain, r"\nint track_chain\(")
    assert "b->single_row" in chain and "gl_storage == 2" in chain and chain.count("GLV_ERR_STATE") >= 2
    for plan in (r"\nint plan_track_windows\(", r"\nint plan_track_columns\(", r"\nint plan_track_live\("):
        assert "track_chain(b," in function_body(plain, plan), plan
    # the batch's own ur is read by fill_common and update_gravity_step alone, and written by the two functions that set parameters: no track path writes it
    track_unit = strip_comments(read_csrc("glv_track.cpp"))
    assert "->p.ur" not in track_unit and "b->p = " not in track_unit and "update_gravity_step" not in track_unit
    # one place hands the table to the plan, one to the kernel; every older entry leaves it null
    assert "const float* ur = nullptr;" in plain and plain.count("tp.ur = ") == 1 and plain.count("g.ur = tp.ur;") == 1
    assert "tp.ur = d_ur" in function_body(plain, r"\nint track_at\(glv_batch\* b,")
    assert "const float* d_ur = nullptr)" in plain                                # track_at's default
    assert plain.count("launch_track_scan(") == 1                                 # still one scan launch in the host sources
    # the launcher launches and nothing else; the rates kind is picked by the table, and the two older kinds are still instantiated as they were
    misc = read_csrc("glv_misc.hip")
    assert_launch_only(misc, [r"\nhipError_t launch_track_scan\("])
    body = strip_comments(function_body(misc, r"\nhipError_t launch_track_scan\("))
    for kind in ("glv_track_scan_kernel<true, true>", "glv_track_scan_kernel<false, true>", "glv_track_scan_kernel<true>", "glv_track_scan_kernel<false>"):
        assert kind in body, kind
    assert "if (t.ur)" in body
    # the kernel: the table is read in the rates kind alone, the step is the host's expression, texel state takes the float form
    kernel = strip_comments(function_body(misc, r"glv_track_scan_kernel\(const FrameArgs a, const TrackGeometry t\)"))
    assert kernel.count("t.ur[") == 2 and "t.gravity_step * (1.0F / rate[j])" in kernel and "gravity_r16_flt(tex, store, g)" in kernel
    for line in kernel.split("\n"):
        if "t.ur[" in line or "gravity_r16_flt(" in line or "t.gravity_step" in line:
            assert "if constexpr (RATES)" in line, line


# ---- live_session_rates ------------------------------------------------------------------------------------------------------------------------------
def _walk(rate, fps, frames, update_frames):
    """render.c:2358-2399 frame by frame, independent of the module: gl->ur starts at 1.0F (:906); a frame whose audio position shows a newer complete
    update than the one last shown is `modified` and runs a step at the ur that stands; then its counters are added"""
    ur = F32(1.0)
    tcounter, ucounter, shown = 0.0, 0, 0
    starts, step_of_frame, urs = [], [], []
    for j in range(frames):
        updates = (j * rate // fps) // update_frames
        modified = updates != shown
        if modified:
            shown = updates
            starts.append(updates * update_frames)
            urs.append(float(ur))
        step_of_frame.append(len(starts) - 1)
        duration = 1.0 / float(fps)                   # :2362, :2370: the frame meets its target
        if modified: ucounter += 1                    # :2380-2381
        tcounter += duration                          # :2384
        if tcounter >= 1.0:                           # :2385
            ur = F32(ucounter / tcounter)             # :2387
            tcounter, ucounter = 0.0, 0               # :2397-2399
    return starts, step_of_frame, urs


def _distinct(values):
    out = []
    for v in values:
        if not out or out[-1] != v: out.append(v)
    return out


@pytest.mark.parametrize("rate,fps,update_frames", [(22050, 60, 256), (22050, 30, 256), (22050, 144, 256), (22050, 24, 256), (44100, 60, 256), (22050, 4, 64), (48000, 75, 512),
                                                    (22050, 100, 16), (8000, 7, 1024)])
def test_live_session_rates_follow_the_reference_counters(rate, fps, update_frames):
    frames = 6 * fps + 5
    starts, step_of_frame, ur = live_session_rates(rate, fps, frames, update_frames)
    assert (starts, step_of_frame) == live_update_starts(rate, fps, 1, frames, update_frames)
    want = _walk(rate, fps, frames, update_frames)
    assert starts == want[0] and step_of_frame == want[1] and ur == want[2]
    assert len(ur) == len(starts)
    assert all(isinstance(v, float) and float(F32(v)) == v for v in ur)           # exact float32 values
    assert ur[0] == 1.0


def test_live_session_rates_literals():
    _, _, ur = live_session_rates(22050, 60, 245, 256)
    assert len(ur) == 244                                                         # frame 0 sees no update
    assert ur[:59] == [1.0] * 59 and ur[59:119] == [59.0] * 60 and ur[119:] == [60.0] * (len(ur) - 119)
    for fps, want in ((30, [1.0, 29.032258987426758, 30.0]), (144, [1.0, 85.40689849853516, 86.4000015258789]), (24, [1.0, 23.040000915527344, 24.0])):
        _, _, ur = live_session_rates(22050, fps, 5 * fps, 256)
        assert _distinct(ur) == want, (fps, _distinct(ur))
    # why one table entry is not integer arithmetic: 60 additions of 1 / 60 reach 1.0 in doubles, 30 of 1 / 30 do not
    t = 0.0
    for _ in range(60): t += 1.0 / 60.0
    assert t == 1.0000000000000013
    t = 0.0
    for _ in range(30): t += 1.0 / 30.0
    assert t < 1.0
    # the GPU file's session
    starts, step_of_frame, ur = live_session_rates(22050, 4, 12, 64)
    assert ur == [1.0, 1.0, 1.0, 3.0, 3.0, 3.0, 3.0, 4.0, 4.0, 4.0, 4.0] and len(starts) == STEPS and step_of_frame[0] == -1


def test_live_session_rates_refuses_what_is_not_a_positive_integer():
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            live_session_rates(22050, bad, 4, 256)
        with pytest.raises(ValueError):
            live_session_rates(bad, 60, 4, 256)
        with pytest.raises(ValueError):
            live_session_rates(22050, 60, 4, bad)


# ---- the GPU file's tables ---------------------------------------------------------------------------------------------------------------------------
def test_the_texel_table_exercises_both_kinds_of_step():
    """the rates kind evaluates every step in float; the sequential side takes the packed integer step wherever the host's exhaustive check accepts it.  The
    equivalence is only tested if the table holds both: held to the counts, so that a change of the table cannot quietly drop one kind"""
    kinds = classify(TEXEL_STEP, TEXEL_UR)
    in_float = [t for t, (flt, _) in enumerate(kinds) if flt]
    integer = [d for flt, d in kinds if not flt]
    assert len(in_float) >= 4 and len(integer) >= 6
    assert in_float == TEXEL_FLOAT_STEPS and integer == TEXEL_INTEGER_D


def test_the_classification_agrees_with_the_library_s_host_emulator(emu):
    """the numpy restatement against glv_tables.h gravity_r16_integer_step itself, compiled into the host emulator"""
    emu.glvemu_gravity_step.argtypes = [C.c_float, C.c_float, C.POINTER(C.c_uint32)]
    emu.glvemu_gravity_step.restype = C.c_int
    for ur, (flt, d) in zip(TEXEL_UR, classify(TEXEL_STEP, TEXEL_UR)):
        d_lib = C.c_uint32(0)
        assert bool(emu.glvemu_gravity_step(TEXEL_STEP, ur, C.byref(d_lib))) == (not flt), ur
        if not flt: assert d_lib.value == d, (ur, d, d_lib.value)


def test_the_float_table_holds_the_edge_rates():
    g = [step_of(FLOAT_STEP, ur) for ur in FLOAT_UR]
    assert np.isposinf(g[1]) and g[3] < 0 and 1e30 < g[4] < np.inf and 0 < g[5] < 1e-29 and g[9] == F32(4.2)
    assert all(float(F32(v)) == v for v in FLOAT_UR) and all(float(F32(v)) == v for v in TEXEL_UR)
    assert len(FLOAT_UR) == STEPS > 8
