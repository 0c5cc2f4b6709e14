"""CPU: the host side of track mode from planar float recordings -- the table of a uniform hop, the tensor checks of the Python methods, the four symbols in the
header and in the mirror, and where the source keeps the new kinds apart from the existing ones."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from glava_amd import track_starts
from src_scan import function_body, read_csrc, read_host_src, strip_comments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("glv_batch_track_at_f32_planar", "glv_batch_track_rates_f32_planar", "glv_batch_track_frames_f32_planar", "glv_batch_track_wave_frames_f32_planar")


def test_hop_starts_is_the_hop_entries_table():
    assert track_starts.hop_starts(5, 735) == [0, 735, 1470, 2205, 2940]
    assert track_starts.hop_starts(1, 1 << 40) == [0]                                # one window: no product to refuse
    assert track_starts.hop_starts(2048, 1 << 21)[-1] == (1 << 32) - (1 << 21)         # the largest entry still a uint32
    assert np.asarray(track_starts.hop_starts(3, (1 << 31) - 1), dtype=np.uint32)[-1] == (1 << 32) - 2
    with pytest.raises(ValueError):
        track_starts.hop_starts(3, 1 << 31)                                          # 2 * 2^31 == 2^32: at the limit
    with pytest.raises(ValueError):
        track_starts.hop_starts(1 << 20, 1 << 13)                                    # beyond it
    for bad in ((0, 1), (1, 0), (-1, 4), (2.0, 4), (True, 4)):
        with pytest.raises(ValueError):
            track_starts.hop_starts(*bad)


def test_the_methods_take_a_contiguous_float32_tensor_of_streams_by_two_by_frames():
    import torch
    from glava_amd.spectrum import planar_pitch_frames
    x = torch.zeros((3, 2, 1027), dtype=torch.float32)
    assert planar_pitch_frames(x, 3) == 1027
    assert planar_pitch_frames(torch.zeros((3 * 2 * 1027 + 1,))[1:].view(3, 2, 1027), 3) == 1027      # a view one float into a buffer: 4-byte aligned is enough
    assert planar_pitch_frames(np.zeros((3, 2, 5), np.float32), 3) == 5
    for bad in (x[:2], x[:, :1], x.reshape(3, 2 * 1027), x.reshape(3, 2, 13, 79), x.double(), x.to(torch.int16), x[:, :, 1:], x.transpose(1, 2), x[:, :, :0], [0.0], None):
        with pytest.raises(ValueError):
            planar_pitch_frames(bad, 3)
    with pytest.raises(ValueError):
        planar_pitch_frames(x, 4)
    # each method asks it before it calls the library
    from glava_amd import spectrum
    src = open(spectrum.__file__).read()
    for name in ("track_at_f32_planar", "track_rates_f32_planar", "track_frames_f32_planar", "track_wave_frames_f32_planar"):
        body = src[src.index(f"    def {name}("):]
        body = body[:body.index("\n    def ", 10)]
        assert "planar_pitch_frames(rows, self.streams)" in body and "pitch_frames" not in body.split('"""')[0], name


def test_the_header_declares_the_four_symbols_and_the_mirror_binds_them(glvlib):
    header = open(os.path.join(ROOT, "include", "glv_spectrum.h")).read()
    L = glvlib.lib()
    for name in ENTRIES:
        assert re.search(r"\nint " + name + r"\(glv_batch\* b, const float\* d_rows, uint32_t pitch_frames,", header), name
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
        sib = getattr(L, name[:-len("_planar")])
        assert len(getattr(L, name).argtypes) == len(sib.argtypes), name            # the sibling's argument list
        nulls = [0 if t in (C.c_uint32, C.c_uint) else None for t in sib.argtypes]
        assert getattr(L, name)(*nulls) == glvlib.ERR_INVALID                          # a NULL batch: refused without a device
    assert L.glv_abi_version() == 7
    plain = strip_comments(header)
    assert "no mono mix" in header.lower() and "glv_batch_track_at_work_bytes" in header[header.index("PLANAR float recordings"):header.index(ENTRIES[0] + "(")]
    assert plain.count("_f32_planar(") == 4


def test_the_entries_hand_the_executors_the_layout_and_nothing_else():
    src = strip_comments(read_host_src())
    for name, executor in zip(ENTRIES, ("track_at(b, d_rows, TrackInput::F32_PLANAR,", "track_rates(b, d_rows, TrackInput::F32_PLANAR,",
                                        "track_frames_call(b, d_rows, TrackInput::F32_PLANAR,", "track_frames_call(b, d_rows, TrackInput::F32_PLANAR,")):
        body = function_body(src, r"\nint " + name + r"\(")
        assert executor in body and "glv::launch_" not in body and "for (" not in body and "hipMalloc" not in body and "Synchronize" not in body, name
    # the 4-byte rule, the planar kinds of the transform and of the decimation, no mix anywhere
    assert "& 3u" in function_body(src, r"\nint refuse_track_pointers\(")
    body = function_body(src, r"\nint track_windows\(")
    assert "hop_mode = glv::IN_F32_PLANAR; mode = glv::IN_F32_PLANAR_TRACK_AT;" in body and "glv::DEC_F32_PLANAR_TRACK" in body and "!tp.f32.planar()" in body
    assert "!f32.planar()" in function_body(src, r"\nint track_wave\(glv_batch\* b,") and "w.planar = " in function_body(src, r"\nint track_wave\(glv_batch\* b,")


def test_the_new_kinds_are_kinds_of_their_own():
    frame, tmpl, inst = (strip_comments(read_csrc(f)) for f in ("glv_frame.h", "glv_kernel_tmpl.h", "glv_inst.hip"))
    assert "constexpr int IN_F32_PLANAR_TRACK_AT = kFrameKinds;" in frame and "in_mode == IN_F32_PLANAR_TRACK_AT" in function_body(frame, r"bool in_track_table\(")
    assert "constexpr bool TRACKP = IN_MODE == IN_F32_PLANAR_TRACK_AT;" in tmpl
    assert inst.count("launch_log<IN_F32_PLANAR_TRACK_AT, 0>") == 1 and inst.count("launch_log<IN_F32_PLANAR_TRACK_AT, 1>") == 1
    assert "if (in_mode == IN_F32_PLANAR_TRACK_AT) return GLV_CAT(GLV_CAT(launch_frame_, GLV_LOG_NN), _part7)" in inst
    from glava_amd import build as B
    assert B.PARTS == tuple(range(8))
    # the loads of a window that begins at any float: 8 bytes where the window lies on them, dwords elsewhere
    loader = function_body(frame, r"void load_f32_raw_at\(")
    assert "& 7u" in loader and "load_f32_raw(r, window, tid)" in loader and loader.count("ld<float>(") == 2
    misc, dec, frames = (strip_comments(read_csrc(f)) for f in ("glv_misc.hip", "glv_decimate.hip", "glv_track_frames.hip"))
    for k in ("glv_wave_kernel<5, true>", "glv_wave_kernel<5, false>"):
        assert k in function_body(misc, r"\nhipError_t launch_wave_track\("), k
    assert "glv_decimate_kernel<DEC_F32_PLANAR_TRACK>" in function_body(dec, r"\nhipError_t launch_decimate\(")
    assert "if (kind == DEC_F32_PLANAR) { if (d.w.steps != 1u || d.w.starts) return hipErrorInvalidValue; }" in dec      # a process call's kind is what it was
    assert "glv_wave_frames_planar_kernel<true>" in function_body(frames, r"\nhipError_t launch_wave_frames\(")
    assert "glv_wave_keys_planar_kernel" in function_body(frames, r"\nhipError_t launch_wave_keys\(")
    assert "asm" not in frames and "asm" not in dec
