"""CPU: track mode at render frames for the wave module (glv_batch_track_wave_frames_s16 / _f32) without a device -- the exported symbols and their Python
prototypes, the numpy restatement of a wave keyframe that tests/test_track_wave_frames.py compares the kernel with (pinned here to the oracle's unpack followed
by the compiled reference's transform_wrange), the numpy lerp (pinned to glvo_lerp, which tests/test_handle_audio.py holds to the real rd_update), and the
path's freedom from allocating / synchronising HIP calls.

The null GL of integration/nullgl_harness.c binds the bars module's transforms only, so the composition -- a wave bind uploads `ilb`, the interpolated buffer
(render.c:2185), when interpolation is on, and nothing forces it off for a bind without an `fft` transform (render.c:2131-2135, :2161-2168) -- is read from the
reference's code, not executed: DESIGN 4.14 says so in those words."""
import ctypes as C
import os

import numpy as np
import pytest

from gpu_lib import wrange
from oracle_lib import Oracle, lcg_pcm_fast
from src_scan import ROOT, TRACK_COMMON, assert_launch_only, function_body, read_csrc, read_host_src, strip_comments

F32 = np.float32
SYMBOLS = ("glv_batch_track_wave_frames_work_bytes", "glv_batch_track_wave_frames_s16", "glv_batch_track_wave_frames_f32")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def np_keyframes(x, starts, n, f32, channels):
    """float32 [len(starts)][streams * 2][n]: keyframe 2 + t of a wave frames call in numpy -- the backend's unpack of the n frames of every stream from starts[t]
    on (x: [streams][pitch][2], int16 or float32; starts already clamped), then (u + 1.0F) / 2.0F, each operation rounded to float32"""
    out = np.empty((len(starts), x.shape[0] * 2, n), F32)
    with np.errstate(all="ignore"):
        for t, a in enumerate(starts):
            win = x[:, a:a + n, :]
            if f32:
                l, r = win[..., 0].astype(F32), win[..., 1].astype(F32)
                if channels == 1: l = r = ((l + r).astype(F32) / F32(2)).astype(F32)             # pulse_input.c:167
            else:
                li, ri = win[..., 0].astype(np.int32), win[..., 1].astype(np.int32)
                if channels == 1: li = ri = np.fix((li + ri) / 2).astype(np.int32)               # fifo.c:98-102: C int division truncates toward zero
                l, r = (li.astype(F32) / F32(65535)).astype(F32), (ri.astype(F32) / F32(65535)).astype(F32)
            out[t, 0::2] = ((l + F32(1)).astype(F32) / F32(2)).astype(F32)                        # render.c:777-778
            out[t, 1::2] = ((r + F32(1)).astype(F32) / F32(2)).astype(F32)
    return out


def np_lerp(s, e, m):
    """s + ((e - s) * m), three float32 operations in the order of render.c:1806"""
    with np.errstate(all="ignore"):
        return (s + ((e - s).astype(F32) * F32(m)).astype(F32)).astype(F32)


def test_wave_frames_symbols_are_exported_bound_and_declared(glvlib):
    L = C.CDLL(glvlib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(L, name), name
    lib = glvlib.lib()
    assert lib.glv_batch_track_wave_frames_work_bytes.restype is C.c_uint64
    assert len(lib.glv_batch_track_wave_frames_work_bytes.argtypes) == 4
    assert len(lib.glv_batch_track_wave_frames_s16.argtypes) == 10 and len(lib.glv_batch_track_wave_frames_f32.argtypes) == 10
    for meth in ("track_wave_frames_work_bytes", "track_wave_frames_s16", "track_wave_frames_f32"):
        assert callable(getattr(glvlib.Batch, meth)), meth
    header = open(os.path.join(ROOT, "include", "glv_spectrum.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header, name
    assert "(u + 1.0F) / 2.0F" in header and "min(d_where[t], pitch_frames - n)" in header      # the keyframe and the clamp are part of the contract
    assert lib.glv_abi_version() == 7                                            # added within the ABI: detected by the symbol


def test_wave_frames_refuse_without_a_device(glvlib):
    lib = glvlib.lib()
    ops = glvlib.OP_WAVE | glvlib.OP_R16
    fr = glvlib.TrackFrames()
    assert lib.glv_batch_track_wave_frames_work_bytes(None, 1, 1, ops) == 0
    assert lib.glv_last_error().decode().startswith("batch is NULL")
    assert lib.glv_batch_track_wave_frames_s16(None, None, 0, None, 0, C.byref(fr), None, None, ops, None) == glvlib.ERR_INVALID
    assert lib.glv_last_error().decode().startswith("batch is NULL")
    assert lib.glv_batch_track_wave_frames_f32(None, None, 0, None, 0, None, None, None, ops, None) == glvlib.ERR_INVALID


@pytest.mark.parametrize("channels", [2, 1], ids=["stereo", "mono"])
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
def test_the_numpy_keyframe_is_the_oracles_unpack_and_the_references_wrange(oracle, ref, f32, channels):
    n, streams = 256, 2
    starts = [0, 3, 130]
    pitch = starts[-1] + n
    if f32:
        x = (np.random.default_rng(77).standard_normal((streams, pitch, 2)) * 0.4).astype(F32)
        x[0, 5, :] = [-0.0, 0.0]; x[1, 131, :] = [1.5, -1.5]; x[1, 140, :] = [-1.0, 1.0]
    else:
        x = lcg_pcm_fast(9200, streams * pitch * 2).reshape(streams, pitch, 2).copy()
        x[0, 4, :] = [-32768, -32768]; x[0, 6, :] = [32767, 32767]; x[1, 7, :] = [-3, 0]; x[1, 8, :] = [3, -6]; x[1, 9, :] = [-32768, 32767]
    got = np_keyframes(x, starts, n, f32, channels)
    for t, a in enumerate(starts):
        for s in range(streams):
            flat = np.ascontiguousarray(x[s, a:a + n, :]).reshape(-1)
            if f32:
                l, r = np.empty(n, F32), np.empty(n, F32)
                Oracle.lib().glvo_unpack_f32(flat, n, channels, l, r)
            else:
                l, r = Oracle.unpack_s16(flat, channels)
            want = wrange(np.stack([l, r]), use_ref=True)
            assert (bits(got[t, 2 * s:2 * s + 2]) == bits(want)).all(), (t, s)


def test_the_numpy_lerp_is_the_oracles():
    rng = np.random.default_rng(78)
    n = 512
    s, e = rng.random(n, dtype=F32), rng.random(n, dtype=F32)
    for uratio, kcounter in ((0.59310347, 0), (0.59310347, 1), (0.3, 2), (0.3, 5), (0.9, 1)):
        ref = np.empty(n, F32)
        Oracle.lib().glvo_lerp(s, e, ref, n, F32(uratio), kcounter)
        m = min(F32(F32(uratio) * F32(kcounter)), F32(1.0))                      # render.c:1804-1805
        assert (bits(np_lerp(s, e, m)) == bits(ref)).all(), (uratio, kcounter)


def test_wave_frames_path_has_no_allocating_or_synchronising_call():
    src = read_host_src()
    assert_launch_only(src, [r"\nint plan_track_wave\(", r"\nint track_wave\(glv_batch\* b,", r"\nint track_wave_frames\(glv_batch\* b,", r"\nint track_frames_call\(",
                             r"\nint track_at\(glv_batch\* b,", r"\nint plan_wave\(", r"\nint windows_args\(", r"\nuint64_t glv_batch_track_wave_frames_work_bytes\(",
                             r"\nint glv_batch_track_wave_frames_s16\(", r"\nint glv_batch_track_wave_frames_f32\("] + TRACK_COMMON)
    plain = strip_comments(src)
    # the entries add no stage: the frames' own refusals, then the table call's wave executor with the frames handed on
    for name, f32 in (("glv_batch_track_wave_frames_s16", "false"), ("glv_batch_track_wave_frames_f32", "true")):
        body = function_body(plain, r"\nint " + name + r"\(")
        assert f"track_frames_call(b, d_pcm, {f32}, pitch_frames, d_where, nullptr, steps, fr," in body and "glv::launch_" not in body and "for (" not in body, name
    body = function_body(plain, r"\nint track_at\(glv_batch\* b,")
    assert "track_wave(b, d_pcm, f32, pitch_frames, 0u, steps, d_out, d_work, ops, st, fr, d_starts)" in body
    # one executor for the wave form: the frames are a branch of track_wave, whose plan is plan_track_wave's and whose bars arithmetic, row format and limit plan_wave's
    assert plain.count("int track_wave(") == 1 and plain.count("int plan_track_wave(") == 1
    body = function_body(plain, r"\nint track_wave\(glv_batch\* b,")
    assert body.count("track_wave_frames(b, tp,") == 1 and body.count("plan_track_wave(") == 1 and "d_scratch" not in body
    assert body.index("track_wave_frames(b, tp,") < body.index("launch_bars_pass(")
    body = function_body(plain, r"\nint track_wave_frames\(glv_batch\* b,")
    assert body.count("glv::launch_wave_frames(") == 1 and body.count("glv::launch_wave_keys(") == 1 and body.count("++b->last_launches") == 2
    assert "tp.pl.wave_limit" in body and "tp.pl.wave_r16" in body and "for (" not in body and "while (" not in body
    assert plain.count("launch_wave_frames(") == 1 and plain.count("launch_wave_keys(") == 1
    body = function_body(plain, r"\nint plan_track_wave\(")
    for refusal in ("frames == 0", "0xffffffffull", "check_ops(", "b->single_row", "windows_args("):
        assert refusal in body, refusal
    assert body.count("plan_wave(") == 2                                          # no third decision about the bars
    # the launchers launch and nothing else; the kernels reuse the waveform kernel's helpers, clamp where an index is taken and loop instead of capping the grid
    unit = read_csrc("glv_track_frames.hip")
    assert_launch_only(unit, [r"\nhipError_t launch_wave_frames\(", r"\nhipError_t launch_wave_keys\("])
    kernel = strip_comments(function_body(unit, r"glv_wave_frames_kernel\(const void\* pcm,"))
    assert "item += gridDim.x" in kernel and "pack_unorm16(" in kernel and "unorm16_to_float(" in kernel
    assert "wl = sl + ((el - sl) * m)" in kernel and "wr = sr + ((er - sr) * m)" in kernel
    assert "__builtin_fmaf" not in kernel and "fma(" not in kernel and "asm" not in kernel
    assert kernel.count("< last_key ? ") == 2 and kernel.count("wave_key<F32_IN>(") == 2
    key = strip_comments(function_body(unit, r"void wave_key\(const void\* pcm,"))
    for reused in ("wave_window_start(w, stream, step, w.starts[step])", "unpack_s16_mono(", "unpack_s16(", "+ 1.0f) / 2.0f", "& 15u"):
        assert reused in key, reused
    assert "asm" not in strip_comments(unit)
