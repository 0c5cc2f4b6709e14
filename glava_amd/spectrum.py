"""ctypes binding of the C ABI (include/glv_spectrum.h) -- plumbing, not the product.

The product is libglvspectrum.so (hand-written HIP for gfx950, glava_amd/csrc).  This
module only loads it, mirrors `glv_params`, and passes raw device pointers (from torch
tensors or any other allocator) across.  There is no fallback of any kind: if the shared
object is missing or the device is unusable, calls raise `GlvError`.

Names follow the reference's operator table (glava/render.c:849-856): fft, gravity,
avg(average), wrange.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# GLV_SPECTRUM_LIB: an A/B build of the SAME library (glava_amd.build --variant, tools/ab_bench.sh); never a fallback
LIB_PATH = os.environ.get("GLV_SPECTRUM_LIB") or os.path.join(HERE, "csrc", "libglvspectrum.so")

OP_FFT, OP_GRAVITY, OP_AVERAGE, OP_RAW, OP_WRANGE, OP_BARS, OP_SMOOTH, OP_MAGNITUDE, OP_R16 = 1, 2, 4, 8, 16, 32, 64, 128, 256
OP_PRIVATE_STATE, OP_RING_S16, OP_RING_F32, OP_OUTPUT_IS_STATE, OP_BARS_ONLY = 512, 1024, 2048, 4096, 8192
OP_WAVE = 1 << 14                  # the wave module's bind: unpack -> wrange -> GL_R16 upload (with OP_BARS: + the pre-smoothing pass)
OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_NOMEM, ERR_STATE = 0, 1, 2, 3, 4, 5
BARS_NONE, BARS_F32_CHAIN, BARS_F32_MATRIX, BARS_I8_EXACT, BARS_F32_SEQ = 0, 1, 2, 3, 4
ROUND_SINUSOIDAL, ROUND_CIRCULAR, ROUND_LINEAR = 0, 1, 2          # glv_params.round_formula
SAMPLE_AVERAGE, SAMPLE_MAXIMUM, SAMPLE_HYBRID = 0, 1, 2            # glv_params.sample_mode
# glv_params.gl_storage: float state and float rows (the CPU operators) / GL_R16 state, one launch (GLava as shipped) / the GL passes one by one on
# float state / the CPU operators on float state as with 0, and OP_BARS samples the GL_R16 upload of the finished buffer (GLava with `setaccelfft false`;
# added within ABI 7: a library that has it accepts the value in glv_batch_create)
GL_STORAGE_FLOAT, GL_STORAGE_R16, GL_STORAGE_PASSES, GL_STORAGE_UPLOAD = 0, 1, 2, 3
MAX_BUFSCALE = 16                  # GLV_MAX_BUFSCALE: the largest k of Batch.set_bufscale


class GlvError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"glv error {code}: {msg}")
        self.code = code


class CParams(C.Structure):
    _fields_ = [("n", C.c_uint32), ("channels", C.c_uint32), ("fft_scale", C.c_float), ("fft_cutoff", C.c_float),
                ("gravity_step", C.c_float), ("ur", C.c_float), ("avg_frames", C.c_uint32),
                ("avg_window", C.c_uint32), ("avg_window_kind", C.c_uint32), ("log_mode", C.c_uint32),
                ("bars", C.c_uint32), ("smooth_factor", C.c_float),
                ("smooth_distance", C.c_float), ("smooth_ratio", C.c_float), ("gl_storage", C.c_uint32),
                ("bar_phase", C.c_float),
                # ABI 7: smooth_audio()'s shape (smooth_parameters.glsl:17-42); 0 = the shipped value in every field
                ("round_formula", C.c_uint32), ("sample_mode", C.c_uint32), ("sample_hybrid_weight", C.c_float),
                ("sample_scale", C.c_float), ("sample_range", C.c_float)]


class MultiStats(C.Structure):
    """glv_multi_stats: the 32-byte record every rank contributes to the RCCL all-gather"""
    _fields_ = [("frames", C.c_uint64), ("seconds", C.c_double), ("bytes", C.c_uint64), ("kernel_ms", C.c_double)]


class TrackFrames(C.Structure):
    """glv_track_frames: the render frames of a glv_batch_track_frames_s16 / _f32 call -- three device tables of `frames` entries, the caller-owned keyframes
    and the pair of keyframe indices written back to them"""
    _fields_ = [("d_from", C.c_void_p), ("d_to", C.c_void_p), ("d_mod", C.c_void_p), ("frames", C.c_uint32), ("d_keys", C.c_void_p),
                ("keep_from", C.c_uint32), ("keep_to", C.c_uint32)]


class TrackTables(C.Structure):
    """glv_track_tables: the per-stream tables of a glv_batch_track_each_s16 / _f32 / _f32_planar call, all in device memory -- window starts uint32
    [streams][steps], update rates float32 [streams][steps] or NULL (the batch's own ur), steps per stream uint32 [streams] or NULL (every stream takes all)"""
    _fields_ = [("d_starts", C.c_void_p), ("d_ur", C.c_void_p), ("d_counts", C.c_void_p)]


class TrackFramesEach(C.Structure):
    """glv_track_frames_each: the render frames of a glv_batch_track_each_frames_* / glv_batch_track_pool_frames_* call, a row per stream -- three device tables
    [streams][frames], frames per stream uint32 [streams] or NULL (every stream takes all), the keep pairs uint32 [streams][2], the longest row, and the
    caller-owned keyframes"""
    _fields_ = [("d_from", C.c_void_p), ("d_to", C.c_void_p), ("d_mod", C.c_void_p), ("d_frame_counts", C.c_void_p), ("d_keep", C.c_void_p), ("frames", C.c_uint32),
                ("d_keys", C.c_void_p)]


class TrackSpan(C.Structure):
    """glv_track_span: where one stream's recording lies in the pool of a glv_batch_track_pool_s16 / _f32 / _f32_planar call -- its first frame counted from
    the pool's first frame (64-bit: a pool may pass 2^32 frames), its length in frames, and a word that is never read.  One 16-byte record per stream, in
    device memory, 16-byte aligned; as a numpy dtype: glava_amd.track_starts.SPAN_DTYPE."""
    _fields_ = [("first", C.c_uint64), ("frames", C.c_uint32), ("reserved", C.c_uint32)]


class StreamStateDesc(C.Structure):
    """glv_stream_state_desc: what a blob of Batch.save_streams is -- the batch's n, F and element size, the form gravity's state was kept in, the regions
    present (bit 0 gravity rows, 1 average ring, 2 s16 PCM ring, 3 f32 PCM ring), the bins kept and the bytes of one stream (glava_amd/stream_slots.py
    restates the layout)"""
    _fields_ = [("n", C.c_uint32), ("avg_frames", C.c_uint32), ("elem_bytes", C.c_uint32), ("gravity_form", C.c_uint32), ("regions", C.c_uint32),
                ("kept_bins", C.c_uint32), ("bytes", C.c_uint64)]


_lib = None


def lib() -> C.CDLL:
    """Load libglvspectrum.so (built in-tree by glava_amd.build); fail loudly if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GlvError(ERR_NO_DEVICE, f"{LIB_PATH} not built -- run `python -m glava_amd.build` "
                                          "(there is no Python/CPU fallback)")
        # One HIP runtime per process: PyTorch bundles its own libamdhip64 with the same soname as
        # /opt/rocm's.  Whichever is loaded first wins for everybody, and torch.cuda only comes up on
        # its own copy -- so make sure torch (when installed) is imported before our library pulls in
        # the system one.  This is process plumbing, not a dependency: the C ABI itself is torch-free.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        P = C.POINTER(CParams)
        vp = C.c_void_p
        L.glv_params_default.argtypes = [P]; L.glv_params_default.restype = None
        L.glv_abi_version.restype = C.c_int
        L.glv_last_error.restype = C.c_char_p
        L.glv_device_count.restype = C.c_int
        L.glv_state_create.argtypes = [P, C.c_int, C.POINTER(vp)]
        L.glv_state_reset.argtypes = [vp]
        L.glv_state_destroy.argtypes = [vp]
        for name in ("glv_fft", "glv_gravity", "glv_average", "glv_wrange", "glv_smooth", "glv_magnitude", "glv_fft_gravity_average"):
            getattr(L, name).argtypes = [P, vp, vp]
        L.glv_texels_r16.argtypes = [P, vp, vp, vp]
        L.glv_gl_texture.argtypes = [P, vp, vp, C.c_int, vp]
        if hasattr(L, "glv_wave_texture"):              # (added within ABI 7: callers detect it by the symbol)
            L.glv_wave_texture.argtypes = [P, vp, vp, C.c_int, vp]
        L.glv_unpack_s16.argtypes = [C.c_int, vp, C.c_size_t, C.c_int, vp, vp]
        L.glv_batch_create.argtypes = [P, C.c_uint32, C.c_uint, C.c_int, C.POINTER(vp)]
        L.glv_batch_reset.argtypes = [vp]
        L.glv_batch_set_params.argtypes = [vp, P]
        L.glv_batch_destroy.argtypes = [vp]
        L.glv_batch_process_s16.argtypes = [vp, vp, vp, C.c_uint, vp]
        L.glv_batch_process_f32.argtypes = [vp, vp, vp, C.c_uint, vp]
        L.glv_batch_process_f32_stereo.argtypes = [vp, vp, vp, C.c_uint, vp]
        L.glv_batch_ring_update_s16.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint, vp]
        L.glv_batch_ring_update_f32.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint, vp]
        L.glv_batch_bars.argtypes = [vp, vp, vp, vp]
        if hasattr(L, "glv_batch_set_bar_texels"):      # (added within ABI 7: callers detect it by the symbol)
            L.glv_batch_set_bar_texels.argtypes = [vp, vp, C.c_uint32]
        if hasattr(L, "glv_batch_set_column_texels"):   # (likewise)
            L.glv_batch_set_column_texels.argtypes = [vp, vp, C.c_uint32]
        for form in ("track", "track_windows", "track_wave", "track_columns", "track_live"):   # (likewise, each pair by its call's symbol)
            _bind_track_pair(L, form)
        if hasattr(L, "glv_batch_track_at_s16"):        # (likewise: a table of window starts in place of the hop, a query without hop and pitch)
            L.glv_batch_track_at_work_bytes.argtypes = [vp, C.c_uint32, C.c_uint]
            L.glv_batch_track_at_work_bytes.restype = C.c_uint64
            L.glv_batch_track_at_s16.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp, vp, C.c_uint, vp]
            L.glv_batch_track_at_f32.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp, vp, C.c_uint, vp]
        if hasattr(L, "glv_batch_track_rates_s16"):     # (likewise: a table call with a second table, the update rate gravity runs at per step)
            L.glv_batch_track_rates_s16.argtypes = [vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, vp, C.c_uint, vp]
            L.glv_batch_track_rates_f32.argtypes = [vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, vp, C.c_uint, vp]
        if hasattr(L, "glv_batch_track_frames_s16"):    # (likewise: a table or rates call on gl_storage 3 whose output is every render frame's texture, keyframes interpolated)
            FR = C.POINTER(TrackFrames)
            L.glv_batch_track_frames_work_bytes.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint]
            L.glv_batch_track_frames_work_bytes.restype = C.c_uint64
            L.glv_batch_track_frames_s16.argtypes = [vp, vp, C.c_uint32, vp, vp, C.c_uint32, FR, vp, vp, C.c_uint, vp]
            L.glv_batch_track_frames_f32.argtypes = [vp, vp, C.c_uint32, vp, vp, C.c_uint32, FR, vp, vp, C.c_uint, vp]
        if hasattr(L, "glv_batch_track_wave_frames_s16"):   # (likewise: the wave module's render frames, keyframes read from the recording)
            FR = C.POINTER(TrackFrames)
            L.glv_batch_track_wave_frames_work_bytes.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint]
            L.glv_batch_track_wave_frames_work_bytes.restype = C.c_uint64
            L.glv_batch_track_wave_frames_s16.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, FR, vp, vp, C.c_uint, vp]
            L.glv_batch_track_wave_frames_f32.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, FR, vp, vp, C.c_uint, vp]
        if hasattr(L, "glv_batch_track_at_f32_planar"):    # (likewise: the table, rates, frames and wave-frames calls from planar float rows [streams][2][pitch_frames])
            FR = C.POINTER(TrackFrames)
            L.glv_batch_track_at_f32_planar.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp, vp, C.c_uint, vp]
            L.glv_batch_track_rates_f32_planar.argtypes = [vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, vp, C.c_uint, vp]
            L.glv_batch_track_frames_f32_planar.argtypes = [vp, vp, C.c_uint32, vp, vp, C.c_uint32, FR, vp, vp, C.c_uint, vp]
            L.glv_batch_track_wave_frames_f32_planar.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, FR, vp, vp, C.c_uint, vp]
        if hasattr(L, "glv_batch_track_each_s16"):      # (likewise: the table and rates calls with a table row and a count of steps per stream)
            TT = C.POINTER(TrackTables)
            L.glv_batch_track_each_s16.argtypes = [vp, vp, C.c_uint32, TT, C.c_uint32, vp, vp, C.c_uint, vp]
            L.glv_batch_track_each_f32.argtypes = [vp, vp, C.c_uint32, TT, C.c_uint32, vp, vp, C.c_uint, vp]
            L.glv_batch_track_each_f32_planar.argtypes = [vp, vp, C.c_uint32, TT, C.c_uint32, vp, vp, C.c_uint, vp]
        if hasattr(L, "glv_batch_track_pool_s16"):      # (likewise: the per-stream calls over one pool of recordings, a span per stream)
            TT = C.POINTER(TrackTables)
            L.glv_batch_track_pool_s16.argtypes = [vp, vp, C.c_uint64, vp, TT, C.c_uint32, vp, vp, C.c_uint, vp]
            L.glv_batch_track_pool_f32.argtypes = [vp, vp, C.c_uint64, vp, TT, C.c_uint32, vp, vp, C.c_uint, vp]
            L.glv_batch_track_pool_f32_planar.argtypes = [vp, vp, C.c_uint64, vp, TT, C.c_uint32, vp, vp, C.c_uint, vp]
        if hasattr(L, "glv_batch_track_each_frames_s16"):      # (likewise: the frames calls with frame tables, a frame count and a keep pair per stream)
            TT, FE = C.POINTER(TrackTables), C.POINTER(TrackFramesEach)
            for kind in ("s16", "f32", "f32_planar"):
                getattr(L, "glv_batch_track_each_frames_" + kind).argtypes = [vp, vp, C.c_uint32, TT, C.c_uint32, FE, vp, vp, C.c_uint, vp]
                getattr(L, "glv_batch_track_pool_frames_" + kind).argtypes = [vp, vp, C.c_uint64, vp, TT, C.c_uint32, FE, vp, vp, C.c_uint, vp]
        if hasattr(L, "glv_batch_track_each_wave_frames_s16"):      # (likewise: the wave module's frames calls per stream, the same argument lists)
            TT, FE = C.POINTER(TrackTables), C.POINTER(TrackFramesEach)
            for kind in ("s16", "f32", "f32_planar"):
                getattr(L, "glv_batch_track_each_wave_frames_" + kind).argtypes = [vp, vp, C.c_uint32, TT, C.c_uint32, FE, vp, vp, C.c_uint, vp]
                getattr(L, "glv_batch_track_pool_wave_frames_" + kind).argtypes = [vp, vp, C.c_uint64, vp, TT, C.c_uint32, FE, vp, vp, C.c_uint, vp]
        if hasattr(L, "glv_batch_set_bufscale"):        # (likewise: `setbufscale k` for a batch -- windows of k * n frames, decimated on the device)
            L.glv_batch_set_bufscale.argtypes = [vp, C.c_uint32]
            L.glv_batch_bufscale.argtypes = [vp]
            L.glv_batch_bufscale.restype = C.c_uint32
        if hasattr(L, "glv_batch_reset_streams"):       # (likewise: reset, save and load chosen streams of a batch)
            SD = C.POINTER(StreamStateDesc)
            L.glv_batch_stream_state_desc.argtypes = [vp, SD]
            L.glv_batch_reset_streams.argtypes = [vp, vp, C.c_uint32, vp]
            L.glv_batch_save_streams.argtypes = [vp, vp, C.c_uint32, vp, SD, vp]
            L.glv_batch_load_streams.argtypes = [vp, vp, C.c_uint32, vp, SD, vp]
        if hasattr(L, "glv_batch_copy_streams"):        # (likewise: the first `count` streams of a batch only; streams copied from slot to slot)
            for name in ("s16", "f32", "f32_stereo"):
                getattr(L, "glv_batch_process_first_" + name).argtypes = [vp, C.c_uint32, vp, vp, C.c_uint, vp]
            L.glv_batch_ring_update_first_s16.argtypes = [vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint, vp]
            L.glv_batch_ring_update_first_f32.argtypes = [vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint, vp]
            L.glv_batch_copy_streams.argtypes = [vp, vp, vp, vp, C.c_uint32, vp]
        L.glv_batch_ring_append_s16.argtypes = [vp, vp, C.c_uint32, vp]
        L.glv_batch_ring_append_f32.argtypes = [vp, vp, C.c_uint32, vp]
        L.glv_batch_ring_planar.argtypes = [vp, C.c_int, vp, vp]
        if hasattr(L, "glv_batch_ring_track_s16"):      # (likewise: several updates of a ring batch in one track call)
            L.glv_batch_ring_track_work_bytes.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint]
            L.glv_batch_ring_track_work_bytes.restype = C.c_uint64
            L.glv_batch_ring_track_s16.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint, vp]
            L.glv_batch_ring_track_f32.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint, vp]
        if hasattr(L, "glv_batch_ring_track_each_s16"):      # (likewise: ring updates in one track call with a count of updates and a rate row per stream)
            L.glv_batch_ring_track_each_work_bytes.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint]
            L.glv_batch_ring_track_each_work_bytes.restype = C.c_uint64
            L.glv_batch_ring_track_each_s16.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_uint, vp]
            L.glv_batch_ring_track_each_f32.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_uint, vp]
        L.glv_batch_gravity_state.argtypes = [vp, C.POINTER(C.c_void_p)]
        L.glv_prelude_bufscale.argtypes = [C.c_int, vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, vp]
        L.glv_prelude_lerp.argtypes = [C.c_int, vp, vp, vp, C.c_size_t, C.c_float, C.c_int, vp]
        L.glv_batch_timing_begin.argtypes = [vp]
        L.glv_batch_timing_end.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        L.glv_batch_live_bins.argtypes = [vp]; L.glv_batch_live_bins.restype = C.c_uint32
        L.glv_batch_tune_placement.argtypes = [vp, vp, vp, C.c_uint, C.c_int, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.glv_batch_bars_arithmetic.argtypes = [vp]; L.glv_batch_bars_arithmetic.restype = C.c_int
        L.glv_batch_algorithmic_bytes.argtypes = [vp, C.c_uint, C.c_int]
        L.glv_batch_algorithmic_bytes.restype = C.c_uint64
        L.glv_batch_kernel_name.argtypes = [vp]; L.glv_batch_kernel_name.restype = C.c_char_p
        L.glv_batch_set_grid.argtypes = [vp, C.c_int]
        L.glv_batch_last_grid.argtypes = [vp]
        L.glv_batch_last_launches.argtypes = [vp]
        L.glv_batch_variants.argtypes = [vp]
        L.glv_batch_set_variant.argtypes = [vp, C.c_int]
        L.glv_batch_last_variant.argtypes = [vp]
        L.glv_batch_describe_variant.argtypes = [vp, C.c_int, C.c_char_p, C.c_size_t]
        L.glv_batch_window_selftest.argtypes = [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_int)]
        L.glv_batch_autotune.argtypes = [vp, vp, vp, C.c_uint, vp, C.POINTER(C.c_int), C.POINTER(C.c_float)]
        L.glv_wisdom_save.argtypes = [C.c_char_p]; L.glv_wisdom_load.argtypes = [C.c_char_p]
        L.glv_multi_shard_range.argtypes = [C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.glv_multi_shard_range.restype = None
        L.glv_multi_create.argtypes = [P, C.c_uint64, C.c_uint, C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
        L.glv_multi_destroy.argtypes = [vp]
        L.glv_multi_devices.argtypes = [vp]
        L.glv_multi_uses_rccl.argtypes = [vp]
        L.glv_multi_shard.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(vp)]
        L.glv_multi_run_s16.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_uint, C.c_int, C.c_int, C.POINTER(MultiStats), C.POINTER(C.c_double)]
        _lib = L
    return _lib


def _bind_track_pair(L, form: str) -> None:
    """prototypes of a track entry and its sizing query (glv_batch_<form>_s16, glv_batch_<form>_work_bytes), where the library has them"""
    if not hasattr(L, f"glv_batch_{form}_s16"):
        return
    vp, u32 = C.c_void_p, C.c_uint32
    query = getattr(L, f"glv_batch_{form}_work_bytes")
    query.argtypes = [vp, u32, u32, u32, C.c_uint]
    query.restype = C.c_uint64
    getattr(L, f"glv_batch_{form}_s16").argtypes = [vp, vp, u32, u32, u32, vp, vp, C.c_uint, vp]
    if hasattr(L, f"glv_batch_{form}_f32"):         # the float twin (track_windows, track_wave, track_columns), sized by the same query
        getattr(L, f"glv_batch_{form}_f32").argtypes = [vp, vp, u32, u32, u32, vp, vp, C.c_uint, vp]


def _check(rc: int) -> None:
    if rc != OK:
        raise GlvError(rc, lib().glv_last_error().decode())


@dataclass
class Params:
    """Mirror of glv_params; defaults are the shipped GLava configuration.

    gl_storage: GL_STORAGE_FLOAT (0, the CPU operators on float state), GL_STORAGE_R16 (1, the GL passes on GL_R16 state in one launch),
    GL_STORAGE_PASSES (2, the GL passes one by one) or GL_STORAGE_UPLOAD (3, GLava with `setaccelfft false`: everything as with 0, and OP_BARS -- the
    pre-smoothing pass, bar texels, column texels, maximum / hybrid -- samples the GL_R16 upload of the finished float rows; OP_WAVE | OP_BARS as with 1).
    A batch moves between 0, 2 and 3 through set_params; 1 is a state class of its own."""
    n: int = 4096
    channels: int = 2
    fft_scale: float = 10.2
    fft_cutoff: float = 0.3
    gravity_step: float = 4.2
    ur: float = 22050.0 / 256.0
    avg_frames: int = 5
    avg_window: bool = True
    avg_window_kind: int = 0
    log_mode: int = 1
    bars: int = 80
    smooth_factor: float = 0.025
    smooth_distance: float = 0.01
    smooth_ratio: float = 4.0
    gl_storage: int = 0
    bar_phase: float = 0.0
    round_formula: int = 0          # ROUND_SINUSOIDAL / ROUND_CIRCULAR / ROUND_LINEAR
    sample_mode: int = 0            # SAMPLE_AVERAGE / SAMPLE_MAXIMUM / SAMPLE_HYBRID
    sample_hybrid_weight: float = 0.0
    sample_scale: float = 0.0
    sample_range: float = 0.0

    def c(self) -> CParams:
        return CParams(self.n, self.channels, self.fft_scale, self.fft_cutoff, self.gravity_step, self.ur,
                       self.avg_frames, int(self.avg_window), self.avg_window_kind, self.log_mode,
                       self.bars, self.smooth_factor, self.smooth_distance, self.smooth_ratio, self.gl_storage, self.bar_phase,
                       self.round_formula, self.sample_mode, self.sample_hybrid_weight, self.sample_scale, self.sample_range)


def _ptr(x) -> C.c_void_p:
    """Raw pointer of a torch tensor / numpy array / int / None."""
    if x is None:
        return C.c_void_p(None)
    if isinstance(x, int):
        return C.c_void_p(x)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    if hasattr(x, "ctypes"):
        return C.c_void_p(x.ctypes.data)
    raise TypeError(type(x))


def planar_pitch_frames(rows, streams: int) -> int:
    """pitch_frames of a planar recording handed to the track_*_f32_planar methods: `rows` must be a contiguous float32 tensor (or array) of shape
    [streams, 2, frames] -- its last dimension is returned.  Raises ValueError on anything else, before the library is called."""
    shape = tuple(int(d) for d in getattr(rows, "shape", ()))
    if len(shape) != 3 or shape[0] != streams or shape[1] != 2:
        raise ValueError(f"a planar recording is a tensor [streams={streams}, 2, frames], not {list(shape) if shape else type(rows).__name__}")
    if not str(getattr(rows, "dtype", "")).endswith("float32"):
        raise ValueError(f"a planar recording holds float32 samples, not {getattr(rows, 'dtype', None)}")
    contiguous = rows.is_contiguous() if hasattr(rows, "is_contiguous") else bool(rows.flags["C_CONTIGUOUS"])
    if not contiguous:
        raise ValueError("a planar recording must be contiguous: rows pitch_frames floats apart, two to a stream (call .contiguous())")
    if shape[2] < 1 or shape[2] > 0xffffffff:
        raise ValueError(f"frames={shape[2]} does not fit pitch_frames, a uint32 >= 1")
    return shape[2]


class Batch:
    """B independent stereo streams on one GPU (glv_batch)."""

    def __init__(self, params: Params, streams: int, ops_mask: int = OP_FFT, device: int = 0):
        self.params, self.streams, self.ops_mask, self.device = params, streams, ops_mask, device
        self._h = C.c_void_p(None)
        cp = params.c()
        _check(lib().glv_batch_create(C.byref(cp), streams, ops_mask, device, C.byref(self._h)))

    def set_params(self, params: Params) -> None:
        """glv_batch_set_params: change scalar knobs (synchronous: tables are regenerated); n, avg_frames and the state's storage
        class are fixed at creation"""
        cp = params.c()
        _check(lib().glv_batch_set_params(self._h, C.byref(cp)))
        self.params = params

    def set_bufscale(self, k: int) -> None:
        """glv_batch_set_bufscale: `setbufscale k` of rc.glsl (1: off, the default; up to MAX_BUFSCALE).  While k > 1 a window of every process call and of the
        FFT track entries (windows, columns, live, at, rates, frames) is k * n frames -- [streams][k * n][2] interleaved, [streams][2][k * n] for process_f32 --
        and is decimated on the device to the n samples per channel the chain transforms: means of k consecutive samples, summed in float32 in index order
        and divided once (render.c:1765-1790).  Synchronous, and the only call of the feature that allocates; state, head, tables and texel tables are kept,
        set_params and reset keep k.  track_s16, the wave track entries, the ring entries, autotune and tune_placement refuse while k > 1."""
        _check(lib().glv_batch_set_bufscale(self._h, k))

    @property
    def bufscale(self) -> int:
        """the batch's bufscale k (glv_batch_bufscale)"""
        return int(lib().glv_batch_bufscale(self._h))

    def stream_state_desc(self) -> StreamStateDesc:
        """what a blob of this batch is now (glv_batch_stream_state_desc): .bytes per stream, the regions present, the gravity form and kept bins as the
        calls the batch has run left them"""
        d = StreamStateDesc()
        _check(lib().glv_batch_stream_state_desc(self._h, C.byref(d)))
        return d

    def reset_streams(self, d_idx, count: int, stream: int | None = None) -> None:
        """glv_batch_reset_streams: the streams listed in d_idx (uint32 [count] in device memory, read when the kernel runs; entries >= streams are skipped)
        become streams of a batch reset() has just cleared, every other stream is untouched; head, ring positions and gravity form stay.  One launch,
        stream-ordered, capturable; a captured reset is re-aimed by rewriting d_idx.  Reset a slot when a listener attaches to it."""
        _check(lib().glv_batch_reset_streams(self._h, _ptr(d_idx), count, _ptr(stream)))

    def save_streams(self, d_idx, count: int, d_blob, stream: int | None = None) -> StreamStateDesc:
        """glv_batch_save_streams: the state of the listed streams into d_blob (count * stream_state_desc().bytes bytes, 16-byte aligned; blob j belongs to
        d_idx[j]) in the portable form -- gravity rows, the average ring oldest frame first, the PCM rings oldest frame first: no position of this batch
        survives.  Returns the descriptor load_streams checks.  One launch, stream-ordered."""
        d = StreamStateDesc()
        _check(lib().glv_batch_save_streams(self._h, _ptr(d_idx), count, _ptr(d_blob), C.byref(d), _ptr(stream)))
        return d

    def load_streams(self, d_idx, count: int, d_blob, desc: StreamStateDesc, stream: int | None = None) -> None:
        """glv_batch_load_streams: blobs of save_streams into the listed streams, rotated by THIS batch's positions -- the stream then continues bit for
        bit as the saved one would have.  desc must match the batch (n, F, element size, regions: ERR_STATE), the gravity forms must agree unless one is
        still 0, a live blob (kept_bins < n) loads only into an OP_BARS_ONLY batch whose live_bins() are no more than that.  Duplicates in d_idx are the caller's error."""
        _check(lib().glv_batch_load_streams(self._h, _ptr(d_idx), count, _ptr(d_blob), C.byref(desc), _ptr(stream)))

    def copy_streams(self, d_dst_idx, src: "Batch", d_src_idx, count: int, stream: int | None = None) -> None:
        """glv_batch_copy_streams, called on the destination: stream d_dst_idx[j] of this batch continues as stream d_src_idx[j] of `src` (another batch of
        the same kind on the same device, or this one) would have -- save_streams + load_streams in one launch, without the blob, whatever positions the two
        batches are at.  Both tables are uint32 [count] in device memory, read when the kernel runs; pairs with an entry >= its batch's streams are skipped.
        Within one batch a destination must not be a source of the same call, and no destination may appear twice."""
        _check(lib().glv_batch_copy_streams(self._h, _ptr(d_dst_idx), src._h, _ptr(d_src_idx), count, _ptr(stream)))

    def process_first_s16(self, count: int, d_pcm, d_out, ops: int = OP_FFT, stream: int | None = None) -> None:
        """process_s16 on streams [0, count) as a batch of `count` streams would run it (glv_batch_process_first_s16): d_pcm and d_out are dense for `count`
        streams, the other streams are neither read nor written.  head and the gravity form are the batch's and advance as for a full call: a stream that
        joins the prefix later is first the target of reset_streams, load_streams or copy_streams (glava_amd.stream_slots.DensePool keeps that protocol)."""
        _check(lib().glv_batch_process_first_s16(self._h, count, _ptr(d_pcm), _ptr(d_out), ops, _ptr(stream)))

    def process_first_f32(self, count: int, d_in, d_out, ops: int = OP_FFT, stream: int | None = None) -> None:
        _check(lib().glv_batch_process_first_f32(self._h, count, _ptr(d_in), _ptr(d_out), ops, _ptr(stream)))

    def process_first_f32_stereo(self, count: int, d_in, d_out, ops: int = OP_FFT, stream: int | None = None) -> None:
        _check(lib().glv_batch_process_first_f32_stereo(self._h, count, _ptr(d_in), _ptr(d_out), ops, _ptr(stream)))

    def ring_update_first_s16(self, count: int, d_new, new_frames: int, d_out, ops: int = OP_FFT, stream: int | None = None) -> None:
        """ring_update_s16 on streams [0, count): d_new [count][new_frames][2]; the ring position is the batch's and advances as for a full call"""
        _check(lib().glv_batch_ring_update_first_s16(self._h, count, _ptr(d_new), new_frames, _ptr(d_out), ops, _ptr(stream)))

    def ring_update_first_f32(self, count: int, d_new, new_frames: int, d_out, ops: int = OP_FFT, stream: int | None = None) -> None:
        _check(lib().glv_batch_ring_update_first_f32(self._h, count, _ptr(d_new), new_frames, _ptr(d_out), ops, _ptr(stream)))

    def process_s16(self, d_pcm, d_out, ops: int = OP_FFT, stream: int | None = None) -> None:
        """one update of every stream; stream-ordered (never allocates, never copies synchronously).  Chains ending in gravity
        keep their state in a batch-owned buffer; with OP_OUTPUT_IS_STATE d_out itself becomes the state the next update reads
        (leave it intact until then; see include/glv_spectrum.h)."""
        _check(lib().glv_batch_process_s16(self._h, _ptr(d_pcm), _ptr(d_out), ops, _ptr(stream)))

    def process_f32(self, d_in, d_out, ops: int = OP_FFT, stream: int | None = None) -> None:
        _check(lib().glv_batch_process_f32(self._h, _ptr(d_in), _ptr(d_out), ops, _ptr(stream)))

    def process_f32_stereo(self, d_in, d_out, ops: int = OP_FFT, stream: int | None = None) -> None:
        _check(lib().glv_batch_process_f32_stereo(self._h, _ptr(d_in), _ptr(d_out), ops, _ptr(stream)))

    def _track_work_bytes(self, form: str, pitch_frames: int, hop: int, steps: int, ops: int) -> int:
        """glv_batch_<form>_work_bytes; 0 is a refusal, whose message names its code"""
        nbytes = int(getattr(lib(), f"glv_batch_{form}_work_bytes")(self._h, pitch_frames, hop, steps, ops))
        if nbytes == 0:
            msg = lib().glv_last_error().decode()
            raise GlvError(ERR_STATE if msg.startswith("GLV_ERR_STATE") else ERR_INVALID, msg)
        return nbytes

    def _track_call(self, form: str, d_pcm, pitch_frames: int, hop: int, steps: int, d_out, d_work, ops: int, stream: int | None, kind: str = "s16") -> None:
        """glv_batch_<form>_<kind>"""
        _check(getattr(lib(), f"glv_batch_{form}_{kind}")(self._h, _ptr(d_pcm), pitch_frames, hop, steps, _ptr(d_out), _ptr(d_work), ops, _ptr(stream)))

    def track_work_bytes(self, pitch_frames: int, hop: int, steps: int, ops: int) -> int:
        """bytes of device workspace track_s16 needs for these arguments (glv_batch_track_work_bytes); raises on arguments the call refuses"""
        return self._track_work_bytes("track", pitch_frames, hop, steps, ops)

    def track_s16(self, d_pcm, pitch_frames: int, hop: int, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """`steps` consecutive updates of every stream from one long buffer (glv_batch_track_s16): d_pcm int16 [streams][pitch_frames][2], window t of
        stream s = its frames [t * hop, t * hop + n); d_out step-major, step t exactly what process_s16 call t would have written; d_work at least
        track_work_bytes(...) bytes, 256-byte aligned.  Output and state bit for bit those of the sequential calls; stream-ordered, kernels only."""
        self._track_call("track", d_pcm, pitch_frames, hop, steps, d_out, d_work, ops, stream)

    def track_windows_work_bytes(self, pitch_frames: int, hop: int, steps: int, ops: int) -> int:
        """bytes of device workspace track_windows_s16 needs for these arguments (glv_batch_track_windows_work_bytes; 256 where the call needs none); raises
        on arguments the call refuses"""
        return self._track_work_bytes("track_windows", pitch_frames, hop, steps, ops)

    def track_windows_s16(self, d_pcm, pitch_frames: int, hop: int, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """track_s16 at ANY hop >= 1 and any pitch_frames >= n + (steps - 1) * hop (glv_batch_track_windows_s16): one transform launch reads each window
        where it lies; d_pcm 4-byte aligned; d_work at least track_windows_work_bytes(...) bytes, 256-byte aligned.  Output and state bit for bit those of
        the sequential calls; stream-ordered, kernels only."""
        self._track_call("track_windows", d_pcm, pitch_frames, hop, steps, d_out, d_work, ops, stream)

    def track_windows_f32(self, d_pcm, pitch_frames: int, hop: int, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """track_windows_s16 from a float recording (glv_batch_track_windows_f32): d_pcm float32 [streams][pitch_frames][2], interleaved L R, 8-byte
        aligned; any hop >= 1; d_work at least track_windows_work_bytes(...) bytes (the same query), 256-byte aligned.  Output and state bit for bit
        those of `steps` process_f32_stereo calls on the windows; stream-ordered, kernels only."""
        self._track_call("track_windows", d_pcm, pitch_frames, hop, steps, d_out, d_work, ops, stream, "f32")

    def track_columns_work_bytes(self, pitch_frames: int, hop: int, steps: int, ops: int) -> int:
        """bytes of device workspace track_columns_s16 / _f32 need for these arguments (glv_batch_track_columns_work_bytes: two regions of
        steps * streams * 2 texel rows, each rounded up to 256 bytes); raises on arguments the call refuses"""
        return self._track_work_bytes("track_columns", pitch_frames, hop, steps, ops)

    def track_columns_s16(self, d_pcm, pitch_frames: int, hop: int, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """the graph module's columns of `steps` consecutive updates of every stream from one long buffer (glv_batch_track_columns_s16), on a gl_storage 1
        batch with set_column_texels: d_pcm int16 [streams][pitch_frames][2], any hop >= 1; d_out float32 [steps][streams * 2][cols], step t bit for bit
        what process_s16 on window t would have written, the state afterwards what those calls leave; ops OP_FFT | OP_BARS with OP_GRAVITY / OP_AVERAGE;
        d_work at least track_columns_work_bytes(...) bytes, 256-byte aligned.  Stream-ordered, three kernels."""
        self._track_call("track_columns", d_pcm, pitch_frames, hop, steps, d_out, d_work, ops, stream)

    def track_columns_f32(self, d_pcm, pitch_frames: int, hop: int, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """track_columns_s16 from a float recording (glv_batch_track_columns_f32): d_pcm float32 [streams][pitch_frames][2], 8-byte aligned; step t bit for
        bit what process_f32_stereo on window t would have written; the same workspace query."""
        self._track_call("track_columns", d_pcm, pitch_frames, hop, steps, d_out, d_work, ops, stream, "f32")

    def track_live_work_bytes(self, pitch_frames: int, hop: int, steps: int, ops: int) -> int:
        """bytes of device workspace track_live_s16 / _f32 need for these arguments (glv_batch_track_live_work_bytes: what the windows or the columns query
        gives for the same batch without OP_BARS_ONLY); raises on arguments the call refuses"""
        return self._track_work_bytes("track_live", pitch_frames, hop, steps, ops)

    def track_live_s16(self, d_pcm, pitch_frames: int, hop: int, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """track mode for a batch created with OP_BARS_ONLY (glv_batch_track_live_s16): the bars, bar texels or columns -- whichever the batch has set -- of
        `steps` consecutive updates of every stream from one long buffer, d_pcm int16 [streams][pitch_frames][2], any hop >= 1; ops OP_FFT | OP_BARS with
        OP_GRAVITY / OP_AVERAGE.  Step t bit for bit what process_s16 on window t would have written on this batch, head, gravity form and the state below
        live_bins() as those calls leave them; d_work at least track_live_work_bytes(...) bytes, 256-byte aligned.  Stream-ordered, three kernels."""
        self._track_call("track_live", d_pcm, pitch_frames, hop, steps, d_out, d_work, ops, stream)

    def track_live_f32(self, d_pcm, pitch_frames: int, hop: int, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """track_live_s16 from a float recording (glv_batch_track_live_f32): d_pcm float32 [streams][pitch_frames][2], 8-byte aligned; step t bit for bit
        what process_f32_stereo on window t would have written; the same workspace query."""
        self._track_call("track_live", d_pcm, pitch_frames, hop, steps, d_out, d_work, ops, stream, "f32")

    def track_at_work_bytes(self, steps: int, ops: int) -> int:
        """bytes of device workspace track_at_s16 / _f32 need for these arguments (glv_batch_track_at_work_bytes: what the query of the form the call takes
        reports for the same steps; 256 where the call needs none); raises on arguments the call refuses"""
        nbytes = int(lib().glv_batch_track_at_work_bytes(self._h, steps, ops))
        if nbytes == 0:
            msg = lib().glv_last_error().decode()
            raise GlvError(ERR_STATE if msg.startswith("GLV_ERR_STATE") else ERR_INVALID, msg)
        return nbytes

    def track_at_s16(self, d_pcm, pitch_frames: int, d_starts, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """track mode at given window starts (glv_batch_track_at_s16): d_starts uint32 [steps] in device memory, shared by all streams; window t of stream
        s is the n frames of its recording from track_at_start(pitch_frames, n, d_starts[t]) on -- any order, repeats and backward jumps included.  The
        form is the one the ops and the batch select (OP_WAVE: wave; an OP_BARS_ONLY batch: live; column texels set: columns; else windows), d_out and
        d_work as that form takes them, d_work at least track_at_work_bytes(...) bytes.  Output and state bit for bit those of the sequential calls;
        stream-ordered, kernels only; the table is read when the kernels run."""
        _check(lib().glv_batch_track_at_s16(self._h, _ptr(d_pcm), pitch_frames, _ptr(d_starts), steps, _ptr(d_out), _ptr(d_work), ops, _ptr(stream)))

    def track_at_f32(self, d_pcm, pitch_frames: int, d_starts, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """track_at_s16 from a float recording (glv_batch_track_at_f32): d_pcm float32 [streams][pitch_frames][2], interleaved L R, 8-byte aligned; step t
        bit for bit what process_f32_stereo on window t would have written"""
        _check(lib().glv_batch_track_at_f32(self._h, _ptr(d_pcm), pitch_frames, _ptr(d_starts), steps, _ptr(d_out), _ptr(d_work), ops, _ptr(stream)))

    def track_rates_s16(self, d_pcm, pitch_frames: int, d_starts, d_ur, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """track_at_s16 with a per-step update rate (glv_batch_track_rates_s16): d_ur float32 [steps] in device memory, shared by all streams; step t
        applies gravity with gravity_step * (1.0F / d_ur[t]), as a process call preceded by set_params(ur=d_ur[t]) does -- output and state bit for bit
        those calls'; the batch's own ur is not changed.  ops must have OP_GRAVITY and no OP_WAVE; d_work at least track_at_work_bytes(steps, ops) bytes.
        Tables of a live session: glava_amd.track_starts.live_session_rates.  Stream-ordered, kernels only; both tables are read when the kernels run."""
        _check(lib().glv_batch_track_rates_s16(self._h, _ptr(d_pcm), pitch_frames, _ptr(d_starts), _ptr(d_ur), steps, _ptr(d_out), _ptr(d_work), ops, _ptr(stream)))

    def track_rates_f32(self, d_pcm, pitch_frames: int, d_starts, d_ur, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """track_rates_s16 from a float recording (glv_batch_track_rates_f32): d_pcm float32 [streams][pitch_frames][2], interleaved L R, 8-byte aligned"""
        _check(lib().glv_batch_track_rates_f32(self._h, _ptr(d_pcm), pitch_frames, _ptr(d_starts), _ptr(d_ur), steps, _ptr(d_out), _ptr(d_work), ops, _ptr(stream)))

    def track_frames_work_bytes(self, steps: int, frames: int, ops: int) -> int:
        """bytes of device workspace track_frames_s16 / _f32 need for these arguments (glv_batch_track_frames_work_bytes: the steps' float rows, the scan's where
        the chain keeps state, and with OP_BARS the frames' texel rows); raises on arguments the call refuses"""
        nbytes = int(lib().glv_batch_track_frames_work_bytes(self._h, steps, frames, ops))
        if nbytes == 0:
            msg = lib().glv_last_error().decode()
            raise GlvError(ERR_STATE if msg.startswith("GLV_ERR_STATE") else ERR_INVALID, msg)
        return nbytes

    def _track_frames(self, kind: str, d_pcm, pitch_frames, d_starts, d_ur, steps, d_from, d_to, d_mod, frames, d_keys, keep, d_out, d_work, ops, stream) -> None:
        fr = TrackFrames(_ptr(d_from), _ptr(d_to), _ptr(d_mod), frames, _ptr(d_keys), keep[0], keep[1])
        _check(getattr(lib(), f"glv_batch_track_frames_{kind}")(self._h, _ptr(d_pcm), pitch_frames, _ptr(d_starts), _ptr(d_ur), steps, C.byref(fr), _ptr(d_out),
                                                                 _ptr(d_work), ops, _ptr(stream)))

    def track_frames_s16(self, d_pcm, pitch_frames: int, d_starts, d_ur, steps: int, d_from, d_to, d_mod, frames: int, d_keys, keep: tuple[int, int], d_out, d_work,
                         ops: int, stream: int | None = None) -> None:
        """track mode at render frames on a gl_storage 3 batch (glv_batch_track_frames_s16): the `steps` updates of track_at_s16 (d_ur None) or track_rates_s16
        run and leave the batch exactly as those calls do; d_out then holds, frame-major, what a process call with `ops` would write for each of `frames`
        render frames if its finished float row were the frame's buffer -- keyframe d_from[j] itself where d_from[j] == d_to[j], else
        s + ((e - s) * d_mod[j]) of keyframes d_from[j] and d_to[j] in float32 (`setinterpolate true`).  Keyframes 0 and 1 are d_keys float32
        [2][streams][2][n] (zeros before a session's first call), keyframe 2 + t the finished float row of step t; afterwards d_keys holds keyframes
        keep[0] and keep[1], what the next call of the session starts from.  d_from / d_to uint32 [frames], d_mod float32 [frames], all in device memory;
        ops OP_FFT with OP_R16 and / or OP_BARS; d_work at least track_frames_work_bytes(steps, frames, ops) bytes, 256-byte aligned.  Tables:
        glava_amd.track_starts.keyframe_tables / live_session_frames.  Stream-ordered, kernels only; every table is read when the kernels run."""
        self._track_frames("s16", d_pcm, pitch_frames, d_starts, d_ur, steps, d_from, d_to, d_mod, frames, d_keys, keep, d_out, d_work, ops, stream)

    def track_frames_f32(self, d_pcm, pitch_frames: int, d_starts, d_ur, steps: int, d_from, d_to, d_mod, frames: int, d_keys, keep: tuple[int, int], d_out, d_work,
                         ops: int, stream: int | None = None) -> None:
        """track_frames_s16 from a float recording (glv_batch_track_frames_f32): d_pcm float32 [streams][pitch_frames][2], interleaved L R, 8-byte aligned"""
        self._track_frames("f32", d_pcm, pitch_frames, d_starts, d_ur, steps, d_from, d_to, d_mod, frames, d_keys, keep, d_out, d_work, ops, stream)

    def track_wave_frames_work_bytes(self, steps: int, frames: int, ops: int) -> int:
        """bytes of device workspace track_wave_frames_s16 / _f32 need for these arguments (glv_batch_track_wave_frames_work_bytes: 256 without OP_BARS, else the
        frames' rows as the bars kernel takes them); raises on arguments the call refuses"""
        nbytes = int(lib().glv_batch_track_wave_frames_work_bytes(self._h, steps, frames, ops))
        if nbytes == 0:
            msg = lib().glv_last_error().decode()
            raise GlvError(ERR_STATE if msg.startswith("GLV_ERR_STATE") else ERR_INVALID, msg)
        return nbytes

    def _track_wave_frames(self, kind: str, d_pcm, pitch_frames, d_starts, steps, d_from, d_to, d_mod, frames, d_keys, keep, d_out, d_work, ops, stream) -> None:
        fr = TrackFrames(_ptr(d_from), _ptr(d_to), _ptr(d_mod), frames, _ptr(d_keys), keep[0], keep[1])
        _check(getattr(lib(), f"glv_batch_track_wave_frames_{kind}")(self._h, _ptr(d_pcm), pitch_frames, _ptr(d_starts), steps, C.byref(fr), _ptr(d_out), _ptr(d_work),
                                                                      ops, _ptr(stream)))

    def track_wave_frames_s16(self, d_pcm, pitch_frames: int, d_starts, steps: int, d_from, d_to, d_mod, frames: int, d_keys, keep: tuple[int, int], d_out, d_work,
                              ops: int, stream: int | None = None) -> None:
        """track mode at render frames for the wave module, on any gl_storage (glv_batch_track_wave_frames_s16): d_out holds, frame-major, what a process call with
        `ops` (OP_WAVE [| OP_BARS] [| OP_R16]) would write for each of `frames` render frames if its wrange'd buffer were the frame's -- keyframe d_from[j] itself
        where d_from[j] == d_to[j], else s + ((e - s) * d_mod[j]) in float32 (`setinterpolate true`).  Keyframes 0 and 1 are d_keys float32 [2][streams][2][n]
        (zeros before a session's first call); keyframe 2 + t is (u + 1.0F) / 2.0F of the unpacked window that begins track_at_start(pitch_frames, n, d_starts[t])
        frames into each recording, read where it lies: `steps` keyframes, nothing computed per step.  Afterwards d_keys holds keyframes keep[0] and keep[1] as
        floats.  d_starts, d_from, d_to uint32, d_mod float32, all in device memory; d_work at least track_wave_frames_work_bytes(steps, frames, ops) bytes, 256-byte
        aligned.  Tables: glava_amd.track_starts.keyframe_tables / live_session_frames.  Stream-ordered, two kernels, three with OP_BARS."""
        self._track_wave_frames("s16", d_pcm, pitch_frames, d_starts, steps, d_from, d_to, d_mod, frames, d_keys, keep, d_out, d_work, ops, stream)

    def track_wave_frames_f32(self, d_pcm, pitch_frames: int, d_starts, steps: int, d_from, d_to, d_mod, frames: int, d_keys, keep: tuple[int, int], d_out, d_work,
                              ops: int, stream: int | None = None) -> None:
        """track_wave_frames_s16 from a float recording (glv_batch_track_wave_frames_f32): d_pcm float32 [streams][pitch_frames][2], interleaved L R, 8-byte aligned"""
        self._track_wave_frames("f32", d_pcm, pitch_frames, d_starts, steps, d_from, d_to, d_mod, frames, d_keys, keep, d_out, d_work, ops, stream)

    # ---- track mode from planar float recordings: a tensor [streams, 2, frames], the layout of process_f32's rows and of every channel-major decoder
    def track_at_f32_planar(self, rows, d_starts, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """track_at_f32 from a planar recording (glv_batch_track_at_f32_planar): `rows` a contiguous float32 tensor [streams, 2, frames] on the batch's device, any
        4-byte aligned view of one included (rows[..., 1:] is not contiguous; a flat buffer sliced from any float and viewed as [streams, 2, frames] is);
        pitch_frames is its last dimension.  Window t of stream s, channel c, begins min(d_starts[t], frames - bufscale * n) floats into rows[s, c].  No mono mix:
        the rows are taken as they are whatever Params.channels says, so step t is bit for bit what process_f32 on the window's two rows would have written.
        Forms, refusals, state and d_work (track_at_work_bytes) are track_at_f32's."""
        pitch = planar_pitch_frames(rows, self.streams)
        _check(lib().glv_batch_track_at_f32_planar(self._h, _ptr(rows), pitch, _ptr(d_starts), steps, _ptr(d_out), _ptr(d_work), ops, _ptr(stream)))

    def track_rates_f32_planar(self, rows, d_starts, d_ur, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """track_rates_f32 from a planar recording (glv_batch_track_rates_f32_planar); `rows` as track_at_f32_planar takes them"""
        pitch = planar_pitch_frames(rows, self.streams)
        _check(lib().glv_batch_track_rates_f32_planar(self._h, _ptr(rows), pitch, _ptr(d_starts), _ptr(d_ur), steps, _ptr(d_out), _ptr(d_work), ops, _ptr(stream)))

    def track_frames_f32_planar(self, rows, d_starts, d_ur, steps: int, d_from, d_to, d_mod, frames: int, d_keys, keep: tuple[int, int], d_out, d_work,
                                ops: int, stream: int | None = None) -> None:
        """track_frames_f32 from a planar recording (glv_batch_track_frames_f32_planar); `rows` as track_at_f32_planar takes them"""
        self._track_frames("f32_planar", rows, planar_pitch_frames(rows, self.streams), d_starts, d_ur, steps, d_from, d_to, d_mod, frames, d_keys, keep, d_out, d_work, ops, stream)

    def track_wave_frames_f32_planar(self, rows, d_starts, steps: int, d_from, d_to, d_mod, frames: int, d_keys, keep: tuple[int, int], d_out, d_work,
                                     ops: int, stream: int | None = None) -> None:
        """track_wave_frames_f32 from a planar recording (glv_batch_track_wave_frames_f32_planar); `rows` as track_at_f32_planar takes them"""
        self._track_wave_frames("f32_planar", rows, planar_pitch_frames(rows, self.streams), d_starts, steps, d_from, d_to, d_mod, frames, d_keys, keep, d_out, d_work, ops, stream)

    # ---- track mode per stream: a table row, a rate row and a count of steps for every stream of the batch
    def _track_each(self, kind: str, d_pcm, pitch_frames: int, d_starts, d_ur, d_counts, steps: int, d_out, d_work, ops: int, stream) -> None:
        tb = TrackTables(_ptr(d_starts), _ptr(d_ur), _ptr(d_counts))
        _check(getattr(lib(), "glv_batch_track_each_" + kind)(self._h, _ptr(d_pcm), pitch_frames, C.byref(tb), steps, _ptr(d_out), _ptr(d_work), ops, _ptr(stream)))

    def track_each_s16(self, d_pcm, pitch_frames: int, d_starts, d_ur, d_counts, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """track_at_s16 / track_rates_s16 with tables per stream (glv_batch_track_each_s16): d_starts uint32 [streams][steps], row s is stream s's table; d_ur
        float32 [streams][steps] or None (the batch's own ur at every step; not None: OP_GRAVITY and no OP_WAVE); d_counts uint32 [streams] or None (every stream
        takes all steps; not None: a chain with OP_GRAVITY and / or OP_AVERAGE).  Stream s runs its first c = min(d_counts[s], steps) steps as if alone in a batch
        with its own row; the rows of d_out behind c are what the call's last stage makes of a row of zeros; the batch's head advances by `steps` and every
        stream's ring is left where that head expects it, so the next call continues each bit for bit and a stream with count 0 keeps its state.  All three in
        device memory, read when the kernels run.  Forms, refusals, d_out and d_work (track_at_work_bytes) are track_at_s16's.
        Tables: glava_amd.track_starts.stack_tables."""
        self._track_each("s16", d_pcm, pitch_frames, d_starts, d_ur, d_counts, steps, d_out, d_work, ops, stream)

    def track_each_f32(self, d_pcm, pitch_frames: int, d_starts, d_ur, d_counts, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """track_each_s16 from a float recording (glv_batch_track_each_f32): d_pcm float32 [streams][pitch_frames][2], interleaved L R, 8-byte aligned"""
        self._track_each("f32", d_pcm, pitch_frames, d_starts, d_ur, d_counts, steps, d_out, d_work, ops, stream)

    def track_each_f32_planar(self, rows, d_starts, d_ur, d_counts, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """track_each_f32 from a planar recording (glv_batch_track_each_f32_planar); `rows` as track_at_f32_planar takes them, no mono mix"""
        self._track_each("f32_planar", rows, planar_pitch_frames(rows, self.streams), d_starts, d_ur, d_counts, steps, d_out, d_work, ops, stream)

    # ---- track mode over a pool of recordings: one buffer, a span per stream
    def _track_pool(self, kind: str, d_pool, pool_frames: int, d_spans, d_starts, d_ur, d_counts, steps: int, d_out, d_work, ops: int, stream) -> None:
        tb = TrackTables(_ptr(d_starts), _ptr(d_ur), _ptr(d_counts))
        _check(getattr(lib(), "glv_batch_track_pool_" + kind)(self._h, _ptr(d_pool), pool_frames, _ptr(d_spans), C.byref(tb), steps, _ptr(d_out), _ptr(d_work), ops,
                                                              _ptr(stream)))

    def track_pool_s16(self, d_pool, pool_frames: int, d_spans, d_starts, d_ur, d_counts, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """track_each_s16 over ONE buffer of recordings (glv_batch_track_pool_s16): d_pool int16 [pool_frames][2]; d_spans one TrackSpan (16 bytes: first uint64,
        frames uint32, a word never read) per stream in device memory, 16-byte aligned -- any number of streams may name the same span, overlapping spans or
        disjoint ones.  Window t of stream s begins at pool frame min(first[s] + min(d_starts[s][t], frames[s] - k n or 0), pool_frames - k n), evaluated in the
        kernels in 64-bit arithmetic (glava_amd.track_starts.pool_window_start): with well-formed spans no table moves a stream out of its own recording, with
        malformed ones no launch reads outside the pool.  Everything else -- tables, forms, refusals, state, d_out, d_work (track_at_work_bytes) -- is
        track_each_s16's, bit for bit on the materialised copy.  Spans: glava_amd.track_starts.pool_spans."""
        self._track_pool("s16", d_pool, pool_frames, d_spans, d_starts, d_ur, d_counts, steps, d_out, d_work, ops, stream)

    def track_pool_f32(self, d_pool, pool_frames: int, d_spans, d_starts, d_ur, d_counts, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """track_pool_s16 from a float pool (glv_batch_track_pool_f32): d_pool float32 [pool_frames][2], interleaved L R, 8-byte aligned"""
        self._track_pool("f32", d_pool, pool_frames, d_spans, d_starts, d_ur, d_counts, steps, d_out, d_work, ops, stream)

    def track_pool_f32_planar(self, d_rows, pool_frames: int, d_spans, d_starts, d_ur, d_counts, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """track_pool_f32 from a planar pool (glv_batch_track_pool_f32_planar): d_rows float32 [2][pool_frames], channel c of frame i at c * pool_frames + i,
        4-byte aligned, any pool_frames, no mono mix"""
        self._track_pool("f32_planar", d_rows, pool_frames, d_spans, d_starts, d_ur, d_counts, steps, d_out, d_work, ops, stream)

    # ---- track mode at render frames per stream: frame tables, a frame count and a keep pair for every stream, on the per-stream or the pool call's updates
    def _track_each_frames(self, kind: str, d_pcm, pitch_frames: int, tables, steps: int, frame_tables, frames: int, d_keys, d_out, d_work, ops: int, stream) -> None:
        tb = TrackTables(*(_ptr(t) for t in tables))
        fe = TrackFramesEach(*(_ptr(t) for t in frame_tables), frames, _ptr(d_keys))
        _check(getattr(lib(), "glv_batch_track_each_frames_" + kind)(self._h, _ptr(d_pcm), pitch_frames, C.byref(tb), steps, C.byref(fe), _ptr(d_out), _ptr(d_work), ops,
                                                                     _ptr(stream)))

    def track_each_frames_s16(self, d_pcm, pitch_frames: int, tables, steps: int, frame_tables, frames: int, d_keys, d_out, d_work, ops: int,
                              stream: int | None = None) -> None:
        """track_frames_s16 with everything per stream (glv_batch_track_each_frames_s16).  tables = (d_starts, d_ur, d_counts) as track_each_s16 takes them: the
        updates, state, head and refusals are that call's.  frame_tables = (d_from, d_to, d_mod, d_frame_counts, d_keep): uint32 / uint32 / float32
        [streams][frames], row s is stream s's; d_frame_counts uint32 [streams] or None (every stream takes all `frames`); d_keep uint32 [streams][2], the
        keyframes written back to d_keys[0] / d_keys[1] of each stream.  Every index is clamped on the device to c_s + 1, c_s = min(d_counts[s], steps); frames
        behind a stream's count are what the call's last stage makes of a zero texel row.  d_out [frames][streams][2][w]; d_work at least
        track_frames_work_bytes(steps, frames, ops) bytes.  Each stream is bit for bit track_frames_s16 on a one-stream batch.  OP_WAVE is refused.
        Tables: glava_amd.track_starts.stack_frame_tables."""
        self._track_each_frames("s16", d_pcm, pitch_frames, tables, steps, frame_tables, frames, d_keys, d_out, d_work, ops, stream)

    def track_each_frames_f32(self, d_pcm, pitch_frames: int, tables, steps: int, frame_tables, frames: int, d_keys, d_out, d_work, ops: int,
                              stream: int | None = None) -> None:
        """track_each_frames_s16 from a float recording (glv_batch_track_each_frames_f32): d_pcm float32 [streams][pitch_frames][2], interleaved L R, 8-byte aligned"""
        self._track_each_frames("f32", d_pcm, pitch_frames, tables, steps, frame_tables, frames, d_keys, d_out, d_work, ops, stream)

    def track_each_frames_f32_planar(self, rows, tables, steps: int, frame_tables, frames: int, d_keys, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """track_each_frames_f32 from a planar recording (glv_batch_track_each_frames_f32_planar); `rows` as track_at_f32_planar takes them, no mono mix"""
        self._track_each_frames("f32_planar", rows, planar_pitch_frames(rows, self.streams), tables, steps, frame_tables, frames, d_keys, d_out, d_work, ops, stream)

    def _track_pool_frames(self, kind: str, d_pool, pool_frames: int, d_spans, tables, steps: int, frame_tables, frames: int, d_keys, d_out, d_work, ops: int, stream) -> None:
        tb = TrackTables(*(_ptr(t) for t in tables))
        fe = TrackFramesEach(*(_ptr(t) for t in frame_tables), frames, _ptr(d_keys))
        _check(getattr(lib(), "glv_batch_track_pool_frames_" + kind)(self._h, _ptr(d_pool), pool_frames, _ptr(d_spans), C.byref(tb), steps, C.byref(fe), _ptr(d_out),
                                                                     _ptr(d_work), ops, _ptr(stream)))

    def track_pool_frames_s16(self, d_pool, pool_frames: int, d_spans, tables, steps: int, frame_tables, frames: int, d_keys, d_out, d_work, ops: int,
                              stream: int | None = None) -> None:
        """track_each_frames_s16 over ONE buffer of recordings (glv_batch_track_pool_frames_s16): d_pool, pool_frames and d_spans as track_pool_s16 takes them,
        everything else as track_each_frames_s16"""
        self._track_pool_frames("s16", d_pool, pool_frames, d_spans, tables, steps, frame_tables, frames, d_keys, d_out, d_work, ops, stream)

    def track_pool_frames_f32(self, d_pool, pool_frames: int, d_spans, tables, steps: int, frame_tables, frames: int, d_keys, d_out, d_work, ops: int,
                              stream: int | None = None) -> None:
        """track_pool_frames_s16 from a float pool (glv_batch_track_pool_frames_f32): d_pool float32 [pool_frames][2], interleaved L R, 8-byte aligned"""
        self._track_pool_frames("f32", d_pool, pool_frames, d_spans, tables, steps, frame_tables, frames, d_keys, d_out, d_work, ops, stream)

    def track_pool_frames_f32_planar(self, d_rows, pool_frames: int, d_spans, tables, steps: int, frame_tables, frames: int, d_keys, d_out, d_work, ops: int,
                                     stream: int | None = None) -> None:
        """track_pool_frames_f32 from a planar pool (glv_batch_track_pool_frames_f32_planar): d_rows float32 [2][pool_frames], 4-byte aligned, no mono mix"""
        self._track_pool_frames("f32_planar", d_rows, pool_frames, d_spans, tables, steps, frame_tables, frames, d_keys, d_out, d_work, ops, stream)

    # ---- ... for the wave module: keyframes read from each stream's own windows of its recording, or of its span of a pool
    def _track_each_wave_frames(self, kind: str, d_pcm, pitch_frames: int, tables, steps: int, frame_tables, frames: int, d_keys, d_out, d_work, ops: int, stream) -> None:
        tb = TrackTables(*(_ptr(t) for t in tables))
        fe = TrackFramesEach(*(_ptr(t) for t in frame_tables), frames, _ptr(d_keys))
        _check(getattr(lib(), "glv_batch_track_each_wave_frames_" + kind)(self._h, _ptr(d_pcm), pitch_frames, C.byref(tb), steps, C.byref(fe), _ptr(d_out), _ptr(d_work),
                                                                          ops, _ptr(stream)))

    def track_each_wave_frames_s16(self, d_pcm, pitch_frames: int, tables, steps: int, frame_tables, frames: int, d_keys, d_out, d_work, ops: int,
                                   stream: int | None = None) -> None:
        """track_wave_frames_s16 with everything per stream (glv_batch_track_each_wave_frames_s16).  tables = (d_starts, None, d_counts): d_starts uint32
        [streams][steps], row s is stream s's; no rate table; d_counts uint32 [streams] or None -- stream s contributes its first c_s = min(d_counts[s], steps)
        windows as keyframes 2 .. c_s + 1.  frame_tables = (d_from, d_to, d_mod, d_frame_counts, d_keep) as track_each_frames_s16 takes them.  Every index is
        clamped on the device to c_s + 1; a stream with c_s = 0 lerps between its two carried keyframes; frames behind a stream's count are what the call's last
        stage makes of a zero texel row.  ops OP_WAVE [| OP_BARS] [| OP_R16]; d_out [frames][streams][2][w]; d_work at least
        track_wave_frames_work_bytes(steps, frames, ops) bytes.  Each stream is bit for bit track_wave_frames_s16 on a one-stream batch.
        Tables: glava_amd.track_starts.stack_tables and stack_frame_tables."""
        self._track_each_wave_frames("s16", d_pcm, pitch_frames, tables, steps, frame_tables, frames, d_keys, d_out, d_work, ops, stream)

    def track_each_wave_frames_f32(self, d_pcm, pitch_frames: int, tables, steps: int, frame_tables, frames: int, d_keys, d_out, d_work, ops: int,
                                   stream: int | None = None) -> None:
        """track_each_wave_frames_s16 from a float recording (glv_batch_track_each_wave_frames_f32): d_pcm float32 [streams][pitch_frames][2], 8-byte aligned"""
        self._track_each_wave_frames("f32", d_pcm, pitch_frames, tables, steps, frame_tables, frames, d_keys, d_out, d_work, ops, stream)

    def track_each_wave_frames_f32_planar(self, rows, tables, steps: int, frame_tables, frames: int, d_keys, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """track_each_wave_frames_f32 from a planar recording (glv_batch_track_each_wave_frames_f32_planar); `rows` as track_at_f32_planar takes them, no mono mix"""
        self._track_each_wave_frames("f32_planar", rows, planar_pitch_frames(rows, self.streams), tables, steps, frame_tables, frames, d_keys, d_out, d_work, ops, stream)

    def _track_pool_wave_frames(self, kind: str, d_pool, pool_frames: int, d_spans, tables, steps: int, frame_tables, frames: int, d_keys, d_out, d_work, ops: int,
                                stream) -> None:
        tb = TrackTables(*(_ptr(t) for t in tables))
        fe = TrackFramesEach(*(_ptr(t) for t in frame_tables), frames, _ptr(d_keys))
        _check(getattr(lib(), "glv_batch_track_pool_wave_frames_" + kind)(self._h, _ptr(d_pool), pool_frames, _ptr(d_spans), C.byref(tb), steps, C.byref(fe), _ptr(d_out),
                                                                          _ptr(d_work), ops, _ptr(stream)))

    def track_pool_wave_frames_s16(self, d_pool, pool_frames: int, d_spans, tables, steps: int, frame_tables, frames: int, d_keys, d_out, d_work, ops: int,
                                   stream: int | None = None) -> None:
        """track_each_wave_frames_s16 over ONE buffer of recordings (glv_batch_track_pool_wave_frames_s16): d_pool, pool_frames and d_spans as track_pool_s16 takes
        them, everything else as track_each_wave_frames_s16"""
        self._track_pool_wave_frames("s16", d_pool, pool_frames, d_spans, tables, steps, frame_tables, frames, d_keys, d_out, d_work, ops, stream)

    def track_pool_wave_frames_f32(self, d_pool, pool_frames: int, d_spans, tables, steps: int, frame_tables, frames: int, d_keys, d_out, d_work, ops: int,
                                   stream: int | None = None) -> None:
        """track_pool_wave_frames_s16 from a float pool (glv_batch_track_pool_wave_frames_f32): d_pool float32 [pool_frames][2], interleaved L R, 8-byte aligned"""
        self._track_pool_wave_frames("f32", d_pool, pool_frames, d_spans, tables, steps, frame_tables, frames, d_keys, d_out, d_work, ops, stream)

    def track_pool_wave_frames_f32_planar(self, d_rows, pool_frames: int, d_spans, tables, steps: int, frame_tables, frames: int, d_keys, d_out, d_work, ops: int,
                                          stream: int | None = None) -> None:
        """track_pool_wave_frames_f32 from a planar pool (glv_batch_track_pool_wave_frames_f32_planar): d_rows float32 [2][pool_frames], 4-byte aligned, no mono mix"""
        self._track_pool_wave_frames("f32_planar", d_rows, pool_frames, d_spans, tables, steps, frame_tables, frames, d_keys, d_out, d_work, ops, stream)

    def track_wave_work_bytes(self, pitch_frames: int, hop: int, steps: int, ops: int) -> int:
        """bytes of device workspace track_wave_s16 needs for these arguments (glv_batch_track_wave_work_bytes; 256 where the call needs none); raises on
        arguments the call refuses"""
        return self._track_work_bytes("track_wave", pitch_frames, hop, steps, ops)

    def track_wave_s16(self, d_pcm, pitch_frames: int, hop: int, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """the wave module's texture of `steps` consecutive updates of every stream from one long buffer (glv_batch_track_wave_s16): d_pcm int16
        [streams][pitch_frames][2], window t of stream s = its frames [t * hop, t * hop + n), any hop >= 1; ops OP_WAVE [| OP_BARS] [| OP_R16]; d_out
        step-major, step t bit for bit what process_s16 on window t would have written; d_work at least track_wave_work_bytes(...) bytes, 256-byte
        aligned.  Stateless; stream-ordered, kernels only."""
        self._track_call("track_wave", d_pcm, pitch_frames, hop, steps, d_out, d_work, ops, stream)

    def track_wave_f32(self, d_pcm, pitch_frames: int, hop: int, steps: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """track_wave_s16 from a float recording (glv_batch_track_wave_f32): d_pcm float32 [streams][pitch_frames][2], 8-byte aligned; step t bit for
        bit what process_f32_stereo on window t would have written; d_work at least track_wave_work_bytes(...) bytes (the same query).  With OP_BARS
        always two launches."""
        self._track_call("track_wave", d_pcm, pitch_frames, hop, steps, d_out, d_work, ops, stream, "f32")

    def ring_update_s16(self, d_new, new_frames: int, d_out, ops: int = OP_FFT, stream: int | None = None) -> None:
        _check(lib().glv_batch_ring_update_s16(self._h, _ptr(d_new), new_frames, _ptr(d_out), ops, _ptr(stream)))

    def gravity_state(self) -> int:
        """device address of the gravity state float [streams][2][n] (the spectra when d_out is None)"""
        p = C.c_void_p()
        _check(lib().glv_batch_gravity_state(self._h, C.byref(p)))
        return int(p.value)

    def ring_update_f32(self, d_new, new_frames: int, d_out, ops: int = OP_FFT, stream: int | None = None) -> None:
        _check(lib().glv_batch_ring_update_f32(self._h, _ptr(d_new), new_frames, _ptr(d_out), ops, _ptr(stream)))

    def ring_append_s16(self, d_new, new_frames: int, stream: int | None = None) -> None:
        _check(lib().glv_batch_ring_append_s16(self._h, _ptr(d_new), new_frames, _ptr(stream)))

    def ring_append_f32(self, d_new, new_frames: int, stream: int | None = None) -> None:
        _check(lib().glv_batch_ring_append_f32(self._h, _ptr(d_new), new_frames, _ptr(stream)))

    def ring_planar(self, d_planar, f32_ring: bool = False, stream: int | None = None) -> None:
        """the ring as the reference's backends publish it: float [streams][2][n], oldest sample first"""
        _check(lib().glv_batch_ring_planar(self._h, int(f32_ring), _ptr(d_planar), _ptr(stream)))

    def ring_track_work_bytes(self, new_frames: int, updates: int, ops: int) -> int:
        """bytes of device workspace ring_track_s16 / _f32 need for these arguments (glv_batch_ring_track_work_bytes: the staged recordings, the table of
        starts, and what track_at_work_bytes(updates, ops) reports); raises on arguments the call refuses"""
        nbytes = int(lib().glv_batch_ring_track_work_bytes(self._h, new_frames, updates, ops))
        if nbytes == 0:
            msg = lib().glv_last_error().decode()
            raise GlvError(ERR_STATE if msg.startswith("GLV_ERR_STATE") else ERR_INVALID, msg)
        return nbytes

    def ring_track_s16(self, d_new, new_frames: int, updates: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """`updates` ring updates of new_frames frames each in one track call (glv_batch_ring_track_s16): d_new int16 [streams][updates * new_frames][2], each
        stream's new frames back to back (None: zero fill); d_out [updates][streams * 2][row] as track_at_s16 lays it out for the batch and ops; d_work at
        least ring_track_work_bytes(...) bytes, 256-byte aligned.  Output, state and rings bit for bit those of `updates` ring_update_s16 calls."""
        _check(lib().glv_batch_ring_track_s16(self._h, _ptr(d_new), new_frames, updates, _ptr(d_out), _ptr(d_work), ops, _ptr(stream)))

    def ring_track_f32(self, d_new, new_frames: int, updates: int, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """ring_track_s16 on the interleaved f32 ring (glv_batch_ring_track_f32): d_new float32 [streams][updates * new_frames][2], 8-byte aligned, never None"""
        _check(lib().glv_batch_ring_track_f32(self._h, _ptr(d_new), new_frames, updates, _ptr(d_out), _ptr(d_work), ops, _ptr(stream)))

    def ring_track_each_work_bytes(self, new_frames: int, updates: int, ops: int) -> int:
        """bytes of device workspace ring_track_each_s16 / _f32 need for these arguments (glv_batch_ring_track_each_work_bytes: the staged recordings, a row
        of starts per stream, and what track_at_work_bytes(updates, ops) reports); raises on arguments the call refuses"""
        nbytes = int(lib().glv_batch_ring_track_each_work_bytes(self._h, new_frames, updates, ops))
        if nbytes == 0:
            msg = lib().glv_last_error().decode()
            raise GlvError(ERR_STATE if msg.startswith("GLV_ERR_STATE") else ERR_INVALID, msg)
        return nbytes

    def ring_track_each_s16(self, d_new, new_frames: int, updates: int, d_ur, d_counts, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """ring_track_s16 with a count of updates and a row of rates per stream (glv_batch_ring_track_each_s16): stream s takes its first c = min(d_counts[s],
        updates) updates -- d_counts uint32 [streams] or None (everybody takes all) -- and update t of it applies gravity with d_ur[s * updates + t], d_ur
        float32 [streams][updates] or None (the batch's own ur), both in device memory and read when the kernels run.  d_new int16 [streams][updates *
        new_frames][2] (None: zero fill): of stream s only the first c * new_frames frames are read.  d_out [updates][streams * 2][row] as track_each_s16 lays
        it out: the rows behind a count are what the call's last stage makes of a row of zeros.  Every stream is left, bit for bit, as c ring_update_s16
        calls leave a one-stream batch at its state; a stream with count 0 keeps state and ring.  OP_WAVE is refused (ring_track_s16 takes it).  d_work at
        least ring_track_each_work_bytes(...) bytes, 256-byte aligned.  Counts: glava_amd.track_starts.ring_update_counts."""
        _check(lib().glv_batch_ring_track_each_s16(self._h, _ptr(d_new), new_frames, updates, _ptr(d_ur), _ptr(d_counts), _ptr(d_out), _ptr(d_work), ops, _ptr(stream)))

    def ring_track_each_f32(self, d_new, new_frames: int, updates: int, d_ur, d_counts, d_out, d_work, ops: int, stream: int | None = None) -> None:
        """ring_track_each_s16 on the interleaved f32 ring (glv_batch_ring_track_each_f32): d_new float32 [streams][updates * new_frames][2], 8-byte aligned,
        never None"""
        _check(lib().glv_batch_ring_track_each_f32(self._h, _ptr(d_new), new_frames, updates, _ptr(d_ur), _ptr(d_counts), _ptr(d_out), _ptr(d_work), ops, _ptr(stream)))

    def bars(self, d_spec, d_bars, stream: int | None = None) -> None:
        _check(lib().glv_batch_bars(self._h, _ptr(d_spec), _ptr(d_bars), _ptr(stream)))

    def set_bar_texels(self, texels) -> None:
        """GLV_OP_BARS at texels of the pre-smoothed texture (glv_batch_set_bar_texels): bar k = texel texels[k] of the
        pre-smoothing pass (bars = n, bar_phase 0.5); None / empty turns it off.  glava_amd.bar_positions computes the
        texels the shipped modules sample."""
        if texels is None or len(texels) == 0:
            _check(lib().glv_batch_set_bar_texels(self._h, None, 0))
            return
        t = np.ascontiguousarray(np.asarray(texels, dtype=np.int64))
        if t.ndim != 1 or (t < 0).any() or (t >= 1 << 32).any():
            raise ValueError("texels: a 1-d list of non-negative 32-bit indices")
        t = t.astype(np.uint32)
        _check(lib().glv_batch_set_bar_texels(self._h, t.ctypes.data_as(C.c_void_p), len(t)))

    def set_column_texels(self, table) -> None:
        """GLV_OP_BARS as the graph module's columns (glv_batch_set_column_texels): column x = the float mean of texels
        table[x] = (left, middle, right) of the pre-smoothing pass, (T(l) + T(m) + T(r)) / 3 in the shader's float order;
        None / empty turns it off.  glava_amd.bar_positions.graph_column_texels computes the table of a window width."""
        if table is None or len(table) == 0:
            _check(lib().glv_batch_set_column_texels(self._h, None, 0))
            return
        t = np.ascontiguousarray(np.asarray(table, dtype=np.int64))
        if t.ndim != 2 or t.shape[1] != 3 or (t < 0).any() or (t >= 1 << 32).any():
            raise ValueError("table: [count][3] non-negative 32-bit indices (left, middle, right)")
        t = np.ascontiguousarray(t.astype(np.uint32))
        _check(lib().glv_batch_set_column_texels(self._h, t.ctypes.data_as(C.c_void_p), t.shape[0]))

    def reset(self) -> None:
        _check(lib().glv_batch_reset(self._h))

    def timing_begin(self) -> None:
        _check(lib().glv_batch_timing_begin(self._h))

    def timing_end(self) -> tuple[float, int]:
        ms, n = C.c_double(0), C.c_uint64(0)
        _check(lib().glv_batch_timing_end(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def live_bins(self) -> int:
        return int(lib().glv_batch_live_bins(self._h))

    def bars_arithmetic(self) -> int:
        """BARS_NONE / BARS_F32_CHAIN / BARS_F32_MATRIX / BARS_I8_EXACT (include/glv_spectrum.h glv_batch_bars_arithmetic)"""
        return int(lib().glv_batch_bars_arithmetic(self._h))

    def algorithmic_bytes(self, ops: int, input_is_s16: bool = True) -> int:
        return int(lib().glv_batch_algorithmic_bytes(self._h, ops, int(input_is_s16)))

    def kernel_name(self) -> str:
        return lib().glv_batch_kernel_name(self._h).decode()

    def set_grid(self, grid: int) -> None:
        """workgroups of every frame-kernel launch of this batch (glv_batch_set_grid); grid <= 0: automatic.  The result does not depend on it."""
        _check(lib().glv_batch_set_grid(self._h, grid))

    def last_grid(self) -> int:
        return int(lib().glv_batch_last_grid(self._h))

    def last_launches(self) -> int:
        """kernels the last process / ring-update call launched"""
        return int(lib().glv_batch_last_launches(self._h))

    def variants(self) -> int:
        """kernel configurations built for this size (glv_inst.hip Tuned<K, V>)"""
        return int(lib().glv_batch_variants(self._h))

    def set_variant(self, variant: int) -> None:
        _check(lib().glv_batch_set_variant(self._h, variant))

    def last_variant(self) -> int:
        return int(lib().glv_batch_last_variant(self._h))

    def window_selftest(self) -> tuple[int, int]:
        """(mismatches, shifted): every (s16 sample value, window position) pair of this size, float-pair product against the
        reference's fp64 product, on the device; positions whose low part was moved to make the identity hold"""
        m, sh = C.c_ulonglong(0), C.c_int(0)
        _check(lib().glv_batch_window_selftest(self._h, C.byref(m), C.byref(sh)))
        return int(m.value), int(sh.value)

    def describe_variant(self, variant: int) -> str:
        buf = C.create_string_buffer(256)
        _check(lib().glv_batch_describe_variant(self._h, variant, buf, len(buf)))
        return buf.value.decode()

    def autotune(self, d_pcm, d_out, ops: int = OP_FFT, stream: int | None = None) -> tuple[int, float]:
        """time the candidate workgroup counts on the device, record the winner in the process-wide wisdom"""
        g, ms = C.c_int(0), C.c_float(0)
        _check(lib().glv_batch_autotune(self._h, _ptr(d_pcm), _ptr(d_out), ops, _ptr(stream), C.byref(g), C.byref(ms)))
        return g.value, ms.value

    def tune_placement(self, d_pcm, d_out, ops: int, candidates: int = 6, stream: int | None = None) -> tuple[float, float]:
        """placement wisdom (include/glv_spectrum.h glv_batch_tune_placement): keep the fastest of `candidates` placements of the state arrays
        for THESE buffers; resets the state.  Returns (ms per update of the placement it had, of the one it has now)"""
        f, b = C.c_float(0), C.c_float(0)
        _check(lib().glv_batch_tune_placement(self._h, _ptr(d_pcm), _ptr(d_out), ops, candidates, _ptr(stream), C.byref(f), C.byref(b)))
        return f.value, b.value

    def close(self) -> None:
        if self._h:
            lib().glv_batch_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def track_residues(n: int, hop: int, pitch_frames: int, streams: int, steps: int) -> list[int]:
    """Windows K_r of the n / hop transform launches of a track call (include/glv_spectrum.h glv_batch_track_s16): launch r transforms the
    back-to-back windows that start at frame r * hop + k * n, k < K_r, of the sequence that ends with the last window of the last stream."""
    frames = (streams - 1) * pitch_frames + (steps - 1) * hop + n
    return [(frames - r * hop) // n for r in range(n // hop)]


def track_window(n: int, hop: int, pitch_frames: int, s: int, t: int) -> tuple[int, int]:
    """(r, k): window t of stream s of a track call is row k of transform launch r"""
    start = s * pitch_frames + t * hop
    return (start % n) // hop, start // n


def track_window_start(pitch_frames: int, hop: int, s: int, t: int) -> int:
    """first frame (of the whole [streams][pitch_frames] buffer) of window t of stream s of a track call"""
    return s * pitch_frames + t * hop


def track_at_start(pitch_frames: int, n: int, start: int) -> int:
    """Where a window whose table entry is `start` begins in its stream's recording (glava_amd/csrc/glv_frame.h track_window_start with a table; the wave
    kernel's wave_window_start): the kernels clamp the entry to pitch_frames - n, so the window lies inside the recording whatever the table holds."""
    if pitch_frames < n or not 0 <= start < 1 << 32:
        raise ValueError("pitch_frames >= n and a uint32 start")
    return min(start, pitch_frames - n)


def track_windows_rows(streams: int, steps: int, step_major: bool) -> list[int]:
    """The transform launch of glv_batch_track_windows_s16 (glava_amd/csrc/glv_frame.h TrackWindows): the kernel enumerates frames stream-major,
    f = s * steps + t; entry f is the channel-0 row frame f writes (channel 1: the next row) -- 2 f (stream-major: what the scan over time reads) or
    (t * streams + s) * 2 (step_major: what d_out and the bars pass take)."""
    return [(t * streams + s) * 2 if step_major else (s * steps + t) * 2 for s in range(streams) for t in range(steps)]


def track_wave_rows(n: int, hop: int, pitch_frames: int, streams: int, steps: int) -> list[int]:
    """First frame (of the whole [streams][pitch_frames] buffer) of every output row of a wave track call (include/glv_spectrum.h
    glv_batch_track_wave_s16): row t * streams * 2 + 2 s + c is channel c of the n frames from s * pitch_frames + t * hop on."""
    if hop < 1 or steps < 1 or pitch_frames < n + (steps - 1) * hop:
        raise ValueError("hop >= 1, steps >= 1 and pitch_frames >= n + (steps - 1) * hop")
    return [s * pitch_frames + t * hop for t in range(steps) for s in range(streams) for _ in range(2)]


def multi_shard_range(total_streams: int, rank: int, world: int) -> tuple[int, int]:
    """(first, count) of rank's contiguous shard -- the C twin of glava_amd.sharding.shard_range"""
    lo, cnt = C.c_uint64(0), C.c_uint64(0)
    lib().glv_multi_shard_range(total_streams, rank, world, C.byref(lo), C.byref(cnt))
    return int(lo.value), int(cnt.value)


class Multi:
    """One host, several GPUs (glv_multi): contiguous shards, one host thread per device, RCCL only for the stats."""

    def __init__(self, params: Params, total_streams: int, ops_mask: int = OP_FFT, devices: list[int] | None = None, ndev: int | None = None):
        self._h = C.c_void_p(None)
        cp = params.c()
        n = len(devices) if devices is not None else (1 if ndev is None else int(ndev))
        arr = (C.c_int * max(n, 1))(*devices) if devices is not None else None
        _check(lib().glv_multi_create(C.byref(cp), total_streams, ops_mask, arr, n, C.byref(self._h)))
        self.ndev = n

    def uses_rccl(self) -> bool:
        return bool(lib().glv_multi_uses_rccl(self._h))

    def shard(self, idx: int) -> tuple[int, int, int]:
        dev, lo, cnt = C.c_int(0), C.c_uint64(0), C.c_uint32(0)
        _check(lib().glv_multi_shard(self._h, idx, C.byref(dev), C.byref(lo), C.byref(cnt), None))
        return dev.value, int(lo.value), int(cnt.value)

    def run_s16(self, d_pcm: list, d_out: list, ops: int, warmup: int, steps: int) -> tuple[list[dict], float]:
        pin = (C.c_void_p * self.ndev)(*[_ptr(x) for x in d_pcm])
        pout = (C.c_void_p * self.ndev)(*[_ptr(x) for x in d_out])
        st = (MultiStats * self.ndev)()
        mx = C.c_double(0)
        _check(lib().glv_multi_run_s16(self._h, pin, pout, ops, warmup, steps, st, C.byref(mx)))
        return [{"frames": s.frames, "seconds": s.seconds, "bytes": s.bytes, "kernel_ms": s.kernel_ms} for s in st], mx.value

    def close(self) -> None:
        if self._h:
            lib().glv_multi_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class State:
    """Per-(stream, channel) state behind the single-buffer drop-ins (glv_state): the
    replacement for the `*udata` slot of the reference's operator seam (render.c:106-118)."""

    def __init__(self, params: Params, device: int = 0):
        self.params = params
        self._h = C.c_void_p(None)
        cp = params.c()
        _check(lib().glv_state_create(C.byref(cp), device, C.byref(self._h)))

    def _call(self, name: str, buf) -> None:
        cp = self.params.c()
        _check(getattr(lib(), name)(C.byref(cp), self._h, _ptr(buf)))

    def fft(self, buf) -> None: self._call("glv_fft", buf)                 # transform_fft
    def gravity(self, buf) -> None: self._call("glv_gravity", buf)         # transform_gravity
    def average(self, buf) -> None: self._call("glv_average", buf)         # transform_average
    def wrange(self, buf) -> None: self._call("glv_wrange", buf)           # transform_wrange
    def smooth(self, buf) -> None: self._call("glv_smooth", buf)           # transform_smooth
    def magnitude(self, buf) -> None: self._call("glv_magnitude", buf)     # tail of transform_fft
    def fft_gravity_average(self, buf) -> None: self._call("glv_fft_gravity_average", buf)

    def texels_r16(self, buf, texels) -> None:
        """the GL_R16 texels handle_audio's upload stores for buf (render.c:521-524); host buffers"""
        cp = self.params.c()
        _check(lib().glv_texels_r16(C.byref(cp), self._h, _ptr(buf), _ptr(texels)))

    def gl_texture(self, buf, texels, smooth_pass: bool = True) -> None:
        """handle_audio's accel_fft branch from the per-frame transform_fft to the texture the module samples (render.c:2176-2303);
        host buffers: n float samples in (not modified), n GL_R16 texels out; the state must have gl_storage = 1"""
        cp = self.params.c()
        _check(lib().glv_gl_texture(C.byref(cp), self._h, _ptr(buf), 1 if smooth_pass else 0, _ptr(texels)))

    def wave_texture(self, buf, texels, smooth_pass: bool = True) -> None:
        """handle_audio for the wave module's bind (transforms window, wrange): transform_wrange, the GL_R16 upload and -- smooth_pass --
        the pre-smoothing pass (render.c:773-781, :521-524, :2276-2303); host buffers: n floats of lb / rb in (not modified), n GL_R16
        texels out; the pass needs a state with gl_storage = 1, bars = n, bar_phase = 0.5"""
        cp = self.params.c()
        _check(lib().glv_wave_texture(C.byref(cp), self._h, _ptr(buf), 1 if smooth_pass else 0, _ptr(texels)))

    def reset(self) -> None:
        _check(lib().glv_state_reset(self._h))

    def close(self) -> None:
        if self._h:
            lib().glv_state_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def unpack_s16(pcm, frames: int, channels, l, r, device: int = 0) -> None:
    """fifo.c:94-110 on the device; host numpy buffers in/out."""
    _check(lib().glv_unpack_s16(device, _ptr(pcm), frames, channels, _ptr(l), _ptr(r)))


def prelude_bufscale(d_in, d_out, rows: int, n_out: int, k: int, device: int = 0, stream: int | None = None) -> None:
    """render.c:1768-1781 box decimation on device buffers."""
    _check(lib().glv_prelude_bufscale(device, _ptr(d_in), _ptr(d_out), rows, n_out, k, _ptr(stream)))


def prelude_lerp(d_start, d_end, d_out, count: int, uratio: float, kcounter: int, device: int = 0,
                 stream: int | None = None) -> None:
    """render.c:1794-1809 keyframe interpolation on device buffers."""
    _check(lib().glv_prelude_lerp(device, _ptr(d_start), _ptr(d_end), _ptr(d_out), count, uratio, kcounter, _ptr(stream)))


def wisdom_save(path: str) -> None: _check(lib().glv_wisdom_save(path.encode()))
def wisdom_load(path: str) -> None: _check(lib().glv_wisdom_load(path.encode()))
def wisdom_clear() -> None: lib().glv_wisdom_clear()
def wisdom_count() -> int: return int(lib().glv_wisdom_count())


def device_count() -> int:
    return int(lib().glv_device_count())
