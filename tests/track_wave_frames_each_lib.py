"""The rule of a per-stream wave frames call (glv_batch_track_each_wave_frames_* / glv_batch_track_pool_wave_frames_*) restated in numpy: a plain module, like
track_frames_each_lib.py, whose clamp_each / lerp_each / keep_each it reuses as they are -- the clamp to c_s + 1, the lerp and the write-back do not care where
a keyframe comes from.  What the wave form adds is the keyframes themselves: keyframe 2 + t of stream s is np_keyframes (tests/test_track_wave_frames_host.py,
pinned there to the oracle's unpack and the reference's wrange) of the window of ITS step t in ITS recording, and a step behind the stream's count has no
keyframe at all -- `rows_each` fills those rows with NaN, which lerp_each's own assertion never lets a clamped index reach.

Shared by tests/test_track_wave_frames_each_host.py (hand-computed cases) and tests/test_track_wave_frames_each.py (the kernels)."""
import numpy as np

from glava_amd.track_starts import pool_window_start
from test_track_wave_frames_host import np_keyframes
from track_frames_each_lib import clamp_each, keep_each, lerp_each  # noqa: F401  (part of this module's interface)

F32 = np.float32


def each_starts(starts, pitch_frames, n):
    """[streams][steps] frames into each stream's own recording: min(entry, pitch_frames - n)"""
    return np.minimum(np.asarray(starts, dtype=np.uint64), np.uint64(pitch_frames - n)).astype(np.int64)


def pool_starts(spans, starts, pool_frames, n):
    """[streams][steps] pool frames: the kernels' rule (glava_amd.track_starts.pool_window_start) for stream s's span (first, frames) and its entries"""
    return np.asarray([[pool_window_start(int(first), int(frames), int(e), int(pool_frames), n) for e in row] for (first, frames), row in zip(spans, starts)], dtype=np.int64)


def rows_each(recordings, where, counts, n, f32, channels):
    """float32 [steps][streams * 2][n]: keyframe 2 + t of every stream.  recordings: one [pitch][2] host array per stream (any may be the same array: a pool);
    where: [streams][steps] absolute first frames, already clamped; counts [streams] or None.  Rows of steps behind a stream's count are NaN"""
    where = np.asarray(where, dtype=np.int64)
    streams, steps = where.shape
    counts = [steps] * streams if counts is None else [min(int(c), steps) for c in counts]
    out = np.full((steps, streams * 2, n), np.nan, dtype=F32)
    for s in range(streams):
        if counts[s]:
            out[:counts[s], 2 * s:2 * s + 2] = np_keyframes(np.asarray(recordings[s])[None], [int(a) for a in where[s, :counts[s]]], n, f32, channels)
    return out
