"""The shapes, the caps and the per-stream variety of tests/test_track_each_launch_geometry.py: a plain module, like track_lib.py (default collection does not
pick it up; torch is imported inside the functions).

Everything a stream is handed in those tests is a function of its index, with periods (5, 6, 7, 9, 11, 13, 17) that do not divide 4096 or 8192: two streams on
either side of a trip boundary never agree by accident, and an item number truncated to 12 or 13 bits names a stream with other counts, other tables, another
keep pair and another recording.  `plant` names the streams that are handed another stream's index on purpose: the planted copies."""
import numpy as np

from track_lib import rec

F32 = np.float32
BIG = 0xFFFFFFFF
N = 256
SPEC, WAVE, SMALL = 4100, 8200, 6

# ---- the caps, restated next to the file and the constant they come from ------------------------------------------------------------------------------------
K_GRID_CAP = 256 * 8              # glv_launch_util.h kGridCap: workgroups of 256 lanes of glv_wave_kernel / glv_wave_pool_kernel (glv_misc.hip, glv_pool.hip) and of
                                  # the write-backs glv_track_keys[_each]_kernel, glv_wave_keys[_planar|_each]_kernel (glv_track_frames.hip)
K_DECIMATE_GRID_CAP = 256 * 8     # glv_launch.h kDecimateGridCap: workgroups of 256 lanes of glv_decimate_kernel (glv_decimate.hip) and glv_decimate_pool_kernel (glv_pool.hip)
K_FRAMES_GRID_CAP = 256 * 32      # glv_track_frames.hip kFramesGridCap: workgroups of ONE work item each of the six frames kernels
LANES = 256                       # ... the lanes of a workgroup of the first two groups, one work item each: four floats of a row (the write-backs and the
                                  # decimation: n / 4 items a row or a window), a group of 8 frames (wave)
WAVE_GROUP = 8                   # glv_misc.hip glv_wave_kernel: one lane per group of 8 frames
WAVE_LIMIT_MIN = 64               # glv_chain.cpp plan_wave: in front of the bars the waveform stops at bins_needed, a whole multiple of 64 bins
FRAMES_LANES = 64                 # glv_track_frames.hip kFramesLanes: a work item is one wave, 64 lanes x 4 bins = one row of n = 256
ROWS_PER_BLOCK = 64               # glv_bars.hip: 64 rows per workgroup of glv_bars_rows_i8_kernel
# update rates a session meets, none of which empties a row for good (a rate of 0 makes the step infinite, and rows that are -inf or 0 in every stream compare equal
# whatever was read): the float chains' (tests/test_track_frames.py, tests/track_rates_lib.py) and the texel chain's, whose step is 100.5 / ur texels
FLOAT_RATES = [1.0, 59.0, 60.0, 86.1328125, 61.0, 40.5, 29.032258987426758]
TEXEL_RATES = [1.0, 0.5, 3.0, 0.25, 1e6, float(np.float32(1) / np.float32(3)), 2.0]

SPEC_STEPS, SPEC_FRAMES, SEGMENT = 3, 7, 4      # segments of 4 and 3 frames: the second one ragged, rest / units = 1 in it
WAVE_STEPS, WAVE_BARS_STEPS = 3, 9
SOURCE = 35                                     # the stream whose recording, rows, counts and keyframes are planted (it runs every step and shows every frame) ...
SPEC_COPIES = (2046, 2050, 2728, 2732, 4094, 4097)      # ... on both sides of stream 2048, of stream 2730 and of stream 4096
WAVE_COPIES = (2728, 2732, 4094, 4097, 8190, 8193)      # ... of stream 2730, of stream 4096 and of stream 8192


def decimate_boundary_stream(steps):
    """the stream in which window 8192 of the [stream][step] order falls: where the decimation stage's second trip begins"""
    return K_DECIMATE_GRID_CAP * LANES // (N // 4) // steps


def small_batches(streams, boundary, steps=SPEC_STEPS):
    """the first streams of the four small batches: the first six, the last six, the six that straddle the write-back's trip boundary, the six around the
    decimation boundary"""
    return (0, streams - SMALL, boundary - 3, decimate_boundary_stream(steps) - 3)


# ---- per-stream variety ----------------------------------------------------------------------------------------------------------------------------------------
def plant(streams, copies, source=SOURCE):
    """int64 [streams]: the index every per-stream function below is evaluated at -- a stream's own, or for a planted copy the source's"""
    idx = np.arange(streams, dtype=np.int64)
    idx[list(copies)] = source
    return idx


def counts_of(idx, steps):
    """uint32 [streams], a cycle of 5: c_s = steps, 1, a count above steps, 0, 2"""
    return np.asarray((steps, 1, steps + 3, 0, 2), dtype=np.uint32)[idx % 5]


def frame_counts_of(idx, frames):
    """uint32 [streams], a cycle of 7: f_s = frames, 1, frames - 2, 0, a count above frames, 3, frames - 1"""
    return np.asarray((frames, 1, frames - 2, 0, frames + 4, 3, frames - 1), dtype=np.uint32)[idx % 7]


def keep_of(idx, steps):
    """uint32 [streams][2], periods steps + 3 and steps + 4 with 0xFFFFFFFF every 11th: equal, swapped and backward pairs, and indices above c_s + 1"""
    kf, kt = (3 * idx + 1) % (steps + 3), (5 * idx + 2) % (steps + 4)
    kt = np.where(idx % 11 == 5, BIG, kt)
    return np.stack([kf, kt], axis=1).astype(np.uint32)


def frame_tables_of(idx, steps, frames, frame_counts=None):
    """(from, to uint32, mod float32) [streams][frames]: indices in [0, steps + 2] with 0xFFFFFFFF sprinkled in, mod in sixteenths; frame_counts: behind every
    stream's count 0xFFFFFFFF and NaN"""
    s, j = idx[:, None], np.arange(frames, dtype=np.int64)[None, :]
    frm = np.where((s + j) % 13 == 0, BIG, (3 * s + 2 * j) % (steps + 3)).astype(np.uint32)
    to = np.where((s + 2 * j) % 17 == 0, BIG, (s + 5 * j + 1) % (steps + 3)).astype(np.uint32)
    mod = (((7 * s + 3 * j) % 16).astype(F32) / F32(16)).astype(F32)
    if frame_counts is not None:
        behind = j >= np.minimum(np.asarray(frame_counts, dtype=np.int64), frames)[:, None]
        frm[behind] = BIG; to[behind] = BIG; mod[behind] = np.nan
    return frm, to, mod


def starts_of(idx, steps, room, counts=None):
    """uint32 [streams][steps]: another offset and stride per stream (periods 9 and 11), repeats and backward jumps through the modulus, entries up to 24 frames
    beyond `room` (the last start a window fits at: they clamp); counts: behind every stream's count 0xFFFFFFFF"""
    s, t = idx[:, None], np.arange(steps, dtype=np.int64)[None, :]
    starts = ((13 * s + 5 * (s % 9) + t * (37 + 4 * (s % 11))) % (room + 25)).astype(np.uint32)
    if counts is not None:
        starts[t >= np.minimum(np.asarray(counts, dtype=np.int64), steps)[:, None]] = BIG
    return starts


def rates_of(idx, steps, base, counts=None):
    """float32 [streams][steps]: the rate table `base` turned by one entry per stream (a period of len(base)); counts: NaN behind every stream's count"""
    s, t = idx[:, None], np.arange(steps, dtype=np.int64)[None, :]
    ur = np.asarray(base, dtype=F32)[(s + t) % len(base)]
    if counts is not None:
        ur = np.where(t >= np.minimum(np.asarray(counts, dtype=np.int64), steps)[:, None], F32(np.nan), ur).astype(F32)
    return ur


def spans_of(idx, pool_frames, window):
    """[(first, frames)] per stream, a cycle of 9 over one small pool: two streams on ONE span, one nested in it off a group of 8 frames, one with exactly a window
    (every entry clamps to 0), one that ends on the pool's last frame, one that reaches beyond the pool and one that begins behind it (both clamp to the pool's
    last window), and two more recordings"""
    a = (16, 2 * window + 700)
    cycle = [a, a, (a[0] + 257, window + 300), (a[0] + a[1] + 47, window), (pool_frames - (window + 123), window + 123), (pool_frames - window - 10, window + 4 * N),
             (pool_frames + 5, 2 * window), (515, window + 1200), (8, pool_frames - 8)]
    assert (cycle[2][0] - a[0]) % 8 != 0 and all(first + frames <= pool_frames for first, frames in cycle[:5] + cycle[7:])
    return [cycle[i] for i in idx % 9]


def keys_of(idx, n, seed):
    """float32 [2][streams * 2][n] on the host: seeded values that straddle [0, 1], a planted copy's rows its source's"""
    streams = len(idx)
    k = (np.random.default_rng(seed).random((2, streams, 2, n), dtype=F32) * F32(1.3) - F32(0.1)).astype(F32)
    return np.ascontiguousarray(k[:, idx].reshape(2, streams * 2, n))


def recording(seed, idx, pitch, f32):
    """[streams][pitch][2] on the host, every stream at a level of its own, a planted copy's recording its source's"""
    return np.ascontiguousarray(rec(seed, len(idx), pitch, f32)[idx])


def rows_of(x, s0, count=SMALL):
    """the channel rows of streams [s0, s0 + count) of a [..][streams * 2][w] array or tensor"""
    return x[:, 2 * s0:2 * (s0 + count)]
