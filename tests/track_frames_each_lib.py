"""The rule of a per-stream frames call (glv_batch_track_each_frames_* / glv_batch_track_pool_frames_*) restated in numpy: a plain module, like track_lib.py,
shared by tests/test_track_frames_each_host.py (which holds it to hand-computed cases) and tests/test_track_frames_each.py (which holds the kernels to it).

Stream s has c_s = min(counts[s], steps) steps and f_s = min(frame_counts[s], frames) frames.  Keyframe k of the stream is keys[k] for k < 2 and rows[k - 2]
beyond; every index its tables or its keep pair hold is clamped to c_s + 1.  Frame j < f_s is the keyframe itself where from == to, else s + ((e - s) * mod)
in three float32 operations; frame j >= f_s is a row of zero TEXELS, which `lerp_each` reports through its second result."""
import numpy as np

F32 = np.float32


def clamp_each(table, counts, steps):
    """uint64 [streams][...]: every entry of a per-stream table clamped to its stream's c_s + 1"""
    table = np.asarray(table, dtype=np.uint64)
    last = np.minimum(np.asarray(counts, dtype=np.uint64), np.uint64(steps)) + np.uint64(1)
    return np.minimum(table, last.reshape((-1,) + (1,) * (table.ndim - 1)))


def lerp_each(keys, rows, frm, to, mod, counts, frame_counts, steps):
    """keys float32 [2][units][n], rows float32 [steps][units][n], frm / to / mod [streams][frames]; counts, frame_counts [streams] or None.
    Returns (w float32 [frames][units][n], shown bool [frames][streams]): w of a frame a stream does not show is 0.0 and its texels are zeros"""
    frm, to, mod = np.asarray(frm), np.asarray(to), np.asarray(mod, dtype=F32)
    streams, frames = frm.shape
    counts = [steps] * streams if counts is None else [min(int(c), steps) for c in counts]
    frame_counts = [frames] * streams if frame_counts is None else [min(int(f), frames) for f in frame_counts]
    kf, kt = clamp_each(frm, counts, steps), clamp_each(to, counts, steps)
    w = np.zeros((frames,) + keys.shape[1:], dtype=F32)
    shown = np.zeros((frames, streams), dtype=bool)
    with np.errstate(all="ignore"):
        for s in range(streams):
            r = slice(2 * s, 2 * s + 2)
            key = lambda k: keys[k, r] if k < 2 else rows[k - 2, r]              # noqa: E731
            for j in range(frame_counts[s]):
                a, b = int(kf[s, j]), int(kt[s, j])
                assert a <= counts[s] + 1 and b <= counts[s] + 1
                st, en = key(a), key(b)
                w[j, r] = st if a == b else (st + ((en - st).astype(F32) * mod[s, j]).astype(F32)).astype(F32)
                shown[j, s] = True
    return w, shown


def keep_each(keys, rows, keep, counts, steps):
    """d_keys after the write-back: float32 [2][units][n], both kept keyframes read before either is written"""
    keep = clamp_each(keep, [steps] * len(keep) if counts is None else counts, steps)
    out = np.array(keys, copy=True)
    for s in range(keep.shape[0]):
        r = slice(2 * s, 2 * s + 2)
        key = lambda k: keys[k, r] if k < 2 else rows[k - 2, r]                  # noqa: E731
        out[0, r], out[1, r] = key(int(keep[s, 0])), key(int(keep[s, 1]))
    return out
