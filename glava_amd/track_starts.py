"""Tables of window starts for track mode at given positions (include/glv_spectrum.h glv_batch_track_at_s16 / _f32; Batch.track_at_s16 / _f32).

Integer arithmetic only: a table is a list of frame positions, and a position that went through a float would drift or tie differently from one
machine to the next.  The one exception is live_session_rates' table of update rates: the reference accumulates frame durations in a double
(render.c:2384) and closes its measuring second when the sum reaches 1.0, so whether 60 additions of 1 / 60 reach 1.0 decides which frame closes the
second -- they do: the sum is 1.0000000000000013 -- and only the same IEEE double additions give the same answer.  They give it on every machine.  A frame rate is the fraction fps_num / fps_den (60 / 1, 24 / 1, 60000 / 1001), a sample rate an integer of frames per second.
The functions return Python ints; a caller uploads them as uint32 (numpy.asarray(starts, dtype=numpy.uint32))."""
from __future__ import annotations


def _positive(**kw) -> None:
    for name, v in kw.items():
        if not isinstance(v, int) or isinstance(v, bool) or v < 1:
            raise ValueError(f"{name} must be an integer >= 1, not {v!r}")


def hop_starts(steps: int, hop: int) -> list[int]:
    """The table of a uniform hop: window t starts t * hop frames in -- what the hop entries (glv_batch_track_windows_s16 / _f32) compute themselves, for the
    entries that take a table only (glv_batch_track_at_f32_planar).  Refuses a table whose last entry does not fit a uint32."""
    _positive(steps=steps, hop=hop)
    if (steps - 1) * hop >= 1 << 32:
        raise ValueError(f"(steps - 1) * hop = {(steps - 1) * hop} does not fit a uint32 table entry: cut the track into chunks")
    return [t * hop for t in range(steps)]


def renderer_starts(rate: int, fps_num: int, fps_den: int, steps: int) -> list[int]:
    """Window starts of a renderer that draws `steps` frames at fps_num / fps_den frames per second from a recording of `rate` frames per second: frame
    t shows the window that starts floor(t * rate * fps_den / fps_num) frames in -- the audio position at the frame's time t * fps_den / fps_num,
    rounded down to a whole frame, with no error carried from one step to the next.  At the shipped `setsamplerate 22050` (rc.glsl) and 60 fps the
    steps are 367 and 368 frames in turn; at 44100 Hz and 60 fps the table is t * 735, the uniform hop of glv_batch_track_windows_s16."""
    _positive(rate=rate, fps_num=fps_num, fps_den=fps_den, steps=steps)
    return [t * rate * fps_den // fps_num for t in range(steps)]


def live_update_starts(rate: int, fps_num: int, fps_den: int, frames: int, update_frames: int) -> tuple[list[int], list[int]]:
    """The windows a live GLava shows over `frames` render frames at fps_num / fps_den per second, from audio at `rate` frames per second that the
    audio thread publishes `update_frames` frames at a time.  Returns (starts, step_of_frame): the table of the distinct consecutive windows, and for
    every render frame the step whose result it shows (-1: no update has arrived yet).

    What it restates.  The FIFO backend reads sample_sz / 2 int16 values = sample_sz / 4 stereo frames per read (fifo.c:38), shifts its buffers by
    that many frames and appends them (fifo.c:91-112), and sets `modified`: one update every update_frames = sample_sz / 4 frames (256 at the
    shipped setsamplesize 1024).  The main loop (glava.c:528-537) takes a snapshot of the buffers once per render frame, and only when `modified` is
    set, which it then clears; rd_update runs the transform chain for a frame with `modified` and redraws the previous result for one without.  So
    render frame j, at time j * fps_den / fps_num, sees U = floor(floor(j * rate * fps_den / fps_num) / update_frames) complete updates, and its
    snapshot holds the n frames that END at audio frame U * update_frames.

    The recording handed to the track call carries n frames of silence in front of the audio's first frame, as GLava's zeroed buffers do: the window
    that ends at audio frame U * update_frames then STARTS at frame U * update_frames of the recording, which is the table's entry.

    Where the reference differs from the plain formula "one window per render frame", the reference wins: a render frame that sees no update newer
    than its predecessor's has `modified` clear and runs nothing -- it maps to its predecessor's step and adds no entry (a repeated entry would
    advance gravity and the average a second time); and the frames before the first update (U = 0) have nothing to show -- GLava draws its initial
    state without running the chain -- so they map to -1 and the table starts at the first U >= 1.  Updates that no render frame sees (at 60 fps
    against 86 updates per second, about every third) are skipped, as they are live: consecutive entries differ by 1 or 2 updates, irregularly."""
    _positive(rate=rate, fps_num=fps_num, fps_den=fps_den, frames=frames, update_frames=update_frames)
    starts: list[int] = []
    step_of_frame: list[int] = []
    last = 0
    for j in range(frames):
        updates = (j * rate * fps_den // fps_num) // update_frames
        if updates != last:
            starts.append(updates * update_frames)
            last = updates
        step_of_frame.append(len(starts) - 1)
    return starts, step_of_frame


def live_session_rates(rate: int, fps: int, frames: int, update_frames: int) -> tuple[list[int], list[int], list[float]]:
    """The windows a live GLava shows over `frames` render frames at `fps` per second (an integer >= 1, as gl->rate is) AND the update rate gravity runs
    at for each of them.  Returns (starts, step_of_frame, ur): the first two are exactly live_update_starts(rate, fps, 1, frames, update_frames); ur[t]
    is the value gl->ur holds while the render frame that runs step t runs it, as a Python float that is an exact float32 -- the second table of
    glv_batch_track_rates_s16 / _f32 (numpy.asarray(ur, dtype=numpy.float32)).

    What it restates (render.c:2358-2399).  gl->ur starts at 1.0 (render.c:906) and both gravity paths read it at every update (render.c:728, :2224).
    After every render frame the loop adds the frame's duration to tcounter, a double, and counts the frame in ucounter if it ran an update; when
    tcounter >= 1.0 it sets ur = (float) (ucounter / tcounter) and resets both.  Frames before the first update count like any other.  Render frame j
    therefore uses the value as it stands before frame j's own counters are added.  At 22050 Hz, 60 fps and updates of 256 frames: 59 steps at 1.0 (the
    step is the whole gravity_step and every value falls to 0), 60 steps at 59.0, then 60.0 -- never the 22050 / 256 = 86.13 updates the audio thread
    publishes, because a render frame shows the latest one only.

    What is modelled: every frame meets its target -- its duration is exactly 1.0 / fps (render.c:2362-2370, the frame that sleeps up to its target) --
    and updates arrive on the audio clock, as in live_update_starts.  What is not: wall-clock jitter.  A frame that overruns its target adds its real
    duration, the second then closes on another frame and ur takes values near, not at, these; a recorded session's durations are not reproducible."""
    _positive(fps=fps)
    starts, step_of_frame = live_update_starts(rate, fps, 1, frames, update_frames)
    from struct import pack, unpack
    duration = 1.0 / float(fps)                     # render.c:2362
    ur, cur, tcounter, ucounter = [], 1.0, 0.0, 0
    for j in range(frames):
        ran = step_of_frame[j] >= 0 and (j == 0 or step_of_frame[j] != step_of_frame[j - 1])      # `modified`
        if ran:
            ur.append(cur)
            ucounter += 1                           # render.c:2380-2381
        tcounter += duration                        # render.c:2384
        if tcounter >= 1.0:
            cur = unpack("f", pack("f", ucounter / tcounter))[0]      # render.c:2387: a double quotient stored in a float
            tcounter, ucounter = 0.0, 0
    return starts, step_of_frame, ur


def stack_tables(rows, steps: int | None = None):
    """The three tables of glv_batch_track_each_s16 / _f32 / _f32_planar (Batch.track_each_*) from one (starts, ur) pair per stream, of any lengths -- as
    renderer_starts / live_update_starts (ur None) and live_session_rates return them.  Every pair is padded to `steps` entries (default: the longest pair) by
    repeating its last entry -- an entry behind a stream's count is never applied to state, and a window the recording holds costs no clamp -- and its own
    length is its count.  Returns numpy arrays (starts uint32 [streams][steps], ur float32 [streams][steps], counts uint32 [streams]); ur is None where every
    pair's is None, and a stream without rates among streams with them runs at 1.0, the value gl->ur starts from.  An empty pair is a stream that stands
    still: count 0, its rows zeros and ones.  Refuses a pair whose tables differ in length, one longer than `steps`, and a start that does not fit a uint32."""
    import numpy as np
    rows = [(list(s), None if u is None else list(u)) for s, u in rows]
    if not rows:
        raise ValueError("stack_tables needs at least one stream")
    for s, u in rows:
        if u is not None and len(u) != len(s):
            raise ValueError(f"a stream's tables differ in length: {len(s)} starts, {len(u)} rates")
    longest = max(len(s) for s, _ in rows)
    if steps is None:
        steps = longest
    _positive(steps=steps)
    if longest > steps:
        raise ValueError(f"a stream has {longest} steps, more than steps = {steps}")
    with_rates = any(u is not None for _, u in rows)
    starts = np.zeros((len(rows), steps), dtype=np.uint32)
    ur = np.ones((len(rows), steps), dtype=np.float32) if with_rates else None
    counts = np.zeros((len(rows),), dtype=np.uint32)
    for i, (s, u) in enumerate(rows):
        if any(not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < 0 or v >= 1 << 32 for v in s):
            raise ValueError("a start must be an integer in [0, 2^32)")
        counts[i] = len(s)
        if s:
            starts[i, :len(s)] = s
            starts[i, len(s):] = s[-1]
        if with_rates and u:
            ur[i, :len(u)] = u
            ur[i, len(u):] = u[-1]
    return starts, ur, counts


def ring_update_counts(pending_frames, new_frames: int, cap: int | None = None):
    """The counts of a per-stream ring track call (glv_batch_ring_track_each_s16 / _f32; Batch.ring_track_each_*) from the frames every listener has pending:
    stream s takes counts[s] = pending_frames[s] // new_frames whole updates -- at most `cap` where one is given, the bound of a call's workspace or of what a
    host wants to catch up in one call -- and keeps leftover[s] = pending_frames[s] - counts[s] * new_frames frames for the next call, its oldest pending
    frames first in d_new.  Returns (counts, updates, leftover_frames): numpy uint32 [streams], the longest row (the call's `updates`; 0: nobody has a whole
    update pending and there is nothing to call), and a list of Python ints.  Integer arithmetic only.  Refuses an empty list, a pending count that is not
    an integer >= 0, and counts that do not fit a uint32."""
    import numpy as np
    pending = list(pending_frames)
    _positive(new_frames=new_frames)
    if cap is not None:
        _positive(cap=cap)
    if not pending:
        raise ValueError("ring_update_counts needs at least one stream")
    counts, leftover = [], []
    for v in pending:
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < 0:
            raise ValueError("a stream's pending frames must be an integer >= 0")
        c = int(v) // new_frames
        if cap is not None and c > cap:
            c = cap
        if c >= 1 << 32:
            raise ValueError(f"{c} updates do not fit a uint32 count: give a cap")
        counts.append(c)
        leftover.append(int(v) - c * new_frames)
    return np.asarray(counts, dtype=np.uint32), max(counts), leftover


# one glv_track_span as a numpy record: what d_spans of Batch.track_pool_* holds, 16 bytes a stream (glava_amd.spectrum.TrackSpan field by field)
SPAN_DTYPE = [("first", "<u8"), ("frames", "<u4"), ("reserved", "<u4")]       # numpy.dtype(SPAN_DTYPE)


def pool_spans(lengths, align: int = 8):
    """Where recordings of the given lengths (frames each) lie when packed into one pool for glv_batch_track_pool_s16 / _f32 / _f32_planar (Batch.track_pool_*):
    back to back in the order given, each beginning on a multiple of `align` frames -- 8 by default, so that a window that begins on a group of 8 frames of its
    recording lies on 32 bytes of an s16 pool and takes the wide loads.  Returns (first, pool_frames): the list of first frames and the frames the pool has to
    hold (the last recording's end, unpadded).  A listener's span is (first[i], lengths[i]) of the recording it hears; any number of listeners share one.
    Refuses an empty list, a length that is not an integer in [1, 2^32), and an `align` that is not a positive integer."""
    import numpy as np
    lengths = list(lengths)
    _positive(align=align)
    if not lengths:
        raise ValueError("pool_spans needs at least one recording")
    first, at = [], 0
    for v in lengths:
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < 1 or v >= 1 << 32:
            raise ValueError("a recording's length must be an integer in [1, 2^32)")
        at = (at + align - 1) // align * align
        first.append(at)
        at += int(v)
    return first, at


def pool_window_start(first: int, frames: int, entry: int, pool_frames: int, window: int) -> int:
    """The pool frame at which a window of `window` = k * n frames begins in a glv_batch_track_pool_* call -- the kernels' rule (glv_frame.h pool_window_start)
    restated in integers: `entry` frames into the span [first, first + frames), clamped to the span's last whole window, and whatever the span holds clamped
    to the pool's last whole window.  first: uint64, frames and entry: uint32, pool_frames >= window >= 1."""
    for name, v, top in (("first", first, 1 << 64), ("frames", frames, 1 << 32), ("entry", entry, 1 << 32), ("pool_frames", pool_frames, 1 << 64)):
        if not isinstance(v, int) or isinstance(v, bool) or v < 0 or v >= top:
            raise ValueError(f"{name} must be an integer in [0, {top})")
    _positive(window=window)
    if pool_frames < window:
        raise ValueError(f"pool_frames={pool_frames} holds no window of {window} frames")
    ext = frames - window if frames >= window else 0
    return min(first + min(entry, ext), pool_frames - window)


def _f32(x: float) -> float:
    from struct import pack, unpack
    return unpack("f", pack("f", x))[0]


def _f32_mul(a: float, b: float) -> float:
    """the float32 product of two float32 values: their double product is exact (48 significant bits), so one rounding gives it"""
    return _f32(a * b)


def keyframe_tables(modified, on, uratio, kcounter: int = 0) -> tuple[list[int], list[int], list[float], int, int]:
    """The keyframe tables of glv_batch_track_frames_s16 / _f32 for one call's render frames.  Per frame: modified[j] -- the frame runs an update (the next
    step of the call, in order); on[j] -- keyframe interpolation is configured on (`setinterpolate true`); uratio[j] -- gl->ur / gl->fr as the frame computes
    it (render.c:1761), any number that float32 holds.  Returns (from, to, mod, keep_from, keep_to) in the call's keyframe indices: 0 and 1 are the `start` and
    `end` keyframes the call is handed in d_keys, 2 + t is the finished row of the call's step t.

    What it restates.  A frame interpolates when on[j] and uratio[j] <= 0.9F (render.c:1763).  It then uploads start + (end - start) * mod of the keyframes as
    they stand BEFORE its own update is pushed, mod = min(uratio * kcounter, 1.0F) in float32 (render.c:1804-1806, :2185): from = start, to = end.  A frame
    that does not interpolate uploads its buffer (render.c:2185), which holds the spectrum its own update just finished or, without one, the last one
    finished: from = to = that row.  Before the call's first update that row is keyframe 1 -- exact where the previous call's last update was pushed, and the
    zeros of a fresh d_keys at the start of a session (GLava's buffers are zeroed too); a call cut while interpolation is off is best cut at a frame that runs
    an update.  After the upload, a frame with an update pushes start <- end, end <- its row only if it interpolated (render.c:2348: keyframes go stale while
    interpolation is off) and resets kcounter; any other frame increments it (render.c:2380-2383).  keep_from / keep_to are start and end after the last
    frame: what the next call finds in d_keys.  kcounter: the frames without an update directly in front of the call's first frame (gl->kcounter as the call
    finds it; 0 at the start of a session and wherever a call begins right after a frame with an update) -- with it the tables of a session cut into calls are
    the uncut session's."""
    modified, on, uratio = list(modified), list(on), list(uratio)
    if not (len(modified) == len(on) == len(uratio)) or not modified:
        raise ValueError("modified, on and uratio must be equally long lists of at least one render frame")
    if not isinstance(kcounter, int) or isinstance(kcounter, bool) or kcounter < 0:
        raise ValueError(f"kcounter must be an integer >= 0, not {kcounter!r}")
    start, end, shown, step = 0, 1, 1, 0
    frm: list[int] = []
    to: list[int] = []
    mod: list[float] = []
    for m, o, u in zip(modified, on, uratio):
        u = _f32(float(u))
        lerp = bool(o) and u <= _f32(0.9)                    # render.c:1763
        if m:
            shown = 2 + step
            step += 1
        if lerp:
            frm.append(start); to.append(end)
            mod.append(min(_f32_mul(u, float(kcounter)), 1.0))     # render.c:1804-1805 (kcounter < 2^24: exact as a float)
        else:
            frm.append(shown); to.append(shown)
            mod.append(0.0)
        if m:
            if lerp: start, end = end, shown                 # render.c:2347-2353
            kcounter = 0
        else:
            kcounter += 1
    return frm, to, mod, start, end


def stack_frame_tables(rows, frames: int | None = None):
    """The frame tables of glv_batch_track_each_frames_* / glv_batch_track_pool_frames_* (Batch.track_each_frames_* / track_pool_frames_*) from one
    (from, to, mod, keep_from, keep_to) tuple per stream, of any lengths -- as keyframe_tables returns them, and live_session_frames behind its first two tables.
    Every tuple is padded to `frames` entries (default: the longest, at least 1) with from = to = 0 and mod = 0.0 -- an entry behind a stream's frame count is
    never read -- and its own length is its frame count.  Returns numpy arrays (from uint32 [streams][frames], to uint32 [streams][frames], mod float32
    [streams][frames], frame_counts uint32 [streams], keep uint32 [streams][2]).  An empty tuple is a stream that shows nothing: frame count 0, and its keep
    pair as given ((0, 1) leaves its keyframes as they are).  Refuses tables of one stream that differ in length, one longer than `frames`, and an index or a
    keep entry that does not fit a uint32."""
    import numpy as np
    rows = [(list(f), list(t), list(m), kf, kt) for f, t, m, kf, kt in rows]
    if not rows:
        raise ValueError("stack_frame_tables needs at least one stream")
    for f, t, m, _, _ in rows:
        if not (len(f) == len(t) == len(m)):
            raise ValueError(f"a stream's tables differ in length: {len(f)} from, {len(t)} to, {len(m)} mod")
    longest = max(len(f) for f, _, _, _, _ in rows)
    if frames is None:
        frames = max(longest, 1)
    _positive(frames=frames)
    if longest > frames:
        raise ValueError(f"a stream has {longest} frames, more than frames = {frames}")
    index = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 <= v < 1 << 32      # noqa: E731
    frm = np.zeros((len(rows), frames), dtype=np.uint32)
    to = np.zeros((len(rows), frames), dtype=np.uint32)
    mod = np.zeros((len(rows), frames), dtype=np.float32)
    counts = np.zeros((len(rows),), dtype=np.uint32)
    keep = np.zeros((len(rows), 2), dtype=np.uint32)
    for i, (f, t, m, kf, kt) in enumerate(rows):
        if not all(index(v) for v in f + t + [kf, kt]):
            raise ValueError("a keyframe index must be an integer in [0, 2^32)")
        counts[i] = len(f)
        frm[i, :len(f)] = f
        to[i, :len(t)] = t
        mod[i, :len(m)] = m
        keep[i] = (kf, kt)
    return frm, to, mod, counts, keep


def live_session_frames(rate: int, fps: int, frames: int, update_frames: int) -> tuple[list[int], list[float], list[int], list[int], list[float], int, int]:
    """live_session_rates extended by the measured frame rate gl->fr: a `setinterpolate true` session on `setaccelfft false` (gl_storage 3) over `frames`
    render frames.  Returns (starts, ur, from, to, mod, keep_from, keep_to): the first two are live_session_rates' tables, the rest keyframe_tables' for the
    session's frames -- everything glv_batch_track_frames_s16 / _f32 takes besides the recording.

    What it restates.  gl->fr starts at 1.0 like gl->ur (render.c:905-906); when tcounter reaches 1.0 both are set from the same counters, fr = (float)
    (fcounter / tcounter) (render.c:2386), and frame j computes uratio = ur / fr in float from the values as they stand before its own counters are added.
    At 22050 Hz and updates of 256 frames a 60 fps session never interpolates (uratio 1.0, then 59 / 60); a 144 fps session does from its second second on
    (85.4 / 144).  The double additions are live_session_rates' own, and so is the disclaimer: every frame meets its target, wall-clock jitter is not modelled."""
    _positive(fps=fps)
    starts, step_of_frame = live_update_starts(rate, fps, 1, frames, update_frames)
    duration = 1.0 / float(fps)                     # render.c:2362
    ur: list[float] = []
    modified: list[bool] = []
    uratio: list[float] = []
    cur_ur, cur_fr, tcounter, ucounter, fcounter = 1.0, 1.0, 0.0, 0, 0
    for j in range(frames):
        ran = step_of_frame[j] >= 0 and (j == 0 or step_of_frame[j] != step_of_frame[j - 1])      # `modified`
        modified.append(ran)
        uratio.append(_f32(cur_ur / cur_fr))        # render.c:1761: a float quotient (the double quotient of two floats rounds to it)
        fcounter += 1                               # render.c:2379
        if ran:
            ur.append(cur_ur)
            ucounter += 1                           # render.c:2380-2381
        tcounter += duration                        # render.c:2384
        if tcounter >= 1.0:
            cur_fr = _f32(fcounter / tcounter)      # render.c:2386
            cur_ur = _f32(ucounter / tcounter)      # render.c:2387
            tcounter, ucounter, fcounter = 0.0, 0, 0
    frm, to, mod, keep_from, keep_to = keyframe_tables(modified, [True] * frames, uratio)
    return starts, ur, frm, to, mod, keep_from, keep_to
