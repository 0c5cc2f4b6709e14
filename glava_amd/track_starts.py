"""Tables of window starts for track mode at given positions (include/glv_spectrum.h glv_batch_track_at_s16 / _f32; Batch.track_at_s16 / _f32).

Integer arithmetic only: a table is a list of frame positions, and a position that went through a float would drift or tie differently from one
machine to the next.  A frame rate is the fraction fps_num / fps_den (60 / 1, 24 / 1, 60000 / 1001), a sample rate an integer of frames per second.
The functions return Python ints; a caller uploads them as uint32 (numpy.asarray(starts, dtype=numpy.uint32))."""
from __future__ import annotations


def _positive(**kw) -> None:
    for name, v in kw.items():
        if not isinstance(v, int) or isinstance(v, bool) or v < 1:
            raise ValueError(f"{name} must be an integer >= 1, not {v!r}")


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
