"""GPU: track mode from planar float recordings (glv_batch_track_at_f32_planar, _rates_, _frames_ and _wave_frames_f32_planar).

Contract.  d_rows is float [streams][2][pitch_frames]; window t of stream s, channel c, is the w = bufscale * n floats from min(starts[t], pitch_frames - w) on in
row 2 s + c, taken as it is (no mono mix).  Two references, both bit for bit (floats compared as int32):
  * the interleaved _f32 sibling on the interleaved copy of the same samples, channels = 2 -- output, and state through glv_batch_save_streams blobs;
  * sequential glv_batch_process_f32 calls on the windows' rows, channels = 1 and 2 -- which pins the no-mix rule.
Shapes: n in {256, 4096}, 3 streams, 7 steps, pitch_frames = 4 n + 3 (row 2 s + 1 starts off every boundary row 2 s starts on), d_rows one float behind the
allocation's first, and a table with starts of every residue mod 4, a repeat, a backward jump and 0xffffffff, which the kernels clamp.  The recording lies between
two guard regions of NaN inside one allocation, so a read outside the rows shows as wrong bits and never leaves the allocation; every workspace is exactly as large
as the sibling's query says and has a guard behind it, as every output has."""
import ctypes as C

import numpy as np
import pytest

from glava_amd import spectrum as _G
from glava_amd.bar_positions import graph_column_texels
from glava_amd.track_starts import keyframe_tables
from gpu_lib import eq

pytestmark = pytest.mark.gpu

STREAMS, STEPS, F = 3, 7, 5
SIZES = [256, 4096]
GUARD = 4096                                  # floats of NaN on either side of the rows; bytes behind a workspace; elements behind an output
CLAMPED = 0xffffffff


def _pitch(n):
    return 4 * n + 3


def _table(n):
    """starts = 0, 1, 1 (a repeat), 2, 3 (a backward jump) mod 4, the entry that must clamp, 3 mod 4"""
    s = [4, 9, 9, 2 * n + 2, 7, CLAMPED, n + 3]
    assert [v % 4 for v in s[:5]] == [0, 1, 1, 2, 3] and len(s) == STEPS
    return s


def _clamp(start, pitch, w):
    return min(start, pitch - w)


def _dev(a, dtype):
    import torch
    a = np.asarray(a, dtype=dtype)
    return torch.from_numpy(a.view(np.int32).copy() if dtype == np.uint32 else a.copy()).cuda()


_HOST = {}


def _host(n, streams=STREAMS, seed=0):
    """float32 [streams][2][pitch], every stream at a level of its own, the two channels unlike each other; made once per shape, never written"""
    key = (n, streams, seed)
    if key not in _HOST:
        x = (np.random.default_rng(1000 + n + seed).standard_normal((streams, 2, _pitch(n))) * 0.3).astype(np.float32)
        for s in range(streams):
            x[s] *= np.float32((1.0, 0.125, 0.015625)[s % 3])
        x[:, 1] *= np.float32(0.5)
        x.setflags(write=False)
        _HOST[key] = x
    return _HOST[key]


class _Rec:
    """a host recording on the device in both layouts: planar between NaN guards, one float behind a 16-byte boundary; interleaved at a 16-byte boundary"""

    def __init__(self, x):
        import torch
        self.x, self.streams, self.pitch = x, x.shape[0], x.shape[2]
        self.flat = torch.full((GUARD + 1 + x.size + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        assert self.flat.data_ptr() % 16 == 0
        self.rows = self.flat[GUARD + 1:GUARD + 1 + x.size].view(self.streams, 2, self.pitch)
        self.rows.copy_(torch.from_numpy(np.array(x, copy=True)))
        assert self.rows.data_ptr() % 16 == 4 and self.rows.is_contiguous()
        self.inter = torch.from_numpy(np.ascontiguousarray(np.transpose(x, (0, 2, 1)))).cuda()      # [streams][pitch][2]
        self.before = self.flat.clone()

    def intact(self):
        import torch
        torch.cuda.synchronize()
        return bool((self.flat.view(torch.int32) == self.before.view(torch.int32)).all())

    def windows(self, w, starts):
        """process_f32's inputs: [streams][2][w] contiguous, at each clamped start"""
        import torch
        return [torch.from_numpy(np.ascontiguousarray(self.x[:, :, a:a + w])).cuda() for a in (_clamp(s, self.pitch, w) for s in starts)]


def _dt(G, ops):
    import torch
    return torch.int16 if ops & G.OP_R16 else torch.float32


def _buffers(nbytes, count, dt):
    import torch
    work = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert work.data_ptr() % 256 == 0
    flat = torch.zeros((count + GUARD,), dtype=dt, device="cuda")
    flat[count:] = 77
    return work, flat


def _guards(work, nbytes, flat, count):
    import torch
    torch.cuda.synchronize()
    assert bool((work[nbytes:] == 0xA5).all()), "the call wrote behind the workspace the sibling's query asks for"
    assert bool((flat[count:] == 77).all()), "the call wrote behind its output"


def _at(b, R, planar, d_starts, steps, ops, w, d_ur=None, stream=None):
    """one table (d_ur: rates) call from the planar rows or from the interleaved copy: [steps][streams * 2][w]"""
    nbytes = b.track_at_work_bytes(steps, ops)
    count = steps * b.streams * 2 * w
    work, flat = _buffers(nbytes, count, _dt(_G, ops))
    if planar:
        if d_ur is None: b.track_at_f32_planar(R.rows, d_starts, steps, flat, work, ops, stream=stream)
        else: b.track_rates_f32_planar(R.rows, d_starts, d_ur, steps, flat, work, ops, stream=stream)
    elif d_ur is None: b.track_at_f32(R.inter, R.pitch, d_starts, steps, flat, work, ops, stream=stream)
    else: b.track_rates_f32(R.inter, R.pitch, d_starts, d_ur, steps, flat, work, ops, stream=stream)
    _guards(work, nbytes, flat, count)
    return flat[:count].view(steps, b.streams * 2, w)


def _blob(b):
    """the state of every stream in the portable form, or None for a batch that keeps none"""
    import torch
    nbytes = b.stream_state_desc().bytes
    if nbytes == 0:
        return None
    blob = torch.zeros((b.streams * nbytes,), dtype=torch.uint8, device="cuda")
    b.save_streams(_dev(list(range(b.streams)), np.uint32), b.streams, blob)
    torch.cuda.synchronize()
    return blob


def _same_state(a, b):
    import torch
    x, y = _blob(a), _blob(b)
    return (x is None and y is None) or bool(torch.equal(x, y))


def _seq_planar(b, wins, ops, w, dt):
    import torch
    outs = []
    for x in wins:
        o = torch.zeros((b.streams * 2, w), dtype=dt, device="cuda")
        b.process_f32(x, o, ops)
        outs.append(o)
    torch.cuda.synchronize()
    return torch.stack(outs)


def _forms(G, n):
    """name -> (parameters, creation mask, ops, width of an output row, column texels or None): every form a table call takes"""
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    cols = graph_column_texels(n, 64 if n == 256 else 320)[0]
    gl = dict(gl_storage=1, avg_window_kind=1, avg_frames=F)
    return {
        "fft":         (dict(), G.OP_FFT, G.OP_FFT, n, None),
        "windows":     (dict(avg_frames=F), GA, G.OP_FFT | GA, n, None),
        "windows_gl":  (gl, GA, G.OP_FFT | GA | G.OP_R16, n, None),
        "windows_bars": (dict(avg_frames=F, bars=80), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS, 80, None),
        "live":        (dict(bars=n, bar_phase=0.5, **gl), GA | G.OP_BARS | G.OP_BARS_ONLY, G.OP_FFT | GA | G.OP_BARS | G.OP_R16, n, None),
        "columns":     (dict(bars=len(cols), **gl), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS, len(cols), cols),
        "wave":        (dict(gl_storage=1, bars=n, bar_phase=0.5), G.OP_WAVE, G.OP_WAVE | G.OP_R16, n, None),
        "wave_floats": (dict(gl_storage=1, bars=n, bar_phase=0.5), G.OP_WAVE, G.OP_WAVE, n, None),
        "wave_bars":   (dict(gl_storage=1, bars=n, bar_phase=0.5), G.OP_WAVE | G.OP_BARS, G.OP_WAVE | G.OP_BARS | G.OP_R16, n, None),
    }


def _batch(G, n, form, streams=STREAMS, **more):
    kw, mask, ops, w, cols = _forms(G, n)[form]
    b = G.Batch(G.Params(n=n, **dict(kw, **more)), streams, mask)
    if cols is not None: b.set_column_texels(cols)
    return b, ops, w


# ---- 1. against the interleaved entry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["fft", "windows", "windows_gl", "windows_bars", "live", "columns", "wave", "wave_floats", "wave_bars"])
@pytest.mark.parametrize("n", SIZES)
def test_planar_equals_the_interleaved_entry(glvlib, n, form):
    G = glvlib
    R = _Rec(_host(n))
    d_starts = _dev(_table(n), np.uint32)
    bp, ops, w = _batch(G, n, form)
    bi, _, _ = _batch(G, n, form)
    got, want = _at(bp, R, True, d_starts, STEPS, ops, w), _at(bi, R, False, d_starts, STEPS, ops, w)
    assert eq(got, want), form
    assert bp.last_launches() == bi.last_launches() and bp.kernel_name() == bi.kernel_name()
    assert bp.last_launches() == (2 if form == "wave_bars" else bi.last_launches())      # with bars the wave form takes two launches, as from interleaved floats
    assert _same_state(bp, bi), form
    assert R.intact()
    bp.close(); bi.close()


@pytest.mark.parametrize("n", SIZES)
def test_rates_equal_the_interleaved_entry(glvlib, n):
    G = glvlib
    R = _Rec(_host(n))
    d_starts = _dev(_table(n), np.uint32)
    d_ur = _dev([1.0, 59.0, 60.0, 30.5, 59.0, 144.0, 24.0], np.float32)
    for form in ("windows", "windows_gl"):
        bp, ops, w = _batch(G, n, form)
        bi, _, _ = _batch(G, n, form)
        assert eq(_at(bp, R, True, d_starts, STEPS, ops, w, d_ur), _at(bi, R, False, d_starts, STEPS, ops, w, d_ur)), form
        assert _same_state(bp, bi), form
        bp.close(); bi.close()


# the render frames of 7 updates: a session of 15 frames, cut in front of the frame that runs step 3
MODIFIED = [True, False, True, True, False, False, True, False, True, True, False, False, False, True, False]
FRAMES = len(MODIFIED)
CUT = [j for j, m in enumerate(MODIFIED) if m][3]
assert sum(MODIFIED) == STEPS and CUT == 6


def _frames(b, R, planar, wave, d_starts, t0, steps, tables, d_keys, ops, w):
    import torch
    frm, to, mod, keep_from, keep_to = tables
    frames = len(frm)
    nbytes = (b.track_wave_frames_work_bytes if wave else b.track_frames_work_bytes)(steps, frames, ops)
    count = frames * b.streams * 2 * w
    work, flat = _buffers(nbytes, count, _dt(_G, ops))
    t = (_dev(frm, np.uint32), _dev(to, np.uint32), _dev(mod, np.float32))
    where = d_starts.data_ptr() + 4 * t0
    if wave:
        if planar: b.track_wave_frames_f32_planar(R.rows, where, steps, *t, frames, d_keys, (keep_from, keep_to), flat, work, ops)
        else: b.track_wave_frames_f32(R.inter, R.pitch, where, steps, *t, frames, d_keys, (keep_from, keep_to), flat, work, ops)
    elif planar: b.track_frames_f32_planar(R.rows, where, None, steps, *t, frames, d_keys, (keep_from, keep_to), flat, work, ops)
    else: b.track_frames_f32(R.inter, R.pitch, where, None, steps, *t, frames, d_keys, (keep_from, keep_to), flat, work, ops)
    _guards(work, nbytes, flat, count)
    return flat[:count].view(frames, b.streams * 2, w)


@pytest.mark.parametrize("wave", [False, True], ids=["fft", "wave"])
@pytest.mark.parametrize("bars", [False, True], ids=["texels", "bars"])
@pytest.mark.parametrize("n", SIZES)
def test_frames_entries_equal_the_interleaved_ones_with_the_session_cut_in_two(glvlib, n, bars, wave):
    """the planar session in two calls with d_keys carried == the interleaved session in one call: frames, keyframes kept and state"""
    import torch
    G = glvlib
    R = _Rec(_host(n))
    d_starts = _dev(_table(n), np.uint32)
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    if wave:
        kw, mask = dict(gl_storage=1, bars=n, bar_phase=0.5), G.OP_WAVE | (G.OP_BARS if bars else 0)
        ops = mask | G.OP_R16
    else:
        kw, mask = dict(gl_storage=G.GL_STORAGE_UPLOAD, bars=n, bar_phase=0.5, avg_frames=F), GA | (G.OP_BARS if bars else 0)
        ops = G.OP_FFT | mask | G.OP_R16
    bp, bi = G.Batch(G.Params(n=n, **kw), STREAMS, mask), G.Batch(G.Params(n=n, **kw), STREAMS, mask)
    uratio = [0.4] * FRAMES
    whole = keyframe_tables(MODIFIED, [True] * FRAMES, uratio)
    first = keyframe_tables(MODIFIED[:CUT], [True] * CUT, uratio[:CUT])
    idle = CUT - 1 - max(j for j in range(CUT) if MODIFIED[j])
    rest = keyframe_tables(MODIFIED[CUT:], [True] * (FRAMES - CUT), uratio[CUT:], kcounter=idle)
    seed = torch.from_numpy((np.random.default_rng(7).random((2, STREAMS * 2, n), dtype=np.float32) * np.float32(1.3) - np.float32(0.1)).astype(np.float32)).cuda()
    ki, kp = seed.clone(), seed.clone()
    want = _frames(bi, R, False, wave, d_starts, 0, STEPS, whole, ki, ops, n)
    a = _frames(bp, R, True, wave, d_starts, 0, 3, first, kp, ops, n)
    b = _frames(bp, R, True, wave, d_starts, 3, STEPS - 3, rest, kp, ops, n)
    assert eq(a, want[:CUT]) and eq(b, want[CUT:])
    assert eq(kp, ki)
    assert _same_state(bp, bi)
    assert R.intact()
    bp.close(); bi.close()


# ---- 2. against one-by-one calls: the rows are taken as they are -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("form", ["windows", "windows_gl", "wave"])
@pytest.mark.parametrize("n", SIZES)
def test_planar_equals_one_by_one_process_f32_calls(glvlib, n, form, channels):
    """channels = 1 too: glv_batch_process_f32 mixes nothing, and neither does the planar entry (the interleaved entries would)"""
    G = glvlib
    R = _Rec(_host(n))
    starts = _table(n)
    bp, ops, w = _batch(G, n, form, channels=channels)
    bs, _, _ = _batch(G, n, form, channels=channels)
    got = _at(bp, R, True, _dev(starts, np.uint32), STEPS, ops, w)
    want = _seq_planar(bs, R.windows(n, starts), ops, w, _dt(G, ops))
    assert eq(got, want), (form, channels)
    assert _same_state(bp, bs), (form, channels)
    bp.close(); bs.close()


# ---- 3. bufscale ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("form", ["fft", "windows", "windows_gl", "columns"])
@pytest.mark.parametrize("n", SIZES)
def test_bufscale_equals_one_by_one_calls_under_the_same_k(glvlib, n, form, k):
    G = glvlib
    R = _Rec(_host(n))
    starts = _table(n)
    bp, ops, w = _batch(G, n, form, channels=1)
    bs, _, _ = _batch(G, n, form, channels=1)
    bp.set_bufscale(k); bs.set_bufscale(k)
    got = _at(bp, R, True, _dev(starts, np.uint32), STEPS, ops, w)
    want = _seq_planar(bs, R.windows(k * n, starts), ops, w, _dt(G, ops))
    assert eq(got, want), (form, k)
    assert _same_state(bp, bs), (form, k)
    assert R.intact()
    bp.close(); bs.close()


@pytest.mark.parametrize("frames", [False, True], ids=["at", "wave_frames"])
def test_wave_forms_are_refused_under_bufscale_as_the_interleaved_entries_are(glvlib, frames):
    import torch
    G = glvlib
    n = 256
    R = _Rec(_host(n))
    d_starts = _dev(_table(n), np.uint32)
    b, ops, w = _batch(G, n, "wave")
    b.set_bufscale(2)
    out = torch.zeros((STEPS, STREAMS * 2, n), dtype=torch.int16, device="cuda")
    work = torch.zeros((4096,), dtype=torch.uint8, device="cuda")
    keys = torch.zeros((2, STREAMS * 2, n), dtype=torch.float32, device="cuda")
    t = (_dev([0] * 4, np.uint32), _dev([1] * 4, np.uint32), _dev([0.5] * 4, np.float32))
    said = []
    for planar in (True, False):
        with pytest.raises(G.GlvError) as ei:
            if frames and planar: b.track_wave_frames_f32_planar(R.rows, d_starts, STEPS, *t, 4, keys, (0, 1), out, work, ops)
            elif frames: b.track_wave_frames_f32(R.inter, R.pitch, d_starts, STEPS, *t, 4, keys, (0, 1), out, work, ops)
            elif planar: b.track_at_f32_planar(R.rows, d_starts, STEPS, out, work, ops)
            else: b.track_at_f32(R.inter, R.pitch, d_starts, STEPS, out, work, ops)
        assert ei.value.code == G.ERR_STATE and "glv_batch_set_bufscale" in str(ei.value)
        said.append(str(ei.value))
    assert said[0] == said[1]
    b.close()


# ---- 4. float specials -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["fft", "windows", "wave", "wave_floats"])
@pytest.mark.parametrize("n", SIZES)
def test_float_specials_pass_as_through_the_interleaved_entry(glvlib, n, form):
    G = glvlib
    starts = _table(n)
    x = np.array(_host(n), copy=True)
    pitch = x.shape[2]
    x[0, 0, 5:40] = -0.0
    x[0, 1, starts[0] + 3] = np.inf
    x[1, 0, starts[3] + n - 2] = -np.inf
    x[1, 1, pitch - 1] = np.nan                       # the last float of a row: inside the clamped window only
    x[2, 0, starts[1] + 1] = np.nan
    x[2, 1, 8:12] = [-0.0, np.inf, -np.inf, np.nan]
    R = _Rec(x)
    d_starts = _dev(starts, np.uint32)
    bp, ops, w = _batch(G, n, form)
    bi, _, _ = _batch(G, n, form)
    assert eq(_at(bp, R, True, d_starts, STEPS, ops, w), _at(bi, R, False, d_starts, STEPS, ops, w)), form
    assert _same_state(bp, bi)
    bp.close(); bi.close()


# ---- 5. bounds -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,k", [("fft", 1), ("windows", 1), ("wave", 1), ("wave_bars", 1), ("fft", 2), ("windows", 2)])      # (the wave forms refuse bufscale > 1)
@pytest.mark.parametrize("n", SIZES)
def test_a_table_of_entries_that_all_clamp_reads_the_last_window_and_nothing_outside(glvlib, n, form, k):
    """NaN on both sides of the rows: 0xffffffff everywhere == pitch_frames - w everywhere, and no NaN reaches a result"""
    import torch
    G = glvlib
    R = _Rec(_host(n))
    bp, ops, w = _batch(G, n, form)
    bq, _, _ = _batch(G, n, form)
    if k > 1: bp.set_bufscale(k); bq.set_bufscale(k)
    got = _at(bp, R, True, _dev([CLAMPED] * STEPS, np.uint32), STEPS, ops, w)
    want = _at(bq, R, True, _dev([R.pitch - k * n] * STEPS, np.uint32), STEPS, ops, w)
    assert eq(got, want), form
    if got.dtype == torch.float32: assert not bool(torch.isnan(got).any())
    assert _same_state(bp, bq)
    assert R.intact(), "the guard regions or the rows changed"
    bp.close(); bq.close()


# ---- 6. past the launch caps of the new kinds ------------------------------------------------------------------------------------------------------------
CAP_STREAMS, CAP_N = 2731, 256
K_GRID_CAP, K_DECIMATE_CAP = 256 * 8, 256 * 8       # glv_launch_util.h kGridCap (grid_256 of glv_wave_kernel), glv_launch.h kDecimateGridCap: workgroups of 256 lanes


def test_the_large_call_lies_beyond_the_caps():
    windows = CAP_STREAMS * STEPS
    assert windows * (CAP_N // 8) > K_GRID_CAP * 256            # glv_wave_kernel: one lane per group of 8 samples of a window
    assert windows * (CAP_N // 4) > K_DECIMATE_CAP * 256        # glv_decimate_kernel: one lane per four output samples of a window
    assert (CAP_STREAMS - 1) * STEPS * (CAP_N // 8) > K_GRID_CAP * 256      # ... and the loop has begun before the last stream's items


@pytest.mark.parametrize("what", ["wave", "decimate"])
def test_past_the_launch_caps(glvlib, what):
    """the item loops of the planar wave and decimate kinds, 256 samples wide: against the interleaved entry, whose kinds tests/test_track_launch_geometry.py
    and tests/test_track_bufscale.py pin past the same caps"""
    G = glvlib
    n = CAP_N
    R = _Rec(_host(n, CAP_STREAMS, seed=5))
    d_starts = _dev(_table(n), np.uint32)
    form = "wave" if what == "wave" else "fft"
    bp, ops, w = _batch(G, n, form, streams=CAP_STREAMS)
    bi, _, _ = _batch(G, n, form, streams=CAP_STREAMS)
    if what == "decimate": bp.set_bufscale(2); bi.set_bufscale(2)
    assert eq(_at(bp, R, True, d_starts, STEPS, ops, w), _at(bi, R, False, d_starts, STEPS, ops, w))
    assert R.intact()
    bp.close(); bi.close()


# ---- 7. grid and graph -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("form", ["fft", "windows_gl"])
@pytest.mark.parametrize("n", SIZES)
def test_a_forced_grid_equals_the_automatic_one(glvlib, n, form, grid):
    G = glvlib
    R = _Rec(_host(n))
    d_starts = _dev(_table(n), np.uint32)
    ba, ops, w = _batch(G, n, form)
    bg, _, _ = _batch(G, n, form)
    bg.set_grid(grid)
    want, got = _at(ba, R, True, d_starts, STEPS, ops, w), _at(bg, R, True, d_starts, STEPS, ops, w)
    assert bg.last_grid() == grid and ba.last_grid() != grid
    assert eq(got, want) and _same_state(ba, bg)
    ba.close(); bg.close()


def test_a_captured_call_is_reaimed_by_rewriting_the_table(glvlib):
    """the FIRST call after creation, captured; replayed with the table rewritten in between == eager calls on a second batch"""
    import torch
    G = glvlib
    hip = C.CDLL("libamdhip64.so")
    n = 256
    R = _Rec(_host(n))
    table_a = _table(n)[:F]
    table_b = [3 * n, 1, CLAMPED, 17, n + 5]
    bg, ops, w = _batch(G, n, "windows_gl")
    be, _, _ = _batch(G, n, "windows_gl")
    work = torch.zeros((bg.track_at_work_bytes(F, ops),), dtype=torch.uint8, device="cuda")
    og = torch.zeros((F, STREAMS * 2, n), dtype=torch.int16, device="cuda")
    d_starts = _dev(table_a, np.uint32)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = C.c_void_p(st.cuda_stream)
    assert hip.hipStreamBeginCapture(sp, 0) == 0
    try:
        bg.track_at_f32_planar(R.rows, d_starts, F, og, work, ops, stream=st.cuda_stream)
    finally:
        graph = C.c_void_p()
        rc = hip.hipStreamEndCapture(sp, C.byref(graph))
    assert rc == 0
    count = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(count)) == 0 and count.value == bg.last_launches() == 2
    exe = C.c_void_p()
    assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
    for table in (table_a, table_b):
        d_starts.copy_(_dev(table, np.uint32))
        torch.cuda.synchronize()
        assert hip.hipGraphLaunch(exe, sp) == 0
        st.synchronize()
        assert eq(og, _at(be, R, True, _dev(table, np.uint32), F, ops, w)), table
    hip.hipGraphExecDestroy(exe); hip.hipGraphDestroy(graph)
    bg.close(); be.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_are_the_siblings_and_leave_the_batch_usable(glvlib):
    import torch
    G = glvlib
    L = G.lib()
    n = 256
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    ops = G.OP_FFT | GA
    R = _Rec(_host(n))
    starts = _table(n)
    d_starts = _dev(starts, np.uint32)
    b = G.Batch(G.Params(n=n), STREAMS, GA | G.OP_BARS)
    work = torch.zeros((b.track_at_work_bytes(STEPS, ops | G.OP_BARS),), dtype=torch.uint8, device="cuda")
    out = torch.zeros((STEPS, STREAMS * 2, n), dtype=torch.float32, device="cuda")
    b.track_at_f32_planar(R.rows, d_starts, 2, out, work, ops)
    torch.cuda.synchronize()
    before = out.clone()
    rows, inter, tab, o, wk = R.rows.data_ptr(), R.inter.data_ptr(), d_starts.data_ptr(), out.data_ptr(), work.data_ptr()

    def call(batch, planar, pcm, pitch, where, steps, d_out, d_work, ops_):
        f = L.glv_batch_track_at_f32_planar if planar else L.glv_batch_track_at_f32
        rc = f(batch._h, pcm, pitch, where, steps, d_out, d_work, ops_, None)
        return rc, L.glv_last_error().decode()

    def own(code, word, **kw):
        a = dict(pcm=rows, pitch=R.pitch, where=tab, steps=STEPS, d_out=o, d_work=wk, ops_=ops)
        a.update(kw)
        launches = b.last_launches()
        rc, msg = call(b, True, **a)
        assert rc == code and word in msg, (rc, msg)
        assert b.last_launches() == launches

    own(G.ERR_INVALID, "NULL", pcm=None)
    own(G.ERR_INVALID, "NULL", where=None)
    own(G.ERR_INVALID, "NULL", d_out=None)
    own(G.ERR_INVALID, "NULL", d_work=None)
    own(G.ERR_INVALID, "4 bytes", pcm=rows + 2)                                   # misaligned by 2 bytes
    own(G.ERR_INVALID, "pitch_frames", pitch=n - 1)                               # pitch_frames < w
    b2 = G.Batch(G.Params(n=n), STREAMS, GA); b2.set_bufscale(2)
    rc, msg = call(b2, True, rows, 2 * n - 1, tab, STEPS, o, wk, ops)
    assert rc == G.ERR_INVALID and "pitch_frames" in msg                           # ... with w = bufscale * n
    b2.close()

    # every refusal of the sibling, on code and message: the same call through both entries
    gl2 = G.Batch(G.Params(n=n, gl_storage=2), STREAMS, GA)
    unannounced = G.Batch(G.Params(n=n), STREAMS, G.OP_FFT)
    live = G.Batch(G.Params(n=n, gl_storage=1), STREAMS, GA | G.OP_BARS | G.OP_BARS_ONLY)
    mixed = G.Batch(G.Params(n=n), STREAMS, GA)
    mixed.process_f32(R.windows(n, [0])[0], out[0].clone(), G.OP_FFT | G.OP_GRAVITY)
    cases = [(b, dict(steps=0)), (b, dict(where=tab + 2)), (b, dict(d_work=wk + 64)), (b, dict(steps=(2 ** 32 - 1) // (2 * STREAMS) + 1)), (b, dict(ops_=GA)),
             (b, dict(ops_=G.OP_FFT | G.OP_WAVE)), (b, dict(pitch=n - 1)), (gl2, dict()), (unannounced, dict()), (live, dict()), (mixed, dict())]
    cases += [(b, dict(ops_=ops | bad)) for bad in (G.OP_RAW, G.OP_SMOOTH, G.OP_WRANGE, G.OP_MAGNITUDE)]
    for batch, kw in cases:
        a = dict(pitch=R.pitch, where=tab, steps=STEPS, d_out=o, d_work=wk, ops_=ops)
        a.update(kw)
        launches = batch.last_launches()
        got, want = call(batch, True, rows, **a), call(batch, False, inter, **a)
        assert got[0] != G.OK and got == want, (kw, got, want)
        assert batch.last_launches() == launches
    ur = _dev([60.0] * STEPS, np.float32).data_ptr()
    for ops_ in (G.OP_FFT | G.OP_AVERAGE, G.OP_WAVE):                               # the rates entry's own: no gravity reads the table
        got = (L.glv_batch_track_rates_f32_planar(b._h, rows, R.pitch, tab, ur, STEPS, o, wk, ops_, None), L.glv_last_error().decode())
        want = (L.glv_batch_track_rates_f32(b._h, inter, R.pitch, tab, ur, STEPS, o, wk, ops_, None), L.glv_last_error().decode())
        assert got[0] == G.ERR_INVALID and got == want
    for x_ in (gl2, unannounced, live, mixed): x_.close()
    torch.cuda.synchronize()
    assert eq(out, before), "a refused call wrote to the output"
    # the batch continues from untouched state: steps [2, 7) here == the sequential calls all the way on a fresh batch
    bs = G.Batch(G.Params(n=n), STREAMS, GA | G.OP_BARS)
    want = _seq_planar(bs, R.windows(n, starts), ops, n, torch.float32)
    nbytes = b.track_at_work_bytes(STEPS - 2, ops)
    b.track_at_f32_planar(R.rows, tab + 8, STEPS - 2, out[2:], work[:nbytes], ops)
    torch.cuda.synchronize()
    assert eq(out, want)
    b.close(); bs.close()
