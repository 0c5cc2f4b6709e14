"""GPU: track mode per stream (glv_batch_track_each_s16 / _f32 / _f32_planar) -- the table and rates calls with a table row, a rate row and a count of
steps for every stream of the batch.

Contract: stream s behaves as if it were alone in a batch with its own table for its own number of updates, bit for bit.  The expected values come from the
existing entries: for every stream a ONE-stream twin batch is brought to the stream's state by glv_batch_copy_streams and runs glv_batch_track_rates_* (or
_at_* where d_ur is NULL) over the first c_s entries of the stream's rows on the stream's own recording -- an entry that tests/test_track_rates.py holds to
the sequential calls and to the oracle.  Compared, floats as int32: the rows t < c_s; the rows t >= c_s against the result of a finished row of zeros (zeros
without bars; with bars the texel and column results of a zero row are zeros too -- the integer sums of the snapped bars and of the i8 pass are 0 and round
to texel 0, column_mean(0, 0, 0) is 0.0F -- and the float bars of the float chain come from one glv_batch_bars evaluation of a zero row on the same
batch); glv_batch_save_streams blobs of every stream against its twin's; one further process call of the whole batch against the twins' next update.

In every call the workspace is exactly as large as glv_batch_track_at_work_bytes asks and the output exactly steps * streams * 2 * w elements, with a guard
behind each; the rate table has 8 NaN entries behind it, the starts a row of 0xFFFFFFFF and the counts an entry of 0xFFFFFFFF (a read past a table shows as
wrong bits, never as a fault).  5 streams, 11 steps (more than the scan's look-ahead of 8), F = 5 with the head off 0 (three process calls first), n = 256
(two scan workgroups a row) and 1024; counts {0, 1, 7, 8, 11} straddle the look-ahead."""
import ctypes as C

import numpy as np
import pytest

from glava_amd.bar_positions import graph_column_texels, radial_bar_texels
from track_lib import GUARD, differing, eq, out_dtype, rec
from track_rates_lib import FLOAT_STEP, FLOAT_UR, STEPS, TEXEL_STEP, TEXEL_UR

pytestmark = pytest.mark.gpu

STREAMS, F = 5, 5
COUNTS = [0, 1, 7, 8, 11]
NAN_TAIL = 8


# ---- tables ----------------------------------------------------------------------------------------------------------------------------------------------
def _pitch(n, k=1):
    return (STEPS * 131 + k * n + 38) | 1                                        # odd, with slack


def _starts(n, k=1, steps=STEPS):
    """[streams][steps]: another stride and offset per stream; stream 2 repeats entries and jumps backwards; stream 4 ends beyond pitch - k n (the clamp)"""
    pitch = _pitch(n, k)
    rows = [[7 * s + t * (61 + 23 * s) for t in range(steps)] for s in range(STREAMS)]
    rows[2] = [40, 40, 40, 300, 300, 12, 13, 500, 499, 498, 0][:steps]
    rows[4][-3:] = [pitch - k * n + 1, pitch, 0xFFFFFFF0]
    return np.asarray(rows, dtype=np.uint32)


def _rates(texel, steps=STEPS):
    """[streams][steps]: the rates file's table, turned by one entry per stream"""
    base = TEXEL_UR if texel else FLOAT_UR
    return np.asarray([[base[(t + s) % len(base)] for t in range(steps)] for s in range(STREAMS)], dtype=np.float32)


def _dev_u32(a, guard):
    """uint32 values on the device, `guard` entries of 0xFFFFFFFF behind them"""
    import torch
    flat = np.concatenate([np.asarray(a, dtype=np.uint32).reshape(-1), np.full(guard, 0xFFFFFFFF, np.uint32)])
    return torch.from_numpy(flat.view(np.int32).copy()).cuda()


def _dev_ur(a):
    import torch
    return torch.from_numpy(np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1), np.full(NAN_TAIL, np.nan, np.float32)])).cuda()


# ---- recordings: [streams][pitch][2] s16 / f32, [streams][2][pitch] planar; one frame off a load boundary ---------------------------------------------------
def _recording(kind, seed, pitch):
    """(host array, device view, bytes between two streams' recordings)"""
    import torch
    x = rec(seed, STREAMS, pitch, kind != "s16")
    if kind == "planar":
        x = np.ascontiguousarray(np.transpose(x, (0, 2, 1)))                     # [streams][2][pitch]: an odd pitch, so row 1 of a stream is 4-byte aligned and no more
    flat = torch.zeros((x.size + 2 * 1024 + 8,), dtype=torch.int16 if kind == "s16" else torch.float32, device="cuda")
    off = 2 if kind != "planar" else 1                                           # one frame (planar: one float) behind a load boundary
    view = flat[off:off + x.size]
    view.copy_(torch.from_numpy(np.array(x, copy=True).reshape(-1)))
    flat[off + x.size:] = 3                                                      # another pattern behind the last stream: a read past it shows as wrong bits
    stride = x[0].size * (2 if kind == "s16" else 4)
    return x, view.view(x.shape), stride


def _window(x, kind, s, start, frames):
    """the host window of stream s (None: every stream) as the process call of its kind takes it"""
    import torch
    sel = slice(None) if s is None else slice(s, s + 1)
    w = x[sel, :, start:start + frames] if kind == "planar" else x[sel, start:start + frames, :]
    return torch.from_numpy(np.ascontiguousarray(w)).cuda()


def _process(b, kind, win, ops, w, dt):
    import torch
    o = torch.zeros((b.streams * 2, w), dtype=dt, device="cuda")
    {"s16": b.process_s16, "f32": b.process_f32_stereo, "planar": b.process_f32}[kind](win, o, ops)
    torch.cuda.synchronize()
    return o


# ---- calls -----------------------------------------------------------------------------------------------------------------------------------------------
def _buffers(b, steps, ops, w, dt):
    import torch
    nbytes = b.track_at_work_bytes(steps, ops)
    work = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert work.data_ptr() % 256 == 0
    count = steps * b.streams * 2 * w
    fill = 23130 if dt == torch.int16 else -7.0
    flat = torch.full((count + GUARD,), fill, dtype=dt, device="cuda")           # (the output too: a row the call leaves stale shows)
    return work, nbytes, flat, count, fill


def _guards(work, nbytes, flat, count, fill):
    assert bool((work[nbytes:] == 0xA5).all()), "the call wrote behind the workspace it asked for"
    assert bool((flat[count:] == fill).all()), "the call wrote behind its output"


def _each(b, kind, d_rec, pitch, d_starts, d_ur, d_counts, steps, ops, w, dt, stream=None):
    """one per-stream call: exact workspace and output, a guard behind each"""
    import torch
    work, nbytes, flat, count, fill = _buffers(b, steps, ops, w, dt)
    if kind == "planar": b.track_each_f32_planar(d_rec, d_starts, d_ur, d_counts, steps, flat, work, ops, stream=stream)
    else: getattr(b, "track_each_" + kind)(d_rec, pitch, d_starts, d_ur, d_counts, steps, flat, work, ops, stream=stream)
    torch.cuda.synchronize()
    _guards(work, nbytes, flat, count, fill)
    return flat[:count].view(steps, b.streams * 2, w)


def _shared(b, kind, d_rec, pitch, d_starts, d_ur, steps, ops, w, dt):
    """the existing entries: glv_batch_track_rates_* where d_ur is set, glv_batch_track_at_* else; d_rec a tensor ([.., 2, pitch] for planar) of b.streams streams"""
    import torch
    work, nbytes, flat, count, fill = _buffers(b, steps, ops, w, dt)
    name = ("track_rates_" if d_ur is not None else "track_at_") + ("f32_planar" if kind == "planar" else kind)
    args = ([d_rec] if kind == "planar" else [d_rec, pitch]) + [d_starts] + ([d_ur] if d_ur is not None else []) + [steps, flat, work, ops]
    getattr(b, name)(*args)
    torch.cuda.synchronize()
    _guards(work, nbytes, flat, count, fill)
    return flat[:count].view(steps, b.streams * 2, w)


# ---- chains ----------------------------------------------------------------------------------------------------------------------------------------------
def _chain(G, name, n):
    """(parameters, creation mask, ops, table, output row width, texel state)"""
    S, A, GA = G.OP_GRAVITY, G.OP_AVERAGE, G.OP_GRAVITY | G.OP_AVERAGE
    gl = dict(gl_storage=1, avg_window_kind=1)
    radial, cols = radial_bar_texels(n, 160)[0], graph_column_texels(n, 120)[0]
    return {
        "gravity":      (dict(), S, G.OP_FFT | S, None, n, False),
        "average":      (dict(), A, G.OP_FFT | A, None, n, False),
        "chain":        (dict(), GA, G.OP_FFT | GA, None, n, False),
        "chain_F1":     (dict(avg_frames=1), GA, G.OP_FFT | GA, None, n, False),
        "chain_F2":     (dict(avg_frames=2), GA, G.OP_FFT | GA | G.OP_R16, None, n, False),
        "chain_mono":   (dict(channels=1), GA, G.OP_FFT | GA, None, n, False),
        "chain_bars":   (dict(bars=80), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS, None, 80, False),
        "gl_chain_r16": (gl, GA, G.OP_FFT | GA | G.OP_R16, None, n, True),
        "gl_bars":      (dict(gl, bars=n, bar_phase=0.5), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16, None, n, True),
        "gl_bar_texels": (dict(gl, bars=len(radial)), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16, ("bar", radial), len(radial), True),
        "live":         (dict(gl, bars=len(radial)), GA | G.OP_BARS | G.OP_BARS_ONLY, G.OP_FFT | GA | G.OP_BARS | G.OP_R16, ("bar", radial), len(radial), True),
        "columns":      (dict(gl, bars=len(cols)), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS, ("col", cols), len(cols), True),
        "upload":       (dict(gl_storage=G.GL_STORAGE_UPLOAD, bars=n, bar_phase=0.5), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16, None, n, False),
    }[name]


def _make(G, pkw, mask, table, streams, bufscale=1, grid=None):
    b = G.Batch(G.Params(**pkw), streams, mask)
    if table: (b.set_bar_texels if table[0] == "bar" else b.set_column_texels)(table[1])
    if bufscale > 1: b.set_bufscale(bufscale)
    if grid: b.set_grid(grid)
    return b


def _zero_rows(G, b, name, ops, w, dt):
    """what the call's last stage makes of a finished row of zeros, one row of w elements (the module's docstring)"""
    import torch
    if name == "chain_bars":
        spec, bars = torch.zeros((b.streams * 2, b.params.n), dtype=torch.float32, device="cuda"), torch.full((b.streams * 2, w), -7.0, dtype=torch.float32, device="cuda")
        b.bars(spec, bars)
        torch.cuda.synchronize()
        assert bool((bars.view(torch.int32) == bars.view(torch.int32)[0:1]).all())
        return bars[0]
    return torch.zeros((w,), dtype=dt, device="cuda")


def _blobs(b):
    import torch
    idx = _dev_u32(np.arange(b.streams), 0)
    nbytes = b.stream_state_desc().bytes
    blob = torch.zeros((b.streams * nbytes,), dtype=torch.uint8, device="cuda")
    b.save_streams(idx, b.streams, blob)
    torch.cuda.synchronize()
    return blob.view(b.streams, nbytes)


def _run(G, name, n, kind, counts=COUNTS, with_ur=True, bufscale=1, grid=None, log_mode=1):
    """the whole comparison of the module's docstring for one chain, size and input kind; returns the call's output and the batch (the caller closes it)"""
    import torch
    kw, mask, ops, table, w, texel = _chain(G, name, n)
    with_ur = with_ur and bool(ops & G.OP_GRAVITY)
    pkw = dict(dict(n=n, avg_frames=F, log_mode=log_mode, gravity_step=TEXEL_STEP if texel else FLOAT_STEP), **kw)
    dt = out_dtype(G, ops)
    span = bufscale * n
    pitch = _pitch(n, bufscale)
    x, d_rec, stride = _recording(kind, 1000 + n, pitch)
    starts, urs = _starts(n, bufscale), _rates(texel)
    d_starts = _dev_u32(starts, STEPS)
    d_ur = _dev_ur(urs) if with_ur else None
    d_counts = _dev_u32(counts, 1) if counts is not None else None
    b = _make(G, pkw, mask, table, STREAMS, bufscale, grid)
    for start in (3, 11, 29):                                                    # the head off 0, state in every stream
        _process(b, kind, _window(x, kind, None, start, span), ops, w, dt)
    # every stream's twin, at the stream's state
    twins = []
    for s in range(STREAMS):
        t = _make(G, pkw, mask, table, 1, bufscale, grid)
        t.copy_streams(_dev_u32([0], 0), b, _dev_u32([s], 0), 1)
        twins.append(t)
    torch.cuda.synchronize()
    got = _each(b, kind, d_rec, pitch, d_starts, d_ur, d_counts, STEPS, ops, w, dt)
    launches = 1 + 1 + (1 if ops & G.OP_BARS else 0) + (1 if bufscale > 1 else 0)
    assert b.last_launches() == launches, b.last_launches()
    zero = _zero_rows(G, b, name, ops, w, dt)
    for s in range(STREAMS):
        c = min(STEPS, counts[s]) if counts is not None else STEPS
        if c > 0:
            rows_s = d_rec[s:s + 1]
            want = _shared(twins[s], kind, rows_s, pitch, _dev_u32(starts[s, :c], 0), _dev_ur(urs[s, :c]) if with_ur else None, c, ops, w, dt)
            for t in range(c):
                assert eq(got[t, 2 * s:2 * s + 2], want[t]), (name, s, t, differing(got[t, 2 * s:2 * s + 2], want[t]))
        for t in range(c, STEPS):
            for ch in range(2):
                assert eq(got[t, 2 * s + ch], zero), (name, s, t, "a step behind the count")
    # the state: the portable blobs, then one more update of everything
    mine = _blobs(b)
    for s in range(STREAMS):
        assert bool((mine[s] == _blobs(twins[s])[0]).all()), (name, s, "blob")
    more = _process(b, kind, _window(x, kind, None, 17, span), ops, w, dt)
    for s in range(STREAMS):
        assert eq(more[2 * s:2 * s + 2], _process(twins[s], kind, _window(x, kind, s, 17, span), ops, w, dt)), (name, s, "next update")
    for t in twins: t.close()
    return got, b


# ---- 1. every chain, against the twins ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,kind", [("gravity", 256, "s16"), ("gravity", 1024, "f32"), ("average", 256, "f32"), ("average", 1024, "s16"), ("chain", 256, "planar"),
                                         ("chain", 1024, "s16"), ("chain_F1", 256, "s16"), ("chain_F2", 1024, "f32"), ("chain_mono", 1024, "s16"), ("chain_mono", 256, "f32"),
                                         ("chain_bars", 1024, "s16"), ("gl_chain_r16", 256, "s16"), ("gl_chain_r16", 1024, "planar"), ("gl_bars", 1024, "f32"),
                                         ("gl_bar_texels", 1024, "s16"), ("live", 1024, "s16"), ("columns", 1024, "f32"), ("upload", 1024, "s16"), ("upload", 256, "planar")])
def test_every_stream_is_its_one_stream_twin(glvlib, name, n, kind):
    _, b = _run(glvlib, name, n, kind)
    b.close()


@pytest.mark.parametrize("name", ["chain", "gl_chain_r16"])
def test_counts_alone_keep_the_batch_s_own_rate(glvlib, name):
    """d_ur NULL: the twins run glv_batch_track_at_*, whose texel state takes the packed integer step -- a count-only call must not take the float form"""
    _, b = _run(glvlib, name, 1024, "s16", with_ur=False)
    b.close()


def test_a_count_above_steps_is_clamped(glvlib):
    _, b = _run(glvlib, "gl_chain_r16", 256, "s16", counts=[12, 1000, 3, 11, 0])
    b.close()


@pytest.mark.parametrize("kind", ["s16", "f32", "planar"])
def test_bufscale_2(glvlib, kind):
    _, b = _run(glvlib, "chain", 256, kind, bufscale=2)
    b.close()


@pytest.mark.parametrize("grid", [1, 2])
def test_forced_grids(glvlib, grid):
    _, b = _run(glvlib, "gl_chain_r16", 256, "s16", grid=grid)
    b.close()


# ---- 2. equal rows and no counts: the shared-table entries on the same batch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,with_ur", [("chain", "s16", True), ("gl_chain_r16", "f32", True), ("gl_chain_r16", "s16", False), ("gl_bars", "planar", True),
                                               ("fft", "s16", False)])
def test_equal_rows_and_null_counts_are_the_shared_table_call(glvlib, name, kind, with_ur):
    import torch
    G = glvlib
    n = 1024
    if name == "fft": kw, mask, ops, table, w, texel = dict(), G.OP_FFT, G.OP_FFT, None, n, False          # stateless: no scan, the per-stream kinds of the transform alone
    else: kw, mask, ops, table, w, texel = _chain(G, name, n)
    pkw = dict(dict(n=n, avg_frames=F, gravity_step=TEXEL_STEP if texel else FLOAT_STEP), **kw)
    dt = out_dtype(G, ops)
    pitch = _pitch(n)
    x, d_rec, _ = _recording(kind, 77, pitch)
    row, ur = _starts(n)[4], _rates(texel)[1]
    be, bs = _make(G, pkw, mask, table, STREAMS), _make(G, pkw, mask, table, STREAMS)
    d_ur = _dev_ur(np.tile(ur, (STREAMS, 1))) if with_ur else None
    got = _each(be, kind, d_rec, pitch, _dev_u32(np.tile(row, (STREAMS, 1)), STEPS), d_ur, None, STEPS, ops, w, dt)
    want = _shared(bs, kind, d_rec, pitch, _dev_u32(row, 0), _dev_ur(ur) if with_ur else None, STEPS, ops, w, dt)
    assert eq(got, want), differing(got, want)
    assert be.last_launches() == bs.last_launches()
    win = _window(x, kind, None, 5, n)
    assert eq(_process(be, kind, win, ops, w, dt), _process(bs, kind, win, ops, w, dt)), "state"
    torch.cuda.synchronize()
    be.close(); bs.close()


# ---- 3. a call cut in two ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain", "gl_chain_r16"])
def test_a_call_cut_in_two_is_the_uncut_call(glvlib, name):
    """steps [0, 6) then [6, 11), the counts split accordingly"""
    import torch
    G = glvlib
    n = 256
    kw, mask, ops, table, w, texel = _chain(G, name, n)
    pkw = dict(dict(n=n, avg_frames=F, gravity_step=TEXEL_STEP if texel else FLOAT_STEP), **kw)
    dt = out_dtype(G, ops)
    pitch = _pitch(n)
    x, d_rec, _ = _recording("s16", 31, pitch)
    starts, urs, counts = _starts(n), _rates(texel), np.asarray(COUNTS)
    whole, parts = _make(G, pkw, mask, table, STREAMS), _make(G, pkw, mask, table, STREAMS)
    for b in (whole, parts): _process(b, "s16", _window(x, "s16", None, 9, n), ops, w, dt)
    one = _each(whole, "s16", d_rec, pitch, _dev_u32(starts, STEPS), _dev_ur(urs), _dev_u32(counts, 1), STEPS, ops, w, dt)
    a = _each(parts, "s16", d_rec, pitch, _dev_u32(starts[:, :6].copy(), 6), _dev_ur(urs[:, :6].copy()), _dev_u32(np.minimum(counts, 6), 1), 6, ops, w, dt)
    c = _each(parts, "s16", d_rec, pitch, _dev_u32(starts[:, 6:].copy(), 5), _dev_ur(urs[:, 6:].copy()), _dev_u32(np.maximum(counts, 6) - 6, 1), 5, ops, w, dt)
    assert eq(torch.cat([a, c]), one)
    assert bool((_blobs(parts) == _blobs(whole)).all())
    win = _window(x, "s16", None, 2, n)
    assert eq(_process(parts, "s16", win, ops, w, dt), _process(whole, "s16", win, ops, w, dt))
    whole.close(); parts.close()


# ---- 4. the wave form: per-stream windows, nothing else ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,bars", [("s16", False), ("s16", True), ("f32", True), ("planar", False)])
def test_the_wave_form_reads_every_stream_s_own_windows(glvlib, kind, bars):
    G = glvlib
    n = 1024
    ops = G.OP_WAVE | G.OP_R16 | (G.OP_BARS if bars else 0)
    pkw = dict(n=n, gl_storage=1, bars=n, bar_phase=0.5)
    pitch = _pitch(n)
    _, d_rec, _ = _recording(kind, 55, pitch)
    starts = _starts(n)
    dt = out_dtype(G, ops)
    b = G.Batch(G.Params(**pkw), STREAMS, ops)
    got = _each(b, kind, d_rec, pitch, _dev_u32(starts, STEPS), None, None, STEPS, ops, n, dt)
    assert b.last_launches() == (2 if bars else 1)
    for s in range(STREAMS):
        t = G.Batch(G.Params(**pkw), 1, ops)
        want = _shared(t, kind, d_rec[s:s + 1], pitch, _dev_u32(starts[s], 0), None, STEPS, ops, n, dt)
        assert eq(got[:, 2 * s:2 * s + 2], want), (s, differing(got[:, 2 * s:2 * s + 2], want))
        t.close()
    b.close()


# ---- 5. graph capture: all three tables are read when the kernels run ---------------------------------------------------------------------------------------------
def test_a_captured_call_is_reaimed_by_rewriting_the_three_tables(glvlib):
    import torch
    G = glvlib
    hip = C.CDLL("libamdhip64.so")
    n = 1024
    kw, mask, ops, table, w, texel = _chain(G, "gl_chain_r16", n)
    pkw = dict(dict(n=n, avg_frames=F, gravity_step=TEXEL_STEP), **kw)
    pitch = _pitch(n)
    x, d_rec, _ = _recording("s16", 13, pitch)
    starts_b, urs_b, counts_b = _starts(n), _rates(True), np.asarray(COUNTS, dtype=np.uint32)
    starts_a, urs_a, counts_a = np.full_like(starts_b, 5), np.full_like(urs_b, 50.0), np.full_like(counts_b, STEPS)
    bg, be = _make(G, pkw, mask, None, STREAMS), _make(G, pkw, mask, None, STREAMS)
    work = torch.zeros((bg.track_at_work_bytes(STEPS, ops),), dtype=torch.uint8, device="cuda")
    og = torch.zeros((STEPS, STREAMS * 2, n), dtype=torch.int16, device="cuda")
    d_starts, d_ur, d_counts = _dev_u32(starts_a, STEPS), _dev_ur(urs_a), _dev_u32(counts_a, 1)
    n_starts, n_ur, n_counts = _dev_u32(starts_b, STEPS), _dev_ur(urs_b), _dev_u32(counts_b, 1)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = C.c_void_p(st.cuda_stream)
    assert hip.hipStreamBeginCapture(sp, 0) == 0                    # hipStreamCaptureModeGlobal
    try:
        bg.track_each_s16(d_rec, pitch, d_starts, d_ur, d_counts, STEPS, og, work, ops, stream=st.cuda_stream)
    finally:
        graph = C.c_void_p()
        rc = hip.hipStreamEndCapture(sp, C.byref(graph))
    assert rc == 0
    count = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(count)) == 0 and count.value == bg.last_launches() == 2
    exe = C.c_void_p()
    assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
    with torch.cuda.stream(st):
        d_starts.copy_(n_starts); d_ur.copy_(n_ur); d_counts.copy_(n_counts)      # in stream order, in front of the replay
    assert hip.hipGraphLaunch(exe, sp) == 0
    st.synchronize()
    want = _each(be, "s16", d_rec, pitch, n_starts, n_ur, n_counts, STEPS, ops, n, torch.int16)
    assert eq(og, want), differing(og, want)
    assert bool((og[1:, 0:2] == 0).all()) and bool((og[:, 8:10] != 0).any())      # the rewritten counts: stream 0 stands still, stream 4 runs
    hip.hipGraphExecDestroy(exe); hip.hipGraphDestroy(graph)
    bg.close(); be.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_batch_untouched(glvlib):
    import torch
    G = glvlib
    n = 1024
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    pitch = _pitch(n)
    x, d_rec, _ = _recording("s16", 3, pitch)
    d_starts, d_ur, d_counts = _dev_u32(_starts(n), STEPS), _dev_ur(_rates(False)), _dev_u32(COUNTS, 1)
    out = torch.full((STEPS, STREAMS * 2, n), -7.0, dtype=torch.float32, device="cuda")
    work = torch.zeros((1 << 24,), dtype=torch.uint8, device="cuda")
    first = [_window(x, "s16", None, a, n) for a in (0, 5)]

    def refused(make, ops, code, **kw):
        a = dict(pitch_=pitch, tab=d_starts, ur=d_ur, cnt=d_counts, steps_=STEPS, o=out, w=work); a.update(kw)
        b, twin = make(), make()
        run = lambda bb, k: _process(bb, "s16", first[k], ops, n, out_dtype(G, ops))   # noqa: E731
        run(b, 0); run(twin, 0)
        launches = b.last_launches()
        with pytest.raises(G.GlvError) as ei:
            b.track_each_s16(d_rec, a["pitch_"], a["tab"], a["ur"], a["cnt"], a["steps_"], a["o"], a["w"], ops)
        assert ei.value.code == code, (kw, ei.value.code, str(ei.value))
        assert b.last_launches() == launches
        assert eq(run(b, 1), run(twin, 1)), "a refused call touched the state"
        b.close(); twin.close()

    base = G.Params(n=n)
    chain = lambda: G.Batch(base, STREAMS, GA)                                                                      # noqa: E731
    fft = lambda: G.Batch(base, STREAMS, G.OP_FFT)                                                                  # noqa: E731
    refused(fft, G.OP_FFT, G.ERR_INVALID, cnt=None)                                                                 # rates without gravity
    refused(fft, G.OP_FFT, G.ERR_INVALID, ur=None)                                                                  # counts without state
    refused(lambda: G.Batch(base, STREAMS, G.OP_AVERAGE), G.OP_FFT | G.OP_AVERAGE, G.ERR_INVALID)                   # rates without gravity, with state
    wave = G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5)
    refused(lambda: G.Batch(wave, STREAMS, G.OP_WAVE), G.OP_WAVE | G.OP_R16, G.ERR_INVALID, cnt=None)               # rates on the wave form
    refused(lambda: G.Batch(wave, STREAMS, G.OP_WAVE), G.OP_WAVE | G.OP_R16, G.ERR_INVALID, ur=None)                # counts on the wave form
    for kw in (dict(tab=None), dict(tab=d_starts.data_ptr() + 2), dict(ur=d_ur.data_ptr() + 2), dict(cnt=d_counts.data_ptr() + 1), dict(pitch_=n - 1), dict(steps_=0),
               dict(o=None), dict(w=work.data_ptr() + 64)):
        refused(chain, G.OP_FFT | GA, G.ERR_INVALID, **kw)
    refused(lambda: G.Batch(G.Params(n=n, gl_storage=2), STREAMS, GA), G.OP_FFT | GA, G.ERR_STATE)
    # ops no process call takes either: the table call's refusals, with its codes
    for make, ops, code in ((chain, G.OP_FFT | GA | G.OP_SMOOTH, G.ERR_INVALID), (chain, GA, G.ERR_INVALID), (fft, G.OP_FFT | GA, G.ERR_STATE)):
        b = make()
        with pytest.raises(G.GlvError) as ei:
            b.track_each_s16(d_rec, pitch, d_starts, d_ur, d_counts, STEPS, out, work, ops)
        assert ei.value.code == code, (ops, ei.value.code)
        assert b.last_launches() == 0
        b.close()
    # a NULL structure
    b = chain()
    assert G.lib().glv_batch_track_each_s16(b._h, d_rec.data_ptr(), pitch, None, STEPS, out.data_ptr(), work.data_ptr(), G.OP_FFT | GA, None) == G.ERR_INVALID
    assert b.last_launches() == 0
    b.close()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "a refused call wrote to the output"
