"""GPU: track mode over a pool of recordings (glv_batch_track_pool_s16 / _f32 / _f32_planar) -- the per-stream call with ONE buffer of PCM and a span per
stream in the place of a private, padded copy of a recording per stream.

Contract: output, state afterwards, head and launches are bit for bit those of glv_batch_track_each_* on the materialised copy d_pcm[s][i] = pool[first[s] + i],
i < frames[s], at pitch_frames = max frames[s], with table entries pre-clamped to frames[s] - k n.  tests/test_track_each.py holds that entry to one-stream
twins and the oracle; here a twin batch, created alike and brought to the same state by the same process calls, runs it on the copy, and outputs, the zero rows
behind the counts, glv_batch_save_streams blobs and one further process call are compared as integers.

The pool sits in the MIDDLE of a larger tensor with margins of 64 n frames in another pattern, so a wrong start shows as wrong bits and never as a fault; the
workspace and the output are exactly as large as asked with a guard behind each.  Spans: streams 0 and 1 on the same recording, stream 2 nested in it at
first % 8 == 1 and stream 3 at first % 8 == 3 with exactly k n frames (every entry clamps to 0), stream 4 ending on the pool's last frame.  Starts with repeats,
backward jumps and entries up to 0xFFFFFFF0.  5 streams, 11 steps, F = 5 with the head off 0, counts {0, 1, 7, 8, 11} (test_track_each's shape)."""
import ctypes as C

import numpy as np
import pytest

from glava_amd.track_starts import SPAN_DTYPE, pool_window_start
from test_track_each import COUNTS, F, STREAMS, _blobs, _buffers, _chain, _dev_u32, _dev_ur, _each, _guards, _make, _process, _rates
from track_lib import differing, eq, out_dtype, rec
from track_rates_lib import FLOAT_STEP, STEPS, TEXEL_STEP

pytestmark = pytest.mark.gpu


# ---- the pool, its spans, and the materialised copy ------------------------------------------------------------------------------------------------------
def _spans(span, pool_frames):
    """[(first, frames)] for the five streams of the module's docstring; span = k n"""
    a = (16, 3 * span + 700)                                                     # recording A: streams 0 and 1 (A ends on 4 mod 8: + 47 is 3 mod 8)
    return [a, a, (a[0] + 257, span + 300), (a[0] + a[1] + 8 * 5 + 7, span), (pool_frames - (2 * span + 123), 2 * span + 123)]


def _pool_frames(span):
    return 16 + 3 * span + 700 + 43 + span + 64 + 2 * span + 123 + 5            # odd: the planar pool's second row is 4-byte aligned and no more


def _starts(spans, span, steps=STEPS, streams=STREAMS):
    rows = [[7 * s + t * (61 + 23 * s) for t in range(steps)] for s in range(streams)]
    rows[2 % streams] = ([40, 40, 40, 300, 300, 12, 13, 500, 499, 498, 0] * 2)[:steps]
    rows[-1][-3:] = [spans[-1][1] - span + 1, spans[-1][1], 0xFFFFFFF0]
    return np.asarray(rows, dtype=np.uint32)


def _pool(kind, seed, pool_frames, n):
    """(host pool [pool_frames][2], device view of the pool inside a larger tensor: margins of 64 n frames of another pattern on both sides)"""
    import torch
    x = rec(seed, 1, pool_frames, kind != "s16")[0]                              # [pool_frames][2]
    body = np.ascontiguousarray(x.T if kind == "planar" else x).reshape(-1)      # planar: [2][pool_frames]
    margin = 64 * n * 2
    dt = torch.int16 if kind == "s16" else torch.float32
    flat = torch.full((margin + body.size + margin,), 3, dtype=dt, device="cuda")
    view = flat[margin:margin + body.size]
    view.copy_(torch.from_numpy(np.array(body, copy=True)))
    return x, view, flat


def _copy(x, kind, spans):
    """the materialised copy: d_pcm[s][i] = pool[first[s] + i], i < frames[s], zeros behind, at pitch = max frames; (host, device, pitch)"""
    import torch
    pitch = max(f for _, f in spans)
    m = np.zeros((len(spans), pitch, 2), dtype=x.dtype)
    for s, (first, frames) in enumerate(spans):
        m[s, :frames] = x[first:first + frames]
    host = np.ascontiguousarray(np.transpose(m, (0, 2, 1))) if kind == "planar" else m
    return host, torch.from_numpy(host.copy()).cuda(), pitch


def _dev_spans(spans, reserved=0xDEADBEEF):
    """the records on the device, 16-byte aligned, the word that is never read set"""
    import torch
    a = np.zeros((len(spans) + 1,), dtype=np.dtype(SPAN_DTYPE))
    for s, (first, frames) in enumerate(spans):
        a[s] = (first, frames, reserved)
    a[-1] = (0xFFFFFFFFFFFFFFF0, 0xFFFFFFFF, 0)                                  # behind the table: a read past it shows as wrong bits, never as a fault
    t = torch.from_numpy(a.view(np.int32).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _pool_call(b, kind, d_pool, pool_frames, d_spans, d_starts, d_ur, d_counts, steps, ops, w, dt, stream=None):
    import torch
    work, nbytes, flat, count, fill = _buffers(b, steps, ops, w, dt)
    name = "track_pool_" + ("f32_planar" if kind == "planar" else kind)
    getattr(b, name)(d_pool, pool_frames, d_spans, d_starts, d_ur, d_counts, steps, flat, work, ops, stream=stream)
    torch.cuda.synchronize()
    _guards(work, nbytes, flat, count, fill)
    return flat[:count].view(steps, b.streams * 2, w)


def _win(host, kind, start, frames):
    import torch
    w = host[:, :, start:start + frames] if kind == "planar" else host[:, start:start + frames, :]
    return torch.from_numpy(np.ascontiguousarray(w)).cuda()


def _chain_of(G, name, n):
    if name == "fft": return dict(), G.OP_FFT, G.OP_FFT, None, n, False          # stateless: the transform alone
    if name == "bars_only":
        kw, mask, ops, table, w, texel = _chain(G, "live", n)
        return kw, mask, ops, table, w, texel
    return _chain(G, name, n)


def _run(G, name, n, kind, with_ur=True, bufscale=1, grid=None, counts=COUNTS, spans=None, pre_clamp=True, seed=7):
    """the whole comparison of the module's docstring for one chain, size and input kind"""
    import torch
    kw, mask, ops, table, w, texel = _chain_of(G, name, n)
    state = bool(ops & (G.OP_GRAVITY | G.OP_AVERAGE))
    with_ur = with_ur and bool(ops & G.OP_GRAVITY)
    counts = counts if state else None
    pkw = dict(dict(n=n, avg_frames=F, gravity_step=TEXEL_STEP if texel else FLOAT_STEP), **kw)
    dt = out_dtype(G, ops)
    span = bufscale * n
    pool_frames = _pool_frames(span)
    spans = spans or _spans(span, pool_frames)
    x, d_pool, _ = _pool(kind, seed + n, pool_frames, n)
    starts = _starts(spans, span)
    host, d_copy, pitch = _copy(x, kind, spans)
    clamped = np.asarray([[min(int(e), max(fr - span, 0)) for e in row] for row, (_, fr) in zip(starts, spans)], dtype=np.uint32)
    urs = _rates(texel)
    bp, be = _make(G, pkw, mask, table, STREAMS, bufscale, grid), _make(G, pkw, mask, table, STREAMS, bufscale, grid)
    for start in (3, 11, 29):                                                    # the head off 0, the same state in both
        for b in (bp, be): _process(b, kind, _win(host, kind, start, span), ops, w, dt)
    d_ur = _dev_ur(urs) if with_ur else None
    d_counts = _dev_u32(counts, 1) if counts is not None else None
    got = _pool_call(bp, kind, d_pool, pool_frames, _dev_spans(spans), _dev_u32(starts, STEPS), d_ur, d_counts, STEPS, ops, w, dt)
    want = _each(be, kind, d_copy, pitch, _dev_u32(clamped if pre_clamp else starts, STEPS), d_ur, d_counts, STEPS, ops, w, dt)
    assert eq(got, want), (name, n, kind, differing(got, want))
    assert bp.last_launches() == be.last_launches() and bp.kernel_name() == be.kernel_name()
    if counts is not None and not (ops & G.OP_BARS):                             # the zero rows behind the counts
        for s, c in enumerate(counts):
            assert bool((got[min(c, STEPS):, 2 * s:2 * s + 2] == 0).all()), (name, s)
    if state:
        assert bool((_blobs(bp) == _blobs(be)).all()), (name, "blobs")
    win = _win(host, kind, 17, span)
    assert eq(_process(bp, kind, win, ops, w, dt), _process(be, kind, win, ops, w, dt)), (name, "next update")
    bp.close(); be.close()


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ur", [True, False])
@pytest.mark.parametrize("name", ["fft", "chain", "gl_bars"])
@pytest.mark.parametrize("kind", ["s16", "f32", "planar"])
def test_the_pool_call_is_the_per_stream_call_on_the_materialised_copy(glvlib, kind, name, with_ur):
    _run(glvlib, name, 256, kind, with_ur=with_ur)


# ---- 2. forms ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("bars_only", "s16"), ("gl_bar_texels", "f32"), ("columns", "planar"), ("upload", "s16"), ("chain_mono", "s16"), ("chain_mono", "f32"),
                                       ("chain_F1", "planar")])
def test_forms(glvlib, name, kind):
    _run(glvlib, name, 1024 if name in ("bars_only", "gl_bar_texels", "columns") else 256, kind)


@pytest.mark.parametrize("kind,bufscale", [("s16", 2), ("f32", 3), ("planar", 2), ("s16", 3)])
def test_bufscale(glvlib, kind, bufscale):
    _run(glvlib, "chain", 256, kind, bufscale=bufscale)


@pytest.mark.parametrize("kind,extra", [("s16", 0), ("s16", "bars"), ("f32", "bars"), ("planar", 0), ("f32", "float")])
def test_the_wave_form(glvlib, kind, extra):
    G = glvlib
    n = 1024
    ops = G.OP_WAVE | (0 if extra == "float" else G.OP_R16) | (G.OP_BARS if extra == "bars" else 0)
    pkw = dict(n=n, gl_storage=1, bars=n, bar_phase=0.5)
    pool_frames = _pool_frames(n)
    spans = _spans(n, pool_frames)
    x, d_pool, _ = _pool(kind, 55, pool_frames, n)
    host, d_copy, pitch = _copy(x, kind, spans)
    starts = _starts(spans, n)
    clamped = np.asarray([[min(int(e), max(fr - n, 0)) for e in row] for row, (_, fr) in zip(starts, spans)], dtype=np.uint32)
    dt = out_dtype(G, ops)
    bp, be = G.Batch(G.Params(**pkw), STREAMS, ops), G.Batch(G.Params(**pkw), STREAMS, ops)
    got = _pool_call(bp, kind, d_pool, pool_frames, _dev_spans(spans), _dev_u32(starts, STEPS), None, None, STEPS, ops, n, dt)
    want = _each(be, kind, d_copy, pitch, _dev_u32(clamped, STEPS), None, None, STEPS, ops, n, dt)
    assert eq(got, want), differing(got, want)
    assert bp.last_launches() == be.last_launches() == (2 if extra == "bars" else 1) and bp.kernel_name() == be.kernel_name()
    bp.close(); be.close()


# ---- 3. sizes, forced grids ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", [(1024, "f32"), (4096, "s16"), (16384, "planar")])
def test_sizes(glvlib, n, kind):
    _run(glvlib, "gl_chain_r16", n, kind)


@pytest.mark.parametrize("grid", [1, 2, 3])
def test_forced_grids_are_the_automatic_grid(glvlib, grid):
    """7 streams x 13 steps: three trips or more of every workgroup, a ragged last one"""
    import torch
    G = glvlib
    n, streams, steps = 256, 7, 13
    kw, mask, ops, table, w, texel = _chain(G, "gl_chain_r16", n)
    pkw = dict(dict(n=n, avg_frames=F, gravity_step=TEXEL_STEP), **kw)
    pool_frames = _pool_frames(n)
    five = _spans(n, pool_frames)
    spans = five + [five[2], five[4]]
    x, d_pool, _ = _pool("s16", 99, pool_frames, n)
    starts = _starts(spans, n, steps, streams)
    outs = []
    for g in (None, grid):
        b = _make(G, pkw, mask, table, streams, 1, g)
        outs.append(_pool_call(b, "s16", d_pool, pool_frames, _dev_spans(spans), _dev_u32(starts, steps), None, None, steps, ops, w, torch.int16))
        b.close()
    assert eq(outs[0], outs[1]), differing(outs[0], outs[1])


# ---- 4. malformed spans: the window pool_window_start names, never outside the pool ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,bufscale", [("s16", 1), ("f32", 1), ("planar", 1), ("s16", 2)])
def test_malformed_spans_read_where_the_rule_says(glvlib, kind, bufscale):
    """first + frames up to 16 n beyond the pool, frames < k n, first a little beyond pool_frames: values so small that even unclamped arithmetic stays inside
    the margins of 64 n frames.  Expected: glv_batch_track_each_* on a copy of the whole pool per stream, at the windows pool_window_start names."""
    import torch
    G = glvlib
    n = 256
    span = bufscale * n
    ops = G.OP_FFT
    pool_frames = _pool_frames(span)
    bad = [(pool_frames - span - 10, span + 16 * n), (100, span - 7), (pool_frames + 5, 2 * span), (pool_frames - 3, 5), (40, 3 * span)]
    x, d_pool, _ = _pool(kind, 21, pool_frames, n)
    starts = np.asarray([[(13 * s + 97 * t) % (3 * span) for t in range(STEPS)] for s in range(STREAMS)], dtype=np.uint32)
    named = [[pool_window_start(first, frames, int(e), pool_frames, span) for e in row] for row, (first, frames) in zip(starts, bad)]
    for row in named:
        assert all(0 <= w <= pool_frames - span for w in row)
    assert any(w == pool_frames - span for w in named[0]) and all(w == 100 for w in named[1]) and all(w == pool_frames - span for w in named[2])
    b1, b2 = _make(G, dict(n=n), ops, None, STREAMS, bufscale), _make(G, dict(n=n), ops, None, STREAMS, bufscale)
    dt = out_dtype(G, ops)
    got = _pool_call(b1, kind, d_pool, pool_frames, _dev_spans(bad), _dev_u32(starts, STEPS), None, None, STEPS, ops, n, dt)
    whole = [(0, pool_frames)] * STREAMS                                         # every stream over the whole pool, the entries the named windows
    _, d_copy, pitch = _copy(x, kind, whole)                                     # ... through the per-stream call: the reference runs none of the pool code
    assert pitch == pool_frames
    want = _each(b2, kind, d_copy, pitch, _dev_u32(np.asarray(named, dtype=np.uint32), STEPS), None, None, STEPS, ops, n, dt)
    assert eq(got, want), differing(got, want)
    b1.close(); b2.close()


# ---- 5. graph capture: spans and tables are read when the kernels run --------------------------------------------------------------------------------------------
def test_a_captured_call_is_reaimed_by_rewriting_spans_and_tables(glvlib):
    """the FIRST call of a batch captured, replayed as captured, then spans and all three tables rewritten in stream order and replayed again: each replay equal
    to the eager call of a twin (a gravity chain: its state is one row per channel, so two replays are two sequential calls)"""
    import torch
    G = glvlib
    hip = C.CDLL("libamdhip64.so")
    n = 1024
    kw, mask, ops, table, w, texel = _chain(G, "gravity", n)
    pkw = dict(dict(n=n, avg_frames=F, gravity_step=FLOAT_STEP), **kw)
    pool_frames = _pool_frames(n)
    spans_b = _spans(n, pool_frames)
    spans_a = [spans_b[4]] * STREAMS
    x, d_pool, _ = _pool("s16", 13, pool_frames, n)
    starts_b, urs_b, counts_b = _starts(spans_b, n), _rates(False), np.asarray(COUNTS, dtype=np.uint32)
    starts_a, urs_a, counts_a = np.full_like(starts_b, 5), np.full_like(urs_b, 50.0), np.full_like(counts_b, STEPS)
    bg, be = _make(G, pkw, mask, None, STREAMS), _make(G, pkw, mask, None, STREAMS)
    work = torch.zeros((bg.track_at_work_bytes(STEPS, ops),), dtype=torch.uint8, device="cuda")
    og = torch.zeros((STEPS, STREAMS * 2, n), dtype=torch.float32, device="cuda")
    d_spans, d_starts, d_ur, d_counts = _dev_spans(spans_a), _dev_u32(starts_a, STEPS), _dev_ur(urs_a), _dev_u32(counts_a, 1)
    n_spans, n_starts, n_ur, n_counts = _dev_spans(spans_b), _dev_u32(starts_b, STEPS), _dev_ur(urs_b), _dev_u32(counts_b, 1)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = C.c_void_p(st.cuda_stream)
    assert hip.hipStreamBeginCapture(sp, 0) == 0                    # hipStreamCaptureModeGlobal
    try:
        bg.track_pool_s16(d_pool, pool_frames, d_spans, d_starts, d_ur, d_counts, STEPS, og, work, ops, stream=st.cuda_stream)
    finally:
        graph = C.c_void_p()
        rc = hip.hipStreamEndCapture(sp, C.byref(graph))
    assert rc == 0
    count = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(count)) == 0 and count.value == bg.last_launches() == 2
    exe = C.c_void_p()
    assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
    assert hip.hipGraphLaunch(exe, sp) == 0                         # as captured
    st.synchronize()
    want = _pool_call(be, "s16", d_pool, pool_frames, _dev_spans(spans_a), _dev_u32(starts_a, STEPS), _dev_ur(urs_a), _dev_u32(counts_a, 1), STEPS, ops, n, torch.float32)
    assert eq(og, want), differing(og, want)
    with torch.cuda.stream(st):
        d_spans.copy_(n_spans); d_starts.copy_(n_starts); d_ur.copy_(n_ur); d_counts.copy_(n_counts)      # in stream order, in front of the replay
    assert hip.hipGraphLaunch(exe, sp) == 0
    st.synchronize()
    want = _pool_call(be, "s16", d_pool, pool_frames, n_spans, n_starts, n_ur, n_counts, STEPS, ops, n, torch.float32)
    assert eq(og, want), differing(og, want)
    assert bool((og[1:, 0:2] == 0).all()) and bool((og[:, 8:10] != 0).any())      # the rewritten counts: stream 0 runs one step, stream 4 all
    hip.hipGraphExecDestroy(exe); hip.hipGraphDestroy(graph)
    bg.close(); be.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_batch_untouched(glvlib):
    import torch
    G = glvlib
    n = 1024
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    pool_frames = _pool_frames(n)
    spans = _spans(n, pool_frames)
    x, d_pool, _ = _pool("s16", 3, pool_frames, n)
    host, _, _ = _copy(x, "s16", spans)
    d_spans, d_starts, d_ur, d_counts = _dev_spans(spans), _dev_u32(_starts(spans, n), STEPS), _dev_ur(_rates(False)), _dev_u32(COUNTS, 1)
    out = torch.full((STEPS, STREAMS * 2, n), -7.0, dtype=torch.float32, device="cuda")
    work = torch.zeros((1 << 24,), dtype=torch.uint8, device="cuda")
    first = [_win(host, "s16", a, n) for a in (0, 5)]

    def refused(make, ops, code, words, **kw):
        a = dict(pool=d_pool, frames=pool_frames, spans=d_spans, ur=d_ur, cnt=d_counts); a.update(kw)
        b, twin = make(), make()
        run = lambda bb, k: _process(bb, "s16", first[k], ops, n, out_dtype(G, ops))   # noqa: E731
        run(b, 0); run(twin, 0)
        launches = b.last_launches()
        with pytest.raises(G.GlvError) as ei:
            b.track_pool_s16(a["pool"], a["frames"], a["spans"], d_starts, a["ur"], a["cnt"], STEPS, out, work, ops)
        assert ei.value.code == code and words in str(ei.value), (kw, ei.value.code, str(ei.value))
        assert b.last_launches() == launches
        assert eq(run(b, 1), run(twin, 1)), "a refused call touched the state"
        b.close(); twin.close()

    base = G.Params(n=n)
    chain = lambda: G.Batch(base, STREAMS, GA)                                                                      # noqa: E731
    refused(chain, G.OP_FFT | GA, G.ERR_INVALID, "NULL device pointer", spans=None)
    refused(chain, G.OP_FFT | GA, G.ERR_INVALID, "NULL device pointer", pool=None)
    refused(chain, G.OP_FFT | GA, G.ERR_INVALID, "d_spans must be 16-byte aligned", spans=d_spans.data_ptr() + 8)
    refused(chain, G.OP_FFT | GA, G.ERR_INVALID, "holds no window", frames=n - 1)
    wave = G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5)
    refused(lambda: G.Batch(wave, STREAMS, G.OP_WAVE), G.OP_WAVE | G.OP_R16, G.ERR_INVALID, "GLV_OP_WAVE is stateless", cnt=None)      # d_ur with the wave form
    refused(lambda: G.Batch(G.Params(n=n, gl_storage=2), STREAMS, GA), G.OP_FFT | GA, G.ERR_STATE, "gl_storage 2")
    # a batch with bufscale: pool_frames = k n - 1
    b = G.Batch(base, STREAMS, GA); b.set_bufscale(2)
    with pytest.raises(G.GlvError) as ei:
        b.track_pool_s16(d_pool, 2 * n - 1, d_spans, d_starts, d_ur, d_counts, STEPS, out, work, G.OP_FFT | GA)
    assert ei.value.code == G.ERR_INVALID and "holds no window" in str(ei.value) and b.last_launches() == 0
    b.close()
    # a single-row batch: the glv_state drop-ins' batch is one row (the handle's first member is that batch)
    s, twin = G.State(G.Params(n=n)), G.State(G.Params(n=n))
    x0, x1 = np.linspace(-1, 1, n).astype(np.float32), np.linspace(0.5, -0.25, n).astype(np.float32)
    s.gravity(x0.copy()); twin.gravity(x0.copy())
    one_row = C.c_void_p(C.c_void_p.from_address(s._h.value).value)              # glv_state::b
    L = G.lib()
    tb = G.TrackTables(C.c_void_p(d_starts.data_ptr()), None, None)
    rc = L.glv_batch_track_pool_s16(one_row, C.c_void_p(d_pool.data_ptr()), pool_frames, C.c_void_p(d_spans.data_ptr()), C.byref(tb), STEPS, C.c_void_p(out.data_ptr()),
                                    C.c_void_p(work.data_ptr()), G.OP_FFT | G.OP_GRAVITY, None)
    assert rc == G.ERR_STATE and "a track call needs a batch of stereo streams" in L.glv_last_error().decode(), (rc, L.glv_last_error().decode())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "a refused call wrote its output"
    b1, b2 = x1.copy(), x1.copy()
    s.gravity(b1); twin.gravity(b2)
    assert np.array_equal(b1.view(np.int32), b2.view(np.int32)) and not np.array_equal(b1, x1), "a refused call touched the state"
    s.close(); twin.close()
    torch.cuda.synchronize()


# ---- 7. beyond 2^32 frames --------------------------------------------------------------------------------------------------------------------------------------
def test_spans_on_both_sides_of_2_to_the_32(glvlib):
    """an s16 pool of 2^32 + 64 n frames, uninitialised but for the windows used; spans with `first` below and above 2^32 against the same windows in a small pool"""
    import torch
    G = glvlib
    n = 1024
    big = (1 << 32) + 64 * n
    free, _ = torch.cuda.mem_get_info()
    if free < 32 << 30:
        print(f"skipped: {free >> 30} GiB free, the 16 GiB pool wants 32 GiB of headroom")
        pytest.skip("less than 32 GiB of device memory free")
    ops = G.OP_FFT
    src = rec(41, 1, 8 * n, False)[0]                                            # [8 n][2]: four recordings of 2 n frames
    firsts = [(1 << 32) - 4 * n - 3, (1 << 32) - n, (1 << 32) + n + 5, (1 << 32) + 62 * n - 1, 8]      # disjoint pieces of 2 n frames: below, across, above 2^32
    pool = torch.empty((big, 2), dtype=torch.int16, device="cuda")
    small = torch.from_numpy(np.concatenate([src, src[:2 * n]]).copy()).cuda()   # [10 n][2]
    spans_big, spans_small = [], []
    for s, first in enumerate(firsts):
        piece = small[2 * n * s:2 * n * (s + 1)]
        pool[first:first + 2 * n].copy_(piece)
        spans_big.append((first, 2 * n)); spans_small.append((2 * n * s, 2 * n))
    starts = np.asarray([[(37 * s + 101 * t) % (n + 9) for t in range(STEPS)] for s in range(STREAMS)], dtype=np.uint32)
    starts[:, -1] = 0xFFFFFFF0
    b1, b2 = G.Batch(G.Params(n=n), STREAMS, ops), G.Batch(G.Params(n=n), STREAMS, ops)
    dt = out_dtype(G, ops)
    got = _pool_call(b1, "s16", pool, big, _dev_spans(spans_big), _dev_u32(starts, STEPS), None, None, STEPS, ops, n, dt)
    want = _pool_call(b2, "s16", small, 10 * n, _dev_spans(spans_small), _dev_u32(starts, STEPS), None, None, STEPS, ops, n, dt)
    assert eq(got, want), differing(got, want)
    b1.close(); b2.close()
    del pool
