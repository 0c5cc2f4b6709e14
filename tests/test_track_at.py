"""GPU: track mode at given window starts (glv_batch_track_at_s16 / _f32) -- a table of positions in device memory in place of the hop.

Contract (the other track entries', word for word): step t of the output, and the batch's state afterwards, are bit for bit what `steps` consecutive
glv_batch_process_s16 / glv_batch_process_f32_stereo calls on the windows produce and leave behind, window t of stream s being the n frames of that
stream's recording from min(starts[t], pitch_frames - n) on.  The sequential side is a second batch fed windows cut on the host at the CLAMPED starts;
floats are compared as int32; the check runs on every step and, through one more update on both batches, on the state.  Every call gets a workspace
of exactly the queried size followed by a guard region, which must come back intact; pitches are odd with slack; the recording sits one frame behind
a load boundary where a test says `odd`.  The device allocation extends n frames of a different pattern behind the last stream, so that a missing
clamp shows as wrong bits and never as a read outside the allocation (no table entry here exceeds pitch_frames)."""

import ctypes as C

import numpy as np
import pytest

from glava_amd.bar_positions import graph_column_texels, radial_bar_texels
from glava_amd.track_starts import live_update_starts
from oracle_lib import lcg_pcm_fast
from track_lib import S16_CHAIN_SIZES, compare, eq as _eq, fft_kernel as _fft_name, launches_fft as _fft_launches, out_dtype as _dt, rec, s16_chains, seq as _seq
from track_lib import to_device, track, windows

pytestmark = pytest.mark.gpu

STEPS, STREAMS, F = 11, 3, 5          # F = 5: the ring wraps twice


def _table(name, n):
    """(starts [STEPS], pitch_frames): the shipped numbers at n >= 1024, scaled below; the pitch is odd, with slack behind the farthest window"""
    if name == "uniform":
        s = [t * 45 for t in range(STEPS)]
    elif name == "frac":                      # 22050 Hz at 60 fps: 367.5 frames a step, starts of both parities in a row
        k = 735 if n >= 1024 else 91
        s = [t * k // 2 for t in range(STEPS)]
    elif name == "live":                      # a live GLava's windows: updates of n / 16 frames, the latest complete one per render frame
        s = live_update_starts(22050, 60, 1, 4 * STEPS, max(n // 16, 1))[0][:STEPS]
    else:
        s = [5, 5, 0, 3 * n + 7, 3, 2 * n, 1, n // 2 + 1, 3 * n + 7, 2, n - 1]
    assert len(s) == STEPS
    pitch = (max(s) + n + 38) | 1
    if name == "clamped":                     # entries beyond pitch - n by k, 1 <= k <= n: one frame, half a window, a whole window
        for i, k in ((1, 1), (4, n // 2), (9, n)):
            s[i] = pitch - n + k
    return s, pitch


def _starts_dev(starts):
    import torch
    return torch.from_numpy(np.asarray(starts, dtype=np.uint32).view(np.int32).copy()).cuda()


def _windows_at(G, x, n, pitch, starts):
    """the sequential side's inputs: the window of every stream at each CLAMPED start, [streams][n][2] contiguous"""
    return windows(x, n, [G.track_at_start(pitch, n, s) for s in starts])


def _track_at(b, d_pcm, pitch, d_starts, steps, ops, w, dt, f32, **kw):
    """steps [t0, t0 + steps) of the table in one call (track_lib.track: exact workspace and output, guards behind both)"""
    return track(b, "at", d_pcm, pitch, d_starts, steps, ops, w, dt, f32=f32, **kw)


def _compare(G, bt, bs, ops, n, table, f32=False, odd=False, w=None, seed=31, launches=None, name=None):
    """one table call against the sequential calls, every step, and the state through one more update on both batches"""
    starts, pitch = _table(table, n)
    x = rec(seed + n, bt.streams, pitch, f32)
    at = [G.track_at_start(pitch, n, s) for s in starts + [7]]
    return compare(G, bt, bs, "at", x, to_device(x, odd, f32, tail_frames=n), pitch, _starts_dev(starts), at, n, STEPS, ops, n if w is None else w, launches, name,
                   f32=f32, what=(table, odd, starts))


# ---- 1. the windows form against sequential calls ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("log_mode", [0, 1])
@pytest.mark.parametrize("chain,n,variant", S16_CHAIN_SIZES)
def test_track_at_equals_sequential_calls(glvlib, chain, n, variant, log_mode, odd, f32):
    """table `frac`: consecutive windows change between the load forms; with the recording one frame off they change the other way round"""
    G = glvlib
    kw, mask, ops = s16_chains(G)[chain]
    p = G.Params(n=n, log_mode=log_mode, **kw)
    bt, bs = G.Batch(p, STREAMS, mask), G.Batch(p, STREAMS, mask)
    assert bt.variants() > variant
    bt.set_variant(variant)
    _compare(G, bt, bs, ops, n, "frac", f32=f32, odd=odd, launches=_fft_launches(G, ops), name=_fft_name(G, ops))
    assert bt.last_variant() == variant
    bt.close(); bs.close()


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("table", ["uniform", "live", "any_order", "clamped"])
@pytest.mark.parametrize("n,variant", [(256, 0), (1024, 1)])
@pytest.mark.parametrize("chain", ["fft", "chain", "gl_chain_r16", "chain_mono"])
def test_track_at_every_table(glvlib, chain, n, variant, table, f32):
    G = glvlib
    kw, mask, ops = s16_chains(G)[chain]
    p = G.Params(n=n, **kw)
    bt, bs = G.Batch(p, STREAMS, mask), G.Batch(p, STREAMS, mask)
    bt.set_variant(variant)
    _compare(G, bt, bs, ops, n, table, f32=f32, odd=True, launches=_fft_launches(G, ops), name=_fft_name(G, ops))
    bt.close(); bs.close()


# ---- 2. the uniform table against the hop entry ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("chain", ["fft", "fft_r16", "chain", "gl_chain_r16"])
def test_uniform_table_equals_the_hop_entry(glvlib, chain, f32):
    """t * 45 as a table: bit for bit the output and the state of glv_batch_track_windows_s16 / _f32 at hop 45, with its launches, kernel name and workspace"""
    import torch
    G = glvlib
    n, hop = 1024, 45
    kw, mask, ops = s16_chains(G)[chain]
    p = G.Params(n=n, **kw)
    dt = _dt(G, ops)
    starts, pitch = _table("uniform", n)
    x = rec(404, STREAMS, pitch, f32)
    d_pcm = to_device(x, True, f32, tail_frames=n)
    ba, bh = G.Batch(p, STREAMS, mask), G.Batch(p, STREAMS, mask)
    got = _track_at(ba, d_pcm, pitch, _starts_dev(starts), STEPS, ops, n, dt, f32)
    nbytes = bh.track_windows_work_bytes(pitch, hop, STEPS, ops)
    assert ba.track_at_work_bytes(STEPS, ops) == nbytes
    work = torch.zeros((nbytes,), dtype=torch.uint8, device="cuda")
    want = torch.zeros_like(got)
    (bh.track_windows_f32 if f32 else bh.track_windows_s16)(d_pcm, pitch, hop, STEPS, want, work, ops)
    torch.cuda.synchronize()
    assert _eq(got, want)
    assert ba.last_launches() == bh.last_launches() and ba.kernel_name() == bh.kernel_name()
    one_more = _windows_at(G, x, n, pitch, [7])
    assert _eq(_seq(ba, one_more, ops, n, dt, f32), _seq(bh, one_more, ops, n, dt, f32))
    ba.close(); bh.close()


# ---- 3. columns, live and wave -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("table", ["frac", "clamped"])
@pytest.mark.parametrize("n,pixels", [(256, 64), (1024, 320)])
def test_track_at_columns(glvlib, n, pixels, table, f32):
    G = glvlib
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    tex = graph_column_texels(n, pixels)[0]
    p = G.Params(n=n, bars=len(tex), gl_storage=1, avg_window_kind=1, avg_frames=F)
    bt, bs = G.Batch(p, STREAMS, GA | G.OP_BARS), G.Batch(p, STREAMS, GA | G.OP_BARS)
    bt.set_column_texels(tex); bs.set_column_texels(tex)
    ops = G.OP_FFT | GA | G.OP_BARS
    _compare(G, bt, bs, ops, n, table, f32=f32, odd=True, w=len(tex), launches=3, name="glv_columns_kernel")
    starts, pitch = _table(table, n)
    assert bt.track_at_work_bytes(STEPS, ops) == bt.track_columns_work_bytes(pitch, 1, STEPS, ops)
    bt.close(); bs.close()


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("table", ["frac", "clamped"])
@pytest.mark.parametrize("what,gl_storage", [("bars", 0), ("bars", 1), ("bar_texels", 1), ("columns", 1)])
def test_track_at_live(glvlib, what, gl_storage, table, f32):
    """a GLV_OP_BARS_ONLY batch: bars of a float chain and of a GL chain, bar texels, columns -- against the one-by-one live calls"""
    G = glvlib
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    n = 1024
    tex = radial_bar_texels(n, 160)[0] if what == "bar_texels" else graph_column_texels(n, 320)[0] if what == "columns" else None
    if gl_storage == 0:
        kw, ops = dict(bars=80), G.OP_FFT | GA | G.OP_BARS
    elif tex is None:
        kw, ops = dict(bars=n, bar_phase=0.5, gl_storage=1, avg_window_kind=1), G.OP_FFT | GA | G.OP_BARS | G.OP_R16
    else:
        kw, ops = dict(bars=len(tex), gl_storage=1, avg_window_kind=1), G.OP_FFT | GA | G.OP_BARS | (0 if what == "columns" else G.OP_R16)
    p = G.Params(n=n, avg_frames=F, **kw)
    mask = GA | G.OP_BARS | G.OP_BARS_ONLY
    bt, bs = G.Batch(p, STREAMS, mask), G.Batch(p, STREAMS, mask)
    if tex is not None:
        for b in (bt, bs): (b.set_column_texels if what == "columns" else b.set_bar_texels)(tex)
    _compare(G, bt, bs, ops, n, table, f32=f32, odd=True, w=kw["bars"], launches=3)
    starts, pitch = _table(table, n)
    assert bt.track_at_work_bytes(STEPS, ops) == bt.track_live_work_bytes(pitch, 1, STEPS, ops)
    bt.close(); bs.close()


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("table", ["frac", "clamped"])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("bars", [False, True])
def test_track_at_wave(glvlib, bars, channels, table, f32):
    G = glvlib
    n = 1024
    p = G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5, channels=channels)
    mask = G.OP_WAVE | (G.OP_BARS if bars else 0)
    ops = mask | G.OP_R16
    bt, bs = G.Batch(p, STREAMS, mask), G.Batch(p, STREAMS, mask)
    _compare(G, bt, bs, ops, n, table, f32=f32, odd=True, launches=2 if bars else 1)
    starts, pitch = _table(table, n)
    assert bt.track_at_work_bytes(STEPS, ops) == bt.track_wave_work_bytes(pitch, 1, STEPS, ops)
    bt.close(); bs.close()


def test_wave_with_bars_takes_two_launches_even_on_groups_of_eight(glvlib):
    """a 32-byte aligned recording, a pitch and every start multiples of 8 frames: the hop entry fuses into one launch, the table call cannot know and runs two"""
    import torch
    G = glvlib
    n, hop = 1024, 48
    p = G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5)
    mask = G.OP_WAVE | G.OP_BARS
    ops = mask | G.OP_R16
    pitch = n + STEPS * hop + 8
    assert pitch % 8 == 0
    x = lcg_pcm_fast(99, STREAMS * pitch * 2).reshape(STREAMS, pitch, 2)
    d_pcm = torch.from_numpy(x.reshape(-1).copy()).cuda()
    assert d_pcm.data_ptr() % 32 == 0
    starts = [t * hop for t in range(STEPS)]
    bt, bh = G.Batch(p, STREAMS, mask), G.Batch(p, STREAMS, mask)
    got = _track_at(bt, d_pcm, pitch, _starts_dev(starts), STEPS, ops, n, torch.int16, False)
    assert bt.last_launches() == 2
    want = torch.zeros_like(got)
    work = torch.zeros((bh.track_wave_work_bytes(pitch, hop, STEPS, ops),), dtype=torch.uint8, device="cuda")
    bh.track_wave_s16(d_pcm, pitch, hop, STEPS, want, work, ops)
    torch.cuda.synchronize()
    assert _eq(got, want)
    bt.close(); bh.close()


# ---- 4. chunks and mixing ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("chain", ["chain", "gl_chain_r16"])
def test_track_at_chunks_compose_and_calls_mix(glvlib, chain, f32):
    """4 steps then 7 on d_starts + 4 == 11 in one call; a table call, a hop call, two process calls == the sequential batch"""
    import torch
    G = glvlib
    n = 1024
    kw, mask, ops = s16_chains(G)[chain]
    p = G.Params(n=n, **kw)
    dt = _dt(G, ops)
    starts, pitch = _table("any_order", n)
    x = rec(808, STREAMS, pitch, f32)
    d_pcm = to_device(x, True, f32, tail_frames=n)
    d_starts = _starts_dev(starts)
    whole, parts, mixed, bs = (G.Batch(p, STREAMS, mask) for _ in range(4))
    one = _track_at(whole, d_pcm, pitch, d_starts, STEPS, ops, n, dt, f32)
    a = _track_at(parts, d_pcm, pitch, d_starts, 4, ops, n, dt, f32)
    c = _track_at(parts, d_pcm, pitch, d_starts, 7, ops, n, dt, f32, t0=4)
    assert _eq(torch.cat([a, c]), one)
    one_more = _windows_at(G, x, n, pitch, [7])
    assert _eq(_seq(parts, one_more, ops, n, dt, f32), _seq(whole, one_more, ops, n, dt, f32))
    # table(5), windows entry at hop 45 (4 steps from frame 9 on), two process calls
    hop, first = 45, 9
    got = [_track_at(mixed, d_pcm, pitch, d_starts, 5, ops, n, dt, f32)]
    work = torch.zeros((mixed.track_windows_work_bytes(pitch, hop, 4, ops),), dtype=torch.uint8, device="cuda")
    mid = torch.zeros((4, STREAMS * 2, n), dtype=dt, device="cuda")
    (mixed.track_windows_f32 if f32 else mixed.track_windows_s16)(d_pcm.data_ptr() + first * (8 if f32 else 4), pitch, hop, 4, mid, work, ops)
    got.append(mid)
    tail = _windows_at(G, x, n, pitch, [2 * n + 1, 11])
    got.append(_seq(mixed, tail, ops, n, dt, f32))
    order = starts[:5] + [first + t * hop for t in range(4)] + [2 * n + 1, 11]
    want = _seq(bs, _windows_at(G, x, n, pitch, order), ops, n, dt, f32)
    assert _eq(torch.cat(got), want)
    for b in (whole, parts, mixed, bs): b.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_track_at_refusals_leave_the_batch_untouched(glvlib):
    import torch
    G = glvlib
    n = 1024
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    ops = G.OP_FFT | GA
    starts, pitch = _table("any_order", n)
    x = rec(3, STREAMS, pitch, False)
    d_pcm = to_device(x, False, False, tail_frames=n)
    xf = rec(3, STREAMS, pitch, True)
    d_pcmf = to_device(xf, True, True, tail_frames=n)
    d_starts = _starts_dev(starts)
    p = G.Params(n=n)
    b = G.Batch(p, STREAMS, GA | G.OP_BARS)
    work = torch.zeros((b.track_at_work_bytes(STEPS, ops | G.OP_BARS),), dtype=torch.uint8, device="cuda")
    out = torch.zeros((STEPS, STREAMS * 2, n), dtype=torch.float32, device="cuda")
    b.track_at_s16(d_pcm, pitch, d_starts, 2, out, work, ops)
    torch.cuda.synchronize()
    assert b.last_launches() == 2
    before = out.clone()

    def refused(batch, code, ops_=ops, pitch_=pitch, steps_=STEPS, pcm=d_pcm, tab=d_starts, o=out, w=work, f32=False, query=False):
        launches = batch.last_launches()
        with pytest.raises(G.GlvError) as ei:
            (batch.track_at_f32 if f32 else batch.track_at_s16)(pcm, pitch_, tab, steps_, o, w, ops_)
        assert ei.value.code == code, (ei.value.code, str(ei.value))
        assert batch.last_launches() == launches                                   # nothing was launched
        if query:                                                                  # the sizing query refuses the same steps and ops: 0, the code's name first
            assert G.lib().glv_batch_track_at_work_bytes(batch._h, steps_, ops_) == 0
            assert G.lib().glv_last_error().decode().startswith("GLV_ERR_STATE: " if code == G.ERR_STATE else "GLV_ERR_INVALID: ")
            with pytest.raises(G.GlvError) as ei:
                batch.track_at_work_bytes(steps_, ops_)
            assert ei.value.code == code

    refused(b, G.ERR_INVALID, pitch_=n - 1)
    refused(b, G.ERR_INVALID, steps_=0, query=True)
    refused(b, G.ERR_INVALID, pcm=None)
    refused(b, G.ERR_INVALID, tab=None)
    refused(b, G.ERR_INVALID, o=None)
    refused(b, G.ERR_INVALID, w=None)
    refused(b, G.ERR_INVALID, tab=d_starts.data_ptr() + 2)                         # a table that is not 4-byte aligned
    refused(b, G.ERR_INVALID, w=work.data_ptr() + 64)                              # a workspace that is not 256-byte aligned
    refused(b, G.ERR_INVALID, pcm=d_pcmf.data_ptr() + 4, f32=True)                 # a float recording that is not 8-byte aligned
    refused(b, G.ERR_INVALID, steps_=(2 ** 32 - 1) // (2 * STREAMS) + 1, query=True)   # more than 2^32 - 1 rows
    refused(b, G.ERR_INVALID, ops_=GA, query=True)                                 # no GLV_OP_FFT
    for bad in (G.OP_RAW, G.OP_SMOOTH, G.OP_WRANGE, G.OP_MAGNITUDE):
        refused(b, G.ERR_INVALID, ops_=ops | bad, query=True)
    refused(b, G.ERR_INVALID, ops_=G.OP_FFT | G.OP_WAVE, query=True)               # the wave form's own ops rule
    gl2 = G.Batch(G.Params(n=n, gl_storage=2), STREAMS, GA)
    refused(gl2, G.ERR_STATE, query=True)
    unannounced = G.Batch(p, STREAMS, G.OP_FFT)
    refused(unannounced, G.ERR_STATE, query=True)                                  # what the process call refuses
    live = G.Batch(G.Params(n=n, gl_storage=1), STREAMS, GA | G.OP_BARS | G.OP_BARS_ONLY)
    refused(live, G.ERR_INVALID, query=True)                                       # the live form's own ops rule: bars are part of the call
    mixed = G.Batch(p, STREAMS, GA)
    mixed.process_s16(_windows_at(G, x, n, pitch, [0])[0], out[0].clone(), G.OP_FFT | G.OP_GRAVITY)
    refused(mixed, G.ERR_STATE)                                                    # the gravity form mix, as a process call refuses it
    for x_ in (gl2, unannounced, live, mixed): x_.close()
    torch.cuda.synchronize()
    assert _eq(out, before), "a refused call wrote to the output"
    # after all the refused calls the batch continues from untouched state: steps [2, 11) here == sequential all the way on a fresh batch
    bs = G.Batch(p, STREAMS, GA | G.OP_BARS)
    want = _seq(bs, _windows_at(G, x, n, pitch, starts), ops, n, torch.float32, False)
    got = _track_at(b, d_pcm, pitch, d_starts, STEPS - 2, ops, n, torch.float32, False, t0=2)
    assert _eq(before[:2], want[:2]) and _eq(got, want[2:])
    b.close(); bs.close()


# ---- 6. graph capture: the table is read when the kernels run ----------------------------------------------------------------------------------------
def test_a_captured_call_is_reaimed_by_rewriting_the_table(glvlib):
    """the FIRST call after creation captured into a hipGraph (global mode); replayed twice with the table rewritten in between: the first replay shows
    table A, the second table B from the state the first left (F steps a graph: the ring's head, which the host advances, comes round).  The graph is a chain."""
    import torch
    G = glvlib
    hip = C.CDLL("libamdhip64.so")
    n = 1024
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    ops = G.OP_FFT | GA | G.OP_R16
    p = G.Params(n=n, gl_storage=1, avg_window_kind=1, avg_frames=F)
    table_a, pitch = _table("any_order", n)
    table_a = table_a[:F]
    table_b = [3 * n, 1, pitch, 17, n + 5]                                         # (pitch: clamped)
    x = rec(9, STREAMS, pitch, False)
    d_pcm = to_device(x, True, False, tail_frames=n)
    bg, be = G.Batch(p, STREAMS, GA), G.Batch(p, STREAMS, GA)
    work = torch.zeros((bg.track_at_work_bytes(F, ops),), dtype=torch.uint8, device="cuda")
    og = torch.zeros((F, STREAMS * 2, n), dtype=torch.int16, device="cuda")
    d_starts = _starts_dev(table_a)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = C.c_void_p(st.cuda_stream)
    assert hip.hipStreamBeginCapture(sp, 0) == 0                    # hipStreamCaptureModeGlobal
    try:
        bg.track_at_s16(d_pcm, pitch, d_starts, F, og, work, ops, stream=st.cuda_stream)
    finally:
        graph = C.c_void_p()
        rc = hip.hipStreamEndCapture(sp, C.byref(graph))
    assert rc == 0
    # a chain: as many nodes as launches, one root, every other node behind exactly one
    count = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(count)) == 0 and count.value == bg.last_launches() == 2
    roots = C.c_size_t(0)
    assert hip.hipGraphGetRootNodes(graph, None, C.byref(roots)) == 0 and roots.value == 1
    edges = C.c_size_t(0)
    assert hip.hipGraphGetEdges(graph, None, None, C.byref(edges)) == 0 and edges.value == count.value - 1
    exe = C.c_void_p()
    assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
    for table in (table_a, table_b):
        d_starts.copy_(_starts_dev(table))
        torch.cuda.synchronize()
        assert hip.hipGraphLaunch(exe, sp) == 0
        st.synchronize()
        want = _seq(be, _windows_at(G, x, n, pitch, table), ops, n, torch.int16, False)
        assert _eq(og, want), table
    hip.hipGraphExecDestroy(exe); hip.hipGraphDestroy(graph)
    bg.close(); be.close()
