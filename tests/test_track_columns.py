"""GPU: track mode for the graph module (glv_batch_track_columns_s16 / _f32) -- the columns of every update of a recording in one call.

Contract (glv_batch_track_windows_s16's with columns as the output): the columns of step t and the batch's state afterwards are bit for bit what `steps`
consecutive glv_batch_process_s16 (glv_batch_process_f32_stereo) calls with the same column table produce and leave behind.  The sequential side is a
second batch driven window by window, the windows cut on the host from the same recording (the helpers of
tests/track_lib.py); floats are compared as int32.  Every call gets a workspace of exactly glv_batch_track_columns_work_bytes bytes and an output of
exactly steps * streams * 2 * cols floats, each followed by a guard region that must come back intact.

Two table widths per size: with the narrow one the process call fuses the columns into the transform's launch, with the wide one it runs
glv_columns_kernel over float rows as a second launch -- the track call is held to both.  (n = 256 has 16 lanes per row, which no process call fuses
behind: both of its widths are the two-launch form.  sample_mode maximum / hybrid never fuse either.)"""

import ctypes as C

import numpy as np
import pytest

from glava_amd.bar_positions import graph_column_texels
from track_lib import compare_hop, eq as _eq, hop_windows, pcm, pitch_odd, rec, seq as _seq, to_device, track

pytestmark = pytest.mark.gpu

STEPS, STREAMS = 11, 3          # F = 5: the ring wraps twice
LANES = {256: 16, 1024: 64, 4096: 128}                      # lanes per row of the sizes' default kernel configuration
WIDTHS = {256: (40, 200), 1024: (100, 320), 4096: (320, 800)}
F = np.float32


def _table(n, W):
    return np.ascontiguousarray(graph_column_texels(n, W)[0], np.int64)


def _process_launches(n, table, sample_mode=0):
    """the plan of a process call with columns: one launch where the distinct texels (+ the dump slot) fit behind the row as 16-bit values"""
    fused = sample_mode == 0 and LANES[n] % 64 == 0 and len(np.unique(table)) + 1 <= 4 * LANES[n]
    return 1 if fused else 2


def _chains(G):
    S, A = G.OP_GRAVITY, G.OP_AVERAGE
    return {"chain": (dict(avg_frames=5, avg_window_kind=1), S | A), "average_F1": (dict(avg_frames=1), A), "gravity": (dict(), S)}


def _pair(G, n, table, kw, state, streams=STREAMS, count=2):
    bs = []
    for _ in range(count):
        b = G.Batch(G.Params(n=n, bars=len(table), gl_storage=1, **kw), streams, state | G.OP_BARS)
        b.set_column_texels(table)
        bs.append(b)
    return bs


def _track(b, d_pcm, pitch, hop, steps, ops, cols, **kw):
    """steps [t0, t0 + steps) of the recording in one call (track_lib.track: workspace and output exactly as large as documented, a guard behind each)"""
    import torch
    return track(b, "columns", d_pcm, pitch, hop, steps, ops, cols, torch.float32, **kw)


def _compare(G, bt, bs, ops, n, hop, cols, seq_launches, steps=STEPS, odd=False, seed=31, f32=False, x=None):
    """one call against the sequential calls, every step, and the state through one more update on both"""
    pitch = pitch_odd(n, hop, steps + 1)
    if x is None:
        x = (rec if f32 else pcm)(seed + n + hop, bt.streams, pitch)
    got = compare_hop(G, bt, bs, "columns", x, odd, pitch, hop, n, steps, ops, cols, 3, "glv_columns_kernel", f32=f32)
    assert bs.last_launches() == seq_launches, (bs.last_launches(), seq_launches)
    assert bool((got != 0).any())
    return got


# ---- 1. the contract against sequential calls -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_mode", [0, 1])
@pytest.mark.parametrize("chain", ["chain", "average_F1", "gravity"])
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [256, 1024, 4096])
def test_track_columns_equal_sequential_calls(glvlib, n, wide, chain, log_mode):
    """hops 64, 37 and n + 5, odd pitches, the recording at an 8-byte boundary and one frame in"""
    G = glvlib
    kw, state = _chains(G)[chain]
    table = _table(n, WIDTHS[n][wide])
    bt, bs = _pair(G, n, table, dict(log_mode=log_mode, **kw), state)
    ops = G.OP_FFT | G.OP_BARS | state
    for i, hop in enumerate((64, 37, n + 5)):
        bt.reset(); bs.reset()
        _compare(G, bt, bs, ops, n, hop, len(table), _process_launches(n, table), odd=bool(i & 1))
    _compare(G, bt, bs, ops | G.OP_PRIVATE_STATE, n, 37, len(table), _process_launches(n, table), odd=True, seed=5)   # (continues; the flag is ignored)
    bt.close(); bs.close()


@pytest.mark.parametrize("sample_mode,channels", [(0, 1), (1, 2), (1, 1), (2, 2), (2, 1)])
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [256, 1024, 4096])
def test_track_columns_sample_modes_and_mono(glvlib, n, wide, sample_mode, channels):
    G = glvlib
    kw, state = _chains(G)["chain"]
    table = _table(n, WIDTHS[n][wide])
    bt, bs = _pair(G, n, table, dict(sample_mode=sample_mode, channels=channels, **kw), state)
    _compare(G, bt, bs, G.OP_FFT | G.OP_BARS | state, n, 37, len(table), _process_launches(n, table, sample_mode), odd=True)
    bt.close(); bs.close()


# ---- 2. independent of the columns kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1024, 4096])
def test_track_columns_equal_the_twins_texels_through_the_contract(glvlib, n):
    """the same recording through glv_batch_track_windows_s16 on the twin (bars = n, bar_phase 0.5, texels out, no table); its texels pushed through
    fdiv(fadd(fadd(T(l), T(m)), T(r)), 3.0f) in numpy float32 are the new call's output bit for bit"""
    import torch
    G = glvlib
    kw, state = _chains(G)["chain"]
    hop = 37
    pitch = pitch_odd(n, hop, STEPS)
    x = pcm(1234 + n, STREAMS, pitch)
    d_pcm = to_device(x, True, False)
    twin = G.Batch(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=1, **kw), STREAMS, state | G.OP_BARS)
    texels = track(twin, "windows", d_pcm, pitch, hop, STEPS, G.OP_FFT | G.OP_BARS | G.OP_R16 | state, n, torch.int16).cpu().numpy().view(np.uint16)
    T = (texels.astype(F) / F(65535)).astype(F)
    for W in WIDTHS[n]:
        table = _table(n, W)
        (b,) = _pair(G, n, table, kw, state, count=1)
        got = _track(b, d_pcm, pitch, hop, STEPS, G.OP_FFT | G.OP_BARS | state, len(table)).cpu().numpy()
        lm = (T[..., table[:, 0]] + T[..., table[:, 1]]).astype(F)
        want = ((lm + T[..., table[:, 2]]).astype(F) / F(3.0)).astype(F)
        assert (got.view(np.uint32) == want.view(np.uint32)).all(), (W, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        b.close()
    twin.close()


# ---- 3. the f32 entry ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [1024, 4096])
def test_track_columns_f32_equal_sequential_calls(glvlib, n, wide):
    """against glv_batch_process_f32_stereo, from a recording at a 16-byte boundary and one frame (8 bytes) behind one, with -0, +-Inf, NaN and denormal
    samples planted in window 0 and entering later windows one by one"""
    G = glvlib
    kw, state = _chains(G)["chain"]
    table = _table(n, WIDTHS[n][wide])
    hop = 37
    pitch = pitch_odd(n, hop, STEPS + 1)
    x = rec(7000 + n, STREAMS, pitch).copy()
    view = x.reshape(STREAMS, -1)
    for s in range(STREAMS):
        for k, v in enumerate(np.array([-0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 1.4e-45], np.float32)):
            if s == 1 and not np.isfinite(v):
                continue                                            # stream 1 keeps finite samples
            view[s, (97 * (k + 1) + 13 * s) % (2 * n)] = v
            view[s, 2 * (n + 3 * hop) + 2 * k + (k & 1)] = v
    bt, bs = _pair(G, n, table, kw, state)
    for odd in (False, True):
        bt.reset(); bs.reset()
        _compare(G, bt, bs, G.OP_FFT | G.OP_BARS | state, n, hop, len(table), _process_launches(n, table), odd=odd, f32=True, x=x)
    bt.close(); bs.close()


# ---- 4. composition and capture -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["chain", "gravity"])
def test_track_columns_chunks_compose_and_mix_with_process_calls(glvlib, chain):
    """track(4) then track(7) == track(11) in output and state; track(3), a process call, track(7); a track call then process calls == all sequential"""
    import torch
    G = glvlib
    n, hop = 1024, 37
    kw, state = _chains(G)[chain]
    table = _table(n, 320)
    cols = len(table)
    ops = G.OP_FFT | G.OP_BARS | state
    pitch = pitch_odd(n, hop, STEPS + 3)
    x = pcm(77, STREAMS, pitch)
    d_pcm = to_device(x, True, False)
    wins = hop_windows(x, n, hop, 0, STEPS + 3)
    bw, bs, bc, bm = _pair(G, n, table, kw, state, count=4)
    seq = _seq(bs, wins, ops, cols, torch.float32)                             # all sequential, STEPS + 3 updates
    whole = _track(bw, d_pcm, pitch, hop, STEPS, ops, cols)
    assert _eq(whole, seq[:STEPS])
    assert _eq(_seq(bw, wins[STEPS:], ops, cols, torch.float32), seq[STEPS:])  # a track call followed by process calls
    first = _track(bc, d_pcm, pitch, hop, 4, ops, cols)
    rest = _track(bc, d_pcm, pitch, hop, 7, ops, cols, t0=4)
    assert _eq(torch.cat([first, rest]), whole)
    assert _eq(_seq(bc, wins[STEPS:], ops, cols, torch.float32), seq[STEPS:])
    a = _track(bm, d_pcm, pitch, hop, 3, ops, cols)
    mid = _seq(bm, wins[3:4], ops, cols, torch.float32)
    c = _track(bm, d_pcm, pitch, hop, 7, ops, cols, t0=4)
    assert _eq(torch.cat([a, mid, c]), whole)
    assert _eq(_seq(bm, wins[STEPS:], ops, cols, torch.float32), seq[STEPS:])
    # ... and with the other track calls, the table cleared in between: windows(5) on the bars of glv_params, then the columns of steps [5, 11)
    bx, = _pair(G, n, table, kw, state, count=1)
    bx.set_column_texels(None)
    work = torch.zeros((bx.track_windows_work_bytes(pitch, hop, 5, ops),), dtype=torch.uint8, device="cuda")
    bars = torch.zeros((5, STREAMS * 2, cols), dtype=torch.float32, device="cuda")
    bx.track_windows_s16(d_pcm, pitch, hop, 5, bars, work, ops)
    bx.set_column_texels(table)
    assert _eq(_track(bx, d_pcm, pitch, hop, 6, ops, cols, t0=5), whole[5:])
    for b in (bw, bs, bc, bm, bx): b.close()


def test_first_track_columns_call_can_be_captured_and_replayed(glvlib):
    """the FIRST call after creation, captured into a hipGraph (global mode): a linear chain of three kernel nodes; one graph holds one full turn of
    the ring, so a replay continues like the same call issued again"""
    import torch
    G = glvlib
    hip = C.CDLL("libamdhip64.so")
    n, hop, Fr = 1024, 37, 5
    kw, state = _chains(G)["chain"]
    table = _table(n, 320)
    cols = len(table)
    ops = G.OP_FFT | G.OP_BARS | state
    pitch = pitch_odd(n, hop, Fr)
    d_pcm = to_device(pcm(9, STREAMS, pitch), True, False)
    bg, be = _pair(G, n, table, kw, state)
    work = torch.zeros((bg.track_columns_work_bytes(pitch, hop, Fr, ops),), dtype=torch.uint8, device="cuda")
    og = torch.zeros((Fr, STREAMS * 2, cols), dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = C.c_void_p(st.cuda_stream)
    assert hip.hipStreamBeginCapture(sp, 0) == 0                    # hipStreamCaptureModeGlobal
    try:
        bg.track_columns_s16(d_pcm, pitch, hop, Fr, og, work, ops, stream=st.cuda_stream)
    finally:
        graph = C.c_void_p()
        rc = hip.hipStreamEndCapture(sp, C.byref(graph))
    assert rc == 0
    count = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(count)) == 0 and count.value == 3
    nodes = (C.c_void_p * 3)()
    assert hip.hipGraphGetNodes(graph, nodes, C.byref(count)) == 0
    for node in nodes:
        kind = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(kind)) == 0 and kind.value == 0, kind.value     # hipGraphNodeTypeKernel
    edges = C.c_size_t(0)
    assert hip.hipGraphGetEdges(graph, None, None, C.byref(edges)) == 0 and edges.value == 2
    roots = C.c_size_t(0)
    assert hip.hipGraphGetRootNodes(graph, None, C.byref(roots)) == 0 and roots.value == 1                      # 3 nodes, 2 edges, 1 root: a chain
    exe = C.c_void_p()
    assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
    for rep in range(3):
        assert hip.hipGraphLaunch(exe, sp) == 0
        st.synchronize()
        want = _track(be, d_pcm, pitch, hop, Fr, ops, cols)
        assert _eq(og, want), rep
    hip.hipGraphExecDestroy(exe); hip.hipGraphDestroy(graph)
    bg.close(); be.close()


# ---- 5. workspace -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_mode", [0, 1])
def test_track_columns_read_nothing_no_stage_wrote(glvlib, sample_mode):
    """the workspace poisoned with 0xFF bytes (texel 65535 wherever something unwritten were read): the same output as from a zeroed workspace, which is
    the sequential one.  (The scan's store limit was measured and deleted: there is one form.)"""
    import torch
    G = glvlib
    n, hop = 1024, 37
    kw, state = _chains(G)["chain"]
    kw = dict(sample_mode=sample_mode, **kw)
    table = _table(n, 320)
    cols = len(table)
    ops = G.OP_FFT | G.OP_BARS | state
    pitch = pitch_odd(n, hop, STEPS)
    x = pcm(4321, STREAMS, pitch)
    d_pcm = to_device(x, False, False)
    (bs,) = _pair(G, n, table, kw, state, count=1)
    want = _seq(bs, hop_windows(x, n, hop, 0, STEPS), ops, cols, torch.float32)
    outs = []
    for fill in (0xFF, 0x00):
        (b,) = _pair(G, n, table, kw, state, count=1)
        outs.append(_track(b, d_pcm, pitch, hop, STEPS, ops, cols, fill=fill))
        b.close()
    for o in outs:
        assert _eq(o, want)
    bs.close()


# ---- 6. bookkeeping and refusals ----------------------------------------------------------------------------------------------------------
def test_track_columns_launches_name_query_and_timing(glvlib):
    import torch
    G = glvlib
    n, hop = 1024, 37
    kw, state = _chains(G)["chain"]
    table = _table(n, 320)
    ops = G.OP_FFT | G.OP_BARS | state
    pitch = pitch_odd(n, hop, STEPS)
    d_pcm = to_device(pcm(12, STREAMS, pitch), False, False)
    (b,) = _pair(G, n, table, kw, state, count=1)
    up = lambda v: (v + 255) & ~255                                               # noqa: E731
    for steps in (STEPS, 1):
        rows = steps * STREAMS * 2
        assert b.track_columns_work_bytes(pitch, hop, steps, ops) == 2 * up(rows * n * 2)
    b.timing_begin()
    _track(b, d_pcm, pitch, hop, STEPS, ops, len(table))
    ms, calls = b.timing_end()
    torch.cuda.synchronize()
    assert calls >= 1 and ms > 0.0, (ms, calls)
    assert b.last_launches() == 3 and b.kernel_name() == "glv_columns_kernel"
    b.close()


def test_track_columns_refusals_leave_the_batch_untouched(glvlib):
    import torch
    G = glvlib
    n, hop = 1024, 37
    kw, state = _chains(G)["chain"]
    table = _table(n, 320)
    cols = len(table)
    ops = G.OP_FFT | G.OP_BARS | state
    pitch = pitch_odd(n, hop, STEPS)
    x = pcm(3, STREAMS, pitch)
    d_pcm = to_device(x, False, False)
    xf = rec(3, STREAMS, pitch)
    d_f32 = to_device(xf, False, True)
    b, bs = _pair(G, n, table, kw, state)
    work = torch.zeros((b.track_columns_work_bytes(pitch, hop, STEPS, ops),), dtype=torch.uint8, device="cuda")
    out = torch.zeros((STEPS, STREAMS * 2, cols), dtype=torch.float32, device="cuda")
    b.track_columns_s16(d_pcm, pitch, hop, 2, out, work, ops)                    # a call that ran: what a refused one must leave alone
    torch.cuda.synchronize()
    assert b.last_launches() == 3
    before = out.clone()

    def refused(batch, code, ops_=ops, pitch_=pitch, hop_=hop, steps_=STEPS, pcm=d_pcm, o=out, w=work, query=True, f32=False, says=None):
        launches = batch.last_launches()
        with pytest.raises(G.GlvError) as ei:
            (batch.track_columns_f32 if f32 else batch.track_columns_s16)(pcm, pitch_, hop_, steps_, o, w, ops_)
        assert ei.value.code == code, (ei.value.code, str(ei.value))
        assert "glv error" in str(ei.value) and len(str(ei.value)) > 14           # a message in glv_last_error
        if says:
            assert says in str(ei.value), str(ei.value)
        assert batch.last_launches() == launches                                   # nothing was launched
        if query:                                                                  # the sizing query refuses the same arguments: 0, the code's name first
            assert G.lib().glv_batch_track_columns_work_bytes(batch._h, pitch_, hop_, steps_, ops_) == 0
            assert G.lib().glv_last_error().decode().startswith("GLV_ERR_STATE: " if code == G.ERR_STATE else "GLV_ERR_INVALID: ")
            with pytest.raises(G.GlvError) as ei:
                batch.track_columns_work_bytes(pitch_, hop_, steps_, ops_)
            assert ei.value.code == code

    for bad in (G.OP_RAW, G.OP_SMOOTH, G.OP_WRANGE, G.OP_MAGNITUDE, G.OP_WAVE, G.OP_OUTPUT_IS_STATE):
        refused(b, G.ERR_INVALID, ops_=ops | bad)
    refused(b, G.ERR_INVALID, ops_=ops & ~G.OP_FFT)                              # no GLV_OP_FFT
    refused(b, G.ERR_INVALID, ops_=ops & ~G.OP_BARS)                             # no GLV_OP_BARS
    refused(b, G.ERR_INVALID, steps_=0)
    refused(b, G.ERR_INVALID, hop_=0)
    refused(b, G.ERR_INVALID, pitch_=n + (STEPS - 1) * hop - 1)                  # one frame too short for the steps
    refused(b, G.ERR_INVALID, steps_=(2 ** 32 - 1) // (2 * STREAMS) + 1, hop_=1, pitch_=2 ** 32 - 1)     # more than 2^32 - 1 rows
    refused(b, G.ERR_INVALID, pcm=None, query=False)
    refused(b, G.ERR_INVALID, o=None, query=False)
    refused(b, G.ERR_INVALID, w=None, query=False)
    refused(b, G.ERR_INVALID, w=work.data_ptr() + 64, query=False)               # a workspace that is not 256-byte aligned
    refused(b, G.ERR_INVALID, pcm=d_f32.data_ptr() + 4, query=False, f32=True)   # a float d_pcm aligned like a float, not like a float frame
    # the state the call needs
    refused(b, G.ERR_STATE, ops_=ops | G.OP_R16)                                 # as the process call refuses it: the columns are floats
    refused(b, G.ERR_STATE, ops_=G.OP_FFT | G.OP_BARS)                           # a chain without state
    others = []
    none = G.Batch(G.Params(n=n, bars=cols, gl_storage=1, **kw), STREAMS, state | G.OP_BARS)
    refused(none, G.ERR_STATE, says="glv_batch_track_windows_")                  # no column table set
    others.append(none)
    for gl in (0, 2):
        o_ = G.Batch(G.Params(n=n, bars=cols, gl_storage=gl, **kw), STREAMS, state | G.OP_BARS)
        try:
            o_.set_column_texels(table)
        except G.GlvError:
            pass                                                                   # (a float chain has no texels to set columns on: refused for the missing table then)
        refused(o_, G.ERR_STATE)
        others.append(o_)
    live = G.Batch(G.Params(n=n, bars=cols, gl_storage=1, **kw), STREAMS, state | G.OP_BARS | G.OP_BARS_ONLY)
    live.set_column_texels(table)
    refused(live, G.ERR_STATE)
    unannounced = G.Batch(G.Params(n=n, bars=cols, gl_storage=1, **kw), STREAMS, G.OP_GRAVITY | G.OP_BARS)
    unannounced.set_column_texels(table)
    refused(unannounced, G.ERR_STATE)                                            # GLV_OP_AVERAGE without its ring
    mixed, = _pair(G, n, table, kw, state, count=1)
    mixed.process_s16(hop_windows(x, n, hop, 0, 1)[0], out[0].clone(), G.OP_FFT | G.OP_BARS | G.OP_GRAVITY)
    refused(mixed, G.ERR_STATE, query=False)                                     # the gravity form mix
    others += [live, unannounced, mixed]
    # the three existing track entries still refuse a batch with columns set
    for call, args in ((b.track_s16, (d_pcm, 64 * 40, 64, STEPS)), (b.track_windows_s16, (d_pcm, pitch, hop, STEPS))):
        with pytest.raises(G.GlvError) as ei:
            call(*args, out, work, ops)
        assert ei.value.code == G.ERR_STATE and "no columns form" in str(ei.value), str(ei.value)
    wave = G.Batch(G.Params(n=n, bars=cols, gl_storage=1, **kw), STREAMS, state | G.OP_BARS | G.OP_WAVE)
    wave.set_column_texels(table)
    with pytest.raises(G.GlvError) as ei:
        wave.track_wave_s16(d_pcm, pitch, hop, STEPS, out, work, G.OP_WAVE)
    assert ei.value.code == G.ERR_STATE
    others.append(wave)
    for o_ in others: o_.close()
    torch.cuda.synchronize()
    assert _eq(out, before), "a refused call wrote to the output"
    # after all the refused calls the batch continues from untouched state: steps [2, 11) here == sequential all the way on a fresh batch
    want = _seq(bs, hop_windows(x, n, hop, 0, STEPS), ops, cols, torch.float32)
    got = _track(b, d_pcm, pitch, hop, STEPS - 2, ops, cols, t0=2)
    assert _eq(before[:2], want[:2]) and _eq(got, want[2:])
    b.close(); bs.close()
