"""GPU: several updates of a ring batch in one track call (glv_batch_ring_track_s16 / _f32).

Contract: with R_s = stream s's ring read oldest frame first followed by its updates * new_frames new frames, update t transforms frames [(t + 1) * nf,
(t + 1) * nf + n) of R_s, and every output row, the gravity and average state, head and the rings (oldest first) are bit for bit those of `updates`
sequential glv_batch_ring_update_* calls; the call is also bit for bit glv_batch_track_at_* on the materialised R_s with starts[t] = (t + 1) * nf.

Twin batches start from the same history: three glv_batch_ring_update_* calls of 37 frames on each, so that the ring position (111) is neither 0 nor a
multiple of four frames and the state is not zero.  The call under test gets a workspace of exactly the queried size and an output of exactly updates *
streams * 2 * w elements, each followed by a guard (track_lib.GUARD) that must come back intact.  Floats are compared as int32."""
import ctypes as C

import numpy as np
import pytest

from glava_amd import spectrum as _S
from glava_amd.bar_positions import graph_column_texels, radial_bar_texels
from track_lib import GUARD, REDUCED_CHAINS, base_chains, differing, eq as _eq, launches_fft, out_dtype as _dt, rec, to_device, with_table

pytestmark = pytest.mark.gpu

F = 3
UPDATES = 2 * F + 4
HISTORY, HISTORY_NF = 3, 37
FORMS = REDUCED_CHAINS + ["bars_snap", "live", "columns", "upload_r16", "wave_r16", "wave_bars", "wave_mono"]


def _form(G, name, n):
    """(parameters, creation mask, ops, table, row width)"""
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    gl = dict(gl_storage=1, avg_window_kind=1)
    if name in REDUCED_CHAINS:
        kw, mask, ops = base_chains(G)[name]
        return kw, mask, ops, None, n
    if name == "bars_snap":
        tex = radial_bar_texels(n, 256)[0]
        return dict(bars=len(tex), **gl), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16, ("bar", tex), len(tex)
    if name == "live":
        return dict(bars=n, bar_phase=0.5, smooth_factor=0.025, **gl), GA | G.OP_BARS | G.OP_BARS_ONLY, G.OP_FFT | GA | G.OP_BARS | G.OP_R16, None, n
    if name == "columns":
        tex = graph_column_texels(n, 64 if n == 256 else 320)[0]
        return dict(bars=len(tex), **gl), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS, ("col", tex), len(tex)
    if name == "upload_r16":
        return dict(gl_storage=3), GA, G.OP_FFT | GA | G.OP_R16, None, n
    wave = dict(gl_storage=1, bars=n, bar_phase=0.5, channels=1 if name == "wave_mono" else 2)
    if name == "wave_bars":
        return wave, G.OP_WAVE | G.OP_BARS, G.OP_WAVE | G.OP_BARS | G.OP_R16, None, n
    return wave, G.OP_WAVE, G.OP_WAVE | G.OP_R16, None, n


def _launches(G, ops):
    """what include/glv_spectrum.h states for the form: the table call's launches and the two copies around them"""
    if ops & G.OP_WAVE:
        return 2 + (2 if ops & G.OP_BARS else 1)
    return 2 + launches_fft(G, ops)


def _batch(G, name, n, streams, f32, avg_frames=F):
    kw, mask, ops, table, w = _form(G, name, n)
    kw = dict(kw)
    kw.setdefault("avg_frames", avg_frames)
    b = with_table(G.Batch(G.Params(n=n, **kw), streams, mask | (G.OP_RING_F32 if f32 else G.OP_RING_S16)), table)
    return b, ops, w


def _update(b, chunk, nf, ops, w, f32):
    """one glv_batch_ring_update_* call; chunk: host frames [streams][nf][2], or None for the zero fill"""
    import torch
    o = torch.zeros((b.streams * 2, w), dtype=_dt(_S, ops), device="cuda")
    d = None if chunk is None else torch.from_numpy(np.array(chunk, copy=True)).cuda()      # (a copy: the shared recordings are read-only)
    (b.ring_update_f32 if f32 else b.ring_update_s16)(d, nf, o, ops)
    torch.cuda.synchronize()
    return o


def _history(n, streams, f32, seed=5):
    return rec(seed + n, streams, HISTORY * HISTORY_NF, f32)


def _warm(b, ops, w, f32, n):
    """the shared history: three updates of 37 frames"""
    h = _history(n, b.streams, f32)
    for k in range(HISTORY):
        _update(b, h[:, k * HISTORY_NF:(k + 1) * HISTORY_NF], HISTORY_NF, ops, w, f32)


def _sequential(b, new, nf, updates, ops, w, f32):
    import torch
    return torch.stack([_update(b, None if new is None else new[:, t * nf:(t + 1) * nf], nf, ops, w, f32) for t in range(updates)])


def _ring_track(b, d_new, nf, updates, ops, w, f32, fill=0xA5):
    """one call with a workspace of exactly the queried size and an output of exactly updates * streams * 2 * w elements, guards behind both"""
    import torch
    dt = _dt(_S, ops)
    nbytes = b.ring_track_work_bytes(nf, updates, ops)
    work = torch.full((nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
    assert work.data_ptr() % 256 == 0
    count = updates * b.streams * 2 * w
    sentinel = 23130 if dt == torch.int16 else -7.0
    flat = torch.zeros((count + GUARD,), dtype=dt, device="cuda")
    flat[count:] = sentinel
    (b.ring_track_f32 if f32 else b.ring_track_s16)(d_new, nf, updates, flat, work, ops)
    torch.cuda.synchronize()
    assert bool((work[nbytes:] == fill).all()), "the call wrote behind the workspace it asked for"
    assert bool((flat[count:] == sentinel).all()), "the call wrote behind its output"
    return flat[:count].view(updates, b.streams * 2, w)


def _blobs(b):
    import torch
    nbytes = b.stream_state_desc().bytes
    if nbytes == 0:
        return None
    blob = torch.zeros((b.streams * nbytes,), dtype=torch.uint8, device="cuda")
    idx = torch.arange(b.streams, dtype=torch.int32, device="cuda")
    b.save_streams(idx, b.streams, blob)
    torch.cuda.synchronize()
    return blob


def _planar(b, f32):
    import torch
    o = torch.zeros((b.streams, 2, b.params.n), dtype=torch.float32, device="cuda")
    b.ring_planar(o, f32_ring=f32)
    torch.cuda.synchronize()
    return o


def _same_after(bt, bs, ops, w, f32, n, seed=71):
    """the state both batches are left in: the blobs of every stream, the rings as the backends publish them, and one more update on each"""
    import torch
    a, c = _blobs(bt), _blobs(bs)
    assert (a is None) == (c is None)
    if a is not None:
        assert bool((a == c).all()), ("blobs", int((a != c).sum()))
    assert _eq(_planar(bt, f32), _planar(bs, f32)), "rings"
    more = rec(seed, bt.streams, HISTORY_NF, f32)
    assert _eq(_update(bt, more, HISTORY_NF, ops, w, f32), _update(bs, more, HISTORY_NF, ops, w, f32)), "one more update"


def _pair(G, name, n, streams, f32):
    bt, ops, w = _batch(G, name, n, streams, f32)
    bs, _, _ = _batch(G, name, n, streams, f32)
    for b in (bt, bs):
        _warm(b, ops, w, f32, n)
    return bt, bs, ops, w


def _against_sequential(G, name, n, nf, f32, streams, updates=UPDATES, odd=True, seed=900):
    bt, bs, ops, w = _pair(G, name, n, streams, f32)
    new = rec(seed + nf, streams, updates * nf, f32)
    got = _ring_track(bt, to_device(new, odd, f32), nf, updates, ops, w, f32)
    assert bt.last_launches() == _launches(G, ops), (bt.last_launches(), name)
    want = _sequential(bs, new, nf, updates, ops, w, f32)
    for t in range(updates):
        assert _eq(got[t], want[t]), (name, n, nf, f32, t, differing(got[t], want[t]))
    _same_after(bt, bs, ops, w, f32, n)
    bt.close(); bs.close()


# ---- 1. against sequential calls ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("nf", [1, 37, 64, "n"])
@pytest.mark.parametrize("n", [256, 1024])
@pytest.mark.parametrize("form", FORMS)
def test_ring_track_equals_sequential_ring_updates(glvlib, form, n, nf, f32):
    """updates * nf below n (nf 1 and 37; 64 at n = 1024), a ring replaced several times over (nf = n: ten times), odd byte offsets on both sides of the
    copy (the ring at frame 111, the new frames one frame behind a load boundary, 37 frames a stream); 1 and 3 streams"""
    nf = n if nf == "n" else nf
    _against_sequential(glvlib, form, n, nf, f32, streams=3 if nf in (37, n) else 1)


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
def test_ring_track_from_aligned_new_frames(glvlib, f32):
    """the new frames on a load boundary with a multiple of four frames a stream: the 16-byte loads of the new-frames side"""
    _against_sequential(glvlib, "chain", 256, 64, f32, streams=3, odd=False)


# ---- 2. against a table call on the materialised recordings -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
def test_ring_track_equals_the_table_call_on_the_materialised_recordings(glvlib, f32):
    import torch
    G = glvlib
    n, nf, streams, name = 1024, 37, 3, "chain"
    bt, ops, w = _batch(G, name, n, streams, f32)
    _warm(bt, ops, w, f32, n)
    ba, _, _ = _batch(G, name, n, streams, f32)                                   # the table call's batch: the same state, through the same history
    _warm(ba, ops, w, f32, n)
    history = _history(n, streams, f32)
    new = rec(1234, streams, UPDATES * nf, f32)
    # R_s on the host: the ring oldest first (zeros, then the history's frames: what glv_batch_ring_planar publishes) followed by the new frames
    ring = np.zeros((streams, n, 2), dtype=history.dtype)
    ring[:, n - HISTORY * HISTORY_NF:] = history
    planar = _planar(bt, f32).cpu().numpy()
    if f32:
        assert np.array_equal(planar[:, 0], ring[:, :, 0]) and np.array_equal(planar[:, 1], ring[:, :, 1])
    else:                                                                         # (the order, not the unpack: one increasing function of the raw samples, frame for frame)
        for c in range(2):
            raw, pub = ring[:, :, c].ravel().astype(np.int64), planar[:, c].ravel()
            order = np.argsort(raw, kind="stable")
            dr, dp = np.diff(raw[order]), np.diff(pub[order])
            assert (dp[dr > 0] > 0).all() and (dp[dr == 0] == 0).all(), c
    r = np.ascontiguousarray(np.concatenate([ring, new], axis=1))
    pitch = n + UPDATES * nf
    starts = torch.from_numpy(np.asarray([(t + 1) * nf for t in range(UPDATES)], dtype=np.int32)).cuda()
    got = _ring_track(bt, to_device(new, True, f32), nf, UPDATES, ops, w, f32)
    work = torch.zeros((ba.track_at_work_bytes(UPDATES, ops),), dtype=torch.uint8, device="cuda")
    want = torch.zeros_like(got)
    (ba.track_at_f32 if f32 else ba.track_at_s16)(to_device(r, True, f32), pitch, starts, UPDATES, want, work, ops)
    torch.cuda.synchronize()
    assert _eq(got, want), differing(got, want)
    assert bt.last_launches() == ba.last_launches() + 2
    # the state both are left in (head, gravity and average rows), through one process call on a common window: the table call's batch keeps its old ring
    win = torch.from_numpy(np.array(rec(71, streams, n, f32), copy=True)).cuda()
    oa, ot = torch.zeros((streams * 2, w), dtype=torch.float32, device="cuda"), torch.zeros((streams * 2, w), dtype=torch.float32, device="cuda")
    (ba.process_f32_stereo if f32 else ba.process_s16)(win, oa, ops)
    (bt.process_f32_stereo if f32 else bt.process_s16)(win, ot, ops)
    torch.cuda.synchronize()
    assert _eq(ot, oa), "state"
    bt.close(); ba.close()


# ---- 3. zero fill -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["chain", "wave_r16"])
def test_zero_fill_equals_sequential_zero_fills(glvlib, form):
    G = glvlib
    n, nf, streams = 256, 37, 3
    bt, bs, ops, w = _pair(G, form, n, streams, False)
    got = _ring_track(bt, None, nf, UPDATES, ops, w, False)
    want = _sequential(bs, None, nf, UPDATES, ops, w, False)
    assert _eq(got, want), differing(got, want)
    _same_after(bt, bs, ops, w, False, n)
    bt.close(); bs.close()


def test_the_f32_entry_refuses_a_null_d_new(glvlib):
    G = glvlib
    bt, bs, ops, w = _pair(G, "chain", 256, 3, True)
    with pytest.raises(G.GlvError) as ei:
        _ring_track(bt, None, 37, 2, ops, w, True)
    assert ei.value.code == G.ERR_INVALID
    _same_after(bt, bs, ops, w, True, 256)
    bt.close(); bs.close()


# ---- 4. two calls in a row ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("form", ["chain", "gl_chain_r16", "wave_bars"])
def test_two_calls_in_a_row_equal_one_sequential_run(glvlib, form, f32):
    """the second call starts from the ring position the first one chose, a third from the second's, each at another nf"""
    import torch
    G = glvlib
    n, streams = 256, 3
    bt, bs, ops, w = _pair(G, form, n, streams, f32)
    for k, (nf, updates) in enumerate(((37, 5), (64, 4), (n, 3), (1, 6))):
        new = rec(40 + k, streams, updates * nf, f32)
        got = _ring_track(bt, to_device(new, k % 2 == 0, f32), nf, updates, ops, w, f32)
        want = _sequential(bs, new, nf, updates, ops, w, f32)
        assert _eq(got, want), (k, differing(got, want))
    _same_after(bt, bs, ops, w, f32, n)
    bt.close(); bs.close()


# ---- 5. the workspace ---------------------------------------------------------------------------------------------------------------------------------
def test_the_query_is_the_staged_recordings_the_table_and_the_table_call_s_workspace(glvlib):
    G = glvlib
    up = lambda v: (v + 255) & ~255                                                # noqa: E731
    for f32 in (False, True):
        for name, n, nf, updates, streams in (("chain", 256, 37, 10, 3), ("fft", 1024, 1, 7, 1), ("wave_bars", 256, 256, 3, 3), ("columns", 1024, 64, 5, 3)):
            b, ops, w = _batch(G, name, n, streams, f32)
            pitch = (n + updates * nf + 3) & ~3
            want = up(streams * pitch * (8 if f32 else 4)) + up(updates * 4) + b.track_at_work_bytes(updates, ops)
            assert b.ring_track_work_bytes(nf, updates, ops) == want, (name, f32)
            b.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_move_nothing(glvlib):
    import torch
    G = glvlib
    n, streams, nf = 256, 3, 37
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    bt, bs, ops, w = _pair(G, "chain", n, streams, False)
    new = to_device(rec(8, streams, 4 * n, False), False, False)
    newf = to_device(rec(8, streams, 4 * n, True), False, True)
    work = torch.zeros((bt.ring_track_work_bytes(n, 4, ops),), dtype=torch.uint8, device="cuda")
    out = torch.zeros((4, streams * 2, n), dtype=torch.float32, device="cuda")

    def refused(batch, code, d_new=new, nf_=nf, updates=4, o=out, wk=work, ops_=ops, f32=False, text=None):
        with pytest.raises(G.GlvError) as ei:
            (batch.ring_track_f32 if f32 else batch.ring_track_s16)(d_new, nf_, updates, o, wk, ops_)
        assert ei.value.code == code, (ei.value.code, str(ei.value))
        if text is not None:
            assert text in str(ei.value), str(ei.value)

    refused(bt, G.ERR_STATE, d_new=newf, f32=True)                                 # a batch without the f32 ring
    plain = G.Batch(G.Params(n=n, avg_frames=F), streams, GA)
    refused(plain, G.ERR_STATE)                                                    # ... without any ring
    assert G.lib().glv_batch_ring_track_work_bytes(plain._h, nf, 4, ops) == 0 and G.lib().glv_last_error().decode().startswith("GLV_ERR_STATE: ")
    refused(bt, G.ERR_INVALID, nf_=n + 1)
    refused(bt, G.ERR_INVALID, nf_=0)
    refused(bt, G.ERR_INVALID, updates=0)
    refused(bt, G.ERR_INVALID, d_new=new.data_ptr() + 2)                           # s16 frames off 4 bytes
    refused(bt, G.ERR_INVALID, o=None)
    refused(bt, G.ERR_INVALID, wk=None)
    refused(bt, G.ERR_INVALID, wk=work.data_ptr() + 64)
    refused(bt, G.ERR_INVALID, updates=(2 ** 32 - 1) // (2 * streams) + 1, nf_=1)  # more than 2^32 - 1 rows
    bf, bfs, _, _ = _pair(G, "chain", n, streams, True)
    refused(bf, G.ERR_INVALID, d_new=newf.data_ptr() + 4, f32=True)                # float frames off 8 bytes
    # what the table entry refuses for the batch and the ops is refused here in its words (the table entry is asked on a batch of its own)
    d_starts = torch.zeros((4,), dtype=torch.int32, device="cuda")
    staged = torch.zeros((streams * 2 * n * 2,), dtype=torch.int16, device="cuda")
    probe, _, _ = _batch(G, "chain", n, streams, False)
    unannounced = G.Batch(G.Params(n=n, avg_frames=F), streams, G.OP_FFT | G.OP_RING_S16)      # no state arrays: what a process call refuses
    twin_u = G.Batch(G.Params(n=n, avg_frames=F), streams, G.OP_FFT | G.OP_RING_S16)
    cases = [(probe, bt, bad) for bad in (G.OP_FFT | GA | G.OP_RAW, G.OP_FFT | GA | G.OP_SMOOTH, G.OP_FFT | GA | G.OP_MAGNITUDE, GA, G.OP_FFT | G.OP_WAVE)]
    for asked, batch, bad in cases + [(twin_u, unannounced, ops)]:
        with pytest.raises(G.GlvError) as ei:
            asked.track_at_s16(staged, 2 * n, d_starts, 4, out, work, bad)
        with pytest.raises(G.GlvError) as ej:
            batch.ring_track_s16(new, nf, 4, out, work, bad)
        assert ej.value.code == ei.value.code and str(ej.value) == str(ei.value), (hex(bad), str(ej.value), str(ei.value))
    mixed, _, _ = _batch(G, "chain", n, streams, False)
    _update(mixed, rec(8, streams, nf, False), nf, G.OP_FFT | G.OP_GRAVITY, n, False)
    refused(mixed, G.ERR_STATE)                                                    # the gravity form mix, as an update refuses it
    torch.cuda.synchronize()
    assert not bool(out.any()), "a refused call wrote to the output"
    assert not bool(work.any()), "a refused call wrote to the workspace"
    _same_after(bt, bs, ops, w, False, n)                                          # the refusals moved nothing: the twin agrees
    _same_after(bf, bfs, ops, w, True, n)
    for b in (bt, bs, bf, bfs, plain, mixed, probe, unannounced, twin_u): b.close()


# ---- 7. more work items than a grid takes at once -----------------------------------------------------------------------------------------------------
K_RING_TRACK_GRID_CAP = 256 * 8                                                    # glv_launch.h kRingTrackGridCap: workgroups of 256 pieces of 16 bytes


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
def test_more_work_items_than_the_copy_grids_take_at_once(glvlib, f32):
    """n = 256, new_frames = 256, 4 updates of 2100 streams: both copies run past their grid cap -- the staging with two or three chunks of 256 pieces a
    stream, the write-back with one -- and every stream, the last ones included, equals the sequential calls"""
    G = glvlib
    n, nf, updates, streams = 256, 256, 4, 2100
    per_piece = 2 if f32 else 4
    stage_items = streams * -(-((n + updates * nf) // per_piece) // 256)
    keep_items = streams * -(-(n // per_piece) // 256)
    assert stage_items > K_RING_TRACK_GRID_CAP and keep_items > K_RING_TRACK_GRID_CAP
    assert stage_items % K_RING_TRACK_GRID_CAP != 0 and keep_items % K_RING_TRACK_GRID_CAP != 0      # the last trip is a partial one
    _against_sequential(G, "chain", n, nf, f32, streams=streams, updates=updates, odd=False)


# ---- 8. graph capture: from the first call on ---------------------------------------------------------------------------------------------------------
def test_the_first_call_can_be_captured(glvlib):
    """the FIRST ring track call of a batch captured into a hipGraph (global mode: an allocation or a synchronisation would fail the capture); the graph
    is a chain of as many kernel nodes as the call reports launches"""
    import torch
    G = glvlib
    hip = C.CDLL("libamdhip64.so")
    n, nf, updates, streams = 256, 37, F, 3
    bg, ops, w = _batch(G, "gl_chain_r16", n, streams, False)
    be, _, _ = _batch(G, "gl_chain_r16", n, streams, False)
    new = rec(77, streams, updates * nf, False)
    d_new = to_device(new, True, False)
    work = torch.zeros((bg.ring_track_work_bytes(nf, updates, ops),), dtype=torch.uint8, device="cuda")
    og = torch.zeros((updates, streams * 2, w), dtype=torch.int16, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = C.c_void_p(st.cuda_stream)
    assert hip.hipStreamBeginCapture(sp, 0) == 0                                   # hipStreamCaptureModeGlobal
    try:
        bg.ring_track_s16(d_new, nf, updates, og, work, ops, stream=st.cuda_stream)
    finally:
        graph = C.c_void_p()
        rc = hip.hipStreamEndCapture(sp, C.byref(graph))
    assert rc == 0
    count = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(count)) == 0 and count.value == bg.last_launches() == _launches(G, ops)
    roots = C.c_size_t(0)
    assert hip.hipGraphGetRootNodes(graph, None, C.byref(roots)) == 0 and roots.value == 1
    edges = C.c_size_t(0)
    assert hip.hipGraphGetEdges(graph, None, None, C.byref(edges)) == 0 and edges.value == count.value - 1
    exe = C.c_void_p()
    assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
    assert hip.hipGraphLaunch(exe, sp) == 0
    st.synchronize()
    want = _sequential(be, new, nf, updates, ops, w, False)
    assert _eq(og, want), differing(og, want)
    hip.hipGraphExecDestroy(exe); hip.hipGraphDestroy(graph)
    bg.close(); be.close()
