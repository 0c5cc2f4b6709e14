"""GPU: ring batches in track mode per stream (glv_batch_ring_track_each_s16 / _f32) -- several ring updates in one call, with a count of updates and a row
of update rates for every stream of the batch.

Contract: with R_s = stream s's ring read oldest frame first followed by its first c_s * new_frames new frames, c_s = min(d_counts[s], updates), update
t < c_s transforms frames [(t + 1) * nf, (t + 1) * nf + n) of R_s, the ring is afterwards the last n frames of R_s, and every stream is bit for bit -- output
rows, gravity and average state, ring -- what c_s sequential glv_batch_ring_update_* calls make of a ONE-stream ring batch at that stream's state, with
glv_batch_set_params(ur = d_ur[s][t]) before update t where a rate table is given.  Rows t >= c_s are the result of a zero row (zeros for every form here:
floats, texels and columns of a zero row are zeros).  A stream with c_s = 0 keeps state and ring.

The twins are brought to a stream's state by glv_batch_copy_streams, after the history of tests/test_ring_track.py (three updates of 37 frames: the ring at
frame 111).  Every call gets a workspace of exactly the queried size and an output of exactly updates * streams * 2 * w elements, each followed by a guard;
the rate table has 8 NaN entries behind it and the counts an entry of 0xFFFFFFFF.  Floats are compared as int32."""
import ctypes as C

import numpy as np
import pytest

from glava_amd import spectrum as _S
from track_lib import GUARD, differing, eq, out_dtype, rec, to_device, with_table
from track_rates_lib import FLOAT_STEP, TEXEL_STEP
from test_ring_track import F, HISTORY, HISTORY_NF, K_RING_TRACK_GRID_CAP, UPDATES, _form, _history, _launches, _planar, _ring_track, _same_after, _update, _warm
from test_track_each import _dev_u32, _dev_ur, _rates

pytestmark = pytest.mark.gpu

STREAMS = 5
COUNTS = [0, 10, 3, 1, 7]
FORMS = ["chain", "gl_chain_r16", "chain_mono", "bars_snap", "live", "columns", "upload_r16"]
FILL = 0xA5


# ---- batches and calls -----------------------------------------------------------------------------------------------------------------------------------
def _make(G, name, n, streams, f32):
    """(batch, its parameters, ops, row width, texel state): the form of tests/test_ring_track.py with the gravity step the rate tables are made for"""
    kw, mask, ops, table, w = _form(G, name, n)
    texel = kw.get("gl_storage") == 1
    pkw = dict(dict(n=n, avg_frames=F, gravity_step=TEXEL_STEP if texel else FLOAT_STEP), **kw)
    b = with_table(G.Batch(G.Params(**pkw), streams, mask | (G.OP_RING_F32 if f32 else G.OP_RING_S16)), table)
    return b, pkw, ops, w, texel


def _twin(G, name, n, f32, b, s):
    """a one-stream ring batch at stream s's state"""
    t = _make(G, name, n, 1, f32)[0]
    t.copy_streams(_dev_u32([0], 0), b, _dev_u32([s], 0), 1)
    return t


def _work_bytes(b, n, nf, updates, ops, f32):
    """the three regions of include/glv_spectrum.h, each a multiple of 256 bytes"""
    up = lambda v: (v + 255) & ~255                                                # noqa: E731
    pitch = (n + updates * nf + 3) & ~3
    return up(b.streams * pitch * (8 if f32 else 4)) + up(b.streams * updates * 4) + b.track_at_work_bytes(updates, ops)


def _each(b, d_new, nf, updates, d_ur, d_counts, ops, w, f32, stream=None):
    """one call with a workspace of exactly the queried size and an output of exactly updates * streams * 2 * w elements, guards behind both"""
    import torch
    dt = out_dtype(_S, ops)
    nbytes = b.ring_track_each_work_bytes(nf, updates, ops)
    assert nbytes == _work_bytes(b, b.params.n, nf, updates, ops, f32)
    work = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert work.data_ptr() % 256 == 0
    count = updates * b.streams * 2 * w
    sentinel = 23130 if dt == torch.int16 else -7.0
    flat = torch.full((count + GUARD,), sentinel, dtype=dt, device="cuda")         # (the output too: a row the call leaves stale shows)
    (b.ring_track_each_f32 if f32 else b.ring_track_each_s16)(d_new, nf, updates, d_ur, d_counts, flat, work, ops, stream=stream)
    torch.cuda.synchronize()
    assert bool((work[nbytes:] == FILL).all()), "the call wrote behind the workspace it asked for"
    assert bool((flat[count:] == sentinel).all()), "the call wrote behind its output"
    return flat[:count].view(updates, b.streams * 2, w)


def _blob_rows(b):
    import torch
    nbytes = b.stream_state_desc().bytes
    blob = torch.zeros((b.streams * nbytes,), dtype=torch.uint8, device="cuda")
    b.save_streams(_dev_u32(np.arange(b.streams), 0), b.streams, blob)
    torch.cuda.synchronize()
    return blob.view(b.streams, nbytes)


def _sequential(G, t, pkw, chunks, urs, nf, ops, w, f32):
    """the twin's side: one glv_batch_ring_update_* call per chunk (None: the zero fill), glv_batch_set_params with that update's rate before each where
    rates are given; the batch's own ur is set again at the end"""
    outs = []
    for k, chunk in enumerate(chunks):
        if urs is not None:
            t.set_params(G.Params(**pkw, ur=float(urs[k])))
        outs.append(_update(t, chunk, nf, ops, w, f32))
    if urs is not None and chunks:
        t.set_params(G.Params(**pkw))
    return outs


def _poisoned(new, counts, nf, f32):
    """the new frames with everything behind every stream's count overwritten: NaN, or 0x7FFF"""
    x = np.array(new, copy=True)
    for s, c in enumerate(counts):
        x[s, c * nf:] = np.nan if f32 else 0x7FFF
    return x


def _rows_of(urs, streams):
    return None if urs is None else np.ascontiguousarray(urs[np.arange(streams) % len(urs)])


def _run(G, name, n, f32, calls, streams=STREAMS, sample=None, after=True):
    """calls: (nf, updates, counts or None, with_ur, new: "rec" / "odd" / "poison" / None for the zero fill) one after another on one batch, every stream of
    `sample` (default: all) held to its one-stream twin row by row; then blobs, rings and one more lockstep update on both sides"""
    import torch
    b, pkw, ops, w, texel = _make(G, name, n, streams, f32)
    _warm(b, ops, w, f32, n)
    sample = list(range(streams)) if sample is None else sample
    twins = {s: _twin(G, name, n, f32, b, s) for s in sample}
    torch.cuda.synchronize()
    for k, (nf, updates, counts, with_ur, how) in enumerate(calls):
        took = [updates if counts is None else min(int(counts[s]), updates) for s in range(streams)]
        new = None if how is None else rec(900 + 7 * k + nf, streams, updates * nf, f32)
        urs = _rows_of(_rates(texel, updates), streams) if with_ur else None
        sent = new if how != "poison" else _poisoned(new, took, nf, f32)
        d_new = None if new is None else to_device(sent, how != "rec", f32)
        d_ur = _dev_ur(urs) if with_ur else None
        d_counts = _dev_u32(counts, 1) if counts is not None else None
        before = _planar(b, f32) if counts is not None else None
        got = _each(b, d_new, nf, updates, d_ur, d_counts, ops, w, f32)
        assert b.last_launches() == _launches(G, ops), (b.last_launches(), name)
        if before is not None:                                                     # every stream that stood still, sampled or not: its ring, oldest first
            still = [s for s in range(streams) if took[s] == 0]
            assert eq(_planar(b, f32)[still], before[still]), "a stream with count 0 lost its ring"
        behind = torch.tensor([[t >= took[s] for s in range(streams) for _ in (0, 1)] for t in range(updates)], device="cuda")
        assert not bool(got[behind].any()), (name, k, "a row behind a count is not the zero row's result")
        for s in sample:
            chunks = [None if new is None else new[s:s + 1, t * nf:(t + 1) * nf] for t in range(took[s])]
            want = _sequential(G, twins[s], pkw, chunks, None if urs is None else urs[s], nf, ops, w, f32)
            for t in range(took[s]):
                assert eq(got[t, 2 * s:2 * s + 2], want[t]), (name, n, nf, f32, k, s, t, differing(got[t, 2 * s:2 * s + 2], want[t]))
    if after:
        mine, rings = _blob_rows(b), _planar(b, f32)
        more = rec(71, streams, HISTORY_NF, f32)
        last = _update(b, more, HISTORY_NF, ops, w, f32)
        for s in sample:
            assert bool((mine[s] == _blob_rows(twins[s])[0]).all()), (name, s, "blob")
            assert eq(rings[s], _planar(twins[s], f32)[0]), (name, s, "ring")
            assert eq(last[2 * s:2 * s + 2], _update(twins[s], more[s:s + 1], HISTORY_NF, ops, w, f32)), (name, s, "one more update")
    for t in twins.values(): t.close()
    return b, ops, w


def _cases():
    """the two chains with state at every size, update size and ring kind; every other form on a diagonal through them"""
    full = [(n, nf, f32) for n in (256, 1024) for nf in (1, 37, 64, "n") for f32 in (False, True)]
    diagonal = [(256, 37, False), (1024, "n", True), (1024, 64, False), (256, 1, True)]
    return [(form, *c) for form in FORMS for c in (full if form in ("chain", "gl_chain_r16") else diagonal)]


# ---- 1. every stream is its one-stream twin ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,n,nf,f32", _cases())
def test_every_stream_is_its_one_stream_twin(glvlib, form, n, nf, f32):
    """counts [0, 10, 3, 1, 7], a rate row per stream (integer and non-integer steps on texel state), the new frames one frame behind a load boundary"""
    nf = n if nf == "n" else nf
    _run(glvlib, form, n, f32, [(nf, UPDATES, COUNTS, True, "odd")])[0].close()


# ---- 2. / 3. / 4. one table at a time, and the clamp --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["chain", "gl_chain_r16"])
def test_counts_alone_keep_the_batch_s_own_rate(glvlib, form):
    _run(glvlib, form, 256, False, [(37, UPDATES, COUNTS, False, "odd")])[0].close()


@pytest.mark.parametrize("form", ["chain", "gl_chain_r16"])
def test_rates_alone_equal_sequential_calls_with_set_params(glvlib, form):
    _run(glvlib, form, 256, True, [(64, UPDATES, None, True, "rec")])[0].close()


def test_a_count_above_updates_is_clamped(glvlib):
    _run(glvlib, "gl_chain_r16", 256, False, [(37, UPDATES, [11, 1000, 3, 0xFFFFFFFF, 0], True, "odd")])[0].close()


# ---- 5. both tables NULL: the lockstep call ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("form", ["chain", "live"])
def test_null_tables_are_the_lockstep_ring_track_call(glvlib, form, f32):
    G = glvlib
    n, nf = 256, 37
    be, pkw, ops, w, _ = _make(G, form, n, STREAMS, f32)
    bl = _make(G, form, n, STREAMS, f32)[0]
    for b in (be, bl):
        _warm(b, ops, w, f32, n)
    new = rec(31, STREAMS, UPDATES * nf, f32)
    got = _each(be, to_device(new, True, f32), nf, UPDATES, None, None, ops, w, f32)
    want = _ring_track(bl, to_device(new, True, f32), nf, UPDATES, ops, w, f32)
    assert eq(got, want), differing(got, want)
    assert be.last_launches() == bl.last_launches()
    _same_after(be, bl, ops, w, f32, n)
    be.close(); bl.close()


# ---- 6. the per-stream table call on the host-built recordings ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
def test_the_call_is_the_per_stream_table_call_on_the_staged_recordings(glvlib, f32):
    import torch
    G = glvlib
    n, nf, name = 1024, 37, "gl_chain_r16"
    br, pkw, ops, w, texel = _make(G, name, n, STREAMS, f32)
    ba = _make(G, name, n, STREAMS, f32)[0]
    for b in (br, ba):
        _warm(b, ops, w, f32, n)
    history, new = _history(n, STREAMS, f32), rec(1234, STREAMS, UPDATES * nf, f32)
    # R_s on the host: the ring oldest first (zeros, then the history's frames), the first c_s * nf new frames, zeros up to the pitch
    pitch = (n + UPDATES * nf + 3) & ~3
    r = np.zeros((STREAMS, pitch, 2), dtype=new.dtype)
    r[:, n - HISTORY * HISTORY_NF:n] = history
    for s, c in enumerate(COUNTS):
        r[s, n:n + c * nf] = new[s, :c * nf]
    urs = _rates(texel, UPDATES)
    d_ur, d_counts = _dev_ur(urs), _dev_u32(COUNTS, 1)
    starts = np.tile(np.arange(1, UPDATES + 1, dtype=np.uint32) * nf, (STREAMS, 1))
    got = _each(br, to_device(new, True, f32), nf, UPDATES, d_ur, d_counts, ops, w, f32)
    work = torch.zeros((ba.track_at_work_bytes(UPDATES, ops),), dtype=torch.uint8, device="cuda")
    want = torch.zeros_like(got)
    (ba.track_each_f32 if f32 else ba.track_each_s16)(to_device(r, True, f32), pitch, _dev_u32(starts, UPDATES), d_ur, d_counts, UPDATES, want, work, ops)
    torch.cuda.synchronize()
    assert eq(got, want), differing(got, want)
    assert br.last_launches() == ba.last_launches() + 2
    # the state both are left in (head, gravity and average rows), through one process call on a common window: the table call's batch keeps its old ring
    win = torch.from_numpy(np.array(rec(71, STREAMS, n, f32), copy=True)).cuda()
    oa, ot = (torch.zeros((STREAMS * 2, w), dtype=torch.int16, device="cuda") for _ in (0, 1))
    (ba.process_f32_stereo if f32 else ba.process_s16)(win, oa, ops)
    (br.process_f32_stereo if f32 else br.process_s16)(win, ot, ops)
    torch.cuda.synchronize()
    assert eq(ot, oa), "state"
    br.close(); ba.close()


# ---- 7. d_new behind a count is never read -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("nf", [1, 37, 64])
def test_new_frames_behind_a_count_are_never_read(glvlib, nf, f32):
    """NaN (f32) or 0x7FFF (s16) behind every stream's count: the twins, which never see those frames, agree (the new frames one frame behind a load
    boundary), and the call is bit for bit the same call with zeros there (the new frames on a load boundary)"""
    G = glvlib
    _run(G, "chain", 256, f32, [(nf, UPDATES, COUNTS, True, "poison")])[0].close()
    outs = []
    for zeros in (False, True):
        b, pkw, ops, w, texel = _make(G, "chain", 256, STREAMS, f32)
        _warm(b, ops, w, f32, 256)
        new = np.array(rec(907 + nf, STREAMS, UPDATES * nf, f32), copy=True)
        for s, c in enumerate(COUNTS):
            new[s, c * nf:] = 0 if zeros else (np.nan if f32 else 0x7FFF)
        outs.append((_each(b, to_device(new, False, f32), nf, UPDATES, _dev_ur(_rates(texel, UPDATES)), _dev_u32(COUNTS, 1), ops, w, f32), _blob_rows(b), _planar(b, f32)))
        b.close()
    for what, x, y in zip(("rows", "blobs", "rings"), *outs):
        assert eq(x, y), what


# ---- 8. the workspace --------------------------------------------------------------------------------------------------------------------------------------------
def test_the_query_is_the_staged_recordings_a_row_of_starts_per_stream_and_the_table_call_s_workspace(glvlib):
    """(every call above is held to the same sum, with a guard behind exactly that many bytes)"""
    G = glvlib
    for f32 in (False, True):
        for name, n, nf, updates, streams in (("chain", 256, 37, 10, 3), ("chain_mono", 1024, 1, 7, 1), ("live", 256, 256, 3, 5), ("columns", 1024, 64, 5, 67)):
            b, pkw, ops, w, _ = _make(G, name, n, streams, f32)
            assert b.ring_track_each_work_bytes(nf, updates, ops) == _work_bytes(b, n, nf, updates, ops, f32), (name, f32)
            b.close()


# ---- 9. zero fill ------------------------------------------------------------------------------------------------------------------------------------------------
def test_zero_fill_with_mixed_counts_equals_sequential_zero_fills(glvlib):
    _run(glvlib, "chain", 256, False, [(37, UPDATES, COUNTS, True, None)])[0].close()


# ---- 10. two calls in a row --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("form", ["chain", "gl_chain_r16"])
def test_calls_in_a_row_equal_one_sequential_run_per_stream(glvlib, form, f32):
    """every call starts from the ring the last one wrote back and the head it left, with other counts and another new_frames"""
    n = 256
    calls = [(37, 5, [5, 0, 2, 1, 4], True, "odd"), (64, 4, [0, 4, 4, 3, 1], False, "rec"), (n, 3, [1, 3, 0, 2, 3], True, "odd"), (1, 6, None, True, "rec")]
    _run(glvlib, form, n, f32, calls)[0].close()


# ---- 11. refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_move_nothing(glvlib):
    import torch
    G = glvlib
    n, nf = 256, 37
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    pair = lambda f32: [_make(G, "chain", n, STREAMS, f32) for _ in (0, 1)]        # noqa: E731
    (bt, pkw, ops, w, _), (bs, *_) = pair(False)
    (bf, *_), (bfs, *_) = pair(True)
    for b, f32 in ((bt, False), (bs, False), (bf, True), (bfs, True)):
        _warm(b, ops, w, f32, n)
    new = to_device(rec(8, STREAMS, 4 * n, False), False, False)
    newf = to_device(rec(8, STREAMS, 4 * n, True), False, True)
    work = torch.zeros((bt.ring_track_each_work_bytes(n, 4, ops),), dtype=torch.uint8, device="cuda")
    out = torch.zeros((4, STREAMS * 2, n), dtype=torch.float32, device="cuda")
    d_ur, d_counts = _dev_ur(_rates(False, 4)), _dev_u32([1, 2, 3, 4, 0], 1)

    def refused(batch, code, d_new=new, nf_=nf, updates=4, ur=d_ur, cnt=d_counts, o=out, wk=work, ops_=ops, f32=False, text=None):
        launches = batch.last_launches()
        with pytest.raises(G.GlvError) as ei:
            (batch.ring_track_each_f32 if f32 else batch.ring_track_each_s16)(d_new, nf_, updates, ur, cnt, o, wk, ops_)
        assert ei.value.code == code, (ei.value.code, str(ei.value))
        assert batch.last_launches() == launches
        if text is not None:
            assert text in str(ei.value), str(ei.value)

    wave = G.Batch(G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5), STREAMS, G.OP_WAVE | G.OP_RING_S16)
    for kw in (dict(), dict(ur=None), dict(cnt=None), dict(ur=None, cnt=None)):
        refused(wave, G.ERR_INVALID, ops_=G.OP_WAVE | G.OP_R16, text="glv_batch_ring_track_s16 / _f32", **kw)
    refused(bt, G.ERR_INVALID, ops_=G.OP_FFT | G.OP_WAVE, text="glv_batch_ring_track_s16 / _f32")
    assert G.lib().glv_batch_ring_track_each_work_bytes(wave._h, nf, 4, G.OP_WAVE | G.OP_R16) == 0
    assert G.lib().glv_last_error().decode().startswith("GLV_ERR_INVALID: ")
    fft = G.Batch(G.Params(n=n, avg_frames=F), STREAMS, G.OP_FFT | G.OP_RING_S16)
    avg = G.Batch(G.Params(n=n, avg_frames=F), STREAMS, G.OP_AVERAGE | G.OP_RING_S16)
    refused(fft, G.ERR_INVALID, ops_=G.OP_FFT, cnt=None, text="a rates track call needs GLV_OP_GRAVITY")           # rates without gravity
    refused(avg, G.ERR_INVALID, ops_=G.OP_FFT | G.OP_AVERAGE, text="a rates track call needs GLV_OP_GRAVITY")       # ... with state
    refused(fft, G.ERR_INVALID, ops_=G.OP_FFT, ur=None, text="the chain keeps no state for d_counts to protect")    # counts on an FFT-only chain
    refused(bt, G.ERR_INVALID, ur=d_ur.data_ptr() + 2, text="d_ur must be 4-byte aligned")
    refused(bt, G.ERR_INVALID, cnt=d_counts.data_ptr() + 1, text="d_counts must be 4-byte aligned")
    refused(bt, G.ERR_INVALID, nf_=0)
    refused(bt, G.ERR_INVALID, nf_=n + 1)
    refused(bt, G.ERR_INVALID, updates=0)
    refused(bt, G.ERR_STATE, d_new=newf, f32=True)                                 # a batch without the f32 ring
    plain = G.Batch(G.Params(n=n, avg_frames=F), STREAMS, GA)
    refused(plain, G.ERR_STATE)                                                    # ... without any ring
    assert G.lib().glv_batch_ring_track_each_work_bytes(plain._h, nf, 4, ops) == 0 and G.lib().glv_last_error().decode().startswith("GLV_ERR_STATE: ")
    refused(bt, G.ERR_INVALID, o=None)
    refused(bt, G.ERR_INVALID, wk=None)
    refused(bt, G.ERR_INVALID, wk=work.data_ptr() + 64)
    refused(bt, G.ERR_INVALID, d_new=new.data_ptr() + 2)                           # s16 frames off 4 bytes
    refused(bt, G.ERR_INVALID, updates=(2 ** 32 - 1) // (2 * STREAMS) + 1, nf_=1)  # more than 2^32 - 1 rows
    refused(bf, G.ERR_INVALID, d_new=None, f32=True)                               # the f32 entry has no zero fill
    refused(bf, G.ERR_INVALID, d_new=newf.data_ptr() + 4, f32=True)                # float frames off 8 bytes
    for bad in (G.OP_FFT | GA | G.OP_RAW, G.OP_FFT | GA | G.OP_SMOOTH, GA):        # what the table call refuses for the ops
        refused(bt, G.ERR_INVALID, ops_=bad)
    mixed = _make(G, "chain", n, STREAMS, False)[0]
    _update(mixed, rec(8, STREAMS, nf, False), nf, G.OP_FFT | G.OP_GRAVITY, n, False)
    refused(mixed, G.ERR_STATE)                                                    # the gravity form mix, as an update refuses it
    torch.cuda.synchronize()
    assert not bool(out.any()), "a refused call wrote to the output"
    assert not bool(work.any()), "a refused call wrote to the workspace"
    _same_after(bt, bs, ops, w, False, n)                                          # the refusals moved nothing: the twin agrees on the next update
    _same_after(bf, bfs, ops, w, True, n)
    for b in (bt, bs, bf, bfs, wave, fft, avg, plain, mixed): b.close()


# ---- 12. more work items than a grid takes at once -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
def test_more_work_items_than_the_copy_grids_take_at_once(glvlib, f32):
    """n = 256, new_frames = 256, 4 updates of 2100 streams whose counts cycle through 0 .. 4: each of the four launches has more work items than
    kRingTrackGridCap and a ragged last trip -- the staging with two or three chunks of 256 pieces a stream, the transform's windows, the scan's rows, the
    write-back with one chunk a stream.  Held to their twins: the first streams, those around the grid cap, and the last ones; held for every stream:
    zero rows behind the count, the ring of a stream that stood still, and on the f32 ring every stream's ring against the last n frames of R_s"""
    import torch
    G = glvlib
    n, nf, updates, streams = 256, 256, 4, 2100
    per_piece = 2 if f32 else 4
    items = {"stage": streams * -(-((n + updates * nf) // per_piece) // 256), "windows": streams * updates, "rows": streams * 2, "keep": streams * -(-(n // per_piece) // 256)}
    for what, count in items.items():
        assert count > K_RING_TRACK_GRID_CAP and count % K_RING_TRACK_GRID_CAP != 0, what
    counts = [s % (updates + 1) for s in range(streams)]
    sample = [0, 1, 2, 3, 4, 1023, 1024, 2046, 2047, 2048, 2049, 2096, 2097, 2098, 2099]
    b, ops, w = _run(G, "chain", n, f32, [(nf, updates, counts, True, "rec")], streams=streams, sample=sample, after=False)
    if f32:                                                                        # (the f32 ring is published as it lies; nf = n: a stream that ran holds its last update)
        new, rings = rec(900 + nf, streams, updates * nf, True), _planar(b, True).cpu().numpy()
        for s in range(streams):
            if counts[s]:
                last = new[s, (counts[s] - 1) * nf:counts[s] * nf]
                assert np.array_equal(rings[s, 0], last[:, 0]) and np.array_equal(rings[s, 1], last[:, 1]), s
    b.close()


# ---- 13. graph capture: from the first call on, re-aimed by rewriting the tables -----------------------------------------------------------------------------
def test_a_captured_first_call_is_reaimed_by_rewriting_counts_rates_and_new_frames(glvlib):
    import torch
    G = glvlib
    hip = C.CDLL("libamdhip64.so")
    n, nf, name = 256, 37, "gl_chain_r16"
    bg, pkw, ops, w, texel = _make(G, name, n, STREAMS, False)
    be = _make(G, name, n, STREAMS, False)[0]
    new_a, new_b = rec(77, STREAMS, UPDATES * nf, False), rec(78, STREAMS, UPDATES * nf, False)
    urs_b = _rates(texel, UPDATES)
    d_new, d_ur, d_counts = to_device(new_a, True, False), _dev_ur(np.full_like(urs_b, 50.0)), _dev_u32([UPDATES] * STREAMS, 1)
    n_new, n_ur, n_counts = to_device(new_b, True, False), _dev_ur(urs_b), _dev_u32(COUNTS, 1)
    work = torch.zeros((bg.ring_track_each_work_bytes(nf, UPDATES, ops),), dtype=torch.uint8, device="cuda")
    og = torch.zeros((UPDATES, STREAMS * 2, w), dtype=torch.int16, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = C.c_void_p(st.cuda_stream)
    assert hip.hipStreamBeginCapture(sp, 0) == 0                                   # hipStreamCaptureModeGlobal: an allocation or a synchronisation fails it
    try:
        bg.ring_track_each_s16(d_new, nf, UPDATES, d_ur, d_counts, og, work, ops, stream=st.cuda_stream)
    finally:
        graph = C.c_void_p()
        rc = hip.hipStreamEndCapture(sp, C.byref(graph))
    assert rc == 0
    count = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(count)) == 0 and count.value == bg.last_launches() == _launches(G, ops)
    exe = C.c_void_p()
    assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
    with torch.cuda.stream(st):
        d_new.copy_(n_new); d_ur.copy_(n_ur); d_counts.copy_(n_counts)             # in stream order, in front of the replay
    assert hip.hipGraphLaunch(exe, sp) == 0
    st.synchronize()
    want = _each(be, n_new, nf, UPDATES, n_ur, n_counts, ops, w, False)
    assert eq(og, want), differing(og, want)
    assert not bool(og[:, 0:2].any()) and bool(og[:, 2:4].any())                   # the rewritten counts: stream 0 stands still, stream 1 runs
    assert eq(_planar(bg, False), _planar(be, False)) and bool((_blob_rows(bg) == _blob_rows(be)).all())
    hip.hipGraphExecDestroy(exe); hip.hipGraphDestroy(graph)
    bg.close(); be.close()
