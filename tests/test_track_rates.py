"""GPU: track mode with a per-step update rate (glv_batch_track_rates_s16 / _f32) -- glv_batch_track_at_* with a second table in device memory, the
update rate gravity runs at in each step, as a live GLava's measured gl->ur moves from update to update.

Contract: step t of the output, and the batch's state afterwards, are bit for bit what `steps` consecutive glv_batch_process_s16 /
glv_batch_process_f32_stereo calls produce and leave behind when each is preceded by glv_batch_set_params with ur = d_ur[t]; the batch's own ur is not
changed.  The sequential side is a second batch driven that way on windows cut on the host; floats are compared as int32; the state is compared through
one more update on both batches with ur back at its base value -- which also shows the track batch's ur untouched.

In every call of this file the rate table has 8 NaN entries behind its `steps` entries (a read past the end shows as wrong bits, never as a fault),
the workspace is exactly as large as glv_batch_track_at_work_bytes asks and the output exactly steps * streams * 2 * w elements, with a guard behind each
that must come back intact.  3 streams, 11 steps (more than the scan's look-ahead of 8: the ring wraps with a ragged tail), F = 5, n = 256 and 1024.
The tables and what they exercise: tests/track_rates_lib.py (the texel table's classification is held to its counts in tests/test_track_rates_host.py and
repeated here)."""
import ctypes as C

import numpy as np
import pytest

from glava_amd.bar_positions import graph_column_texels, radial_bar_texels
from glava_amd.track_starts import live_session_rates
from oracle_lib import StreamOracle
from track_lib import GUARD, differing, eq, out_dtype, rec, s16_chains, to_device, windows
from track_rates_lib import FLOAT_STEP, FLOAT_UR, STEPS, TEXEL_STEP, TEXEL_UR, classify

pytestmark = pytest.mark.gpu

STREAMS, F = 3, 5
NAN_TAIL = 8
CHAINS = ["gravity", "chain", "chain_plain_sum", "chain_r16", "chain_mono", "gl_gravity", "gl_chain", "gl_chain_r16", "gl_chain_F1", "gl_chain_mono"]


# ---- tables ------------------------------------------------------------------------------------------------------------------------------------------
def _frac(n, steps=STEPS):
    """(starts, pitch): 22050 Hz at 60 fps, 367.5 frames a step (scaled below n = 1024, as in tests/test_track_at.py); the pitch odd, with slack"""
    k = 735 if n >= 1024 else 91
    s = [t * k // 2 for t in range(steps)]
    return s, (max(s) + n + 38) | 1


def _starts_dev(starts):
    import torch
    return torch.from_numpy(np.asarray(starts, dtype=np.uint32).view(np.int32).copy()).cuda()


def _rates_dev(ur):
    """the table on the device, NAN_TAIL NaN entries behind it"""
    import torch
    return torch.from_numpy(np.concatenate([np.asarray(ur, dtype=np.float32), np.full(NAN_TAIL, np.nan, np.float32)])).cuda()


def _knobs(kw):
    """(gravity_step, rate table) of a chain: texel state takes the table that sits on both sides of the host's integer-step test"""
    return (TEXEL_STEP, TEXEL_UR) if kw.get("gl_storage") else (FLOAT_STEP, FLOAT_UR)


def _cycled(table, steps):
    return [table[t % len(table)] for t in range(steps)]


# ---- one rates call, and its sequential side -----------------------------------------------------------------------------------------------------------
def _rates(b, d_pcm, pitch, d_starts, d_ur, steps, ops, w, dt, f32=False, t0=0, stream=None):
    """steps [t0, t0 + steps) of both tables in one call; exact workspace and output, a guard behind each (the method of track_lib.track)"""
    import torch
    nbytes = b.track_at_work_bytes(steps, ops)
    work = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert work.data_ptr() % 256 == 0
    count = steps * b.streams * 2 * w
    fill = 23130 if dt == torch.int16 else -7.0
    flat = torch.zeros((count + GUARD,), dtype=dt, device="cuda")
    flat[count:] = fill
    assert d_ur.numel() >= t0 + steps + NAN_TAIL
    (b.track_rates_f32 if f32 else b.track_rates_s16)(d_pcm, pitch, d_starts.data_ptr() + 4 * t0, d_ur.data_ptr() + 4 * t0, steps, flat, work, ops, stream=stream)
    torch.cuda.synchronize()
    assert bool((work[nbytes:] == 0xA5).all()), "the call wrote behind the workspace it asked for"
    assert bool((flat[count:] == fill).all()), "the call wrote behind its output"
    return flat[:count].view(steps, b.streams * 2, w)


def _process(b, x, ops, w, dt, f32):
    import torch
    o = torch.zeros((b.streams * 2, w), dtype=dt, device="cuda")
    (b.process_f32_stereo if f32 else b.process_s16)(x, o, ops)
    return o


def _seq(G, b, pkw, wins, urs, ops, w, dt, f32=False):
    """one process call per window, glv_batch_set_params with that step's ur before each (None: the batch's base ur); the base ur is set again at the end"""
    import torch
    outs = []
    for x, ur in zip(wins, urs):
        b.set_params(G.Params(**pkw) if ur is None else G.Params(**pkw, ur=ur))
        outs.append(_process(b, x, ops, w, dt, f32))
    b.set_params(G.Params(**pkw))
    torch.cuda.synchronize()
    return torch.stack(outs)


def _compare(G, bt, bs, pkw, n, urs, ops, f32=False, w=None, seed=57, launches=None, name=None, starts_pitch=None, x=None):
    """one rates call on bt against the sequential calls on bs, every step, then the state through one more update at the base ur on both"""
    steps = len(urs)
    starts, pitch = starts_pitch or _frac(n, steps)
    if x is None: x = rec(seed + n, bt.streams, pitch, f32)
    w = n if w is None else w
    dt = out_dtype(G, ops)
    d_pcm = to_device(x, True, f32, tail_frames=n)                                # one frame off a load boundary
    got = _rates(bt, d_pcm, pitch, _starts_dev(starts), _rates_dev(urs), steps, ops, w, dt, f32)
    if launches is not None: assert bt.last_launches() == launches, bt.last_launches()
    if name is not None: assert bt.kernel_name() == name, bt.kernel_name()
    wins = windows(x, n, [G.track_at_start(pitch, n, s) for s in starts + [7]])
    want = _seq(G, bs, pkw, wins[:steps], urs, ops, w, dt, f32)
    for t in range(steps):
        assert eq(got[t], want[t]), (t, urs[t], differing(got[t], want[t]))
    assert eq(_process(bt, wins[steps], ops, w, dt, f32), _process(bs, wins[steps], ops, w, dt, f32)), "state, or the batch's own ur"
    return got, want


def _pair(G, pkw, mask, streams=STREAMS, variant=None, table=None):
    out = []
    for _ in range(2):
        b = G.Batch(G.Params(**pkw), streams, mask)
        if table: (b.set_bar_texels if table[0] == "bar" else b.set_column_texels)(table[1])
        if variant is not None: b.set_variant(variant)
        out.append(b)
    return out


# ---- 1. against the sequential calls -------------------------------------------------------------------------------------------------------------------
def test_the_texel_table_holds_both_kinds_of_step():
    kinds = classify(TEXEL_STEP, TEXEL_UR)
    assert sum(1 for flt, _ in kinds if flt) >= 4 and sum(1 for flt, _ in kinds if not flt) >= 6


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("chain,n,variant,log_mode", [(c, n, v, lm) for c in CHAINS for n, v in ((256, 0), (1024, 1)) for lm in ((0, 1) if c in ("chain", "gl_chain_r16") else (1,))])
def test_track_rates_equals_set_params_before_every_call(glvlib, chain, n, variant, log_mode, f32):
    G = glvlib
    kw, mask, ops = s16_chains(G)[chain]
    step, urs = _knobs(kw)
    pkw = dict(n=n, log_mode=log_mode, gravity_step=step, **kw)
    bt, bs = _pair(G, pkw, mask, variant=variant)
    assert bt.variants() > variant
    _compare(G, bt, bs, pkw, n, urs, ops, f32=f32, launches=2, name="glv_track_scan_kernel")
    assert bt.last_variant() == variant
    bt.close(); bs.close()


# ---- 2. against the oracle -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["gravity", "chain"])
def test_track_rates_follows_the_oracle(glvlib, oracle, chain):
    """every stream against a StreamOracle whose ur is set per update (log_mode 0: bit for bit): the feature does not rest on comparing the device with itself"""
    import torch
    G = glvlib
    n = 1024
    kw, mask, ops = s16_chains(G)[chain]
    b = G.Batch(G.Params(n=n, log_mode=0, avg_frames=F, **kw), STREAMS, mask)
    starts, pitch = _frac(n)
    x = rec(91, STREAMS, pitch, False)
    got = _rates(b, to_device(x, True, False, tail_frames=n), pitch, _starts_dev(starts), _rates_dev(FLOAT_UR), STEPS, ops, n, torch.float32).cpu().numpy()
    for s in range(STREAMS):
        so = StreamOracle(n, avg_frames=F, gravity=True, average=chain == "chain")
        for t in range(STEPS):
            so.ur = FLOAT_UR[t]
            want = so.frame(np.ascontiguousarray(x[s, starts[t]:starts[t] + n, :]).reshape(-1))
            bad = got[t, 2 * s:2 * s + 2].view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
            assert not bad.any(), (chain, s, t, FLOAT_UR[t], int(bad.sum()))
    assert np.isneginf(got[1]).all()                                            # ur = 0: everything falls ...
    if chain == "gravity": assert np.isfinite(got[2]).all()                     # ... and the next step recovers (the ring keeps the -inf frame for F updates)
    b.close()


# ---- 3. the three-launch forms -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("form", ["bars", "live_bar_texels", "columns"])
def test_track_rates_three_launch_forms(glvlib, form, f32):
    G = glvlib
    n = 1024
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    gl = dict(n=n, gl_storage=1, avg_window_kind=1, avg_frames=F, gravity_step=TEXEL_STEP)
    if form == "bars":
        pkw, mask, ops, table, name = dict(gl, bars=n, bar_phase=0.5), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16, None, "glv_track_scan_kernel"
    elif form == "live_bar_texels":
        tex = radial_bar_texels(n, 160)[0]
        pkw, mask, ops, table, name = dict(gl, bars=len(tex)), GA | G.OP_BARS | G.OP_BARS_ONLY, G.OP_FFT | GA | G.OP_BARS | G.OP_R16, ("bar", tex), None
    else:
        tex = graph_column_texels(n, 320)[0]
        pkw, mask, ops, table, name = dict(gl, bars=len(tex)), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS, ("col", tex), "glv_columns_kernel"
    bt, bs = _pair(G, pkw, mask, table=table)
    if form == "live_bar_texels":
        assert 0 < bt.live_bins() < n                                            # the scan walks the kept bins only
    _compare(G, bt, bs, pkw, n, TEXEL_UR, ops, f32=f32, w=pkw["bars"], launches=3, name=name)
    bt.close(); bs.close()


# ---- 4. the constant table -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("chain", ["gravity", "chain", "gl_chain_r16"])
def test_constant_table_equals_the_table_entry(glvlib, chain, f32):
    """every entry the batch's own ur: bit for bit the output and the state of glv_batch_track_at_s16 / _f32, with its launches, kernel name and workspace (the GL
    chain: the shipped step, which the table entry takes as the packed integer step D = 3196 and the rates kind in float)"""
    import torch
    G = glvlib
    n = 1024
    kw, mask, ops = s16_chains(G)[chain]
    p = G.Params(n=n, **kw)
    dt = out_dtype(G, ops)
    starts, pitch = _frac(n)
    x = rec(404, STREAMS, pitch, f32)
    d_pcm = to_device(x, True, f32, tail_frames=n)
    d_starts = _starts_dev(starts)
    br, ba = G.Batch(p, STREAMS, mask), G.Batch(p, STREAMS, mask)
    got = _rates(br, d_pcm, pitch, d_starts, _rates_dev([p.ur] * STEPS), STEPS, ops, n, dt, f32)
    nbytes = ba.track_at_work_bytes(STEPS, ops)
    assert br.track_at_work_bytes(STEPS, ops) == nbytes
    work = torch.zeros((nbytes,), dtype=torch.uint8, device="cuda")
    want = torch.zeros_like(got)
    (ba.track_at_f32 if f32 else ba.track_at_s16)(d_pcm, pitch, d_starts, STEPS, want, work, ops)
    torch.cuda.synchronize()
    assert eq(got, want), differing(got, want)
    assert br.last_launches() == ba.last_launches() and br.kernel_name() == ba.kernel_name()
    one_more = windows(x, n, [7])[0]
    assert eq(_process(br, one_more, ops, n, dt, f32), _process(ba, one_more, ops, n, dt, f32))
    br.close(); ba.close()


# ---- 5. chunks and mixing ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("chain", ["chain", "gl_chain_r16"])
def test_track_rates_chunks_compose_and_calls_mix(glvlib, chain, f32):
    """4 steps then 7 on both pointers advanced == 11 in one call; a process call, a rates chunk, a table chunk at the batch's own ur, a rates chunk == the
    same sequence one by one"""
    import torch
    G = glvlib
    n = 1024
    kw, mask, ops = s16_chains(G)[chain]
    step, urs = _knobs(kw)
    pkw = dict(n=n, gravity_step=step, **kw)
    dt = out_dtype(G, ops)
    starts, pitch = _frac(n)
    x = rec(808, STREAMS, pitch, f32)
    d_pcm = to_device(x, True, f32, tail_frames=n)
    d_starts, d_ur = _starts_dev(starts), _rates_dev(urs)
    whole, parts, mixed, bs = (G.Batch(G.Params(**pkw), STREAMS, mask) for _ in range(4))
    one = _rates(whole, d_pcm, pitch, d_starts, d_ur, STEPS, ops, n, dt, f32)
    a = _rates(parts, d_pcm, pitch, d_starts, d_ur, 4, ops, n, dt, f32)
    c = _rates(parts, d_pcm, pitch, d_starts, d_ur, 7, ops, n, dt, f32, t0=4)
    assert eq(torch.cat([a, c]), one)
    one_more = windows(x, n, [7])[0]
    assert eq(_process(parts, one_more, ops, n, dt, f32), _process(whole, one_more, ops, n, dt, f32))
    # process(window at 13), rates [0, 4), table [4, 7) at the batch's own ur, rates [7, 11)
    got = [_process(mixed, windows(x, n, [13])[0], ops, n, dt, f32).unsqueeze(0), _rates(mixed, d_pcm, pitch, d_starts, d_ur, 4, ops, n, dt, f32)]
    work = torch.zeros((mixed.track_at_work_bytes(3, ops),), dtype=torch.uint8, device="cuda")
    mid = torch.zeros((3, STREAMS * 2, n), dtype=dt, device="cuda")
    (mixed.track_at_f32 if f32 else mixed.track_at_s16)(d_pcm, pitch, d_starts.data_ptr() + 16, 3, mid, work, ops)
    got += [mid, _rates(mixed, d_pcm, pitch, d_starts, d_ur, 4, ops, n, dt, f32, t0=7)]
    want = _seq(G, bs, pkw, windows(x, n, [13] + starts), [None] + urs[:4] + [None] * 3 + urs[7:], ops, n, dt, f32)
    torch.cuda.synchronize()
    assert eq(torch.cat(got), want)
    for b in (whole, parts, mixed, bs): b.close()


# ---- 6. step counts around the look-ahead ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 7, 8, 9, 17])
def test_track_rates_step_counts(glvlib, steps):
    G = glvlib
    n = 256
    kw, mask, ops = s16_chains(G)["gl_chain_r16"]
    pkw = dict(n=n, gravity_step=TEXEL_STEP, **kw)
    bt, bs = _pair(G, pkw, mask)
    _compare(G, bt, bs, pkw, n, _cycled(TEXEL_UR, steps), ops, launches=2)
    bt.close(); bs.close()


# ---- 7. graph capture: the rate table is read when the kernels run -----------------------------------------------------------------------------------------
def test_a_captured_call_is_reaimed_by_rewriting_the_rate_table(glvlib):
    """the FIRST call after creation captured into a hipGraph (global mode) under one table, replayed after the table was rewritten on the same stream: the
    replay shows the second table.  The graph is a chain: as many nodes as launches, one root, every other node behind exactly one."""
    import torch
    G = glvlib
    hip = C.CDLL("libamdhip64.so")
    n = 1024
    kw, mask, ops = s16_chains(G)["gl_chain_r16"]
    pkw = dict(n=n, gravity_step=TEXEL_STEP, **kw)
    table_a, table_b = [50.0] * STEPS, TEXEL_UR
    starts, pitch = _frac(n)
    x = rec(9, STREAMS, pitch, False)
    d_pcm = to_device(x, True, False, tail_frames=n)
    bg, be = _pair(G, pkw, mask)
    work = torch.zeros((bg.track_at_work_bytes(STEPS, ops),), dtype=torch.uint8, device="cuda")
    og = torch.zeros((STEPS, STREAMS * 2, n), dtype=torch.int16, device="cuda")
    d_starts, d_ur, d_next = _starts_dev(starts), _rates_dev(table_a), _rates_dev(table_b)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = C.c_void_p(st.cuda_stream)
    assert hip.hipStreamBeginCapture(sp, 0) == 0                    # hipStreamCaptureModeGlobal
    try:
        bg.track_rates_s16(d_pcm, pitch, d_starts, d_ur, STEPS, og, work, ops, stream=st.cuda_stream)
    finally:
        graph = C.c_void_p()
        rc = hip.hipStreamEndCapture(sp, C.byref(graph))
    assert rc == 0
    count = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(count)) == 0 and count.value == bg.last_launches() == 2
    roots = C.c_size_t(0)
    assert hip.hipGraphGetRootNodes(graph, None, C.byref(roots)) == 0 and roots.value == 1
    edges = C.c_size_t(0)
    assert hip.hipGraphGetEdges(graph, None, None, C.byref(edges)) == 0 and edges.value == count.value - 1
    exe = C.c_void_p()
    assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
    with torch.cuda.stream(st):
        d_ur.copy_(d_next)                                          # in stream order, in front of the replay
    assert hip.hipGraphLaunch(exe, sp) == 0
    st.synchronize()
    want = _seq(G, be, pkw, windows(x, n, starts), table_b, ops, n, torch.int16)
    assert eq(og, want), differing(og, want)
    ba = G.Batch(G.Params(**pkw), STREAMS, mask)
    assert not eq(og, _seq(G, ba, pkw, windows(x, n, starts), table_a, ops, n, torch.int16))      # ... and not the table the call was captured under
    hip.hipGraphExecDestroy(exe); hip.hipGraphDestroy(graph)
    bg.close(); be.close(); ba.close()


# ---- 8. a live session -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["chain", "gl_chain_r16"])
def test_a_live_session_runs_at_the_measured_rates(glvlib, chain):
    """live_session_rates' tables on a recording with n frames of silence in front: equal to the one-by-one calls, and not what one constant default ur gives --
    the feature's point"""
    import torch
    G = glvlib
    n = 1024
    starts, _, urs = live_session_rates(22050, 4, 12, n // 16)
    assert urs == [1.0, 1.0, 1.0, 3.0, 3.0, 3.0, 3.0, 4.0, 4.0, 4.0, 4.0] and len(starts) == STEPS
    kw, mask, ops = s16_chains(G)[chain]
    pkw = dict(n=n, **kw)
    pitch = (max(starts) + n + 38) | 1
    x = np.array(rec(5, STREAMS, pitch, False), copy=True)
    x[:, :n, :] = 0
    bt, bs = _pair(G, pkw, mask)
    got, _ = _compare(G, bt, bs, pkw, n, urs, ops, starts_pitch=(starts, pitch), x=x, launches=2)
    if chain == "gl_chain_r16":
        dt = out_dtype(G, ops)
        bc = G.Batch(G.Params(**pkw), STREAMS, mask)
        work = torch.zeros((bc.track_at_work_bytes(STEPS, ops),), dtype=torch.uint8, device="cuda")
        const = torch.zeros((STEPS, STREAMS * 2, n), dtype=dt, device="cuda")
        bc.track_at_s16(to_device(x, True, False, tail_frames=n), pitch, _starts_dev(starts), STEPS, const, work, ops)
        torch.cuda.synchronize()
        assert not eq(got, const)
        bc.close()
    bt.close(); bs.close()


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_track_rates_refusals_leave_the_batch_untouched(glvlib):
    """(a single-row batch belongs to the drop-ins, which expose no batch: its refusal is track_chain's, shared with every FFT track entry, and is pinned by
    tests/test_track_rates_host.py through the path's sources)"""
    import torch
    G = glvlib
    n = 1024
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    starts, pitch = _frac(n)
    x = rec(3, STREAMS, pitch, False)
    d_pcm = to_device(x, True, False, tail_frames=n)
    d_starts, d_ur = _starts_dev(starts), _rates_dev(FLOAT_UR)
    out = torch.full((STEPS, STREAMS * 2, n), -7.0, dtype=torch.float32, device="cuda")
    work = torch.zeros((1 << 24,), dtype=torch.uint8, device="cuda")
    first = windows(x, n, [0, 5])

    def refused(make, ops, code, d_ur_=d_ur):
        """a batch and its untouched twin after one update each; the refused call; one more update on both"""
        b, twin = make(), make()
        run = lambda bb, k: _process(bb, first[k], ops, n, out_dtype(G, ops), False)   # noqa: E731
        run(b, 0); run(twin, 0)
        launches = b.last_launches()
        with pytest.raises(G.GlvError) as ei:
            b.track_rates_s16(d_pcm, pitch, d_starts, d_ur_, STEPS, out, work, ops)
        assert ei.value.code == code, (ei.value.code, str(ei.value))
        assert b.last_launches() == launches                                       # nothing was launched
        assert eq(run(b, 1), run(twin, 1)), "a refused call touched the state"
        b.close(); twin.close()

    base = G.Params(n=n)
    refused(lambda: G.Batch(base, STREAMS, G.OP_FFT), G.OP_FFT, G.ERR_INVALID)                                      # fft: no gravity, nothing would read the table
    refused(lambda: G.Batch(base, STREAMS, G.OP_FFT), G.OP_FFT | G.OP_R16, G.ERR_INVALID)                           # fft_r16
    refused(lambda: G.Batch(base, STREAMS, G.OP_AVERAGE), G.OP_FFT | G.OP_AVERAGE, G.ERR_INVALID)                   # average
    wave = G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5)
    refused(lambda: G.Batch(wave, STREAMS, G.OP_WAVE), G.OP_WAVE | G.OP_R16, G.ERR_INVALID)                         # stateless
    chain = lambda: G.Batch(base, STREAMS, GA)                                                                      # noqa: E731
    refused(chain, G.OP_FFT | GA, G.ERR_INVALID, d_ur_=None)
    refused(chain, G.OP_FFT | GA, G.ERR_INVALID, d_ur_=d_ur.data_ptr() + 2)
    refused(lambda: G.Batch(G.Params(n=n, gl_storage=2), STREAMS, GA), G.OP_FFT | GA, G.ERR_STATE)
    # what the table entry refuses, the rates entry refuses with the same code
    b = chain()
    for kwargs, code in ((dict(pitch_=n - 1), G.ERR_INVALID), (dict(steps_=0), G.ERR_INVALID), (dict(tab=None), G.ERR_INVALID), (dict(o=None), G.ERR_INVALID),
                         (dict(w=work.data_ptr() + 64), G.ERR_INVALID), (dict(ops_=G.OP_FFT | GA | G.OP_SMOOTH), G.ERR_INVALID), (dict(ops_=GA), G.ERR_INVALID)):
        a = dict(pitch_=pitch, steps_=STEPS, tab=d_starts, o=out, w=work, ops_=G.OP_FFT | GA); a.update(kwargs)
        with pytest.raises(G.GlvError) as ei:
            b.track_rates_s16(d_pcm, a["pitch_"], a["tab"], d_ur, a["steps_"], a["o"], a["w"], a["ops_"])
        assert ei.value.code == code, (kwargs, ei.value.code)
        assert b.last_launches() == 0
    unannounced = G.Batch(base, STREAMS, G.OP_FFT)
    with pytest.raises(G.GlvError) as ei:
        unannounced.track_rates_s16(d_pcm, pitch, d_starts, d_ur, STEPS, out, work, G.OP_FFT | GA)
    assert ei.value.code == G.ERR_STATE
    unannounced.close()
    # the workspace query is the table entry's: there is no other
    assert b.track_at_work_bytes(STEPS, G.OP_FFT | GA) > 0 and not hasattr(G.Batch, "track_rates_work_bytes")
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "a refused call wrote to the output"
    # ... and after all the refusals the batch runs the whole table from untouched state
    bs = chain()
    pkw = dict(n=n)
    _compare(G, b, bs, pkw, n, FLOAT_UR, G.OP_FFT | GA, launches=2)
    b.close(); bs.close()
