"""GPU: track mode for the wave module (glv_batch_track_wave_s16) -- the wave texture of every update of a recording in one call.

Contract: d_out + t * (bytes of one call) is bit for bit what glv_batch_process_s16 with the same GLV_OP_WAVE ops writes for the window
[t * hop, t * hop + n) of every stream, for any hop >= 1; the call is stateless.  The sequential side is a second batch driven window by window, the
windows cut on the host from the same buffer; floats are compared as int32.  Every track call here gets a workspace of exactly
glv_batch_track_wave_work_bytes bytes followed by a guard region, which must come back intact, and a pitch larger than the call consumes.
STEPS x STREAMS x 2 = 66 rows: one full block of 64 rows of the bars kernel and a partial one."""

import ctypes as C

import numpy as np
import pytest

from glava_amd.bar_positions import graph_column_texels, wave_column_texels
from gpu_lib import planar_of_s16, same, texel_floats, upload
from oracle_lib import Oracle
from track_lib import compare, eq as _eq, hop_windows as _windows, pcm as _pcm, pitch_residue as _pitch, seq as _seq, track

pytestmark = pytest.mark.gpu

STEPS, STREAMS = 11, 3          # 66 rows


def _track(b, *args, **kw):
    """steps [t0, t0 + steps) of the buffer in one call of glv_batch_track_wave_s16 (track_lib.track: exact workspace and output, guards behind both)"""
    return track(b, "wave", *args, **kw)


def _launches(G, ops, hop, pitch, fusable=True, address=0):
    """glv_batch_last_launches as the header specifies it"""
    if not ops & G.OP_BARS:
        return 1
    return 1 if fusable and hop % 8 == 0 and pitch % 8 == 0 and address % 32 == 0 else 2


def _compare(G, p, ops, n, hop, steps=STEPS, streams=STREAMS, w=None, prepare=None, fusable=True, seed=131, pitch=None, mask=None, seek=0):
    """one track call against the sequential calls, every step; returns the two batches (track, sequential) for what follows.  seek: the recordings
    begin that many frames into the device buffer -- d_pcm is 4 * seek bytes off the allocation's alignment"""
    import torch
    pitch = _pitch(n, hop, steps) if pitch is None else pitch
    x = _pcm(seed + n + hop, streams, pitch)
    flat = np.concatenate([np.full((seek, 2), 12345, np.int16), x.reshape(-1, 2)])
    mask = G.OP_WAVE | G.OP_BARS if mask is None else mask
    bt, bs = G.Batch(p, streams, mask), G.Batch(p, streams, mask)
    if prepare:
        prepare(bt); prepare(bs)
    d_buf = torch.from_numpy(flat).cuda()
    assert d_buf.data_ptr() % 32 == 0
    d_pcm = d_buf[seek:]
    assert d_pcm.data_ptr() == d_buf.data_ptr() + 4 * seek
    launches = _launches(G, ops, hop, pitch, fusable, 4 * seek)
    name = "glv_bars_rows_i8_kernel" if ops & G.OP_BARS and launches == 1 else "glv_wave_kernel"      # the first launch, as the process call reports
    got = compare(G, bt, bs, "wave", x, d_pcm, pitch, hop, [t * hop for t in range(steps)], n, steps, ops, n if w is None else w, launches, name,
                  state=False, what=(hop, pitch))
    assert int(got.ne(0).sum()) > 0
    return bt, bs, x, pitch


def _ops(G):
    return {"wave": G.OP_WAVE, "wave_r16": G.OP_WAVE | G.OP_R16, "pass": G.OP_WAVE | G.OP_BARS, "pass_r16": G.OP_WAVE | G.OP_BARS | G.OP_R16}


# ---- 1. the contract against sequential calls ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("hop_kind", ["8", "100", "n", "n+8"])
@pytest.mark.parametrize("n", [256, 1024])
@pytest.mark.parametrize("form", ["wave", "wave_r16", "pass", "pass_r16"])
def test_track_wave_equals_sequential_calls(glvlib, form, n, hop_kind, channels):
    """all four output forms; bars = n (256 is the fewest the integer pass takes); hops that keep every window on a group of 8 frames (one launch with
    bars) and one that does not (two)"""
    G = glvlib
    hop = {"8": 8, "100": 100, "n": n, "n+8": n + 8}[hop_kind]
    p = G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5, channels=channels)
    bt, bs, _, pitch = _compare(G, p, _ops(G)[form], n, hop)
    assert bt.bars_arithmetic() == G.BARS_I8_EXACT
    assert pitch % 8 == (0 if hop != 100 else 4)
    bt.close(); bs.close()


@pytest.mark.parametrize("order", ["rows", "steps"])
@pytest.mark.parametrize("hop", [8, 264])
def test_both_row_orders_of_the_one_launch_form(glvlib, monkeypatch, order, hop):
    """which rows share a workgroup of the bars kernel -- 64 consecutive output rows, or 64 consecutive steps of one channel row -- changes no bit
    (GLV_TRACK_WAVE_ORDER at creation: diagnostics).  70 steps: by steps every channel row is one full block and a partial one"""
    G = glvlib
    n = 256
    monkeypatch.setenv("GLV_TRACK_WAVE_ORDER", order)
    p = G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5)
    for ops in (G.OP_WAVE | G.OP_BARS | G.OP_R16, G.OP_WAVE | G.OP_BARS):
        bt, bs, _, _ = _compare(G, p, ops, n, hop, steps=70)
        assert bt.last_launches() == 1
        bt.close(); bs.close()


def test_window_starts_off_the_groups_of_8_frames(glvlib):
    """hop 1, and a hop of 8 in a pitch that is no multiple of 8: windows start at any frame -- two launches with bars"""
    G = glvlib
    n = 256
    p = G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5)
    for hop, pitch in ((1, n + STEPS + 2), (8, n + (STEPS - 1) * 8 + 3)):
        for ops in (G.OP_WAVE | G.OP_R16, G.OP_WAVE | G.OP_BARS | G.OP_R16):
            bt, bs, _, _ = _compare(G, p, ops, n, hop, pitch=pitch)
            bt.close(); bs.close()


@pytest.mark.parametrize("seek", [1, 4])
@pytest.mark.parametrize("form", ["wave", "wave_r16", "pass", "pass_r16"])
def test_recordings_that_begin_at_any_frame_of_the_buffer(glvlib, form, seek):
    """d_pcm one frame (4 bytes) and four frames (16 bytes) off a 32-byte boundary -- a seek into a recording: the waveform kernel's groups fall off their
    16-byte loads, and with bars the hops that would take one launch (8, 256) take two like hop 100, through the workspace the query reported"""
    G = glvlib
    n = 256
    p = G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5)
    for hop in (8, 100, 256):
        bt, bs, _, _ = _compare(G, p, _ops(G)[form], n, hop, seek=seek)
        assert bt.last_launches() == (2 if "pass" in form else 1)
        bt.close(); bs.close()


def test_the_sizing_query_covers_both_forms(glvlib):
    """without bars 256; with bars what the two launches need whatever hop and pitch: the query cannot see d_pcm, whose alignment picks the form"""
    G = glvlib
    n = 256
    b = G.Batch(G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5), STREAMS, G.OP_WAVE | G.OP_BARS)
    rows = STEPS * STREAMS * 2
    for hop in (8, 100):
        pitch = _pitch(n, hop, STEPS)
        assert b.track_wave_work_bytes(pitch, hop, STEPS, G.OP_WAVE) == b.track_wave_work_bytes(pitch, hop, STEPS, G.OP_WAVE | G.OP_R16) == 256
        for ops in (G.OP_WAVE | G.OP_BARS, G.OP_WAVE | G.OP_BARS | G.OP_R16):
            assert b.track_wave_work_bytes(pitch, hop, STEPS, ops) == (rows * n * 2 + 255) // 256 * 256       # (the integer pass takes texel rows)
    b.close()


# ---- 2. the shipped size ------------------------------------------------------------------------------------------------------------
def test_track_wave_at_the_shipped_size(glvlib):
    G = glvlib
    n = 4096
    p = G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5)
    bt, bs, _, _ = _compare(G, p, G.OP_WAVE | G.OP_BARS | G.OP_R16, n, 256, steps=5, streams=2)
    assert bt.last_launches() == 1 and bt.kernel_name() == "glv_bars_rows_i8_kernel"
    bt.close(); bs.close()


# ---- 3. against the oracle, not only the library ------------------------------------------------------------------------------------
def test_track_wave_equals_the_oracle(glvlib, oracle):
    """every step of one stream: the wave bind's upload texels (unpack, wrange, GL_R16 rounding) and the exact integer pre-smoothing pass over them, as
    texels and as floats -- the models tests/test_wave.py holds the process call to"""
    import torch
    G = glvlib
    n, hop, factor = 1024, 256, 0.025
    pitch = _pitch(n, hop, STEPS)
    x = _pcm(6160, STREAMS, pitch)
    d_pcm = torch.from_numpy(x).cuda()
    b = G.Batch(G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5, smooth_factor=factor), STREAMS, G.OP_WAVE | G.OP_BARS)
    tex = _track(b, d_pcm, pitch, hop, STEPS, G.OP_WAVE | G.OP_R16, n, torch.int16).cpu().numpy().view(np.uint16)
    flt = _track(b, d_pcm, pitch, hop, STEPS, G.OP_WAVE, n, torch.float32).cpu().numpy()
    ptex = _track(b, d_pcm, pitch, hop, STEPS, G.OP_WAVE | G.OP_BARS | G.OP_R16, n, torch.int16).cpu().numpy().view(np.uint16)
    pflt = _track(b, d_pcm, pitch, hop, STEPS, G.OP_WAVE | G.OP_BARS, n, torch.float32).cpu().numpy()
    s = 1
    for t in range(STEPS):
        up = upload(planar_of_s16(np.ascontiguousarray(x[s, t * hop:t * hop + n, :]).reshape(-1), 1, n))
        for c in range(2):
            r = 2 * s + c
            assert same(tex[t, r], up[c]), (t, c)
            assert same(flt[t, r], texel_floats(up[c])), (t, c)
            wt, wf = Oracle.bars_int(up[c], n, factor, 0.5)
            assert same(ptex[t, r], wt), (t, c)
            assert same(pflt[t, r], wf), (t, c)
    b.close()


# ---- 4. every other bars form: two launches, equal to the sequential calls ----------------------------------------------------------
@pytest.mark.parametrize("r16", [True, False])
@pytest.mark.parametrize("mode", [1, 2])
def test_track_wave_maximum_and_hybrid(glvlib, mode, r16):
    G = glvlib
    n = 1024
    p = G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5, sample_mode=mode)
    bt, bs, _, _ = _compare(G, p, G.OP_WAVE | G.OP_BARS | (G.OP_R16 if r16 else 0), n, 256, fusable=False)
    assert bt.bars_arithmetic() == G.BARS_F32_SEQ
    bt.close(); bs.close()


@pytest.mark.parametrize("r16", [True, False])
def test_track_wave_fewer_than_256_bars(glvlib, r16):
    G = glvlib
    n = 1024
    p = G.Params(n=n, gl_storage=1, bars=80)
    bt, bs, _, _ = _compare(G, p, G.OP_WAVE | G.OP_BARS | (G.OP_R16 if r16 else 0), n, 256, w=80, fusable=False)
    assert bt.bars_arithmetic() == G.BARS_F32_CHAIN
    bt.close(); bs.close()


@pytest.mark.parametrize("r16", [True, False])
def test_track_wave_bar_texel_table(glvlib, r16):
    G = glvlib
    n = 1024
    tex, _ = wave_column_texels(n, 320)
    p = G.Params(n=n, gl_storage=1, bars=len(tex))
    bt, bs, _, _ = _compare(G, p, G.OP_WAVE | G.OP_BARS | (G.OP_R16 if r16 else 0), n, 256, w=len(tex), fusable=False,
                            prepare=lambda b: b.set_bar_texels(tex))
    bt.close(); bs.close()


def test_track_wave_unfused_at_creation(glvlib, monkeypatch):
    G = glvlib
    n = 1024
    monkeypatch.setenv("GLV_UNFUSED_WAVE", "1")
    p = G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5)
    bt, bs, _, _ = _compare(G, p, G.OP_WAVE | G.OP_BARS | G.OP_R16, n, 256, fusable=False)
    assert bt.kernel_name() == "glv_wave_kernel"
    bt.close(); bs.close()


# ---- 5. chunking and pointer offset; the batch's state ------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [8, 100])
def test_track_wave_chunks_compose_and_touch_no_state(glvlib, hop):
    """track(4) from the buffer's start, then track(7) from 4 hops in == track(11); a GL chain run on the same batch before and after the track calls
    continues exactly like an untouched twin's"""
    import torch
    G = glvlib
    n = 1024
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    p = G.Params(n=n, gl_storage=1, avg_window_kind=1, bars=n, bar_phase=0.5)
    mask = G.OP_WAVE | G.OP_BARS | GA
    ops = G.OP_WAVE | G.OP_BARS | G.OP_R16
    pitch = _pitch(n, hop, STEPS)
    x = _pcm(88 + hop, STREAMS, pitch)
    d_pcm = torch.from_numpy(x).cuda()
    b, twin = G.Batch(p, STREAMS, mask), G.Batch(p, STREAMS, mask)
    wins = _windows(x, n, hop, 0, 3)
    chain = G.OP_FFT | GA | G.OP_R16
    assert _eq(_seq(b, wins[:2], chain, n, torch.int16), _seq(twin, wins[:2], chain, n, torch.int16))
    whole = _track(b, d_pcm, pitch, hop, STEPS, ops, n, torch.int16)
    first = _track(b, d_pcm, pitch, hop, 4, ops, n, torch.int16)
    rest = _track(b, d_pcm, pitch, hop, 7, ops, n, torch.int16, t0=4)
    assert b.last_launches() == (1 if hop == 8 else 2)
    assert _eq(torch.cat([first, rest]), whole)
    assert _eq(_seq(b, wins[2:], chain, n, torch.int16), _seq(twin, wins[2:], chain, n, torch.int16))
    b.close(); twin.close()


# ---- 6. graph capture ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [256, 100])
def test_first_track_wave_call_can_be_captured_and_replayed(glvlib, hop):
    """the FIRST call after creation, captured into a hipGraph (global mode: an allocation or a synchronous copy would invalidate the capture), replayed
    twice on new PCM; one stream, no parallel branches"""
    import torch
    G = glvlib
    hip = C.CDLL("libamdhip64.so")
    n = 1024
    ops = G.OP_WAVE | G.OP_BARS | G.OP_R16
    p = G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5)
    pitch = _pitch(n, hop, STEPS)
    d_pcm = torch.from_numpy(_pcm(19, STREAMS, pitch)).cuda()
    bg, be = G.Batch(p, STREAMS, G.OP_WAVE | G.OP_BARS), G.Batch(p, STREAMS, G.OP_WAVE | G.OP_BARS)
    work = torch.zeros((bg.track_wave_work_bytes(pitch, hop, STEPS, ops),), dtype=torch.uint8, device="cuda")
    og = torch.zeros((STEPS, STREAMS * 2, n), dtype=torch.int16, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = C.c_void_p(st.cuda_stream)
    assert hip.hipStreamBeginCapture(sp, 0) == 0                    # hipStreamCaptureModeGlobal
    try:
        bg.track_wave_s16(d_pcm, pitch, hop, STEPS, og, work, ops, stream=st.cuda_stream)
    finally:
        graph = C.c_void_p()
        rc = hip.hipStreamEndCapture(sp, C.byref(graph))
    assert rc == 0
    assert bg.last_launches() == (1 if hop % 8 == 0 else 2)
    exe = C.c_void_p()
    assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
    for rep in range(2):
        d_pcm.copy_(torch.from_numpy(_pcm(700 + rep, STREAMS, pitch)).cuda())
        torch.cuda.synchronize()
        assert hip.hipGraphLaunch(exe, sp) == 0
        st.synchronize()
        want = _track(be, d_pcm, pitch, hop, STEPS, ops, n, torch.int16)
        assert _eq(og, want), rep
        assert int(og.ne(0).sum()) > 0
    hip.hipGraphExecDestroy(exe); hip.hipGraphDestroy(graph)
    bg.close(); be.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_track_wave_refusals_launch_nothing(glvlib):
    import torch
    G = glvlib
    n, hop = 1024, 256
    ops = G.OP_WAVE | G.OP_BARS | G.OP_R16
    pitch = _pitch(n, hop, STEPS)
    x = _pcm(3, STREAMS, pitch)
    d_pcm = torch.from_numpy(x).cuda()
    p = G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5)
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    b = G.Batch(p, STREAMS, G.OP_WAVE | G.OP_BARS | GA)
    work = torch.zeros((b.track_wave_work_bytes(pitch, 100, STEPS, ops) + 256,), dtype=torch.uint8, device="cuda")
    out = torch.full((STEPS, STREAMS * 2, n), 0x5A5A, dtype=torch.int16, device="cuda")

    def refused(batch, code, ops_=ops, pitch_=pitch, hop_=hop, steps_=STEPS, pcm=d_pcm, o=out, w=work, query=True):
        with pytest.raises(G.GlvError) as ei:
            batch.track_wave_s16(pcm, pitch_, hop_, steps_, o, w, ops_)
        assert ei.value.code == code, (ei.value.code, str(ei.value))
        assert "glv error" in str(ei.value) and len(str(ei.value)) > 14           # a message in glv_last_error
        if query and pcm is not None and o is not None and w is not None:            # the sizing query refuses the same arguments
            with pytest.raises(G.GlvError) as ei:
                batch.track_wave_work_bytes(pitch_, hop_, steps_, ops_)
            assert ei.value.code == code

    for bad in (G.OP_FFT, G.OP_GRAVITY, G.OP_AVERAGE, G.OP_RAW, G.OP_SMOOTH, G.OP_WRANGE, G.OP_MAGNITUDE, G.OP_OUTPUT_IS_STATE, G.OP_PRIVATE_STATE):
        refused(b, G.ERR_INVALID, ops_=ops | bad)
    refused(b, G.ERR_INVALID, ops_=G.OP_BARS | G.OP_R16)                         # no GLV_OP_WAVE
    refused(b, G.ERR_INVALID, ops_=G.OP_FFT | GA)
    refused(b, G.ERR_INVALID, steps_=0)
    refused(b, G.ERR_INVALID, hop_=0)
    refused(b, G.ERR_INVALID, pitch_=n + (STEPS - 1) * hop - 1)                  # too short for the steps
    refused(b, G.ERR_INVALID, hop_=n + 8)                                        # ... as it is for a larger hop
    refused(b, G.ERR_INVALID, pcm=None)
    refused(b, G.ERR_INVALID, o=None)
    refused(b, G.ERR_INVALID, w=None)
    refused(b, G.ERR_INVALID, w=work.data_ptr() + 128, query=False)              # 256-byte alignment
    refused(b, G.ERR_INVALID, steps_=1 << 31, hop_=1, pitch_=0xffffffff)         # 2^31 steps x 6 rows > 2^32 rows
    # what a GLV_OP_WAVE process call is refused for (bar parameters cannot change without glv_batch_set_params through this binding, and a single-row
    # batch belongs to the drop-ins, which expose no batch: those two refusals are not reachable from here)
    fl = G.Batch(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=0), STREAMS, G.OP_WAVE | G.OP_BARS)
    refused(fl, G.ERR_STATE)
    for mask in (G.OP_WAVE, G.OP_BARS, G.OP_BARS | GA):
        nb = G.Batch(p, STREAMS, mask)
        refused(nb, G.ERR_STATE)
        nb.close()
    table = graph_column_texels(n, 200)[0]
    cols = G.Batch(G.Params(n=n, gl_storage=1, bars=len(table)), STREAMS, G.OP_WAVE | G.OP_BARS | GA)
    cols.set_column_texels(table)
    refused(cols, G.ERR_STATE)
    refused(cols, G.ERR_STATE, ops_=G.OP_WAVE | G.OP_R16)
    for x_ in (fl, cols): x_.close()
    # the FFT track call still refuses GLV_OP_WAVE
    w2 = torch.zeros((1 << 20,), dtype=torch.uint8, device="cuda")
    for bad_ops in (G.OP_WAVE, G.OP_FFT | G.OP_WAVE):
        with pytest.raises(G.GlvError) as ei:
            b.track_s16(d_pcm, pitch, hop, STEPS, out, w2, bad_ops)
        assert ei.value.code == G.ERR_INVALID
    # nothing was launched: the output still holds its fill
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A).all())
    # after all the refused calls the batch still produces the sequential results
    bs = G.Batch(p, STREAMS, G.OP_WAVE | G.OP_BARS)
    for h in (hop, 100):
        pt = _pitch(n, h, STEPS)
        xx = _pcm(4 + h, STREAMS, pt)
        got = _track(b, torch.from_numpy(xx).cuda(), pt, h, STEPS, ops, n, torch.int16)
        assert _eq(got, _seq(bs, _windows(xx, n, h, 0, STEPS), ops, n, torch.int16))
    b.close(); bs.close()
