"""GPU: track mode (glv_batch_track_s16) -- every update of a recording in one call, the state kept on chip.

Contract: the output of step t and the batch's state afterwards are bit for bit what `steps` consecutive glv_batch_process_s16 calls on the
windows [t * hop, t * hop + n) of every stream produce and leave behind.  The sequential side is a second batch driven window by window, the
windows cut on the host from the same buffer; floats are compared as int32.  Every track call here gets a workspace of exactly
glv_batch_track_work_bytes bytes followed by a guard region, which must come back intact, and a pitch larger than the call consumes."""

import ctypes as C

import numpy as np
import pytest

from glava_amd.bar_positions import graph_column_texels, radial_bar_texels
from oracle_lib import StreamOracle
from track_lib import S16_CHAIN_NAMES as CHAIN_NAMES, compare_hop, eq as _eq, hop_windows as _windows, pcm as _pcm, pitch_residue as _pitch
from track_lib import s16_chains as _chains, seq as _seq, track

pytestmark = pytest.mark.gpu

STEPS, STREAMS = 11, 3          # F = 5: the ring wraps twice; 11 is no multiple of n / hop: the residue launches hold unequal window counts


def _track(b, *args, **kw):
    """steps [t0, t0 + steps) of the buffer in one call of glv_batch_track_s16 (track_lib.track: exact workspace and output, guards behind both)"""
    return track(b, "residue", *args, **kw)


def _compare(G, p, mask, ops, n, hop, steps=STEPS, streams=STREAMS, w=None, prepare=None, seed=31):
    """one track call against the sequential calls, every step; returns the two batches (track, sequential) for what follows"""
    pitch = _pitch(n, hop, steps)
    x = _pcm(seed + n + hop, streams, pitch)
    bt, bs = G.Batch(p, streams, mask), G.Batch(p, streams, mask)
    if prepare:
        prepare(bt); prepare(bs)
    launches = n // hop + 1 + (1 if ops & G.OP_BARS else 0)
    compare_hop(G, bt, bs, "residue", x, False, pitch, hop, n, steps, ops, n if w is None else w, launches, "glv_track_scan_kernel", state=False)
    return bt, bs, x, pitch


# ---- 1. the contract against sequential calls ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_mode", [0, 1])
@pytest.mark.parametrize("quarter_hop", [True, False])
@pytest.mark.parametrize("n", [256, 1024])
@pytest.mark.parametrize("chain", CHAIN_NAMES)
def test_track_equals_sequential_calls(glvlib, chain, n, quarter_hop, log_mode):
    G = glvlib
    kw, mask, ops = _chains(G)[chain]
    bt, bs, _, _ = _compare(G, G.Params(n=n, log_mode=log_mode, **kw), mask, ops, n, n // 4 if quarter_hop else n)
    bt.close(); bs.close()


@pytest.mark.parametrize("chain", ["chain", "gl_chain_r16"])
def test_track_at_the_shipped_size(glvlib, chain):
    """n = 4096, hop 256: the shipped size's kernels with 16 residue launches"""
    G = glvlib
    kw, mask, ops = _chains(G)[chain]
    bt, bs, _, _ = _compare(G, G.Params(n=4096, **kw), mask, ops, 4096, 256, steps=7, streams=2)
    bt.close(); bs.close()


def test_track_audit_log(glvlib):
    """log_mode 2 on gl_storage 1: the sequential calls run the GL passes one by one, the same texels"""
    G = glvlib
    kw, mask, ops = _chains(G)["gl_chain_r16"]
    # (GLV_OP_BARS in the creation mask: the sequential side's passes park the float spectra in the batch's internal rows, made for announced bars)
    bt, bs, _, _ = _compare(G, G.Params(n=1024, log_mode=2, **kw), mask | G.OP_BARS, ops, 1024, 256)
    bt.close(); bs.close()


# ---- 2. bars ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r16", [True, False])
def test_track_presmoothing_pass(glvlib, r16):
    """gl_storage 1, bars = n, bar_phase 0.5: the integer matrix-core pass over every step's texel rows"""
    G = glvlib
    n = 4096
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    p = G.Params(n=n, gl_storage=1, avg_window_kind=1, bars=n, bar_phase=0.5)
    bt, bs, _, _ = _compare(G, p, GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | (G.OP_R16 if r16 else 0), n, 1024, streams=2, w=n)
    assert bt.bars_arithmetic() == G.BARS_I8_EXACT
    bt.close(); bs.close()


@pytest.mark.parametrize("n", [1024, 4096])
def test_track_eighty_bars_of_a_float_chain(glvlib, n):
    G = glvlib
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    bt, bs, _, _ = _compare(G, G.Params(n=n, bars=80), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS, n, n // 4, w=80)
    bt.close(); bs.close()


@pytest.mark.parametrize("sample_mode", [0, 1])
@pytest.mark.parametrize("r16", [True, False])
def test_track_bar_texel_table(glvlib, r16, sample_mode):
    G = glvlib
    n = 1024
    tex, _ = radial_bar_texels(n, 160)
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    p = G.Params(n=n, gl_storage=1, avg_window_kind=1, bars=len(tex), sample_mode=sample_mode)
    bt, bs, _, _ = _compare(G, p, GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | (G.OP_R16 if r16 else 0), n, n // 4, w=len(tex),
                            prepare=lambda b: b.set_bar_texels(tex))
    bt.close(); bs.close()


# ---- 3. state ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["gravity", "chain", "gl_chain_r16", "gl_gravity"])
def test_track_state_composes(glvlib, chain):
    """chunks compose, a track leaves what a process call continues from and starts from what process calls left, reset starts over"""
    import torch
    G = glvlib
    n, hop = 1024, 256
    kw, mask, ops = _chains(G)[chain]
    p = G.Params(n=n, **kw)
    dt = torch.int16 if ops & G.OP_R16 else torch.float32
    # track(11) against the sequential calls; then one ordinary call on both == the 12th sequential call
    pitch = _pitch(n, hop, STEPS + 1)
    x = _pcm(77, STREAMS, pitch)
    d_pcm = torch.from_numpy(x).cuda()
    wins = _windows(x, n, hop, 0, STEPS + 1)
    bs = G.Batch(p, STREAMS, mask)
    want = _seq(bs, wins, ops, n, dt)                                     # 12 sequential calls: the reference of everything below
    bt = G.Batch(p, STREAMS, mask)
    whole = _track(bt, d_pcm, pitch, hop, STEPS, ops, n, dt)
    assert _eq(whole, want[:STEPS])
    assert _eq(_seq(bt, wins[STEPS:], ops, n, dt)[0], want[STEPS])
    # track(4) then track(7) == track(11)
    bc = G.Batch(p, STREAMS, mask)
    first = _track(bc, d_pcm, pitch, hop, 4, ops, n, dt)
    rest = _track(bc, d_pcm, pitch, hop, 7, ops, n, dt, t0=4)
    assert _eq(torch.cat([first, rest]), whole)
    # reset between two tracks: the first track's output again
    bc.reset()
    assert _eq(_track(bc, d_pcm, pitch, hop, STEPS, ops, n, dt), whole)
    # two sequential calls before a track == sequential all the way
    bm = G.Batch(p, STREAMS, mask)
    head = _seq(bm, wins[:2], ops, n, dt)
    tail = _track(bm, d_pcm, pitch, hop, STEPS - 2, ops, n, dt, t0=2)
    assert _eq(torch.cat([head, tail]), want[:STEPS])
    for b in (bs, bt, bc, bm): b.close()


# ---- 4. against the oracle, not only the library --------------------------------------------------------------------------------------------
def test_track_float_chain_equals_the_oracle(glvlib, oracle):
    """log_mode 0, fft -> gravity -> average: every step of one stream equals StreamOracle.frame on that window bit for bit (the standard of
    tests/test_gpu_parity.py test_log_mode_0_chain_bit_exact_end_to_end)"""
    import torch
    G = glvlib
    n, hop, F = 1024, 256, 5
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    pitch = _pitch(n, hop, STEPS)
    x = _pcm(5150, STREAMS, pitch)
    b = G.Batch(G.Params(n=n, avg_frames=F, log_mode=0), STREAMS, GA)
    got = _track(b, torch.from_numpy(x).cuda(), pitch, hop, STEPS, G.OP_FFT | GA, n, torch.float32).cpu().numpy()
    s = 1
    so = StreamOracle(n, avg_frames=F)
    for t in range(STEPS):
        want = so.frame(x[s, t * hop:t * hop + n, :])
        assert (got[t, 2 * s:2 * s + 2].view(np.uint32) == want.view(np.uint32)).all(), t
    b.close()


# ---- 6. graph capture -------------------------------------------------------------------------------------------------------------------
def test_first_track_call_can_be_captured_and_replayed(glvlib):
    """the FIRST track call after creation, captured into a hipGraph (global mode: an allocation or a synchronous copy would invalidate the capture); one
    graph holds one full turn of the ring (the head advances on the host), so a replay continues like the same call issued again"""
    import torch
    G = glvlib
    hip = C.CDLL("libamdhip64.so")
    n, hop, F = 1024, 256, 5
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    ops = G.OP_FFT | GA | G.OP_R16
    p = G.Params(n=n, gl_storage=1, avg_window_kind=1, avg_frames=F)
    pitch = _pitch(n, hop, F)
    d_pcm = torch.from_numpy(_pcm(9, STREAMS, pitch)).cuda()
    bg, be = G.Batch(p, STREAMS, GA), G.Batch(p, STREAMS, GA)
    work = torch.zeros((bg.track_work_bytes(pitch, hop, F, ops),), dtype=torch.uint8, device="cuda")
    og = torch.zeros((F, STREAMS * 2, n), dtype=torch.int16, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = C.c_void_p(st.cuda_stream)
    assert hip.hipStreamBeginCapture(sp, 0) == 0                    # hipStreamCaptureModeGlobal
    try:
        bg.track_s16(d_pcm, pitch, hop, F, og, work, ops, stream=st.cuda_stream)
    finally:
        graph = C.c_void_p()
        rc = hip.hipStreamEndCapture(sp, C.byref(graph))
    assert rc == 0
    exe = C.c_void_p()
    assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
    for rep in range(3):
        assert hip.hipGraphLaunch(exe, sp) == 0
        st.synchronize()
        want = _track(be, d_pcm, pitch, hop, F, ops, n, torch.int16)
        assert _eq(og, want), rep
    hip.hipGraphExecDestroy(exe); hip.hipGraphDestroy(graph)
    bg.close(); be.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_track_refusals_leave_the_batch_untouched(glvlib):
    import torch
    G = glvlib
    n, hop = 1024, 256
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    ops = G.OP_FFT | GA
    pitch = _pitch(n, hop, STEPS)
    x = _pcm(3, STREAMS, pitch)
    d_pcm = torch.from_numpy(x).cuda()
    p = G.Params(n=n)
    b = G.Batch(p, STREAMS, GA | G.OP_BARS)
    work = torch.zeros((b.track_work_bytes(pitch, hop, STEPS, ops | G.OP_BARS),), dtype=torch.uint8, device="cuda")
    out = torch.zeros((STEPS, STREAMS * 2, n), dtype=torch.float32, device="cuda")

    def refused(batch, code, ops_=ops, pitch_=pitch, hop_=hop, steps_=STEPS, pcm=d_pcm, o=out, w=work):
        with pytest.raises(G.GlvError) as ei:
            batch.track_s16(pcm, pitch_, hop_, steps_, o, w, ops_)
        assert ei.value.code == code, (ei.value.code, str(ei.value))
        assert "glv error" in str(ei.value) and len(str(ei.value)) > 14           # a message in glv_last_error
        if pcm is not None and o is not None and w is not None:                      # the sizing query refuses the same arguments
            with pytest.raises(G.GlvError) as ei:
                batch.track_work_bytes(pitch_, hop_, steps_, ops_)
            assert ei.value.code == code

    for bad in (G.OP_RAW, G.OP_SMOOTH, G.OP_WRANGE, G.OP_MAGNITUDE):
        refused(b, G.ERR_INVALID, ops_=ops | bad)
    refused(b, G.ERR_INVALID, ops_=G.OP_WAVE)
    refused(b, G.ERR_INVALID, ops_=G.OP_FFT | G.OP_WAVE)
    refused(b, G.ERR_INVALID, ops_=G.OP_FFT | G.OP_GRAVITY | G.OP_OUTPUT_IS_STATE)
    refused(b, G.ERR_INVALID, ops_=GA)                                           # no GLV_OP_FFT
    refused(b, G.ERR_INVALID, steps_=0)
    for bad_hop in (0, 2, 192, 2 * n):
        refused(b, G.ERR_INVALID, hop_=bad_hop, pitch_=16 * n)
    refused(b, G.ERR_INVALID, pitch_=pitch + 4)                                  # not a multiple of hop
    refused(b, G.ERR_INVALID, pitch_=n + (STEPS - 1) * hop - hop)                # too short for the steps
    refused(b, G.ERR_INVALID, pcm=None)
    refused(b, G.ERR_INVALID, o=None)
    refused(b, G.ERR_INVALID, w=None)
    # the state the call needs
    gl2 = G.Batch(G.Params(n=n, gl_storage=2), STREAMS, GA)
    refused(gl2, G.ERR_STATE)
    live = G.Batch(G.Params(n=n, gl_storage=1), STREAMS, GA | G.OP_BARS | G.OP_BARS_ONLY)
    refused(live, G.ERR_STATE, ops_=ops | G.OP_BARS)
    table = graph_column_texels(n, 200)[0]
    cols = G.Batch(G.Params(n=n, gl_storage=1, bars=len(table)), STREAMS, GA | G.OP_BARS)
    cols.set_column_texels(table)
    refused(cols, G.ERR_STATE, ops_=ops | G.OP_BARS)
    unannounced = G.Batch(p, STREAMS, G.OP_FFT)
    refused(unannounced, G.ERR_STATE)
    # the gravity form mix: gravity ran without average on this batch, a track with both is refused as a process call is
    mixed = G.Batch(p, STREAMS, GA)
    mixed.process_s16(_windows(x, n, hop, 0, 1)[0], out[0], G.OP_FFT | G.OP_GRAVITY)
    with pytest.raises(G.GlvError) as ei:
        mixed.track_s16(d_pcm, pitch, hop, STEPS, out, work, ops)
    assert ei.value.code == G.ERR_STATE
    for x_ in (gl2, live, cols, unannounced, mixed): x_.close()
    # after all the refused calls the batch still produces the sequential results, from untouched state
    bs = G.Batch(p, STREAMS, GA | G.OP_BARS)
    got = _track(b, d_pcm, pitch, hop, STEPS, ops, n, torch.float32)
    assert _eq(got, _seq(bs, _windows(x, n, hop, 0, STEPS), ops, n, torch.float32))
    b.close(); bs.close()
