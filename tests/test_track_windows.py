"""GPU: track mode at any hop (glv_batch_track_windows_s16) -- one transform launch reads each window where it lies in the recording.

Contract (glv_batch_track_s16's, word for word): the output of step t and the batch's state afterwards are bit for bit what `steps` consecutive
glv_batch_process_s16 calls on the windows [t * hop, t * hop + n) of every stream produce and leave behind.  The sequential side is a second batch
driven window by window, the windows cut on the host from the same buffer; floats are compared as int32.  Every call here gets a workspace of exactly
glv_batch_track_windows_work_bytes bytes followed by a guard region, which must come back intact; pitches are odd and larger than the call consumes;
the recording sits one frame behind an 8-byte boundary where a test says `odd`, so that its windows alternate between the two load forms (odd hop) or
all take the dword form (even hop)."""

import ctypes as C

import numpy as np
import pytest

from glava_amd.bar_positions import graph_column_texels, radial_bar_texels
from oracle_lib import Oracle, StreamOracle
from track_lib import S16_CHAIN_SIZES as CHAIN_SIZES, compare_hop, eq as _eq, fft_kernel, hop_windows as _windows
from track_lib import launches_fft as _launches, pcm as _pcm, pitch_odd as _pitch, s16_chains as _chains, seq as _seq, to_device, track

pytestmark = pytest.mark.gpu

STEPS, STREAMS = 11, 3          # F = 5: the ring wraps twice


def _track(b, *args, old=False, **kw):
    """steps [t0, t0 + steps) of the buffer in one call (track_lib.track: exact workspace and output, guards behind both); old: through the residue entry"""
    return track(b, "residue" if old else "windows", *args, **kw)


def _compare(G, bt, bs, ops, n, hop, steps=STEPS, w=None, odd=False, seed=31):
    """one call against the sequential calls, every step, and the state through one more update on both; the batches start from reset state"""
    pitch = _pitch(n, hop, steps + 1)
    x = _pcm(seed + n + hop, bt.streams, pitch)
    compare_hop(G, bt, bs, "windows", x, odd, pitch, hop, n, steps, ops, n if w is None else w, _launches(G, ops), fft_kernel(G, ops))


def _hops(n):
    return (1, 45, n // 4, n + 3)


# ---- 1. the contract against sequential calls, recording aligned and one frame off ------------------------------------------------------
@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("log_mode", [0, 1])
@pytest.mark.parametrize("chain,n,variant", CHAIN_SIZES)
def test_track_windows_equals_sequential_calls(glvlib, chain, n, variant, log_mode, odd):
    G = glvlib
    kw, mask, ops = _chains(G)[chain]
    p = G.Params(n=n, log_mode=log_mode, **kw)
    bt, bs = G.Batch(p, STREAMS, mask), G.Batch(p, STREAMS, mask)
    assert bt.variants() > variant
    bt.set_variant(variant)
    for hop in _hops(n):
        bt.reset(); bs.reset()
        _compare(G, bt, bs, ops, n, hop, odd=odd)
        assert bt.last_variant() == variant
    bt.close(); bs.close()


@pytest.mark.parametrize("chain", ["chain", "gl_chain_r16"])
def test_track_windows_at_the_shipped_size(glvlib, chain):
    """n = 4096, hop 735 (44.1 kHz at 60 fps): windows alternate between the two load forms"""
    G = glvlib
    kw, mask, ops = _chains(G)[chain]
    p = G.Params(n=4096, **kw)
    bt, bs = G.Batch(p, 2, mask), G.Batch(p, 2, mask)
    _compare(G, bt, bs, ops, 4096, 735, steps=7)
    bt.close(); bs.close()


# ---- 2. bars ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table,gl_storage,r16", [(False, 0, False), (False, 1, True), (False, 1, False), (True, 1, True), (True, 1, False)])
def test_track_windows_bars(glvlib, table, gl_storage, r16):
    """n = 1024, hop 45: 80 bars of a float chain, the pre-smoothing pass of a GL chain (bars = n, bar_phase 0.5) and bars at a bar-texel table (a GL
    chain's), as texels and as floats; then the same from a recording one frame off, continuing from the state the first call left"""
    G = glvlib
    n, hop = 1024, 45
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    tex = radial_bar_texels(n, 160)[0] if table else None
    bars = len(tex) if table else (n if gl_storage == 1 else 80)
    kw = dict() if gl_storage == 0 else dict(gl_storage=1, avg_window_kind=1) if table else dict(gl_storage=1, avg_window_kind=1, bar_phase=0.5)
    p = G.Params(n=n, bars=bars, **kw)
    ops = G.OP_FFT | GA | G.OP_BARS | (G.OP_R16 if r16 else 0)
    bt, bs = G.Batch(p, STREAMS, GA | G.OP_BARS), G.Batch(p, STREAMS, GA | G.OP_BARS)
    if table:
        bt.set_bar_texels(tex); bs.set_bar_texels(tex)
    _compare(G, bt, bs, ops, n, hop, w=bars)
    _compare(G, bt, bs, ops, n, hop, w=bars, odd=True, seed=77)                     # (continues from the state the first comparison left on both)
    bt.close(); bs.close()


def test_track_windows_stateless_bars(glvlib):
    G = glvlib
    n, hop = 1024, 45
    p = G.Params(n=n, bars=80)
    bt, bs = G.Batch(p, STREAMS, G.OP_BARS), G.Batch(p, STREAMS, G.OP_BARS)
    _compare(G, bt, bs, G.OP_FFT | G.OP_BARS, n, hop, w=80)
    assert bt.track_windows_work_bytes(_pitch(n, hop, STEPS), hop, STEPS, G.OP_FFT | G.OP_BARS) == STEPS * STREAMS * 2 * n * 4
    bt.close(); bs.close()


# ---- 3. against the old entry, chunking and mixing ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["fft_r16", "gravity", "chain", "gl_chain_r16"])
def test_track_windows_equals_the_residue_entry_and_composes(glvlib, chain):
    """at hop n / 4, which both entries take: identical output and state (seen through a following process call on both); track(4) then track(7) ==
    track(11); a process call between chunks; a glv_batch_track_s16 chunk followed by a windows chunk"""
    import torch
    G = glvlib
    n, hop = 1024, 256
    kw, mask, ops = _chains(G)[chain]
    p = G.Params(n=n, **kw)
    dt = torch.int16 if ops & G.OP_R16 else torch.float32
    pitch = (STEPS + 4) * hop + n                                                   # a multiple of the hop: the old entry asks for it
    x = _pcm(77, STREAMS, pitch)
    d_pcm = to_device(x, False, False)
    wins = _windows(x, n, hop, 0, STEPS + 1)
    bo, bn = G.Batch(p, STREAMS, mask), G.Batch(p, STREAMS, mask)
    old = _track(bo, d_pcm, pitch, hop, STEPS, ops, n, dt, old=True)
    new = _track(bn, d_pcm, pitch, hop, STEPS, ops, n, dt)
    assert _eq(old, new)
    assert bn.track_windows_work_bytes(pitch, hop, STEPS, ops) <= bo.track_work_bytes(pitch, hop, STEPS, ops)
    after = _seq(bo, wins[STEPS:], ops, n, dt)
    assert _eq(after, _seq(bn, wins[STEPS:], ops, n, dt))
    # chunks
    bc = G.Batch(p, STREAMS, mask)
    first = _track(bc, d_pcm, pitch, hop, 4, ops, n, dt)
    rest = _track(bc, d_pcm, pitch, hop, 7, ops, n, dt, t0=4)
    assert _eq(torch.cat([first, rest]), new)
    assert _eq(_seq(bc, wins[STEPS:], ops, n, dt), after)
    # windows(3), process, windows(7)
    bm = G.Batch(p, STREAMS, mask)
    a = _track(bm, d_pcm, pitch, hop, 3, ops, n, dt)
    mid = _seq(bm, wins[3:4], ops, n, dt)
    c = _track(bm, d_pcm, pitch, hop, 7, ops, n, dt, t0=4)
    assert _eq(torch.cat([a, mid, c]), new)
    # the old entry's chunk, then a windows chunk
    bx = G.Batch(p, STREAMS, mask)
    a = _track(bx, d_pcm, pitch, hop, 5, ops, n, dt, old=True)
    c = _track(bx, d_pcm, pitch, hop, 6, ops, n, dt, t0=5)
    assert _eq(torch.cat([a, c]), new)
    assert _eq(_seq(bx, wins[STEPS:], ops, n, dt), after)
    for b in (bo, bn, bc, bm, bx): b.close()


# ---- 4. against the oracle, not only the library ------------------------------------------------------------------------------------------
def test_track_windows_float_chain_equals_the_oracle(glvlib, oracle):
    """log_mode 0, fft -> gravity -> average at hop 45: every step of one stream equals StreamOracle.frame on that window bit for bit"""
    import torch
    G = glvlib
    n, hop, F = 1024, 45, 5
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    pitch = _pitch(n, hop, STEPS)
    x = _pcm(5150, STREAMS, pitch)
    b = G.Batch(G.Params(n=n, avg_frames=F, log_mode=0), STREAMS, GA)
    got = _track(b, to_device(x, True, False), pitch, hop, STEPS, G.OP_FFT | GA, n, torch.float32).cpu().numpy()
    s = 1
    so = StreamOracle(n, avg_frames=F)
    for t in range(STEPS):
        want = so.frame(x[s, t * hop:t * hop + n, :])
        assert (got[t, 2 * s:2 * s + 2].view(np.uint32) == want.view(np.uint32)).all(), t
    b.close()


def test_track_windows_gl_chain_equals_the_oracle(glvlib, oracle):
    """log_mode 0, the GL_R16 chain at hop 45: every step's texels equal the oracle's transform_fft followed by glvo_gl_chain_r16 (the checker of
    tests/test_gl_storage.py), texel for texel, for every stream"""
    import torch
    G = glvlib
    n, hop, F = 1024, 45, 5
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    pitch = _pitch(n, hop, STEPS)
    x = _pcm(616, STREAMS, pitch) // 16
    b = G.Batch(G.Params(n=n, avg_frames=F, avg_window_kind=1, gl_storage=1, log_mode=0), STREAMS, GA)
    got = _track(b, to_device(x, False, False), pitch, hop, STEPS, G.OP_FFT | GA | G.OP_R16, n, torch.int16).cpu().numpy().view(np.uint16)
    store = np.zeros((STREAMS * 2, n), np.float32); hist = np.zeros((STREAMS * 2, F, n), np.float32)
    heads = [C.c_size_t(0) for _ in range(STREAMS * 2)]
    for t in range(STEPS):
        for s in range(STREAMS):
            spec = StreamOracle(n, gravity=False, average=False).frame(np.ascontiguousarray(x[s, t * hop:t * hop + n, :]))
            for c in range(2):
                want = np.ascontiguousarray(spec[c])
                Oracle.lib().glvo_gl_chain_r16(want, store[2 * s + c], hist[2 * s + c], C.byref(heads[2 * s + c]), n, F, 1, 1, 4.2, 86.1328125)
                assert (got[t, 2 * s + c] == Oracle.texels_r16(want)).all(), (t, s, c)
    b.close()


# ---- 5. launches and workspace ------------------------------------------------------------------------------------------------------------
def test_track_windows_launch_counts_and_workspace(glvlib):
    import torch
    G = glvlib
    n, hop, steps = 1024, 45, STEPS
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    pitch = _pitch(n, hop, steps)
    x = _pcm(12, STREAMS, pitch)
    d_pcm = to_device(x, False, False)
    R = steps * STREAMS * 2
    up = lambda v: (v + 255) & ~255                                               # noqa: E731
    cases = [   # params, mask, ops, launches, workspace, out width, dtype
        (dict(), G.OP_FFT, G.OP_FFT, 1, 256, n, torch.float32),
        (dict(), G.OP_FFT, G.OP_FFT | G.OP_R16, 1, 256, n, torch.int16),
        (dict(bars=80), G.OP_BARS, G.OP_FFT | G.OP_BARS, 2, up(R * n * 4), 80, torch.float32),
        (dict(), GA, G.OP_FFT | GA, 2, up(R * n * 4), n, torch.float32),
        (dict(gl_storage=1), GA, G.OP_FFT | GA | G.OP_R16, 2, up(R * n * 2), n, torch.int16),
        (dict(bars=80), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS, 3, 2 * up(R * n * 4), 80, torch.float32),
        (dict(gl_storage=1, bars=n, bar_phase=0.5), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16, 3, None, n, torch.int16),
    ]
    for kw, mask, ops, launches, nbytes, w, dt in cases:
        b = G.Batch(G.Params(n=n, **kw), STREAMS, mask)
        if nbytes is None:      # a GL chain's texel rows; the scan's results as texels where the integer pass takes them, as floats else (as glv_batch_track_s16)
            nbytes = up(R * n * 2) + up(R * n * (2 if b.bars_arithmetic() == G.BARS_I8_EXACT else 4))
        assert b.track_windows_work_bytes(pitch, hop, steps, ops) == nbytes, (kw, ops)
        out = _track(b, d_pcm, pitch, hop, steps, ops, w, dt)                     # (asserts that a one-launch call leaves workspace and guard untouched)
        assert b.last_launches() == launches, (kw, ops, b.last_launches())
        assert b.kernel_name() == ("glv_track_scan_kernel" if ops & GA else "glv_frame_kernel")
        if launches == 1:
            assert bool((out != 0).any())
        b.close()


# ---- 6. graph capture -------------------------------------------------------------------------------------------------------------------
def test_first_track_windows_call_can_be_captured_and_replayed(glvlib):
    """the FIRST call after creation, captured into a hipGraph (global mode: an allocation or a synchronous copy would invalidate the capture); one
    graph holds one full turn of the ring (the head advances on the host), so a replay continues like the same call issued again"""
    import torch
    G = glvlib
    hip = C.CDLL("libamdhip64.so")
    n, hop, F = 1024, 45, 5
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    ops = G.OP_FFT | GA | G.OP_R16
    p = G.Params(n=n, gl_storage=1, avg_window_kind=1, avg_frames=F)
    pitch = _pitch(n, hop, F)
    d_pcm = to_device(_pcm(9, STREAMS, pitch), True, False)
    bg, be = G.Batch(p, STREAMS, GA), G.Batch(p, STREAMS, GA)
    work = torch.zeros((bg.track_windows_work_bytes(pitch, hop, F, ops),), dtype=torch.uint8, device="cuda")
    og = torch.zeros((F, STREAMS * 2, n), dtype=torch.int16, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = C.c_void_p(st.cuda_stream)
    assert hip.hipStreamBeginCapture(sp, 0) == 0                    # hipStreamCaptureModeGlobal
    try:
        bg.track_windows_s16(d_pcm, pitch, hop, F, og, work, ops, stream=st.cuda_stream)
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
def test_track_windows_refusals_leave_the_batch_untouched(glvlib):
    import torch
    G = glvlib
    n, hop = 1024, 45
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    ops = G.OP_FFT | GA
    pitch = _pitch(n, hop, STEPS)
    x = _pcm(3, STREAMS, pitch)
    d_pcm = to_device(x, False, False)
    p = G.Params(n=n)
    b = G.Batch(p, STREAMS, GA | G.OP_BARS)
    work = torch.zeros((b.track_windows_work_bytes(pitch, hop, STEPS, ops | G.OP_BARS),), dtype=torch.uint8, device="cuda")
    out = torch.zeros((STEPS, STREAMS * 2, n), dtype=torch.float32, device="cuda")
    # a call that ran: what a refused one must leave alone
    b.track_windows_s16(d_pcm, pitch, hop, 2, out, work, ops)
    torch.cuda.synchronize()
    assert b.last_launches() == 2
    before = out.clone()

    def refused(batch, code, ops_=ops, pitch_=pitch, hop_=hop, steps_=STEPS, pcm=d_pcm, o=out, w=work, query=True):
        launches = batch.last_launches()
        with pytest.raises(G.GlvError) as ei:
            batch.track_windows_s16(pcm, pitch_, hop_, steps_, o, w, ops_)
        assert ei.value.code == code, (ei.value.code, str(ei.value))
        assert "glv error" in str(ei.value) and len(str(ei.value)) > 14           # a message in glv_last_error
        assert batch.last_launches() == launches                                   # nothing was launched, the count of the last call that ran stands
        if query and pcm is not None and o is not None and w is not None:          # the sizing query refuses the same arguments: 0, the code's name first
            assert G.lib().glv_batch_track_windows_work_bytes(batch._h, pitch_, hop_, steps_, ops_) == 0
            assert G.lib().glv_last_error().decode().startswith("GLV_ERR_STATE: " if code == G.ERR_STATE else "GLV_ERR_INVALID: ")
            with pytest.raises(G.GlvError) as ei:
                batch.track_windows_work_bytes(pitch_, hop_, steps_, ops_)
            assert ei.value.code == code

    for bad in (G.OP_RAW, G.OP_SMOOTH, G.OP_WRANGE, G.OP_MAGNITUDE):
        refused(b, G.ERR_INVALID, ops_=ops | bad)
    refused(b, G.ERR_INVALID, ops_=G.OP_WAVE)
    refused(b, G.ERR_INVALID, ops_=G.OP_FFT | G.OP_WAVE)
    refused(b, G.ERR_INVALID, ops_=G.OP_FFT | G.OP_GRAVITY | G.OP_OUTPUT_IS_STATE)
    refused(b, G.ERR_INVALID, ops_=GA)                                           # no GLV_OP_FFT
    refused(b, G.ERR_INVALID, steps_=0)
    refused(b, G.ERR_INVALID, hop_=0)
    refused(b, G.ERR_INVALID, pitch_=n + (STEPS - 1) * hop - 1)                  # one frame too short for the steps
    refused(b, G.ERR_INVALID, steps_=(2 ** 32 - 1) // (2 * STREAMS) + 1, hop_=1, pitch_=2 ** 32 - 1)     # more than 2^32 - 1 rows
    refused(b, G.ERR_INVALID, pcm=None)
    refused(b, G.ERR_INVALID, o=None)
    refused(b, G.ERR_INVALID, w=None)
    refused(b, G.ERR_INVALID, w=work.data_ptr() + 64, query=False)               # a workspace that is not 256-byte aligned
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
    mixed.process_s16(_windows(x, n, hop, 0, 1)[0], out[0].clone(), G.OP_FFT | G.OP_GRAVITY)
    refused(mixed, G.ERR_STATE, query=False)
    for x_ in (gl2, live, cols, unannounced, mixed): x_.close()
    torch.cuda.synchronize()
    assert _eq(out, before), "a refused call wrote to the output"
    # hop 45 is still refused by the residue entry, and accepted here
    with pytest.raises(G.GlvError) as ei:
        b.track_s16(d_pcm, 45 * 64, 45, STEPS, out, work, ops)
    assert ei.value.code == G.ERR_INVALID
    # after all the refused calls the batch continues from untouched state: steps [2, 11) here == sequential all the way on a fresh batch
    bs = G.Batch(p, STREAMS, GA | G.OP_BARS)
    want = _seq(bs, _windows(x, n, hop, 0, STEPS), ops, n, torch.float32)
    got = _track(b, d_pcm, pitch, hop, STEPS - 2, ops, n, torch.float32, t0=2)
    assert _eq(before[:2], want[:2]) and _eq(got, want[2:])
    b.close(); bs.close()
