"""GPU: track mode from float recordings (glv_batch_track_windows_f32, glv_batch_track_wave_f32).

Contract (the s16 entries', with the float process call as the sequential side): the output of step t -- and for FFT chains the batch's state
afterwards -- is bit for bit what `steps` consecutive glv_batch_process_f32_stereo calls on the windows [t * hop, t * hop + n) of every stream produce
and leave behind.  The sequential side is a second batch driven window by window, the windows cut on the host from the same recording; floats are
compared as int32.  Every call here gets a workspace of exactly the queried size followed by a guard region, which must come back intact; pitches are
odd and larger than the call consumes, so the streams of one recording alternate between the two alignments; the recording sits one frame (8 bytes)
behind a 16-byte boundary where a test says `odd`.  Windows then alternate between the two load forms (odd hop) or keep one (even hop)."""

import ctypes as C

import numpy as np
import pytest

from glava_amd.bar_positions import graph_column_texels, radial_bar_texels, wave_column_texels
from oracle_lib import Oracle, lcg_pcm_fast
from track_lib import base_chains, compare_hop, eq as _eq, fft_kernel, hop_windows as _windows, launches_fft as _launches, pitch_odd as _pitch, rec as _rec
from track_lib import seq, to_device, track

pytestmark = pytest.mark.gpu

STEPS, STREAMS = 11, 3          # F = 5: the ring wraps twice


def _track(b, *args, wave=False, **kw):
    """steps [t0, t0 + steps) of the float recording in one call (track_lib.track: exact workspace and output, guards behind both)"""
    return track(b, "wave" if wave else "windows", *args, f32=True, **kw)


def _compare(G, bt, bs, ops, n, hop, steps=STEPS, w=None, odd=False, seed=31, x=None):
    """one call against the sequential calls, every step, and the state through one more update on both; the batches start from equal state"""
    pitch = _pitch(n, hop, steps + 1)
    x = _rec(seed + n + hop, bt.streams, pitch) if x is None else x
    return compare_hop(G, bt, bs, "windows", x, odd, pitch, hop, n, steps, ops, n if w is None else w, _launches(G, ops), fft_kernel(G, ops), f32=True)


def _chains(G):
    """the shared chains, a mono transform, and gl_chain_F1 as floats with its texel form beside it (the s16 files' gl_chain_F1 is the texel form)"""
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    return {**base_chains(G),
            "fft_mono":        (dict(channels=1), G.OP_FFT, G.OP_FFT),
            "gl_chain_F1":     (dict(gl_storage=1, avg_frames=1), GA, G.OP_FFT | GA),
            "gl_chain_F1_r16": (dict(gl_storage=1, avg_frames=1), GA, G.OP_FFT | GA | G.OP_R16)}


CHAIN_NAMES = ["fft", "fft_r16", "fft_mono", "gravity", "chain", "chain_plain_sum", "chain_r16", "chain_mono", "average", "gl_gravity", "gl_chain",
               "gl_chain_r16", "gl_chain_F1", "gl_chain_F1_r16", "gl_chain_mono", "gl_fft"]
# (n, kernel configuration).  256 / 512: several slots share a wave, so the load form's branch can diverge (512 configuration 1 puts four windows in
# one wave); 1024 and 4096: the pipelined path (dword loads, the row index carried beside the samples); 16384: the generic loop with 32 points per lane,
# for every chain.  Mono takes the generic loop at every size.  The full chain list runs at one size of each kind; the others run the chains that differ
# in the transform launch: step-major rows straight into d_out (fft, fft_r16), stream-major rows for the scan (chain, gl_chain_r16), the mono mix.
FULL_SIZES = [(256, 0), (1024, 0), (16384, 0)]
SIZES = [(256, 0), (512, 0), (512, 1), (1024, 0), (1024, 1), (4096, 0), (4096, 1), (16384, 0), (16384, 1)]
REDUCED_CHAINS = ["fft", "fft_r16", "chain", "gl_chain_r16", "chain_mono"]
CHAIN_SIZES = [(c, n, v) for c in CHAIN_NAMES for n, v in SIZES if (n, v) in FULL_SIZES or c in REDUCED_CHAINS]


def _hops(n):
    return (1, 45, 735, n, n + 3)


# ---- 1. the contract against sequential calls, recording aligned and one frame off ------------------------------------------------------
@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("log_mode", [0, 1])
@pytest.mark.parametrize("chain,n,variant", CHAIN_SIZES)
def test_track_f32_equals_sequential_calls(glvlib, chain, n, variant, log_mode, odd):
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


@pytest.mark.parametrize("variant", [0, 1])
def test_track_f32_at_the_largest_size(glvlib, variant):
    """n = 32768, once, stateless: one 512-lane row per workgroup, the generic loop"""
    G = glvlib
    n = 32768
    bt, bs = G.Batch(G.Params(n=n), 2, G.OP_FFT), G.Batch(G.Params(n=n), 2, G.OP_FFT)
    bt.set_variant(variant)
    _compare(G, bt, bs, G.OP_FFT, n, 735, steps=5, odd=True)
    assert bt.last_variant() == variant
    bt.close(); bs.close()


# ---- 2. bars ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,table,gl_storage,r16", [(1024, False, 0, False), (1024, False, 1, True), (1024, False, 1, False), (1024, True, 1, True),
                                                    (1024, True, 1, False), (256, False, 1, True)])
def test_track_f32_bars(glvlib, n, table, gl_storage, r16):
    """hop 45: 80 bars of a float chain, the pre-smoothing pass of a GL chain (bars = n, bar_phase 0.5: 1024 bars, and at n = 256 exactly the 256 from
    which the many-bars kernels take over) and bars at a bar-texel table (a GL chain's), as texels and as floats; then the same from a recording one
    frame off, continuing from the state the first call left"""
    G = glvlib
    hop = 45
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


def test_track_f32_stateless_bars(glvlib):
    G = glvlib
    n, hop = 1024, 45
    p = G.Params(n=n, bars=80)
    bt, bs = G.Batch(p, STREAMS, G.OP_BARS), G.Batch(p, STREAMS, G.OP_BARS)
    _compare(G, bt, bs, G.OP_FFT | G.OP_BARS, n, hop, w=80, odd=True)
    assert bt.track_windows_work_bytes(_pitch(n, hop, STEPS), hop, STEPS, G.OP_FFT | G.OP_BARS) == STEPS * STREAMS * 2 * n * 4
    bt.close(); bs.close()


# ---- 3. forced grids: later trips of a workgroup and a ragged last one --------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["fft", "chain_mono", "gl_chain_r16"])
@pytest.mark.parametrize("n,variant", [(256, 0), (512, 1), (1024, 0), (4096, 0), (16384, 0)])
def test_track_f32_forced_grids(glvlib, n, variant, chain):
    """7 streams x 11 steps = 77 windows over 1, 2 and 3 workgroups: every slot makes several trips (the pipeline's look-ahead and its carried row
    index cross them), and the last trip is ragged"""
    G = glvlib
    kw, mask, ops = _chains(G)[chain]
    p = G.Params(n=n, **kw)
    bt, bs = G.Batch(p, 7, mask), G.Batch(p, 7, mask)
    bt.set_variant(variant)
    for grid in (1, 2, 3):
        bt.reset(); bs.reset()
        bt.set_grid(grid)
        _compare(G, bt, bs, ops, n, 45, odd=bool(grid & 1))
        bt.set_grid(0)
    bt.close(); bs.close()


# ---- 4. chunking and mixing ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["fft_r16", "gravity", "chain", "gl_chain_r16"])
def test_track_f32_chunks_compose_and_mix_with_process_calls(glvlib, chain):
    """track(4) then track(7) == track(11); a process call between chunks"""
    import torch
    G = glvlib
    n, hop = 1024, 45
    kw, mask, ops = _chains(G)[chain]
    p = G.Params(n=n, **kw)
    dt = torch.int16 if ops & G.OP_R16 else torch.float32
    pitch = _pitch(n, hop, STEPS + 1)
    x = _rec(77, STREAMS, pitch)
    d_pcm = to_device(x, True, True)
    wins = _windows(x, n, hop, 0, STEPS + 1)
    bw, bs = G.Batch(p, STREAMS, mask), G.Batch(p, STREAMS, mask)
    whole = _track(bw, d_pcm, pitch, hop, STEPS, ops, n, dt)
    assert _eq(whole, seq(bs, wins[:STEPS], ops, n, dt, f32=True))
    after = seq(bs, wins[STEPS:], ops, n, dt, f32=True)
    bc = G.Batch(p, STREAMS, mask)
    first = _track(bc, d_pcm, pitch, hop, 4, ops, n, dt)
    rest = _track(bc, d_pcm, pitch, hop, 7, ops, n, dt, t0=4)
    assert _eq(torch.cat([first, rest]), whole)
    assert _eq(seq(bc, wins[STEPS:], ops, n, dt, f32=True), after)
    bm = G.Batch(p, STREAMS, mask)
    a = _track(bm, d_pcm, pitch, hop, 3, ops, n, dt)
    mid = seq(bm, wins[3:4], ops, n, dt, f32=True)
    c = _track(bm, d_pcm, pitch, hop, 7, ops, n, dt, t0=4)
    assert _eq(torch.cat([a, mid, c]), whole)
    assert _eq(seq(bm, wins[STEPS:], ops, n, dt, f32=True), after)
    for b in (bw, bs, bc, bm): b.close()


@pytest.mark.parametrize("chain", ["chain", "gl_chain_r16"])
def test_track_f32_mixes_with_an_s16_track_call(glvlib, chain):
    """an s16 track call over 5 windows of an s16 recording, then a float track call over 6 windows of a float one, on ONE batch -- against the same
    sequence of process calls (glv_batch_process_s16 five times, glv_batch_process_f32_stereo six times) on another; then the state, through one more"""
    import torch
    G = glvlib
    n, hop = 1024, 45
    kw, mask, ops = _chains(G)[chain]
    p = G.Params(n=n, **kw)
    dt = torch.int16 if ops & G.OP_R16 else torch.float32
    pitch = _pitch(n, hop, 7)
    xi = lcg_pcm_fast(404, STREAMS * pitch * 2).reshape(STREAMS, pitch, 2).copy()
    xf = _rec(405, STREAMS, pitch)
    bt, bs = G.Batch(p, STREAMS, mask), G.Batch(p, STREAMS, mask)
    d_i = torch.from_numpy(xi).cuda()
    got = torch.cat([track(bt, "windows", d_i, pitch, hop, 5, ops, n, dt), _track(bt, to_device(xf, True, True), pitch, hop, 6, ops, n, dt)])
    want = torch.cat([seq(bs, _windows(xi, n, hop, 0, 5), ops, n, dt), seq(bs, _windows(xf, n, hop, 0, 6), ops, n, dt, f32=True)])
    assert _eq(got, want)
    last = _windows(xf, n, hop, 6, 7)
    assert _eq(seq(bt, last, ops, n, dt, f32=True), seq(bs, last, ops, n, dt, f32=True))
    bt.close(); bs.close()


# ---- 5. samples that are not ordinary numbers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["fft", "fft_r16", "fft_mono", "chain", "gl_chain_r16"])
@pytest.mark.parametrize("n", [256, 1024, 16384])
def test_track_f32_keeps_the_bits_of_special_samples(glvlib, n, chain):
    """-0, +-Inf, NaN and denormals planted in the recording, in both channels, at even and odd frames: bit for bit the one-by-one calls (the s16
    conversion a caller had to make before could not carry any of them)"""
    G = glvlib
    kw, mask, ops = _chains(G)[chain]
    hop = 45
    pitch = _pitch(n, hop, STEPS + 1)
    x = _rec(9000 + n, STREAMS, pitch).copy()
    specials = np.array([-0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 1.4e-45], np.float32)
    view = x.reshape(STREAMS, -1)
    for s in range(STREAMS):
        for k, v in enumerate(specials):
            if s == 1 and not np.isfinite(v):
                continue                                            # stream 1 keeps finite samples: -0 and denormals alone must survive too
            view[s, (97 * (k + 1) + 13 * s) % (2 * n)] = v           # inside window 0 ...
            view[s, 2 * (n + 3 * hop) + 2 * k + (k & 1)] = v         # ... and entering later windows one by one
    bt, bs = G.Batch(G.Params(n=n, **kw), STREAMS, mask), G.Batch(G.Params(n=n, **kw), STREAMS, mask)
    for odd in (False, True):
        bt.reset(); bs.reset()
        _compare(G, bt, bs, ops, n, hop, odd=odd, x=x)
    bt.close(); bs.close()


# ---- 6. against the oracle, not only the library ------------------------------------------------------------------------------------------
def test_track_f32_float_chain_equals_the_oracle(glvlib, oracle):
    """log_mode 0, fft -> gravity -> average at hop 45, stereo and mono: every step of one stream equals the oracle's pulse unpack (glvo_unpack_f32),
    transform_fft, gravity and average on that window, bit for bit"""
    import torch
    G = glvlib
    n, hop, F = 1024, 45, 5
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    pitch = _pitch(n, hop, STEPS)
    x = _rec(5150, STREAMS, pitch)
    s = 2
    for ch in (2, 1):
        b = G.Batch(G.Params(n=n, avg_frames=F, log_mode=0, channels=ch), STREAMS, GA)
        got = _track(b, to_device(x, True, True), pitch, hop, STEPS, G.OP_FFT | GA, n, torch.float32).cpu().numpy()
        grav = np.zeros((2, n), np.float32); hist = np.zeros((2, F, n), np.float32)
        heads = [C.c_size_t(0), C.c_size_t(0)]
        for t in range(STEPS):
            pl = np.empty(n, np.float32); pr = np.empty(n, np.float32)
            Oracle.lib().glvo_unpack_f32(np.ascontiguousarray(x[s, t * hop:t * hop + n, :]).reshape(-1), n, ch, pl, pr)
            for c, row in enumerate((pl, pr)):
                want = Oracle.transform_fft(row)
                Oracle.gravity(want, grav[c]); Oracle.average(want, hist[c], heads[c], F, True)
                assert (got[t, 2 * s + c].view(np.uint32) == want.view(np.uint32)).all(), (ch, t, c)
        b.close()


# ---- 7. launches and workspace ------------------------------------------------------------------------------------------------------------
def test_track_f32_launch_counts_and_workspace(glvlib):
    import torch
    G = glvlib
    n, hop, steps = 1024, 45, STEPS
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    pitch = _pitch(n, hop, steps)
    d_pcm = to_device(_rec(12, STREAMS, pitch), False, True)
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
        if nbytes is None:      # a GL chain's texel rows; the scan's results as texels where the integer pass takes them, as floats else
            nbytes = up(R * n * 2) + up(R * n * (2 if b.bars_arithmetic() == G.BARS_I8_EXACT else 4))
        assert b.track_windows_work_bytes(pitch, hop, steps, ops) == nbytes, (kw, ops)
        b.timing_begin()
        out = _track(b, d_pcm, pitch, hop, steps, ops, w, dt)                     # (asserts that a one-launch call leaves workspace and guard untouched)
        ms, calls = b.timing_end()                                                 # glv_batch_timing_* covers the call
        assert calls >= 1 and ms > 0.0, (ms, calls)
        assert b.last_launches() == launches, (kw, ops, b.last_launches())
        assert b.kernel_name() == ("glv_track_scan_kernel" if ops & GA else "glv_frame_kernel")
        if launches == 1:
            assert bool((out != 0).any())
        b.close()


# ---- 8. graph capture -------------------------------------------------------------------------------------------------------------------
def test_first_track_f32_call_can_be_captured_and_replayed(glvlib):
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
    d_pcm = to_device(_rec(9, STREAMS, pitch), True, True)
    bg, be = G.Batch(p, STREAMS, GA), G.Batch(p, STREAMS, GA)
    work = torch.zeros((bg.track_windows_work_bytes(pitch, hop, F, ops),), dtype=torch.uint8, device="cuda")
    og = torch.zeros((F, STREAMS * 2, n), dtype=torch.int16, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = C.c_void_p(st.cuda_stream)
    assert hip.hipStreamBeginCapture(sp, 0) == 0                    # hipStreamCaptureModeGlobal
    try:
        bg.track_windows_f32(d_pcm, pitch, hop, F, og, work, ops, stream=st.cuda_stream)
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


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------
def test_track_f32_refusals_leave_the_batch_untouched(glvlib):
    """every refusal of glv_batch_track_windows_s16, plus a d_pcm that is 4-byte aligned and no more"""
    import torch
    G = glvlib
    n, hop = 1024, 45
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    ops = G.OP_FFT | GA
    pitch = _pitch(n, hop, STEPS)
    x = _rec(3, STREAMS, pitch)
    d_pcm = to_device(x, False, True)
    p = G.Params(n=n)
    b = G.Batch(p, STREAMS, GA | G.OP_BARS)
    work = torch.zeros((b.track_windows_work_bytes(pitch, hop, STEPS, ops | G.OP_BARS),), dtype=torch.uint8, device="cuda")
    out = torch.zeros((STEPS, STREAMS * 2, n), dtype=torch.float32, device="cuda")
    # a call that ran: what a refused one must leave alone
    b.track_windows_f32(d_pcm, pitch, hop, 2, out, work, ops)
    torch.cuda.synchronize()
    assert b.last_launches() == 2
    before = out.clone()

    def refused(batch, code, ops_=ops, pitch_=pitch, hop_=hop, steps_=STEPS, pcm=d_pcm, o=out, w=work, query=True):
        launches = batch.last_launches()
        with pytest.raises(G.GlvError) as ei:
            batch.track_windows_f32(pcm, pitch_, hop_, steps_, o, w, ops_)
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
    refused(b, G.ERR_INVALID, pcm=d_pcm.data_ptr() + 4, query=False)             # a d_pcm aligned like a float, not like a float frame
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
    mixed.process_f32_stereo(_windows(x, n, hop, 0, 1)[0], out[0].clone(), G.OP_FFT | G.OP_GRAVITY)
    refused(mixed, G.ERR_STATE, query=False)
    for x_ in (gl2, live, cols, unannounced, mixed): x_.close()
    torch.cuda.synchronize()
    assert _eq(out, before), "a refused call wrote to the output"
    # after all the refused calls the batch continues from untouched state: steps [2, 11) here == sequential all the way on a fresh batch
    bs = G.Batch(p, STREAMS, GA | G.OP_BARS)
    want = seq(bs, _windows(x, n, hop, 0, STEPS), ops, n, torch.float32, f32=True)
    got = _track(b, d_pcm, pitch, hop, STEPS - 2, ops, n, torch.float32, t0=2)
    assert _eq(before[:2], want[:2]) and _eq(got, want[2:])
    b.close(); bs.close()


# ---- 10. the wave form --------------------------------------------------------------------------------------------------------------------
def _wave_ops(G):
    return {"wave": G.OP_WAVE, "wave_r16": G.OP_WAVE | G.OP_R16, "pass": G.OP_WAVE | G.OP_BARS, "pass_r16": G.OP_WAVE | G.OP_BARS | G.OP_R16}


def _compare_wave(G, p, ops, n, hop, odd, w=None, prepare=None, steps=STEPS, seed=131):
    """one track call against the sequential calls, every step; 1 launch without bars, 2 with -- whatever hop, pitch and alignment"""
    pitch = _pitch(n, hop, steps) if hop != 256 else n + (steps - 1) * hop + 40          # hop 256: pitch and hop multiples of 8, what the s16 form fuses
    x = _rec(seed + n + hop, STREAMS, pitch)
    mask = G.OP_WAVE | G.OP_BARS
    bt, bs = G.Batch(p, STREAMS, mask), G.Batch(p, STREAMS, mask)
    if prepare:
        prepare(bt); prepare(bs)
    got = compare_hop(G, bt, bs, "wave", x, odd, pitch, hop, n, steps, ops, n if w is None else w, 2 if ops & G.OP_BARS else 1,
                      "glv_wave_kernel", f32=True, state=False)                            # (the name: the first launch, as the process call reports)
    assert bs.last_launches() == bt.last_launches()
    assert int(got.ne(0).sum()) > 0
    bt.close(); bs.close()


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("hop", [1, 256, 735])
@pytest.mark.parametrize("n", [256, 1024, 4096])
@pytest.mark.parametrize("form", ["wave", "wave_r16", "pass", "pass_r16"])
def test_track_wave_f32_equals_sequential_calls(glvlib, form, n, hop, channels, odd):
    """all four output forms, stereo and mono; the pre-smoothing pass at bars = n, bar_phase 0.5 (the integer pass, which never fuses from floats: always
    two launches, at hop 256 from an aligned recording too)"""
    G = glvlib
    p = G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5, channels=channels)
    _compare_wave(G, p, _wave_ops(G)[form], n, hop, odd)


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("r16", [True, False])
def test_track_wave_f32_bar_texel_table(glvlib, r16, odd):
    G = glvlib
    n = 1024
    tex, _ = wave_column_texels(n, 320)
    p = G.Params(n=n, gl_storage=1, bars=len(tex))
    _compare_wave(G, p, G.OP_WAVE | G.OP_BARS | (G.OP_R16 if r16 else 0), n, 735, odd, w=len(tex), prepare=lambda b: b.set_bar_texels(tex))


def test_track_wave_f32_special_samples_and_chunks(glvlib):
    """-0, +-Inf, NaN and denormals through the wave bind, bit for bit the one-by-one calls; track(4) then track(7) == track(11)"""
    import torch
    G = glvlib
    n, hop = 1024, 45
    pitch = _pitch(n, hop, STEPS)
    x = _rec(4242, STREAMS, pitch).copy()
    view = x.reshape(STREAMS, -1)
    for k, v in enumerate(np.array([-0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40], np.float32)):
        view[:, 31 * (k + 1) + (k & 1)] = v
        view[:, 2 * (n + 2 * hop) + 2 * k + (k & 1)] = v
    p = G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5)
    for ops in (G.OP_WAVE, G.OP_WAVE | G.OP_BARS | G.OP_R16):
        dt = torch.int16 if ops & G.OP_R16 else torch.float32
        bt, bs = G.Batch(p, STREAMS, G.OP_WAVE | G.OP_BARS), G.Batch(p, STREAMS, G.OP_WAVE | G.OP_BARS)
        d_pcm = to_device(x, True, True)
        whole = _track(bt, d_pcm, pitch, hop, STEPS, ops, n, dt, wave=True)
        assert _eq(whole, seq(bs, _windows(x, n, hop, 0, STEPS), ops, n, dt, f32=True))
        first = _track(bt, d_pcm, pitch, hop, 4, ops, n, dt, wave=True)
        rest = _track(bt, d_pcm, pitch, hop, 7, ops, n, dt, t0=4, wave=True)
        assert _eq(torch.cat([first, rest]), whole)
        bt.close(); bs.close()


def test_track_wave_f32_refusals_launch_nothing(glvlib):
    """every refusal of glv_batch_track_wave_s16, plus a d_pcm that is 4-byte aligned and no more"""
    import torch
    G = glvlib
    n, hop = 1024, 256
    ops = G.OP_WAVE | G.OP_BARS | G.OP_R16
    pitch = _pitch(n, hop, STEPS)
    x = _rec(3, STREAMS, pitch)
    d_pcm = to_device(x, False, True)
    p = G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5)
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    b = G.Batch(p, STREAMS, G.OP_WAVE | G.OP_BARS | GA)
    work = torch.zeros((b.track_wave_work_bytes(pitch, 100, STEPS, ops) + 256,), dtype=torch.uint8, device="cuda")
    out = torch.full((STEPS, STREAMS * 2, n), 0x5A5A, dtype=torch.int16, device="cuda")
    b.process_f32_stereo(_windows(x, n, hop, 0, 1)[0], torch.zeros((STREAMS * 2, n), dtype=torch.int16, device="cuda"), G.OP_WAVE | G.OP_R16)
    ran = b.last_launches()

    def refused(batch, code, ops_=ops, pitch_=pitch, hop_=hop, steps_=STEPS, pcm=d_pcm, o=out, w=work, query=True):
        with pytest.raises(G.GlvError) as ei:
            batch.track_wave_f32(pcm, pitch_, hop_, steps_, o, w, ops_)
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
    refused(b, G.ERR_INVALID, pcm=d_pcm.data_ptr() + 4, query=False)             # a d_pcm aligned like a float, not like a float frame
    refused(b, G.ERR_INVALID, steps_=1 << 31, hop_=1, pitch_=0xffffffff)         # 2^31 steps x 6 rows > 2^32 rows
    assert b.last_launches() == ran                                              # the count of the last call that ran stands
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
            b.track_windows_f32(d_pcm, pitch, hop, STEPS, out, w2, bad_ops)
        assert ei.value.code == G.ERR_INVALID
    # nothing was launched: the output still holds its fill
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A).all())
    # after all the refused calls the batch still produces the sequential results
    bs = G.Batch(p, STREAMS, G.OP_WAVE | G.OP_BARS)
    got = _track(b, d_pcm, pitch, hop, STEPS, ops, n, torch.int16, wave=True)
    assert _eq(got, seq(bs, _windows(x, n, hop, 0, STEPS), ops, n, torch.int16, f32=True))
    b.close(); bs.close()
