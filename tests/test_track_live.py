"""GPU: track mode for GLV_OP_BARS_ONLY batches (glv_batch_track_live_s16 / _f32) -- the live bins only, in one call.

Contract: step t of the output is bit for bit what the t-th of `steps` consecutive glv_batch_process_s16 (_f32: glv_batch_process_f32_stereo) calls on
window t writes on the same flagged batch, and head, gravity form and the state below glv_batch_live_bins are what those calls leave.  The sequential side
is a second flagged batch driven window by window; the output is also compared with an unflagged twin through glv_batch_track_windows_* / _columns_*, which
older tests pin to the oracle.  Every assertion is bit equality (floats as int32).  Every call gets a workspace of exactly
glv_batch_track_live_work_bytes bytes followed by a guard region; hops are odd (45 n / 256), pitches odd and longer than the call consumes.

The five chains are those of tests/test_frame_count.py _live_cases, restated: the GL chain with bars = n (the pre-smoothing pass; at the smallest size with
live bins and at 4096), the float chain with 80 bars, the GL chain with 64 bars, a radial bar-texel table, a graph column table."""
import ctypes as C

import numpy as np
import pytest

from glava_amd.bar_positions import graph_column_texels, radial_bar_texels
from track_lib import bars_batch, eq as _eq, hop_windows, out_dtype as _dt, pcm, pitch_odd, rec, seq as _seq, to_device, track, work_regions

pytestmark = pytest.mark.gpu

FR = 5
STEPS, STREAMS = FR + 9, 3          # past kTrackDepth + F: the ring wraps and the look-ahead refills


def _hop(n):
    return 45 * n // 256


def _cases(G):
    """name -> (candidates (n, parameters, table) in ascending size, ops): the first candidate with live bins runs"""
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    gl = dict(avg_window_kind=1, gl_storage=1)
    chain = G.OP_FFT | GA | G.OP_BARS
    radial = lambda n: ("bar", radial_bar_texels(n, 160)[0])            # noqa: E731
    cols = lambda n: ("col", graph_column_texels(n, 320)[0])            # noqa: E731
    twin = lambda n: (n, dict(bars=n, bar_phase=0.5, smooth_factor=0.025, **gl), None)   # noqa: E731
    return {
        "gl_smallest": ([twin(n) for n in (256, 512, 1024, 2048, 4096)], chain | G.OP_R16),
        "gl_shipped": ([twin(4096)], chain | G.OP_R16),
        "float_80": ([(1024, dict(bars=80), None)], chain),
        "gl_64": ([(2048, dict(bars=64, **gl), None)], chain | G.OP_R16),
        "radial": ([(1024, dict(bars=len(radial(1024)[1]), **gl), radial(1024))], chain | G.OP_R16),
        "columns": ([(4096, dict(bars=len(cols(4096)[1]), **gl), cols(4096))], chain),
    }


def _mask(G):
    return G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS


def _make(G, n, kw, table, F=FR, streams=STREAMS, live=True, variant=None):
    return bars_batch(G, n, kw, table, F, streams, live, variant)


def _choose(G, case, F=FR):
    candidates, ops = _cases(G)[case]
    for n, kw, table in candidates:
        probe = _make(G, n, kw, table, F=F, streams=1)
        L = probe.live_bins(); probe.close()
        if L != 0:
            return n, kw, table, ops
    raise AssertionError(f"no candidate size of {case} has live bins")


def _track(b, *args, entry="live", **kw):
    """steps [t0, t0 + steps) of the recording in one call (track_lib.track: exact workspace and output, guards behind both)"""
    return track(b, entry, *args, **kw)


def _recording(n, hop, steps, seed, f32, streams=STREAMS, odd=True):
    """(host recording, device recording, pitch): int16 or finite float32 samples, -0 among the floats"""
    pitch = pitch_odd(n, hop, steps) + 2                                 # odd, with odd slack
    if f32:
        x = np.array(rec(seed, streams, pitch), copy=True)
        x.reshape(streams, -1)[:, 7::97] = np.float32(-0.0)
    else:
        x = pcm(seed, streams, pitch)
    return x, to_device(x, odd, f32), pitch


# ---- 1. equality with the sequential live calls, and with the unflagged track call -------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("case", ["gl_smallest", "gl_shipped", "float_80", "gl_64", "radial", "columns"])
def test_live_track_equals_sequential_live_calls_and_the_unflagged_track(glvlib, case, f32):
    """one call; chunks F + 1 then 8 and one more process call on both batches (head and ring); process -> track -> process.  Every kernel configuration."""
    import torch
    G = glvlib
    n, kw, table, ops = _choose(G, case)
    hop, w, dt = _hop(n), kw["bars"], _dt(G, ops)
    x, d_pcm, pitch = _recording(n, hop, STEPS + 1, 900 + n, f32)
    wins = hop_windows(x, n, hop, 0, STEPS + 1)
    probe = _make(G, n, kw, table, streams=1)
    nv = probe.variants(); probe.close()
    twin_entry = "columns" if table and table[0] == "col" else "windows"
    for v in range(nv):
        bt, bs, bc, bm = (_make(G, n, kw, table, variant=v) for _ in range(4))
        full = _make(G, n, kw, table, live=False, variant=v)
        assert bt.live_bins() != 0 and bt.live_bins() < n and full.live_bins() == 0
        want = _seq(bs, wins[:STEPS], ops, w, dt, f32)
        got = _track(bt, d_pcm, pitch, hop, STEPS, ops, w, dt, f32=f32)
        assert bt.last_launches() == 3 and bt.last_variant() == v, (bt.last_launches(), bt.last_variant())
        assert bt.kernel_name().startswith("glv_bars_") or bt.kernel_name() == "glv_columns_kernel", bt.kernel_name()
        for t in range(STEPS):
            assert _eq(got[t], want[t]), (case, v, t, int((got[t] != want[t]).sum()))
        assert bool((got != 0).any())
        assert _eq(got, _track(full, d_pcm, pitch, hop, STEPS, ops, w, dt, f32=f32, entry=twin_entry)), (case, v, "unflagged twin")
        after = _seq(bs, wins[STEPS:], ops, w, dt, f32)
        assert _eq(_seq(bt, wins[STEPS:], ops, w, dt, f32), after), (case, v, "state")
        # chunks F + 1 then 8, one more process call
        a = _track(bc, d_pcm, pitch, hop, FR + 1, ops, w, dt, f32=f32)
        b = _track(bc, d_pcm, pitch, hop, 8, ops, w, dt, t0=FR + 1, f32=f32)
        assert _eq(torch.cat([a, b]), want), (case, v, "chunks")
        assert _eq(_seq(bc, wins[STEPS:], ops, w, dt, f32), after), (case, v, "state after chunks")
        # process -> track -> process
        first = _seq(bm, wins[:1], ops, w, dt, f32)
        mid = _track(bm, d_pcm, pitch, hop, STEPS - 1, ops, w, dt, t0=1, f32=f32)
        assert _eq(torch.cat([first, mid]), want), (case, v, "process, track")
        assert _eq(_seq(bm, wins[STEPS:], ops, w, dt, f32), after), (case, v, "process, track, process")
        assert bt.live_bins() != 0
        for b_ in (bt, bs, bc, bm, full): b_.close()


# ---- 2. the scan walks the kept bins and no others, nothing unwritten is read ----------------------------------------------------------------------------
def _kept_of(region, zeroed, rows, n, elem):
    """per row of a workspace region poisoned with 0xFF: the smallest multiple of 64 bins from which on the row still holds 0xFF.  `zeroed`: the same region
    of the same call on a workspace of 0x00 bytes -- a byte is one the call wrote where the two agree (a texel of 65535 is 0xFF bytes by value)"""
    import torch
    r, z = region[:rows * n * elem].view(rows, n, elem), zeroed[:rows * n * elem].view(rows, n, elem)
    assert bool(((r == z) | ((r == 0xFF) & (z == 0x00))).all()), "a byte that is neither the call's nor the fill's"
    written = (r == z).all(dim=2)                                        # [rows][n]
    last = torch.where(written.any(dim=1), n - 1 - written.flip(1).int().argmax(dim=1), torch.full((rows,), -1, device=r.device, dtype=torch.long))
    return ((last + 1 + 63) // 64 * 64).cpu().numpy()


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("case", ["gl_smallest", "gl_shipped", "float_80"])
def test_the_scan_writes_the_kept_bins_only_and_nothing_unwritten_is_read(glvlib, case, f32):
    """the workspace poisoned with 0xFF bytes (NaN as a float, 65535 as a texel): the outputs still equal the sequential calls'; the transform's region is
    written whole (live classes for the transform were measured and taken out: profiles/r15/track_live_rule.txt), the scan's region keeps the poison from
    one multiple of 64 bins K on in every row, L <= K < n"""
    G = glvlib
    n, kw, table, ops = _choose(G, case)
    hop, w, dt = _hop(n), kw["bars"], _dt(G, ops)
    x, d_pcm, pitch = _recording(n, hop, STEPS, 1200 + n, f32)
    wins = hop_windows(x, n, hop, 0, STEPS)
    bt, bs = _make(G, n, kw, table), _make(G, n, kw, table)
    L = bt.live_bins()
    want = _seq(bs, wins, ops, w, dt, f32)
    got, work = _track(bt, d_pcm, pitch, hop, STEPS, ops, w, dt, f32=f32, fill=0xFF, keep_work=True)
    assert _eq(got, want), (case, int((got != want).sum()))
    bz = _make(G, n, kw, table)
    got0, work0 = _track(bz, d_pcm, pitch, hop, STEPS, ops, w, dt, f32=f32, fill=0x00, keep_work=True)
    assert _eq(got0, want)
    bz.close()
    rows = STEPS * STREAMS * 2
    elem = 2 if kw.get("gl_storage") == 1 else 4                        # texel rows all the way (the integer pass) / float rows
    (rows_ff, scan_ff), (rows_00, scan_00) = work_regions(work, rows, n, elem, elem), work_regions(work0, rows, n, elem, elem)
    assert (_kept_of(rows_ff[0], rows_00[0], rows, n, elem) == n).all()
    kept = _kept_of(scan_ff[0], scan_00[0], rows, n, elem)
    K = int(kept.max())
    assert (kept == K).all(), (case, sorted(set(kept.tolist())))
    assert K % 64 == 0 and L <= K < n, (case, L, K, n)
    if elem == 2: assert K == L, (L, K)                                  # texel rows: no kernel reads beyond the taps
    bt.close(); bs.close()


# ---- 3. frame counts -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 6, 64])
@pytest.mark.parametrize("case", ["gl_smallest", "float_80"])
def test_live_track_at_frame_counts(glvlib, case, F):
    """F = 64: a 32 KiB LDS ring, and with kept bins that are an odd multiple of 64 a partly idle wave; steps = F + 9"""
    G = glvlib
    n, kw, table, ops = _choose(G, case, F=F)
    hop, w, dt, steps = _hop(n), kw["bars"], _dt(G, ops), F + 9
    x, d_pcm, pitch = _recording(n, hop, steps + 1, 1500 + n + F, False)
    wins = hop_windows(x, n, hop, 0, steps + 1)
    bt, bs = _make(G, n, kw, table, F=F), _make(G, n, kw, table, F=F)
    assert bt.live_bins() != 0
    got = _track(bt, d_pcm, pitch, hop, steps, ops, w, dt)
    want = _seq(bs, wins[:steps], ops, w, dt, False)
    for t in range(steps):
        assert _eq(got[t], want[t]), (case, F, t, int((got[t] != want[t]).sum()))
    assert bt.last_launches() == 3 and bool((got != 0).any())
    assert _eq(_seq(bt, wins[steps:], ops, w, dt, False), _seq(bs, wins[steps:], ops, w, dt, False)), (case, F, "state")
    bt.close(); bs.close()


# ---- 5. the full-row fall-back -----------------------------------------------------------------------------------------------------------------------------
def _far_sampling(G, n):
    """parameters of the GL chain with bars = n whose bars sample too far for a live class: sample_scale lowered until glv_batch_live_bins is 0"""
    for scale in (6.0, 5.0, 4.0, 3.0, 2.5):
        kw = dict(bars=n, bar_phase=0.5, smooth_factor=0.025, avg_window_kind=1, gl_storage=1, sample_scale=scale)
        probe = _make(G, n, kw, None, streams=1)
        L = probe.live_bins(); probe.close()
        if L == 0:
            return kw
    raise AssertionError("no sample_scale takes the live bins away")


@pytest.mark.parametrize("form", ["log_mode_2", "far"])
def test_flagged_batches_without_live_bins_take_the_full_row_form(glvlib, form):
    """accepted, equal to the sequential calls, and the 0xFF pattern is gone from whole rows of both regions"""
    G = glvlib
    n = 1024
    if form == "log_mode_2":
        kw, ops, e1, e2 = dict(bars=80, log_mode=2), G.OP_FFT | _mask(G), 4, 4
    else:
        kw, ops, e1, e2 = _far_sampling(G, n), G.OP_FFT | _mask(G) | G.OP_R16, 2, 2
    hop, w, dt = _hop(n), kw["bars"], _dt(G, ops)
    x, d_pcm, pitch = _recording(n, hop, STEPS + 1, 2100, False)
    wins = hop_windows(x, n, hop, 0, STEPS + 1)
    bt, bs, bz = _make(G, n, kw, None), _make(G, n, kw, None), _make(G, n, kw, None)
    assert bt.live_bins() == 0
    got, work = _track(bt, d_pcm, pitch, hop, STEPS, ops, w, dt, fill=0xFF, keep_work=True)
    assert bt.last_launches() == 3
    got0, work0 = _track(bz, d_pcm, pitch, hop, STEPS, ops, w, dt, fill=0x00, keep_work=True)
    assert _eq(got0, got)
    want = _seq(bs, wins[:STEPS], ops, w, dt, False)
    assert _eq(got, want) and bool((got != 0).any())
    rows = STEPS * STREAMS * 2
    for (reg, e), (zer, _) in zip(work_regions(work, rows, n, e1, e2), work_regions(work0, rows, n, e1, e2)):
        assert (_kept_of(reg, zer, rows, n, e) == n).all(), form
    assert _eq(_seq(bt, wins[STEPS:], ops, w, dt, False), _seq(bs, wins[STEPS:], ops, w, dt, False))
    bt.close(); bs.close(); bz.close()


# ---- 6. refusals and sizing ------------------------------------------------------------------------------------------------------------------------------
def test_live_track_refusals_and_sizing(glvlib):
    import torch
    G = glvlib
    n, kw, table, ops = _choose(G, "gl_smallest")
    hop, w, dt = _hop(n), kw["bars"], _dt(G, ops)
    x, d_pcm, pitch = _recording(n, hop, STEPS, 2400, False, odd=False)
    _, d_f32, _ = _recording(n, hop, STEPS, 2400, True, odd=False)
    b = _make(G, n, kw, table)
    work = torch.zeros((b.track_live_work_bytes(pitch, hop, STEPS, ops),), dtype=torch.uint8, device="cuda")
    out = torch.zeros((STEPS, STREAMS * 2, w), dtype=dt, device="cuda")

    def refused(batch, code, ops_=ops, pitch_=pitch, hop_=hop, steps_=STEPS, pcm=d_pcm, o=out, w_=work, query=True, f32=False, says=None):
        launches = batch.last_launches()
        with pytest.raises(G.GlvError) as ei:
            (batch.track_live_f32 if f32 else batch.track_live_s16)(pcm, pitch_, hop_, steps_, o, w_, ops_)
        assert ei.value.code == code, (ei.value.code, str(ei.value))
        if says: assert says in str(ei.value), str(ei.value)
        assert batch.last_launches() == launches                                   # nothing was launched
        if query:                                                                  # the sizing query refuses the same arguments: 0, the code's name first
            assert G.lib().glv_batch_track_live_work_bytes(batch._h, pitch_, hop_, steps_, ops_) == 0
            assert G.lib().glv_last_error().decode().startswith("GLV_ERR_STATE: " if code == G.ERR_STATE else "GLV_ERR_INVALID: ")
            with pytest.raises(G.GlvError) as ei:
                batch.track_live_work_bytes(pitch_, hop_, steps_, ops_)
            assert ei.value.code == code

    for bad in (G.OP_RAW, G.OP_SMOOTH, G.OP_WRANGE, G.OP_MAGNITUDE, G.OP_WAVE, G.OP_OUTPUT_IS_STATE):
        refused(b, G.ERR_INVALID, ops_=ops | bad)
    refused(b, G.ERR_INVALID, ops_=ops & ~G.OP_FFT)
    refused(b, G.ERR_INVALID, ops_=ops & ~G.OP_BARS)
    refused(b, G.ERR_INVALID, ops_=ops & ~(G.OP_GRAVITY | G.OP_AVERAGE))          # no state operator
    refused(b, G.ERR_INVALID, steps_=0)
    refused(b, G.ERR_INVALID, hop_=0)
    refused(b, G.ERR_INVALID, pitch_=n + (STEPS - 1) * hop - 1)
    refused(b, G.ERR_INVALID, steps_=(2 ** 32 - 1) // (2 * STREAMS) + 1, hop_=1, pitch_=2 ** 32 - 1)
    refused(b, G.ERR_INVALID, pcm=None, query=False)
    refused(b, G.ERR_INVALID, o=None, query=False)
    refused(b, G.ERR_INVALID, w_=None, query=False)
    refused(b, G.ERR_INVALID, w_=work.data_ptr() + 64, query=False)
    refused(b, G.ERR_INVALID, pcm=d_f32.data_ptr() + 4, query=False, f32=True)
    others = []
    plain = _make(G, n, kw, table, live=False)
    refused(plain, G.ERR_STATE, says="glv_batch_track_windows_")                  # a batch without the flag
    assert "_columns_" in G.lib().glv_last_error().decode()
    others.append(plain)
    gl2 = G.Batch(G.Params(n=n, avg_frames=FR, **dict(kw, gl_storage=2)), STREAMS, _mask(G) | G.OP_BARS_ONLY)
    refused(gl2, G.ERR_STATE)
    others.append(gl2)
    unannounced = G.Batch(G.Params(n=n, avg_frames=FR, **kw), STREAMS, G.OP_GRAVITY | G.OP_BARS | G.OP_BARS_ONLY)
    refused(unannounced, G.ERR_STATE)                                            # what the process call refuses: GLV_OP_AVERAGE without its ring
    others.append(unannounced)
    # the old entries still refuse the flagged batch
    for entry in ("track_windows", "track_columns"):
        with pytest.raises(G.GlvError) as ei:
            getattr(b, entry + "_s16")(d_pcm, pitch, hop, STEPS, out, work, ops)
        assert ei.value.code == G.ERR_STATE
    with pytest.raises(G.GlvError) as ei:
        b.track_s16(d_pcm, 64 * ((pitch + 63) // 64), 64, 1, out, work, ops)
    assert ei.value.code == G.ERR_STATE
    # the query's value: the windows query of an unflagged twin (and the columns query of a twin with columns)
    for steps in (STEPS, 1):
        assert b.track_live_work_bytes(pitch, hop, steps, ops) == plain.track_windows_work_bytes(pitch, hop, steps, ops)
    n4, kw4, table4, ops4 = _choose(G, "columns")
    lc, fc = _make(G, n4, kw4, table4, streams=1), _make(G, n4, kw4, table4, streams=1, live=False)
    p4 = n4 + 3 * _hop(n4)
    assert lc.track_live_work_bytes(p4, _hop(n4), 3, ops4) == fc.track_columns_work_bytes(p4, _hop(n4), 3, ops4)
    lc.close(); fc.close()
    # the refused calls left the batch untouched: the next accepted call gives what a fresh twin gives
    assert b.last_launches() == 0
    fresh = _make(G, n, kw, table)
    assert _eq(_track(b, d_pcm, pitch, hop, STEPS, ops, w, dt), _track(fresh, d_pcm, pitch, hop, STEPS, ops, w, dt))
    for o_ in others + [b, fresh]: o_.close()


# ---- 7. capture --------------------------------------------------------------------------------------------------------------------------------------------
def test_first_live_track_call_can_be_captured_and_replayed(glvlib):
    """the FIRST call after creation, captured into a hipGraph as one linear stream (three kernel nodes, a chain); replayed twice onto reset state: the
    output of the same call issued directly, both times"""
    import torch
    G = glvlib
    hip = C.CDLL("libamdhip64.so")
    n, kw, table, ops = _choose(G, "gl_smallest")
    hop, w, dt = _hop(n), kw["bars"], _dt(G, ops)
    x, d_pcm, pitch = _recording(n, hop, STEPS, 2700, False)
    bg, be = _make(G, n, kw, table), _make(G, n, kw, table)
    work = torch.zeros((bg.track_live_work_bytes(pitch, hop, STEPS, ops),), dtype=torch.uint8, device="cuda")
    og = torch.zeros((STEPS, STREAMS * 2, w), dtype=dt, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = C.c_void_p(st.cuda_stream)
    assert hip.hipStreamBeginCapture(sp, 0) == 0                    # hipStreamCaptureModeGlobal
    try:
        bg.track_live_s16(d_pcm, pitch, hop, STEPS, og, work, ops, stream=st.cuda_stream)
    finally:
        graph = C.c_void_p()
        rc = hip.hipStreamEndCapture(sp, C.byref(graph))
    assert rc == 0
    count = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(count)) == 0 and count.value == 3
    edges = C.c_size_t(0)
    assert hip.hipGraphGetEdges(graph, None, None, C.byref(edges)) == 0 and edges.value == 2
    roots = C.c_size_t(0)
    assert hip.hipGraphGetRootNodes(graph, None, C.byref(roots)) == 0 and roots.value == 1                      # 3 nodes, 2 edges, 1 root: a chain
    exe = C.c_void_p()
    assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
    want = _track(be, d_pcm, pitch, hop, STEPS, ops, w, dt)
    for rep in range(2):
        bg.reset()
        torch.cuda.synchronize()
        og.zero_()
        torch.cuda.synchronize()
        assert hip.hipGraphLaunch(exe, sp) == 0
        st.synchronize()
        assert _eq(og, want), rep
    hip.hipGraphExecDestroy(exe); hip.hipGraphDestroy(graph)
    bg.close(); be.close()
