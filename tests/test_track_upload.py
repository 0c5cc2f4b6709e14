"""GPU: the track entries on gl_storage 3 batches (the CPU operators on float state, GLV_OP_BARS over the GL_R16 upload of the finished rows).

Contract: each entry's own, word for word -- step t of the output, and the batch's state afterwards, are bit for bit what `steps` consecutive process calls
on the windows produce and leave behind on the same kind of batch (tests/track_lib.py: exact workspace and output with guards, every step, the state through
one more update).  What those process calls compute is pinned in tests/test_upload_chain.py.  Stages: the stateless transform with float rows, the scan's
float-state form writing the upload's texels, then the texel-row bars / snap / columns / mode kernel -- three launches; a stateless chain writes texel rows
in the transform and takes two."""
import numpy as np
import pytest

from glava_amd.bar_positions import graph_column_texels, radial_bar_texels
from glava_amd.track_starts import renderer_starts
from track_lib import GUARD, bars_batch, compare, compare_hop, differing, eq, out_dtype, pitch_odd, pitch_residue, rec, seq, to_device, track, windows, work_regions

pytestmark = pytest.mark.gpu

N, STREAMS, F, STEPS, HOP = 1024, 3, 5, 11, 735          # 11 steps: more than the scan's look-ahead, the ring wraps twice


def _tables(n):
    """name -> (parameters, table, width of an output row)"""
    radial = radial_bar_texels(n, 160)[0]
    cols = graph_column_texels(n, 120)[0]
    return {"pass": (dict(bars=n, bar_phase=0.5), None, n), "bar": (dict(bars=len(radial)), ("bar", radial), len(radial)),
            "col": (dict(bars=len(cols)), ("col", cols), len(cols)),
            "maximum": (dict(bars=80, sample_mode=1), None, 80), "hybrid_bar": (dict(bars=len(radial), sample_mode=2), ("bar", radial), len(radial))}


def _pair(G, n, name, live=False, **more):
    kw, table, w = _tables(n)[name]
    kw = dict(kw, gl_storage=G.GL_STORAGE_UPLOAD, **more)
    return bars_batch(G, n, kw, table, F, STREAMS, live=live), bars_batch(G, n, kw, table, F, STREAMS, live=live), w


def _ops(G, r16):
    return G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS | (G.OP_R16 if r16 else 0)


def _starts_dev(starts):
    import torch
    return torch.from_numpy(np.asarray(starts, dtype=np.uint32).view(np.int32).copy()).cuda()


FORMS = [("pass", True), ("pass", False), ("bar", True), ("bar", False), ("col", False), ("maximum", True), ("hybrid_bar", False)]
FORM_IDS = ["%s-%s" % (t, "texels" if r else "floats") for t, r in FORMS]


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("table,r16", FORMS, ids=FORM_IDS)
def test_hop_735_from_an_odd_pitch(glvlib, table, r16, f32):
    G = glvlib
    bt, bs, w = _pair(G, N, table)
    pitch = pitch_odd(N, HOP, STEPS + 1)
    x = rec(71, STREAMS, pitch, f32)
    entry = "columns" if table == "col" else "windows"
    compare_hop(G, bt, bs, entry, x, True, pitch, HOP, N, STEPS, _ops(G, r16), w, 3, "glv_columns_kernel" if table == "col" else "glv_track_scan_kernel", f32=f32,
                what=(table, r16))
    bt.close(); bs.close()


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("table,r16", [("pass", True), ("bar", False), ("col", False)], ids=["pass", "bar", "col"])
def test_renderer_starts_table(glvlib, table, r16, f32):
    """glv_batch_track_at_*: the windows of a 60 fps renderer over a 22050 Hz recording"""
    G = glvlib
    bt, bs, w = _pair(G, N, table)
    starts = renderer_starts(22050, 60, 1, STEPS + 1)
    pitch = (max(starts) + N + 38) | 1
    x = rec(72, STREAMS, pitch, f32)
    at = [G.track_at_start(pitch, N, s) for s in starts]
    compare(G, bt, bs, "at", x, to_device(x, True, f32, tail_frames=N), pitch, _starts_dev(starts[:STEPS]), at, N, STEPS, _ops(G, r16), w, 3, None, f32=f32,
            what=(table, r16))
    bt.close(); bs.close()


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("table,r16", [("pass", True), ("bar", False), ("col", False)], ids=["pass", "bar", "col"])
def test_rates_table(glvlib, table, r16, f32):
    """glv_batch_track_rates_*: a live session's rates -- 1.0 while nothing is measured, then 59.0, then 60.0 -- against set_params(ur) before every call"""
    import torch
    G = glvlib
    kw, tab, w = _tables(N)[table]
    pkw = dict(kw, n=N, avg_frames=F, gl_storage=G.GL_STORAGE_UPLOAD)
    bt, bs, _ = _pair(G, N, table)
    urs = [1.0] * 4 + [59.0] * 4 + [60.0] * 3
    assert len(urs) == STEPS
    starts = renderer_starts(22050, 60, 1, STEPS + 1)
    pitch = (max(starts) + N + 38) | 1
    x = rec(73, STREAMS, pitch, f32)
    d_pcm = to_device(x, True, f32, tail_frames=N)
    ops, dt = _ops(G, r16), out_dtype(G, _ops(G, r16))
    nbytes = bt.track_at_work_bytes(STEPS, ops)
    work = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    count = STEPS * STREAMS * 2 * w
    flat = torch.zeros((count + GUARD,), dtype=dt, device="cuda")
    d_ur = torch.from_numpy(np.asarray(urs + [np.nan] * 8, dtype=np.float32)).cuda()
    (bt.track_rates_f32 if f32 else bt.track_rates_s16)(d_pcm, pitch, _starts_dev(starts[:STEPS]), d_ur, STEPS, flat, work, ops)
    torch.cuda.synchronize()
    assert bool((work[nbytes:] == 0xA5).all()) and bool((flat[count:] == 0).all())
    assert bt.last_launches() == 3
    got = flat[:count].view(STEPS, STREAMS * 2, w)
    wins = windows(x, N, [G.track_at_start(pitch, N, s) for s in starts])
    for t in range(STEPS):
        bs.set_params(G.Params(**pkw, ur=urs[t]))
        want = seq(bs, wins[t:t + 1], ops, w, dt, f32)[0]
        assert eq(got[t], want), (table, t, differing(got[t], want))
    bs.set_params(G.Params(**pkw))
    assert eq(seq(bt, wins[STEPS:], ops, w, dt, f32), seq(bs, wins[STEPS:], ops, w, dt, f32)), "state, or the batch's own ur"
    bt.close(); bs.close()


@pytest.mark.parametrize("table,r16", [("pass", True), ("bar", False), ("col", False)], ids=["pass", "bar", "col"])
def test_eleven_steps_cut_as_4_and_7(glvlib, table, r16):
    G = glvlib
    bt, bs, w = _pair(G, N, table)
    pitch = pitch_odd(N, HOP, STEPS + 1)
    x = rec(74, STREAMS, pitch, False)
    d_pcm = to_device(x, True, False)
    entry = "columns" if table == "col" else "windows"
    ops, dt = _ops(G, r16), out_dtype(G, _ops(G, r16))
    whole = track(bs, entry, d_pcm, pitch, HOP, STEPS, ops, w, dt)
    first = track(bt, entry, d_pcm, pitch, HOP, 4, ops, w, dt)
    rest = track(bt, entry, d_pcm, pitch, HOP, 7, ops, w, dt, t0=4)
    assert eq(first, whole[:4]) and eq(rest, whole[4:]), table
    more = windows(x, N, [STEPS * HOP])
    assert eq(seq(bt, more, ops, w, dt), seq(bs, more, ops, w, dt)), "state"
    bt.close(); bs.close()


@pytest.mark.parametrize("table,r16", [("pass", True), ("bar", True), ("col", False)], ids=["pass", "bar", "col"])
def test_live_entry_takes_the_full_row_form(glvlib, table, r16):
    """a GLV_OP_BARS_ONLY batch has no live bins on this storage: glv_batch_track_live_* runs every bin, in the windows / columns layout"""
    G = glvlib
    bt, bs, w = _pair(G, N, table, live=True)
    assert bt.live_bins() == 0
    pitch = pitch_odd(N, HOP, STEPS + 1)
    x = rec(75, STREAMS, pitch, False)
    compare_hop(G, bt, bs, "live", x, True, pitch, HOP, N, STEPS, _ops(G, r16), w, 3, None, what=(table,))
    bt.close(); bs.close()


def test_workspace_regions_follow_the_element_sizes(glvlib):
    """float rows in the first region, texel rows in the second; a stateless chain with bars: texel rows, one region, two launches"""
    G = glvlib
    bt, bs, w = _pair(G, N, "bar")
    pitch = pitch_odd(N, HOP, STEPS + 1)
    x = rec(76, STREAMS, pitch, False)
    d_pcm = to_device(x, True, False)
    ops = _ops(G, True)
    rows = STEPS * STREAMS * 2
    _, work = track(bt, "windows", d_pcm, pitch, HOP, STEPS, ops, w, out_dtype(G, ops), keep_work=True)
    work_regions(work, rows, N, 4, 2)
    assert bt.track_windows_work_bytes(pitch, HOP, STEPS, ops) == bt.track_at_work_bytes(STEPS, ops)
    bt.close(); bs.close()
    # stateless: FFT | BARS
    bt, bs, w = _pair(G, N, "bar")
    sl = G.OP_FFT | G.OP_BARS | G.OP_R16
    up = lambda v: (v + 255) & ~255                                   # noqa: E731
    assert bt.track_windows_work_bytes(pitch, HOP, STEPS, sl) == up(rows * N * 2)
    compare_hop(G, bt, bs, "windows", x, True, pitch, HOP, N, STEPS, sl, w, 2, "glv_frame_kernel", state=False)
    bt.close(); bs.close()


@pytest.mark.parametrize("table,r16", [("pass", True), ("bar", False)], ids=["pass", "bar"])
def test_residue_entry(glvlib, table, r16):
    """glv_batch_track_s16 (hop a power of two) follows from the same plan: n / hop transform launches, the scan, the bars"""
    G = glvlib
    hop = 256
    bt, bs, w = _pair(G, N, table)
    pitch = pitch_residue(N, hop, STEPS + 1)
    x = rec(77, STREAMS, pitch, False)
    compare_hop(G, bt, bs, "residue", x, False, pitch, hop, N, STEPS, _ops(G, r16), w, N // hop + 2, "glv_track_scan_kernel", what=(table,))
    bt.close(); bs.close()


def test_wave_entry_as_on_gl_storage_1(glvlib):
    G = glvlib
    n, steps, hop = 1024, 6, 367
    ops = G.OP_WAVE | G.OP_BARS | G.OP_R16
    pitch = pitch_odd(n, hop, steps)
    x = rec(78, STREAMS, pitch, False)
    d_pcm = to_device(x, True, False)
    out = []
    for storage in (G.GL_STORAGE_UPLOAD, 1):
        b = G.Batch(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=storage), STREAMS, G.OP_WAVE | G.OP_BARS)
        out.append(track(b, "wave", d_pcm, pitch, hop, steps, ops, n, out_dtype(G, ops)))
        out.append((b.last_launches(), b.kernel_name()))
        b.close()
    assert eq(out[0], out[2]) and out[1] == out[3]


def test_larger_size_and_other_configuration(glvlib):
    """N = 4096 on both kernel configurations of the transform, 37 streams: ragged against the scan's and the bars kernels' row groups"""
    G = glvlib
    n, streams, steps, hop = 4096, 37, 4, 735
    radial = radial_bar_texels(n, 160)[0]
    kw = dict(bars=len(radial), gl_storage=G.GL_STORAGE_UPLOAD)
    pitch = pitch_odd(n, hop, steps + 1)
    x = rec(79, streams, pitch, False)
    for variant in (0, 1):
        bt = bars_batch(G, n, kw, ("bar", radial), F, streams, live=False, variant=variant)
        bs = bars_batch(G, n, kw, ("bar", radial), F, streams, live=False)
        compare_hop(G, bt, bs, "windows", x, True, pitch, hop, n, steps, _ops(G, True), len(radial), 3, "glv_track_scan_kernel", what=(variant,))
        assert bt.last_variant() == variant
        bt.close(); bs.close()


def test_a_track_call_under_graph_capture(glvlib):
    """kernels only: the first track call of a batch can be captured and replayed"""
    import torch
    G = glvlib
    bt, bs, w = _pair(G, N, "bar")
    ops = _ops(G, True)
    pitch = pitch_odd(N, HOP, STEPS + 1)
    x = rec(80, STREAMS, pitch, False)
    d_pcm = to_device(x, True, False)
    work = torch.zeros((bt.track_windows_work_bytes(pitch, HOP, STEPS, ops),), dtype=torch.uint8, device="cuda")
    out = torch.zeros((STEPS, STREAMS * 2, w), dtype=torch.int16, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        bt.track_windows_s16(d_pcm, pitch, HOP, STEPS, out, work, ops, stream=s.cuda_stream)
    assert bt.last_launches() == 3
    g.replay()
    torch.cuda.synchronize()
    want = seq(bs, windows(x, N, [t * HOP for t in range(STEPS)]), ops, w, torch.int16)
    assert eq(out, want), differing(out, want)
    del g
    bt.close(); bs.close()
