"""GPU: track calls on a batch with bufscale k (glv_batch_set_bufscale), on track_lib's contract with windows of k * n frames: step t of the call and the state
afterwards are bit for bit those of `steps` sequential glv_batch_process_s16 / _f32_stereo calls on the k * n-frame windows of a second batch with the same k
(which tests/test_bufscale.py holds to the planar entry on np_bufscale's rows).  Every call gets a workspace of exactly the queried size and track_lib's guards.
Launches: the form's own plus the decimation stage.  The frames entry, whose output no process call writes, is held to the same entry on a k = 1 batch over a
float recording made of the decimated windows laid back to back."""
import numpy as np
import pytest

from bufscale_lib import np_bufscale
from glava_amd.bar_positions import graph_column_texels
from gpu_lib import eq
from track_lib import GUARD, bars_batch, compare, compare_hop, fft_kernel, launches_fft, out_dtype, pitch_odd, rec, seq, to_device, track, windows

pytestmark = pytest.mark.gpu
F = 3
STEPS = 2 * F + 4
SHAPES = [(2, 256, 1), (3, 256, 3), (2, 1024, 3), (3, 1024, 1)]
SHAPE_IDS = ["k%d-n%d-s%d" % s for s in SHAPES]


def _chains(G, n):
    """name -> (parameters, creation mask, ops, width of an output row)"""
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    return {
        "fft":          (dict(), G.OP_FFT, G.OP_FFT, n),                                                     # step-major rows straight into d_out: the workspace holds the decimated rows alone
        "fft_r16":      (dict(), G.OP_FFT, G.OP_FFT | G.OP_R16, n),
        "chain":        (dict(avg_frames=F), GA, G.OP_FFT | GA, n),                                          # stream-major rows for the scan
        "chain_mono":   (dict(avg_frames=F, channels=1), GA, G.OP_FFT | GA, n),
        "gl_chain_r16": (dict(avg_frames=F, gl_storage=1, avg_window_kind=1), GA, G.OP_FFT | GA | G.OP_R16, n),
        "bars":         (dict(avg_frames=F, bars=80), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS, 80),        # three regions behind the decimated rows' one
        "fft_bars":     (dict(bars=80), G.OP_FFT | G.OP_BARS, G.OP_FFT | G.OP_BARS, 80),
    }


CHAIN_NAMES = ["fft", "fft_r16", "chain", "chain_mono", "gl_chain_r16", "bars", "fft_bars"]


def _pair(G, n, streams, name, k):
    kw, mask, ops, w = _chains(G, n)[name]
    p = G.Params(n=n, **kw)
    bt, bs = G.Batch(p, streams, mask), G.Batch(p, streams, mask)
    bt.set_bufscale(k); bs.set_bufscale(k)
    return bt, bs, ops, w


def _starts_dev(starts):
    import torch
    return torch.from_numpy(np.asarray(starts, dtype=np.uint32).view(np.int32).copy()).cuda()


def _decimated_bytes(steps, streams, n):
    return (steps * streams * 2 * n * 4 + 255) & ~255


# ---- the windows entry -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("k,n,streams", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("name", CHAIN_NAMES)
def test_windows_entry_at_hop_1_an_odd_hop_and_a_whole_window(glvlib, name, k, n, streams, f32):
    G = glvlib
    for hop, odd in ((1, True), (77, False), (k * n, True)):
        bt, bs, ops, w = _pair(G, n, streams, name, k)
        pitch = pitch_odd(k * n, hop, STEPS + 1)
        x = rec(1200 + hop + n, streams, pitch, f32)
        compare_hop(G, bt, bs, "windows", x, odd, pitch, hop, k * n, STEPS, ops, w, launches_fft(G, ops) + 1, fft_kernel(G, ops) if not ops & G.OP_BARS else None,
                    f32=f32, what=(name, k))
        # the queries answer for the batch as it is: the form's own regions behind the decimated rows'
        bt.set_bufscale(1)
        plain = bt.track_windows_work_bytes(pitch, hop, STEPS, ops)
        bt.set_bufscale(k)
        extra = _decimated_bytes(STEPS, streams, n)
        assert bt.track_windows_work_bytes(pitch, hop, STEPS, ops) == (extra if plain == 256 else plain + extra), (name, hop)
        with pytest.raises(G.GlvError):                                            # the pitch rule counts k * n frames
            bt.track_windows_work_bytes(k * n + (STEPS - 1) * hop - 1, hop, STEPS, ops)
        bt.close(); bs.close()


# ---- the table entry ---------------------------------------------------------------------------------------------------------------------------------------
def _table(k, n, pitch):
    """repeats, a backward jump, odd starts, entries beyond pitch - k n that clamp (the largest uint32 among them), the last window itself"""
    last = pitch - k * n
    t = [0, 0, 33, 33, 801 % (last + 1), 5, last, last + 1, last + 7 * n, 0xffffffff]
    assert len(t) == STEPS
    return t


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("k,n,streams", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("name", ["fft", "chain", "gl_chain_r16", "bars"])
def test_table_entry_reads_every_window_inside_the_recording(glvlib, name, k, n, streams, f32):
    G = glvlib
    for pitch in ((k * n + 1500) | 1, k * n):                                      # ... and a recording of exactly one window: every entry clamps to 0
        bt, bs, ops, w = _pair(G, n, streams, name, k)
        starts = _table(k, n, pitch)
        x = rec(1300 + n + pitch, streams, pitch, f32)
        at = [min(s, pitch - k * n) for s in starts + [7]]
        d_pcm = to_device(x, True, f32, tail_frames=k * n)                         # one frame behind a load boundary; other frames behind the last stream
        compare(G, bt, bs, "at", x, d_pcm, pitch, _starts_dev(starts), at, k * n, STEPS, ops, w, launches_fft(G, ops) + 1, None, f32=f32, what=(name, k, pitch))
        assert bt.track_at_work_bytes(STEPS, ops) == bt.track_windows_work_bytes(k * n + STEPS, 1, STEPS, ops)      # (neither depends on the pitch)
        table = _starts_dev(starts)
        with pytest.raises(G.GlvError) as e:                                       # a recording one frame short of a window of k * n frames
            (bt.track_at_f32 if f32 else bt.track_at_s16)(d_pcm, k * n - 1, table, STEPS, d_pcm, d_pcm, ops)
        assert e.value.code == G.ERR_INVALID
        bt.close(); bs.close()


# ---- one case each: rates, columns, live, frames -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
def test_rates_entry(glvlib, f32):
    """gravity at a per-step rate: the sequential side sets ur before every update (set_params keeps k)"""
    import torch
    G = glvlib
    k, n, streams = 3, 256, 3
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    ops = G.OP_FFT | GA
    p = G.Params(n=n, avg_frames=F)
    bt, bs = G.Batch(p, streams, GA), G.Batch(p, streams, GA)
    bt.set_bufscale(k); bs.set_bufscale(k)
    pitch = (k * n + 900) | 1
    starts = [(97 * t) % (pitch - k * n) for t in range(STEPS)]
    ur = [60.0, 59.0, 1.0, 86.1328125, 30.0, 144.0, 23.040000915527344, 60.0, 75.0, 100.0]
    x = rec(1400, streams, pitch, f32)
    d_pcm = to_device(x, True, f32, tail_frames=k * n)
    nbytes = bt.track_at_work_bytes(STEPS, ops)
    work = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.zeros((STEPS, streams * 2, n), dtype=torch.float32, device="cuda")
    d_starts, d_ur = _starts_dev(starts), torch.tensor(ur, dtype=torch.float32, device="cuda")
    (bt.track_rates_f32 if f32 else bt.track_rates_s16)(d_pcm, pitch, d_starts, d_ur, STEPS, out, work, ops)
    torch.cuda.synchronize()
    assert bool((work[nbytes:] == 0xA5).all()) and bt.last_launches() == 3
    wins = windows(x, k * n, starts)
    for t in range(STEPS):
        bs.set_params(G.Params(n=n, avg_frames=F, ur=ur[t]))
        assert bs.bufscale == k
        assert eq(out[t], seq(bs, wins[t:t + 1], ops, n, torch.float32, f32)[0]), t
    bs.set_params(p)
    assert eq(seq(bt, wins[:1], ops, n, torch.float32, f32), seq(bs, wins[:1], ops, n, torch.float32, f32)), "state"
    bt.close(); bs.close()


@pytest.mark.parametrize("live", [False, True], ids=["columns", "live"])
def test_columns_and_live_entries(glvlib, live):
    G = glvlib
    k, n, streams, hop = 2, 256, 3, 77
    cols = graph_column_texels(n, 64)[0]
    kw = dict(gl_storage=1, avg_window_kind=1, bars=len(cols))
    bt, bs = bars_batch(G, n, kw, ("col", cols), F, streams, live=live), bars_batch(G, n, kw, ("col", cols), F, streams, live=live)
    bt.set_bufscale(k); bs.set_bufscale(k)
    ops = G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS
    pitch = pitch_odd(k * n, hop, STEPS + 1)
    for f32 in (False, True):
        x = rec(1500 + f32, streams, pitch, f32)
        compare_hop(G, bt, bs, "live" if live else "columns", x, True, pitch, hop, k * n, STEPS, ops, len(cols), 4, None, f32=f32, what=(live,))
    bt.close(); bs.close()


def _frames_call(G, b, f32, d_pcm, pitch, starts, steps, tables, d_keys, keep, ops, w, streams):
    import torch
    frames = len(tables[0])
    nbytes = b.track_frames_work_bytes(steps, frames, ops)
    work = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    count = frames * streams * 2 * w
    flat = torch.zeros((count + GUARD,), dtype=out_dtype(G, ops), device="cuda")
    flat[count:] = 77
    d_from, d_to = _starts_dev(tables[0]), _starts_dev(tables[1])
    d_mod = torch.tensor(tables[2], dtype=torch.float32, device="cuda")
    d_starts = _starts_dev(starts)
    (b.track_frames_f32 if f32 else b.track_frames_s16)(d_pcm, pitch, d_starts, None, steps, d_from, d_to, d_mod, frames, d_keys, keep, flat, work, ops)
    torch.cuda.synchronize()
    assert bool((work[nbytes:] == 0xA5).all()), "the call wrote behind the workspace it asked for"
    assert bool((flat[count:] == 77).all()), "the call wrote behind its output"
    return flat[:count].view(frames, streams * 2, w)


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
def test_frames_entry_on_gl_storage_3_keeps_keyframes_of_n(glvlib, f32):
    """three calls of a session, one per kind of kept pair -- (0, 1), (1, k) and (k, k') -- on A (bufscale k, the recording) and on B (k = 1, a float recording
    made of np_bufscale's rows of A's windows laid back to back, channels 2: the rows as they are): frames, d_keys and state bit for bit"""
    import torch
    G = glvlib
    k, n, streams, steps = 2, 256, 3, 6
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    ops = G.OP_FFT | GA | G.OP_BARS | G.OP_R16
    p = G.Params(n=n, avg_frames=F, gl_storage=G.GL_STORAGE_UPLOAD, bars=n, bar_phase=0.5)
    a, b = G.Batch(p, streams, GA | G.OP_BARS), G.Batch(p, streams, GA | G.OP_BARS)
    a.set_bufscale(k)
    pitch = (k * n + 700) | 1
    keys_a = torch.from_numpy((np.random.default_rng(3).random((2, streams * 2, n), dtype=np.float32) * np.float32(1.3) - np.float32(0.1)).astype(np.float32)).cuda()
    keys_b = keys_a.clone()
    frm = [0, 0, 1, 2, 3, 3, 7, 5, 6, 7, 2]
    to = [1, 1, 2, 3, 3, 4, 2, 6, 7, 7, 9]                                         # (9 clamps to steps + 1 = 7)
    mod = [0.0, 0.59310347, 1.0, 0.25, 0.5, 1.0, 0.3, 0.75, 0.1, 0.6, 0.4]
    for call, keep in enumerate(((0, 1), (1, 4), (3, 7))):
        starts = [(131 * (t + call)) % (pitch - k * n + 40) for t in range(steps)]      # (some clamp)
        x = rec(1600 + call, streams, pitch, f32)
        d_pcm = to_device(x, True, f32, tail_frames=k * n)
        at = [min(s, pitch - k * n) for s in starts]
        rows = np.stack([np_bufscale(x[:, s:s + k * n, :], k, f32, 2) for s in at])          # [steps][streams][2][n]
        y = np.ascontiguousarray(rows.transpose(1, 0, 3, 2).reshape(streams, steps * n, 2))  # [streams][steps * n][2]
        got = _frames_call(G, a, f32, d_pcm, pitch, starts, steps, (frm, to, mod), keys_a, keep, ops, n, streams)
        assert a.last_launches() == 2 + 1 + 1 + 1 + 1
        want = _frames_call(G, b, True, to_device(y, False, True), steps * n, [t * n for t in range(steps)], steps, (frm, to, mod), keys_b, keep, ops, n, streams)
        assert eq(got, want), (call, keep)
        assert eq(keys_a, keys_b), (call, keep)
    with pytest.raises(G.GlvError):
        a.track_frames_work_bytes(steps, len(frm), G.OP_WAVE | G.OP_R16)
    a.close(); b.close()


# ---- past the grid cap ---------------------------------------------------------------------------------------------------------------------------------------
def test_more_work_items_than_the_decimation_grid_takes_at_once(glvlib):
    """7 streams x 1200 steps at n = 256: 8400 windows x 64 lanes, more than the 2048 workgroups x 256 lanes of the stage's grid -- its loop takes the rest"""
    G = glvlib
    k, n, streams, steps, hop = 2, 256, 7, 1200, 1
    assert streams * steps * (n // 4) > 2048 * 256
    bt, bs, ops, w = _pair(G, n, streams, "fft", k)
    pitch = pitch_odd(k * n, hop, steps)
    x = rec(1700, streams, pitch, False)
    compare_hop(G, bt, bs, "windows", x, True, pitch, hop, k * n, steps, ops, w, 2, "glv_frame_kernel", state=False)
    bt.close(); bs.close()


# ---- what refuses --------------------------------------------------------------------------------------------------------------------------------------------
def test_residue_wave_and_wave_frames_entries_refuse(glvlib):
    import torch
    G = glvlib
    k, n, streams = 2, 256, 2
    b = G.Batch(G.Params(n=n), streams, G.OP_FFT | G.OP_WAVE)
    b.set_bufscale(k)
    pitch = 8 * k * n
    d_pcm = torch.from_numpy(rec(1800, streams, pitch, False).copy()).cuda()
    d_f32 = torch.from_numpy(rec(1800, streams, pitch, True).copy()).cuda()
    out = torch.zeros((4, streams * 2, n), dtype=torch.float32, device="cuda")
    work = torch.zeros((1 << 22,), dtype=torch.uint8, device="cuda")
    tab = _starts_dev([0, 1, 2, 3])
    mod = torch.zeros((4,), dtype=torch.float32, device="cuda")
    keys = torch.zeros((2, streams * 2, n), dtype=torch.float32, device="cuda")
    W = G.OP_WAVE | G.OP_R16
    calls = [lambda: b.track_s16(d_pcm, pitch, 64, 4, out, work, G.OP_FFT),
             lambda: b.track_work_bytes(pitch, 64, 4, G.OP_FFT),
             lambda: b.track_wave_s16(d_pcm, pitch, 64, 4, out, work, W),
             lambda: b.track_wave_f32(d_f32, pitch, 64, 4, out, work, W),
             lambda: b.track_wave_work_bytes(pitch, 64, 4, W),
             lambda: b.track_at_s16(d_pcm, pitch, tab, 4, out, work, W),
             lambda: b.track_at_work_bytes(4, W),
             lambda: b.track_wave_frames_s16(d_pcm, pitch, tab, 4, tab, tab, mod, 4, keys, (0, 1), out, work, W),
             lambda: b.track_wave_frames_f32(d_f32, pitch, tab, 4, tab, tab, mod, 4, keys, (0, 1), out, work, W),
             lambda: b.track_wave_frames_work_bytes(4, 4, W)]
    for i, call in enumerate(calls):
        with pytest.raises(G.GlvError) as e:
            call()
        assert e.value.code == G.ERR_STATE and "glv_batch_set_bufscale" in str(e.value), (i, str(e.value))
    # the FFT entries still run on this batch
    got = track(b, "windows", d_pcm, pitch, 64, 4, G.OP_FFT, n, torch.float32)
    assert b.last_launches() == 2 and got.shape == (4, streams * 2, n)
    b.close()
