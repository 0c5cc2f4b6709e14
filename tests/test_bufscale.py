"""GPU: `setbufscale k` on the process calls (glv_batch_set_bufscale).

The second path: a batch A with bufscale k is fed windows of k * n frames -- interleaved s16, interleaved f32, planar f32 -- and a batch B with k = 1 and the
same parameters is fed bufscale_lib.np_bufscale of the same windows through glv_batch_process_f32 (tests/test_bufscale_host.py holds that restatement to the
oracle bit for bit).  Output and state must be equal bit for bit; the state is compared through the outputs of F + 3 updates and one more planar update on each
batch at the end, which reads gravity store, ring and head.  Besides: the oracle's chain directly, float specials, toggling k, launch accounting and graph
capture, guards around every buffer, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from bufscale_lib import F32, np_bufscale, np_bufscale_planar, oracle_bufscale
from glava_amd.bar_positions import radial_bar_texels
from gpu_lib import eq
from oracle_lib import Oracle
from track_lib import pcm, rec, to_device, with_table

pytestmark = pytest.mark.gpu
F = 3
UPDATES = F + 3
KINDS = ("s16", "f32", "planar")


class _Hip:
    """stream capture through the HIP runtime's C interface (global mode: an allocation or a synchronous copy inside would invalidate the capture)"""

    def __init__(self):
        self.L = C.CDLL("libamdhip64.so")

    def capture(self, stream_ptr, fn):
        assert self.L.hipStreamBeginCapture(C.c_void_p(stream_ptr), 0) == 0
        try:
            fn()
        finally:
            graph = C.c_void_p()
            rc = self.L.hipStreamEndCapture(C.c_void_p(stream_ptr), C.byref(graph))
        assert rc == 0, rc
        exe = C.c_void_p()
        assert self.L.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
        return graph, exe

    def launch(self, exe, stream_ptr):
        assert self.L.hipGraphLaunch(exe, C.c_void_p(stream_ptr)) == 0

    def destroy(self, graph, exe):
        self.L.hipGraphExecDestroy(exe); self.L.hipGraphDestroy(graph)


def _chains(G, n):
    """name -> (parameters, creation mask, ops, width of an output row, texel table)"""
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    radial = radial_bar_texels(n, 160)[0]
    return {
        "fft":        (dict(), G.OP_FFT, G.OP_FFT, n, None),
        "chain":      (dict(avg_frames=F), GA, G.OP_FFT | GA, n, None),
        "gl_chain":   (dict(avg_frames=F, gl_storage=1, avg_window_kind=1), GA, G.OP_FFT | GA | G.OP_R16, n, None),
        "shipped":    (dict(avg_frames=F, gl_storage=1, avg_window_kind=1, bars=n, bar_phase=0.5), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16, n, None),
        "upload_bar": (dict(avg_frames=F, gl_storage=3, bars=len(radial)), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16, len(radial), ("bar", radial)),
        "wave":       (dict(), G.OP_WAVE, G.OP_WAVE | G.OP_R16, n, None),
        "wave_bars":  (dict(gl_storage=1, bars=n, bar_phase=0.5), G.OP_WAVE | G.OP_BARS, G.OP_WAVE | G.OP_BARS | G.OP_R16, n, None),
    }


CHAIN_NAMES = ["fft", "chain", "gl_chain", "shipped", "upload_bar", "wave", "wave_bars"]


def _batch(G, n, streams, name, channels=2, k=1):
    kw, mask, ops, w, table = _chains(G, n)[name]
    b = with_table(G.Batch(G.Params(n=n, channels=channels, **kw), streams, mask), table)
    if k != 1: b.set_bufscale(k)
    return b, ops, w


def _window(kind, streams, frames, seed):
    """one update's input on the host: int16 / float32 [streams][frames][2], or planar float32 [streams][2][frames]"""
    if kind == "s16": return pcm(seed, streams, frames)
    x = np.array(rec(seed, streams, frames, True), copy=True)
    return x if kind == "f32" else np.ascontiguousarray(x.transpose(0, 2, 1))


def _decimated(kind, x, k, channels):
    """what batch B is fed: float32 [streams * 2][n]"""
    rows = np_bufscale_planar(x, k) if kind == "planar" else np_bufscale(x, k, kind == "f32", channels)
    return np.ascontiguousarray(rows.reshape(-1, rows.shape[-1]))


def _call(b, kind, d_in, d_out, ops, stream=None):
    {"s16": b.process_s16, "f32": b.process_f32_stereo, "planar": b.process_f32}[kind](d_in, d_out, ops, stream=stream)


def _dtype(G, ops):
    import torch
    return torch.int16 if ops & G.OP_R16 else torch.float32


def _run_pair(G, name, n, streams, k, channels, kind, updates=UPDATES, seed=700):
    """A (bufscale k, the windows) against B (k = 1, np_bufscale of the windows, planar), every update and one more planar update on both"""
    import torch
    a, ops, w = _batch(G, n, streams, name, channels, k)
    b, _, _ = _batch(G, n, streams, name, channels)
    assert a.bufscale == k and b.bufscale == 1
    dt = _dtype(G, ops)
    for u in range(updates):
        x = _window(kind, streams, k * n, seed + u)
        oa = torch.zeros((streams * 2, w), dtype=dt, device="cuda")
        ob = torch.zeros((streams * 2, w), dtype=dt, device="cuda")
        _call(a, kind, torch.from_numpy(x).cuda(), oa, ops)
        b.process_f32(torch.from_numpy(_decimated(kind, x, k, channels)).cuda(), ob, ops)
        assert a.last_launches() == b.last_launches() + 1, (name, kind, u, a.last_launches(), b.last_launches())
        assert eq(oa, ob), (name, n, streams, k, channels, kind, u)
    # the state both are left in (gravity store, ring, head): one more update of the same planar rows on each, A back at k = 1
    a.set_bufscale(1)
    rows = torch.from_numpy(_decimated("planar", _window("planar", streams, n, seed + 99), 1, channels)).cuda()
    oa = torch.zeros((streams * 2, w), dtype=dt, device="cuda")
    ob = torch.zeros((streams * 2, w), dtype=dt, device="cuda")
    a.process_f32(rows, oa, ops); b.process_f32(rows, ob, ops)
    assert a.last_launches() == b.last_launches()
    assert eq(oa, ob), (name, n, streams, k, channels, kind, "state")
    a.close(); b.close()


# ---- 1. process calls against a second path ----------------------------------------------------------------------------------------------------------
# every k with every n, stream count and channel count at least once per chain and input kind; odd k (groups of four frames straddle the sums), one stream
# (fewer lanes than a workgroup at n = 256), seven streams (several workgroups at n = 1024)
SHAPES = [(256, 1, 2, 2), (256, 3, 3, 1), (1024, 7, 4, 2), (1024, 3, 16, 1), (256, 7, 16, 2), (1024, 1, 3, 2)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,streams,k,channels", SHAPES, ids=["n%d-s%d-k%d-c%d" % s for s in SHAPES])
@pytest.mark.parametrize("name", CHAIN_NAMES)
def test_process_calls_equal_the_planar_entry_on_decimated_rows(glvlib, name, n, streams, k, channels, kind):
    _run_pair(glvlib, name, n, streams, k, channels, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_process_calls_at_bufsize_8192(glvlib, kind):
    """`bufsize 8192`, `setbufscale 2`: the shipped pipeline at n = 4096"""
    _run_pair(glvlib, "shipped", 4096, 3, 2, 2, kind, updates=F + 1)


# ---- 2. direct to the oracle ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["s16", "f32"])
def test_chain_on_bufscale_rows_is_the_oracle_s(glvlib, kind):
    """FFT | GRAVITY | AVERAGE, log_mode 0, k = 3: the oracle's chain on glvo_bufscale rows of the oracle's unpack, bit for bit"""
    import torch
    G = glvlib
    n, streams, k = 256, 2, 3
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    b = G.Batch(G.Params(n=n, avg_frames=F, log_mode=0), streams, GA)
    b.set_bufscale(k)
    L = Oracle.lib()
    grav = np.zeros((streams * 2, n), F32); hist = np.zeros((streams * 2, F, n), F32)
    heads = [C.c_size_t(0) for _ in range(streams * 2)]
    for u in range(UPDATES):
        x = _window(kind, streams, k * n, 810 + u)
        out = torch.zeros((streams * 2, n), dtype=torch.float32, device="cuda")
        _call(b, kind, torch.from_numpy(x).cuda(), out, G.OP_FFT | GA)
        got = out.cpu().numpy()
        rows = oracle_bufscale(Oracle, x, k, kind == "f32", 2).reshape(streams * 2, n)
        for r in range(streams * 2):
            want = Oracle.transform_fft(rows[r])
            Oracle.gravity(want, grav[r])
            Oracle.average(want, hist[r], heads[r], F)
            assert (got[r].view(np.uint32) == want.view(np.uint32)).all(), (kind, u, r)
    b.close()


# ---- 3. f32 specials -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "planar"])
@pytest.mark.parametrize("k", [2, 3])
def test_float_specials_pass_through_the_sums_as_in_float32(glvlib, kind, k):
    """-0.0, +-Inf, NaN and denormals at a window's first, a middle and its last frame: the stateless transform of A equals B's on np_bufscale's rows, which
    carry the specials as float32 arithmetic leaves them (0.0F + -0.0F = +0.0F; a NaN keeps its bits through additions and the division)"""
    import torch
    G = glvlib
    n, streams = 256, 3
    a, ops, w = _batch(G, n, streams, "fft", 2, k)
    b, _, _ = _batch(G, n, streams, "fft", 2)
    x = np.array(rec(77, streams, k * n, True), copy=True)                         # [streams][k n][2]
    specials = [F32(-0.0), F32(np.inf), F32(-np.inf), F32(np.nan), F32(1e-41), F32(-1e-45)]
    for i, v in enumerate(specials):
        s, c = i % streams, i % 2
        for frame in (0, (k * n) // 2 + i, k * n - 1):
            x[s, frame, c] = v
    x[2, 0:k, 1] = F32(-0.0)                                                       # a whole sum of -0.0F: +0.0F
    if kind == "planar": x = np.ascontiguousarray(x.transpose(0, 2, 1))
    rows = _decimated(kind, x, k, 2)
    assert rows.view(np.uint32)[5, 0] == 0 and np.isnan(rows).any() and np.isposinf(rows).any() and np.isneginf(rows).any()
    oa = torch.zeros((streams * 2, n), dtype=torch.float32, device="cuda")
    ob = torch.zeros((streams * 2, n), dtype=torch.float32, device="cuda")
    _call(a, kind, torch.from_numpy(x).cuda(), oa, ops)
    b.process_f32(torch.from_numpy(rows).cuda(), ob, ops)
    assert eq(oa, ob)
    a.close(); b.close()


# ---- 4. toggling k -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain", "shipped"])
def test_toggling_k_keeps_the_state_and_k_1_is_the_parent_path(glvlib, name):
    """k = 2 -> 1 -> 2 on a batch with history against a twin that is fed the decimated rows throughout; set_params and reset keep k"""
    import torch
    G = glvlib
    n, streams = 256, 3
    a, ops, w = _batch(G, n, streams, name)
    b, _, _ = _batch(G, n, streams, name)
    dt = _dtype(G, ops)
    ks = [1, 1, 2, 2, 1, 2, 1, 1]
    for u, k in enumerate(ks):
        a.set_bufscale(k)
        assert a.bufscale == k
        x = pcm(900 + u, streams, k * n)
        oa = torch.zeros((streams * 2, w), dtype=dt, device="cuda"); ob = torch.zeros((streams * 2, w), dtype=dt, device="cuda")
        a.process_s16(torch.from_numpy(x).cuda(), oa, ops)
        if k == 1:
            b.process_s16(torch.from_numpy(x).cuda(), ob, ops)
            assert a.last_launches() == b.last_launches() and a.kernel_name() == b.kernel_name()      # the parent's path: its launches, its kernel
        else:
            b.process_f32(torch.from_numpy(_decimated("s16", x, k, 2)).cuda(), ob, ops)
            assert a.last_launches() == b.last_launches() + 1
        assert eq(oa, ob), (name, u, k)
    a.set_bufscale(3)
    p = G.Params(n=n, **dict(_chains(G, n)[name][0], gravity_step=2.5))
    a.set_params(p); b.set_params(p)
    assert a.bufscale == 3
    a.reset(); b.reset()
    assert a.bufscale == 3
    x = pcm(950, streams, 3 * n)
    oa = torch.zeros((streams * 2, w), dtype=dt, device="cuda"); ob = torch.zeros((streams * 2, w), dtype=dt, device="cuda")
    a.process_s16(torch.from_numpy(x).cuda(), oa, ops)
    b.process_f32(torch.from_numpy(_decimated("s16", x, 3, 2)).cuda(), ob, ops)
    assert eq(oa, ob)
    a.close(); b.close()


# ---- 5. launch accounting, graph capture ---------------------------------------------------------------------------------------------------------------
def test_the_stage_is_counted_and_the_first_call_can_be_captured(glvlib):
    """last_launches and the timing pair count the extra launch; the FIRST process call after set_bufscale, captured into a hipGraph and replayed, gives the
    eager bits of a twin"""
    import torch
    G = glvlib
    hip = _Hip()
    n, streams, k = 1024, 3, 2
    a, ops, w = _batch(G, n, streams, "shipped", 2, k)
    e, _, _ = _batch(G, n, streams, "shipped", 2, k)
    b, _, _ = _batch(G, n, streams, "shipped")
    dt = _dtype(G, ops)
    xs = [torch.from_numpy(pcm(30 + u, streams, k * n)).cuda() for u in range(F + 1)]
    oa = [torch.zeros((streams * 2, w), dtype=dt, device="cuda") for _ in xs]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        graph, exe = hip.capture(st.cuda_stream, lambda: [a.process_s16(x, o, ops, stream=st.cuda_stream) for x, o in zip(xs, oa)])
        hip.launch(exe, st.cuda_stream)
    st.synchronize()
    hip.destroy(graph, exe)
    e.timing_begin()
    for u, x in enumerate(xs):
        oe = torch.zeros((streams * 2, w), dtype=dt, device="cuda")
        e.process_s16(x, oe, ops)
        assert eq(oa[u], oe), u
    ms, calls = e.timing_end()
    assert calls == len(xs) and ms > 0.0
    rows = torch.zeros((streams * 2, n), dtype=torch.float32, device="cuda")
    b.process_f32(rows, torch.zeros((streams * 2, w), dtype=dt, device="cuda"), ops)
    assert e.last_launches() == b.last_launches() + 1 == 3
    a.close(); e.close(); b.close()


# ---- 6. bounds ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["s16", "f32"])
@pytest.mark.parametrize("k", [2, 3])
def test_nothing_outside_the_windows_is_read_or_written(glvlib, kind, k):
    """the windows inside a larger allocation, one frame behind a load boundary, other frames before and behind them; guards behind the output.  A read outside
    shows as wrong bits against B, a write as a broken guard"""
    import torch
    G = glvlib
    n, streams = 256, 3
    f32 = kind == "f32"
    a, ops, w = _batch(G, n, streams, "fft", 2, k)
    b, _, _ = _batch(G, n, streams, "fft", 2)
    x = _window(kind, streams, k * n, 41)
    d_in = to_device(x, True, f32, tail_frames=64)                                 # odd alignment, a pattern of other frames behind the last stream
    flat = torch.zeros((streams * 2 * n + 4096,), dtype=torch.float32, device="cuda")
    flat[streams * 2 * n:] = -7.0
    _call(a, kind, d_in.data_ptr(), flat, ops)
    ob = torch.zeros((streams * 2, n), dtype=torch.float32, device="cuda")
    b.process_f32(torch.from_numpy(_decimated(kind, x, k, 2)).cuda(), ob, ops)
    torch.cuda.synchronize()
    assert bool((flat[streams * 2 * n:] == -7.0).all()), "the call wrote behind its output"
    assert eq(flat[:streams * 2 * n].view(streams * 2, n), ob)
    assert bool(torch.equal(d_in, torch.from_numpy(x.reshape(-1)).cuda())), "the recording was written"
    a.close(); b.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def _refused(G, code, call):
    with pytest.raises(G.GlvError) as e:
        call()
    assert e.value.code == code, str(e.value)
    return str(e.value)


def test_refusals_name_the_setter_and_leave_the_batch_usable(glvlib):
    import torch
    G = glvlib
    n, streams, k = 256, 2, 2
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    b = G.Batch(G.Params(n=n, avg_frames=F), streams, GA)
    for bad in (0, G.MAX_BUFSCALE + 1):
        assert "glv_batch_set_bufscale" in _refused(G, G.ERR_INVALID, lambda: b.set_bufscale(bad))
    assert b.bufscale == 1
    ring = G.Batch(G.Params(n=n), streams, G.OP_FFT | G.OP_RING_S16)
    assert "glv_batch_set_bufscale" in _refused(G, G.ERR_STATE, lambda: ring.set_bufscale(2))
    ring.close()
    b.set_bufscale(k)
    ops = G.OP_FFT | GA
    d_pcm = torch.from_numpy(pcm(5, streams, 4 * k * n)).cuda()
    out = torch.zeros((8, streams * 2, n), dtype=torch.float32, device="cuda")
    work = torch.zeros((1 << 22,), dtype=torch.uint8, device="cuda")
    starts = torch.zeros((8,), dtype=torch.int32, device="cuda")
    pitch = 4 * k * n
    refusals = [
        lambda: b.track_work_bytes(pitch, 64, 4, ops),
        lambda: b.track_s16(d_pcm, pitch, 64, 4, out, work, ops),
        lambda: b.track_wave_work_bytes(pitch, 64, 4, G.OP_WAVE),
        lambda: b.track_wave_s16(d_pcm, pitch, 64, 4, out, work, G.OP_WAVE),
        lambda: b.track_at_s16(d_pcm, pitch, starts, 4, out, work, G.OP_WAVE),
        lambda: b.track_wave_frames_work_bytes(4, 4, G.OP_WAVE | G.OP_R16),
        lambda: b.ring_update_s16(d_pcm, 64, out, ops),
        lambda: b.ring_append_s16(d_pcm, 64),
        lambda: b.ring_planar(out),
        lambda: b.autotune(d_pcm, out, ops),
        lambda: b.tune_placement(d_pcm, out, ops, 2),
    ]
    for i, call in enumerate(refusals):
        assert "glv_batch_set_bufscale" in _refused(G, G.ERR_STATE, call), i
    # what the planar entry refuses is refused in its words
    plain = G.Batch(G.Params(n=n), streams, G.OP_FFT)
    fresh = G.Batch(G.Params(n=n), streams, G.OP_FFT); fresh.set_bufscale(k)
    for bad_ops in (G.OP_FFT | G.OP_BARS, G.OP_FFT | G.OP_WAVE, G.OP_FFT | G.OP_GRAVITY):
        with pytest.raises(G.GlvError) as want:
            plain.process_f32(d_pcm, out, bad_ops)
        with pytest.raises(G.GlvError) as got:
            fresh.process_s16(d_pcm, out, bad_ops)
        assert (got.value.code, str(got.value)) == (want.value.code, str(want.value)), bad_ops
    plain.close(); fresh.close()
    # ... and the batch is as usable as before: the same bits as a twin that was never refused anything
    twin = G.Batch(G.Params(n=n, avg_frames=F), streams, GA); twin.set_bufscale(k)
    x = torch.from_numpy(pcm(6, streams, k * n)).cuda()
    oa = torch.zeros((streams * 2, n), dtype=torch.float32, device="cuda"); ob = torch.zeros((streams * 2, n), dtype=torch.float32, device="cuda")
    b.process_s16(x, oa, ops); twin.process_s16(x, ob, ops)
    assert eq(oa, ob)
    b.close(); twin.close()
