"""GPU: track mode at render frames for the wave module (glv_batch_track_wave_frames_s16 / _f32) -- `setinterpolate true` with the wave module, any gl_storage.

Contract (include/glv_spectrum.h): keyframes 0 and 1 are the caller's d_keys, keyframe 2 + t is (u + 1.0F) / 2.0F of the unpacked window of step t, read from the
recording where it lies; frame j is keyframe d_from[j] itself where d_from[j] == d_to[j], else s + ((e - s) * d_mod[j]) in float32, then the upload's quantiser, then
what a GLV_OP_WAVE process call with the same ops does with those texels; d_keys afterwards holds the two keyframes kept, as floats.  Everything is bit for bit.
The keyframes and the lerp are numpy float32 (pinned to the oracle and the compiled reference in tests/test_track_wave_frames_host.py), the upload and the bars
the oracle's.  Every batch under test is created with GLV_TRACK_FRAMES_SEGMENT=5: 23 frames are five segments, the last one ragged.  The recording begins at an
odd frame of its buffer and the windows start where a 60 fps renderer's do, so that groups of four frames on a 16-byte boundary and off one both occur (asserted).
Every call gets a workspace and an output of exactly the size asked for, with guards behind both."""
import ctypes as C
import os

import numpy as np
import pytest

from glava_amd.bar_positions import graph_column_texels, radial_bar_texels
from glava_amd.track_starts import keyframe_tables, renderer_starts
from gpu_lib import eq, texel_floats
from oracle_lib import Oracle
from test_track_frames import CUT, FROM, MOD, MODIFIED, ON, TO, _dev, _keys, _lerp, _same
from test_track_wave_frames_host import np_keyframes
from track_lib import GUARD, out_dtype, rec, seq, to_device, track, windows, with_table

pytestmark = pytest.mark.gpu
F32 = np.float32
STEPS, FRAMES, SEGMENT = 9, 23, 5
SHAPES = [(256, 1), (256, 3), (1024, 1), (1024, 3)]
SHAPE_IDS = ["n%d-s%d" % s for s in SHAPES]
STEP_OF_FRAME = [j * STEPS // FRAMES for j in range(FRAMES)]
assert len(FROM) == len(TO) == len(MOD) == len(MODIFIED) == FRAMES and max(FROM + TO) == STEPS + 1


def _forms(G, n):
    """name -> (parameters, bar-texel table, width of an output row, ops)"""
    radial = radial_bar_texels(n, 160)[0]
    W, B, R = G.OP_WAVE, G.OP_BARS, G.OP_R16
    full = dict(bars=n, bar_phase=0.5)
    return {"floats": (full, None, n, W), "texels": (full, None, n, W | R), "pass": (full, None, n, W | B | R), "pass_floats": (full, None, n, W | B),
            "bar": (dict(bars=len(radial)), ("bar", radial), len(radial), W | B | R), "bar_floats": (dict(bars=len(radial)), ("bar", radial), len(radial), W | B),
            "avg80": (dict(bars=80), None, 80, W | B), "maximum": (dict(bars=80, sample_mode=1), None, 80, W | B)}


def _batch(G, n, streams, form, channels=2, segment=SEGMENT, mask=None, storage=1):
    kw, table, _, _ = _forms(G, n)[form]
    assert "GLV_TRACK_FRAMES_SEGMENT" not in os.environ
    if segment: os.environ["GLV_TRACK_FRAMES_SEGMENT"] = str(segment)
    try:
        return with_table(G.Batch(G.Params(n=n, gl_storage=storage, channels=channels, **kw), streams, G.OP_WAVE | G.OP_BARS if mask is None else mask), table)
    finally:
        os.environ.pop("GLV_TRACK_FRAMES_SEGMENT", None)


def _launches(ops, G):
    return 3 if ops & G.OP_BARS else 2                                          # the frames, the write-back, the bars


class _Session:
    """a recording that begins at an odd frame of its buffer, and the table of a 60 fps renderer's window starts on the device"""

    def __init__(self, G, n, streams, f32, seed, channels=2):
        self.G, self.n, self.streams, self.f32, self.channels = G, n, streams, f32, channels
        self.starts = renderer_starts(22050, 60, 1, STEPS)
        self.pitch = (max(self.starts) + n + 38) | 1
        self.set_recording(rec(seed, streams, self.pitch, f32))
        self.d_starts = _dev(self.starts, np.uint32)
        fb = 8 if f32 else 4
        at = {(self.d_pcm.data_ptr() + (s * self.pitch + a) * fb) % 16 for s in range(streams) for a in self.starts}
        assert 0 in at and len(at) > 1, at                                      # groups that take the wide loads, and groups that do not

    def set_recording(self, x):
        self.x = x
        self.d_pcm = to_device(x, True, self.f32, tail_frames=self.n)

    def keyframes(self, starts=None):
        """float32 [steps][units][n] in numpy"""
        starts = self.starts if starts is None else starts
        return np_keyframes(self.x, [self.G.track_at_start(self.pitch, self.n, a) for a in starts], self.n, self.f32, self.channels)

    def at(self, b, ops, w, d_starts=None, steps=STEPS):
        """glv_batch_track_at_* on `b`: [steps][units][w]"""
        return track(b, "at", self.d_pcm, self.pitch, self.d_starts if d_starts is None else d_starts, steps, ops, w, out_dtype(self.G, ops), f32=self.f32)

    def frames(self, b, frm, to, mod, d_keys, keep, ops, w, steps=STEPS, t0=0, d_starts=None, stream=None):
        """glv_batch_track_wave_frames_* on `b`: [frames][units][w]; the guards behind the workspace and the output are checked"""
        import torch
        frames = len(frm)
        dt = out_dtype(self.G, ops)
        nbytes = b.track_wave_frames_work_bytes(steps, frames, ops)
        up = lambda v: (v + 255) & ~255                                         # noqa: E731
        if not ops & self.G.OP_BARS: assert nbytes == 256
        else: assert nbytes in (up(frames * self.streams * 2 * self.n * 2), up(frames * self.streams * 2 * self.n * 4)), nbytes
        work = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        assert work.data_ptr() % 256 == 0
        count = frames * self.streams * 2 * w
        flat = torch.zeros((count + GUARD,), dtype=dt, device="cuda")
        flat[count:] = 77
        self.tables = (_dev(frm, np.uint32), _dev(to, np.uint32), _dev(mod, np.float32))
        where = (self.d_starts if d_starts is None else d_starts).data_ptr() + 4 * t0
        (b.track_wave_frames_f32 if self.f32 else b.track_wave_frames_s16)(self.d_pcm, self.pitch, where, steps, *self.tables, frames, d_keys, keep, flat, work, ops,
                                                                           stream=stream)
        torch.cuda.synchronize()
        assert bool((work[nbytes:] == 0xA5).all()), "the call wrote behind the workspace it asked for"
        assert bool((flat[count:] == 77).all()), "the call wrote behind its output"
        if not ops & self.G.OP_BARS: assert bool((work[:nbytes] == 0xA5).all()), "a call without bars touched the workspace"
        self.work = work[:nbytes]
        return flat[:count].view(frames, self.streams * 2, w)


def _want(G, form, n, U):
    """what the form gives for one upload row U uint16 [n], from the oracle (None: the form has no oracle here -- it is held to glv_batch_track_at_* in group 1)"""
    kw, table, w, ops = _forms(G, n)[form]
    r16 = bool(ops & G.OP_R16)
    if form == "texels": return U
    if form == "floats": return texel_floats(U)
    if form == "maximum": return Oracle.bars_mode(texel_floats(U), 80, 1, 0.65, 0.025, 0.0)
    if form == "avg80": return None
    t, f = Oracle.bars_int(U, n, 0.025, 0.5)
    if form in ("pass", "pass_floats"): return t if r16 else f
    return (t if r16 else f)[np.asarray(table[1], dtype=np.int64)]


def _check_forms(G, S, forms, frm, to, mod, k_host, keep, rows, every_row=False, steps=STEPS):
    """the call in each of `forms` against numpy and the oracle; returns d_keys of the last as numpy"""
    import torch
    n, streams = S.n, S.streams
    U = Oracle.texels_r16(_lerp(k_host, rows, frm, to, mod, steps).reshape(-1, n)).reshape(len(frm), streams * 2, n)
    check_rows = range(streams * 2) if every_row else sorted({0, streams * 2 - 1})
    kept = None
    for form in forms:
        _, _, w, ops = _forms(G, n)[form]
        bt = _batch(G, n, streams, form, S.channels)
        d_keys = torch.from_numpy(k_host.copy()).cuda()
        got = S.frames(bt, frm, to, mod, d_keys, keep, ops, w, steps=steps).cpu().numpy()
        assert bt.last_launches() == _launches(ops, G) and bt.kernel_name() == "glv_wave_frames_kernel", (form, bt.last_launches(), bt.kernel_name())
        if form in ("texels", "floats"):
            assert _same(got, _want(G, form, n, U)), form                       # every frame, row and sample
        else:
            for j in range(len(frm)):
                for r in check_rows:
                    assert _same(got[j, r], _want(G, form, n, U[j, r])), (form, j, r)
        kept = d_keys.cpu().numpy()
        bt.close()
    return kept


# ---- 1. identity tables ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [2, 1], ids=["stereo", "mono"])
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("n,streams", SHAPES, ids=SHAPE_IDS)
def test_identity_tables_give_the_table_call_s_blocks(glvlib, n, streams, f32, channels):
    """from == to == 2 + step_of_frame: frame j is block step_of_frame[j] of glv_batch_track_at_* with the same wave ops on a twin batch, in every output form"""
    G = glvlib
    S = _Session(G, n, streams, f32, 401, channels)
    idx = [2 + t for t in STEP_OF_FRAME]
    for form, (_, table, w, ops) in _forms(G, n).items():
        bt, bs = _batch(G, n, streams, form, channels), _batch(G, n, streams, form, channels)
        keys = _keys(n, streams, 5)
        before = keys.clone()
        got = S.frames(bt, idx, idx, [0.25] * FRAMES, keys, (0, 1), ops, w)
        if form == "bar":
            limit = _written(S.work, n)                                          # the bar texels sample less than a row, and not a whole number of groups
            assert 0 < limit < n and limit % 4 == 0 and limit % 256 != 0, limit
        assert bt.last_launches() == _launches(ops, G) and bt.kernel_name() == "glv_wave_frames_kernel", (form, bt.last_launches(), bt.kernel_name())
        want = S.at(bs, ops, w)
        for j in range(FRAMES):
            assert eq(got[j], want[STEP_OF_FRAME[j]]), (form, j)
        assert eq(keys, before), form                                          # keep = (0, 1): the keyframes stay
        bt.close(); bs.close()


def _written(work, n):
    """samples of a row the frames kernel wrote into a workspace of texel rows that was filled with 0xA5: n less the samples no row has touched"""
    rows = work.view(-1, n * 2)[:FRAMES * 2].cpu().numpy().view(np.uint16)
    untouched = (rows == 0xA5A5).all(axis=0)
    return n - int(np.argmin(untouched[::-1])) if not untouched.all() else 0


# ---- 2. lerped frames -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [2, 1], ids=["stereo", "mono"])
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("n,streams", SHAPES, ids=SHAPE_IDS)
def test_lerped_frames_against_numpy_and_the_oracle(glvlib, oracle, n, streams, f32, channels):
    """(0, 1), (1, k), (k, k'), backward pairs, equal pairs and the last step's keyframe (tests/test_track_frames.py's tables), d_keys straddling [0, 1]"""
    G = glvlib
    S = _Session(G, n, streams, f32, 402, channels)
    rows = S.keyframes()
    k_host = _keys(n, streams, 6).cpu().numpy()
    assert k_host.min() < 0 and k_host.max() > 1
    forms = [f for f in _forms(G, n) if f != "avg80"]
    kept = _check_forms(G, S, forms, FROM, TO, MOD, k_host, (9, 10), rows)
    assert _same(kept, rows[7:9])                                               # keep = (9, 10): the float keyframes of steps 7 and 8


# ---- 3. a table of starts -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
def test_a_table_with_repeats_backward_jumps_and_entries_beyond_the_recording(glvlib, oracle, f32):
    G = glvlib
    n, streams = 256, 3
    S = _Session(G, n, streams, f32, 403)
    last = S.pitch - n
    table = [S.starts[4], S.starts[4], 3, last + 1, S.starts[2], 2 ** 32 - 1, last, 0, last + 1000]
    assert len(table) == STEPS
    clamped = [min(a, last) for a in table]
    assert clamped != table
    rows = S.keyframes(table)
    for form in ("texels", "bar"):
        _, _, w, ops = _forms(G, n)[form]
        ba, bb = _batch(G, n, streams, form), _batch(G, n, streams, form)
        ka, kb = _keys(n, streams, 9), _keys(n, streams, 9)
        got = S.frames(ba, FROM, TO, MOD, ka, (4, 7), ops, w, d_starts=_dev(table, np.uint32))
        want = S.frames(bb, FROM, TO, MOD, kb, (4, 7), ops, w, d_starts=_dev(clamped, np.uint32))
        assert eq(got, want) and eq(ka, kb), form
        assert _same(ka.cpu().numpy(), rows[[2, 5]]), form
        ba.close(); bb.close()
    S.d_starts = _dev(table, np.uint32)
    _check_forms(G, S, ["texels"], FROM, TO, MOD, _keys(n, streams, 9).cpu().numpy(), (0, 1), rows)


# ---- 4. chunk composition -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", ["on", "late"])
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("n,streams", [(256, 3), (1024, 1)], ids=["n256-s3", "n1024-s1"])
def test_nine_steps_cut_as_4_and_5_at_a_frame_that_runs_an_update(glvlib, n, streams, f32, on):
    G = glvlib
    S = _Session(G, n, streams, f32, 404)
    uratio = [0.4] * FRAMES
    whole = keyframe_tables(MODIFIED, ON[on], uratio)
    first = keyframe_tables(MODIFIED[:CUT], ON[on][:CUT], uratio[:CUT])
    idle = CUT - 1 - max(j for j in range(CUT) if MODIFIED[j])                  # frames without an update in front of the cut: the second chunk's kcounter
    rest = keyframe_tables(MODIFIED[CUT:], ON[on][CUT:], uratio[CUT:], kcounter=idle)
    assert MODIFIED[CUT] and (first[3:], rest[3:], whole[3:]) == (((4, 5), (5, 6), (9, 10)) if on == "on" else ((0, 1), (1, 6), (1, 10)))
    for form in ("texels", "pass", "floats"):
        _, _, w, ops = _forms(G, n)[form]
        bw, bc = _batch(G, n, streams, form), _batch(G, n, streams, form)
        kw_, kc = _keys(n, streams, 7), _keys(n, streams, 7)
        want = S.frames(bw, *whole[:3], kw_, whole[3:], ops, w)
        a = S.frames(bc, *first[:3], kc, first[3:], ops, w, steps=4)
        b = S.frames(bc, *rest[:3], kc, rest[3:], ops, w, steps=5, t0=4)
        assert eq(a, want[:CUT]) and eq(b, want[CUT:]), (form, on)
        assert eq(kc, kw_), (form, on)
        bw.close(); bc.close()


# ---- 5. special values --------------------------------------------------------------------------------------------------------------------------------------
def test_special_values_in_the_recording_and_the_keyframes(glvlib, oracle):
    """Inf, NaN and -0 samples in a float recording, and in d_keys: the keyframes they reach, the lerp over them and the quantiser, bit for bit"""
    G = glvlib
    n, streams = 256, 3
    S = _Session(G, n, streams, True, 405)
    x = np.array(S.x, copy=True)
    x[0, S.starts[8] + n - 3, 0] = np.inf; x[1, S.starts[6] + n - 2, 1] = np.nan; x[2, 5:40, :] = -0.0; x[2, S.starts[4] + 7, 0] = -np.inf
    x[0, S.starts[1] + 1, :] = [np.inf, -np.inf]; x[1, S.starts[0]:S.starts[0] + 4, 0] = [-1.0, -1.0000001, 1.0, 3.0]
    S.set_recording(x)
    rows = S.keyframes()
    assert np.isnan(rows).any() and np.isinf(rows).any()
    k_host = _keys(n, streams, 8).cpu().numpy()
    k_host[0, 0, :8] = [-0.0, np.nan, np.inf, -np.inf, 0.0, 1.0, 2.0, -1.0]
    k_host[1, 0, :8] = [0.5, 0.5, 0.5, 0.5, -0.0, np.nan, np.inf, np.inf]
    kept = _check_forms(G, S, ["texels", "floats", "pass", "maximum"], FROM, TO, MOD, k_host, (1, 8), rows, every_row=True)
    assert _same(kept, np.stack([k_host[1], rows[6]]))                          # the kept keyframes are floats: a NaN stays one


# ---- 6. index clamping --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,streams", [(256, 3), (1024, 1)], ids=["n256-s3", "n1024-s1"])
def test_indices_beyond_the_last_keyframe_are_clamped(glvlib, n, streams):
    G = glvlib
    S = _Session(G, n, streams, False, 406)
    big = [STEPS + 2, 1000, 2 ** 31, 2 ** 32 - 1]
    frm = [big[j % 4] if j % 3 == 0 else FROM[j] for j in range(FRAMES)]
    to = [big[(j + 1) % 4] if j % 5 in (0, 3) else TO[j] for j in range(FRAMES)]
    clamp = lambda t: [min(v, STEPS + 1) for v in t]                           # noqa: E731
    assert clamp(frm) != frm and clamp(to) != to
    for form in ("texels", "bar"):
        _, _, w, ops = _forms(G, n)[form]
        ba, bb = _batch(G, n, streams, form), _batch(G, n, streams, form)
        ka, kb = _keys(n, streams, 9), _keys(n, streams, 9)
        got = S.frames(ba, frm, to, MOD, ka, (2, 3), ops, w)
        want = S.frames(bb, clamp(frm), clamp(to), MOD, kb, (2, 3), ops, w)
        assert eq(got, want) and eq(ka, kb), form
        ba.close(); bb.close()


# ---- 7. the grid cap ----------------------------------------------------------------------------------------------------------------------------------------
def test_more_work_items_than_the_grid_has_workgroups(glvlib, oracle):
    """n = 256, one stream, segments of one frame: 8300 work items of the frames kernel against its 8192 workgroups (glv_track_frames.hip kFramesGridCap) -- the grid
    loops"""
    G = glvlib
    n, streams, frames = 256, 1, 8300
    assert frames > 256 * 32
    S = _Session(G, n, streams, False, 407)
    rows = S.keyframes()
    rng = np.random.default_rng(17)
    frm = [int(v) for v in rng.integers(0, STEPS + 2, frames)]
    to = [int(v) for v in rng.integers(0, STEPS + 2, frames)]
    mod = [float(v) for v in rng.random(frames, dtype=np.float32)]
    keys = _keys(n, streams, 10)
    k_host = keys.cpu().numpy()
    bt = _batch(G, n, streams, "texels", segment=1)
    got = S.frames(bt, frm, to, mod, keys, (0, 1), G.OP_WAVE | G.OP_R16, n).cpu().numpy()
    sample = sorted({0, 1, 2, 8190, 8191, 8192, 8193, frames - 2, frames - 1} | {int(v) for v in rng.integers(0, frames, 40)})
    want = Oracle.texels_r16(_lerp(k_host, rows, [frm[j] for j in sample], [to[j] for j in sample], [mod[j] for j in sample]).reshape(-1, n)).reshape(len(sample), 2, n)
    for i, j in enumerate(sample):
        assert _same(got[j], want[i]), j
    bt.close()


# ---- 8. graph capture ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_first_call_replayed_after_rewriting_d_mod_and_d_where(glvlib, oracle):
    """kernels only: the first call of a batch can be captured (one stream, a linear graph); the tables are read when the kernels run"""
    import torch
    G = glvlib
    n, streams = 1024, 3
    S = _Session(G, n, streams, False, 408)
    keys = _keys(n, streams, 11)
    k_host = keys.cpu().numpy()
    bt = _batch(G, n, streams, "pass")
    ops = G.OP_WAVE | G.OP_BARS | G.OP_R16
    work = torch.zeros((bt.track_wave_frames_work_bytes(STEPS, FRAMES, ops),), dtype=torch.uint8, device="cuda")
    out = torch.zeros((FRAMES, streams * 2, n), dtype=torch.int16, device="cuda")
    d_from, d_to, d_mod = _dev(FROM, np.uint32), _dev(TO, np.uint32), _dev(MOD, np.float32)
    other = [float(F32(1.0) - F32(m)) for m in MOD]
    moved = [S.starts[(t * 4 + 1) % STEPS] + t for t in range(STEPS)]
    d_other, d_moved = _dev(other, np.float32), _dev(moved, np.uint32)
    d_where = S.d_starts.clone()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        bt.track_wave_frames_s16(S.d_pcm, S.pitch, d_where, STEPS, d_from, d_to, d_mod, FRAMES, keys, (0, 1), out, work, ops, stream=s.cuda_stream)
    assert bt.last_launches() == 3
    torch.cuda.synchronize()
    assert not bool(out.any())                                                    # captured, not run
    with torch.cuda.stream(s):
        d_mod.copy_(d_other); d_where.copy_(d_moved)                              # in stream order, in front of the replay
        g.replay()
    torch.cuda.synchronize()
    U = Oracle.texels_r16(_lerp(k_host, S.keyframes(moved), FROM, TO, other).reshape(-1, n)).reshape(FRAMES, streams * 2, n)
    got = out.cpu().numpy()
    for j in range(FRAMES):
        for r in (0, streams * 2 - 1):
            assert _same(got[j, r], _want(G, "pass", n, U[j, r])), (j, r)
    del g
    bt.close()


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_an_fft_batch_s_state_stays(glvlib):
    import torch
    G = glvlib
    n, streams = 256, 3
    S = _Session(G, n, streams, False, 409)
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    mask = G.OP_WAVE | G.OP_BARS | GA
    ops = G.OP_WAVE | G.OP_BARS | G.OP_R16
    chain = G.OP_FFT | GA | G.OP_R16
    kw = dict(n=n, gl_storage=1, avg_window_kind=1, bars=n, bar_phase=0.5)
    bt, twin = G.Batch(G.Params(**kw), streams, mask), G.Batch(G.Params(**kw), streams, mask)
    wins = windows(S.x, n, S.starts[:4])
    assert eq(seq(bt, wins[:2], chain, n, torch.int16), seq(twin, wins[:2], chain, n, torch.int16))
    keys = _keys(n, streams, 12)
    before = keys.clone()
    tabs = (_dev(FROM, np.uint32), _dev(TO, np.uint32), _dev(MOD, np.float32))
    work = torch.zeros((bt.track_wave_frames_work_bytes(STEPS, FRAMES, ops) + 64,), dtype=torch.uint8, device="cuda")
    out = torch.zeros((FRAMES * streams * 2 * n + 64,), dtype=torch.int16, device="cuda")
    L = G.lib()
    launches = bt.last_launches()

    def call(b=bt, pcm=S.d_pcm.data_ptr(), pitch=S.pitch, where=S.d_starts.data_ptr(), steps=STEPS, frm=tabs[0].data_ptr(), to=tabs[1].data_ptr(), mod=tabs[2].data_ptr(),
             frames=FRAMES, d_keys=keys.data_ptr(), keep=(9, 10), fr=True, d_out=out.data_ptr(), d_work=work.data_ptr(), ops=ops):
        s = G.TrackFrames(frm, to, mod, frames, d_keys, keep[0], keep[1])
        return L.glv_batch_track_wave_frames_s16(b._h, pcm, pitch, where, steps, C.byref(s) if fr else None, d_out, d_work, ops, None)

    INVALID, STATE = G.ERR_INVALID, G.ERR_STATE
    refused = [("fr NULL", INVALID, dict(fr=False)), ("d_from NULL", INVALID, dict(frm=None)), ("d_to NULL", INVALID, dict(to=None)), ("d_mod NULL", INVALID, dict(mod=None)),
               ("d_keys NULL", INVALID, dict(d_keys=None)), ("frames 0", INVALID, dict(frames=0)), ("d_keys alignment", INVALID, dict(d_keys=keys.data_ptr() + 4)),
               ("d_from alignment", INVALID, dict(frm=tabs[0].data_ptr() + 2)), ("d_to alignment", INVALID, dict(to=tabs[1].data_ptr() + 1)),
               ("d_mod alignment", INVALID, dict(mod=tabs[2].data_ptr() + 2)), ("rows", INVALID, dict(frames=2 ** 31 // streams + 1)),
               ("no WAVE", INVALID, dict(ops=G.OP_BARS | G.OP_R16)), ("an FFT chain", INVALID, dict(ops=chain)),
               # the table call's own, and the wave form's
               ("steps 0", INVALID, dict(steps=0, keep=(0, 1))), ("d_where NULL", INVALID, dict(where=None)), ("d_where alignment", INVALID, dict(where=S.d_starts.data_ptr() + 2)),
               ("pitch", INVALID, dict(pitch=n - 1)), ("d_pcm NULL", INVALID, dict(pcm=None)), ("d_out NULL", INVALID, dict(d_out=None)), ("d_work NULL", INVALID, dict(d_work=None)),
               ("d_work alignment", INVALID, dict(d_work=work.data_ptr() + 64))]
    for bad in (G.OP_FFT, G.OP_GRAVITY, G.OP_AVERAGE, G.OP_RAW, G.OP_SMOOTH, G.OP_WRANGE, G.OP_MAGNITUDE, G.OP_OUTPUT_IS_STATE, G.OP_PRIVATE_STATE):
        refused.append(("ops 0x%x" % bad, INVALID, dict(ops=ops | bad)))
    for kf, kt in ((1, 0), (0, 0), (0, 2), (1, 1), (2, 2), (3, 2), (2, 1), (1, STEPS + 2), (2, STEPS + 2), (STEPS + 1, STEPS + 2), (0, 2 ** 32 - 1)):
        refused.append(("keep %d %d" % (kf, kt), INVALID, dict(keep=(kf, kt))))
    for name, code, kw_ in refused:
        assert call(**kw_) == code, (name, L.glv_last_error().decode())
        assert L.glv_last_error().decode(), name
        assert bt.last_launches() == launches, name
    # what glv_batch_track_wave_* refuses of a batch, with its codes: gl_storage 0 with bars, a creation mask without both bits, column texels set
    others = [G.Batch(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=0), streams, G.OP_WAVE | G.OP_BARS)]
    others += [G.Batch(G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5), streams, m) for m in (G.OP_WAVE, G.OP_BARS, G.OP_BARS | GA)]
    table = graph_column_texels(n, 64)[0]
    cols = G.Batch(G.Params(n=n, gl_storage=1, bars=len(table)), streams, mask)
    cols.set_column_texels(table)
    for b, o in [(b, ops) for b in others] + [(cols, ops), (cols, G.OP_WAVE | G.OP_R16)]:
        was = b.last_launches()
        assert call(b=b, ops=o) == STATE, L.glv_last_error().decode()
        assert b.last_launches() == was
        with pytest.raises(G.GlvError) as ei:
            b.track_wave_frames_work_bytes(STEPS, FRAMES, o)
        assert ei.value.code == STATE
    for b in others + [cols]: b.close()
    for bad in (dict(steps=0), dict(frames=0), dict(ops=G.OP_BARS | G.OP_R16), dict(ops=chain), dict(frames=2 ** 31 // streams + 1)):
        with pytest.raises(G.GlvError) as ei:
            bt.track_wave_frames_work_bytes(**dict(dict(steps=STEPS, frames=FRAMES, ops=ops), **bad))
        assert ei.value.code == INVALID, bad
    # the FFT frames entry still refuses GLV_OP_WAVE
    s = G.TrackFrames(tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), FRAMES, keys.data_ptr(), 9, 10)
    assert L.glv_batch_track_frames_s16(bt._h, S.d_pcm.data_ptr(), S.pitch, S.d_starts.data_ptr(), None, STEPS, C.byref(s), out.data_ptr(), work.data_ptr(), ops, None) == INVALID
    torch.cuda.synchronize()
    assert eq(keys, before) and not bool(out.any()) and not bool(work.any())      # nothing was launched
    # a call that runs: three launches, and the FFT chain on the same batch continues exactly like an untouched twin's
    got = S.frames(bt, FROM, TO, MOD, keys, (1, STEPS + 1), ops, n)
    assert bt.last_launches() == 3 and bool(got.any()) and not eq(keys, before)
    assert eq(seq(bt, wins[2:], chain, n, torch.int16), seq(twin, wins[2:], chain, n, torch.int16))
    bt.close(); twin.close()
