"""GPU: track mode at render frames (glv_batch_track_frames_s16 / _f32) on gl_storage 3 batches -- `setinterpolate true` on `setaccelfft false`.

Contract (include/glv_spectrum.h): the `steps` updates are glv_batch_track_rates_* 's and leave the batch exactly as that call does; block j of d_out is what a
gl_storage 3 process call with the same ops would write if its finished float row were w_j -- keyframe d_from[j] itself where d_from[j] == d_to[j], else
s + ((e - s) * d_mod[j]) in float32 -- and d_keys afterwards holds the two keyframes kept.  Everything is bit for bit.  The float keyframes come from a
gl_storage 0 twin batch (the same call without GLV_OP_BARS / GLV_OP_R16: the parent's code, pinned elsewhere), the lerp from numpy float32, the upload and
the bars from the oracle as in tests/test_upload_chain.py.  Every batch under test is created with GLV_TRACK_FRAMES_SEGMENT=5: 23 frames are five segments, the
last one ragged.  Every call gets a workspace and an output of exactly the size asked for, with guards behind both."""
import ctypes as C
import os

import numpy as np
import pytest

from glava_amd.bar_positions import graph_column_texels, radial_bar_texels
from glava_amd.track_starts import keyframe_tables, renderer_starts
from gpu_lib import eq, texel_floats
from oracle_lib import Oracle
from track_lib import GUARD, bars_batch, out_dtype, rec, seq, to_device, windows

pytestmark = pytest.mark.gpu
F32 = np.float32
STEPS, FRAMES, F, SEGMENT = 9, 23, 5, 5
URS = [1.0] * 3 + [59.0] * 3 + [60.0] * 3
SHAPES = [(256, 1), (256, 3), (4096, 1), (4096, 3)]
SHAPE_IDS = ["n%d-s%d" % s for s in SHAPES]
STEP_OF_FRAME = [j * STEPS // FRAMES for j in range(FRAMES)]


def _forms(n):
    """name -> (parameters, table, width of an output row, r16)"""
    radial = radial_bar_texels(n, 160)[0]
    cols = graph_column_texels(n, 64 if n == 256 else 320)[0]
    return {"texels": (dict(bars=n, bar_phase=0.5), None, n, True), "pass": (dict(bars=n, bar_phase=0.5), None, n, True),
            "bar": (dict(bars=len(radial)), ("bar", radial), len(radial), True), "bar_floats": (dict(bars=len(radial)), ("bar", radial), len(radial), False),
            "col": (dict(bars=len(cols)), ("col", cols), len(cols), False), "maximum": (dict(bars=80, sample_mode=1), None, 80, False)}


def _ops(G, form, r16):
    return G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | (0 if form == "texels" else G.OP_BARS) | (G.OP_R16 if r16 else 0)


def _batch(G, n, streams, form, storage=None, segment=SEGMENT):
    kw, table, _, _ = _forms(n)[form]
    kw = dict(kw, gl_storage=G.GL_STORAGE_UPLOAD if storage is None else storage)
    if storage == 0: kw, table = dict(gl_storage=0), None
    assert "GLV_TRACK_FRAMES_SEGMENT" not in os.environ
    if segment: os.environ["GLV_TRACK_FRAMES_SEGMENT"] = str(segment)
    try:
        return bars_batch(G, n, kw, table, F, streams, live=False)
    finally:
        os.environ.pop("GLV_TRACK_FRAMES_SEGMENT", None)


def _dev(a, dtype):
    import torch
    a = np.asarray(a, dtype=dtype)
    return torch.from_numpy(a.view(np.int32).copy() if dtype == np.uint32 else a.copy()).cuda()


class _Session:
    """a recording, its windows at a 60 fps renderer's starts, and the two tables of the updates on the device"""

    def __init__(self, G, n, streams, f32, seed):
        self.G, self.n, self.streams, self.f32 = G, n, streams, f32
        self.starts = renderer_starts(22050, 60, 1, STEPS + 1)
        self.pitch = (max(self.starts) + n + 38) | 1
        self.x = rec(seed, streams, self.pitch, f32)
        self.set_recording(self.x)
        self.d_starts = _dev(self.starts[:STEPS], np.uint32)
        self.d_ur = _dev(URS + [np.nan] * 8, np.float32)

    def set_recording(self, x):
        self.x = x
        self.d_pcm = to_device(x, True, self.f32, tail_frames=self.n)
        self.wins = windows(x, self.n, [self.G.track_at_start(self.pitch, self.n, s) for s in self.starts])

    def rates(self, b, ops, w, steps=STEPS, t0=0):
        """glv_batch_track_rates_* on `b`: [steps][units][w]"""
        import torch
        dt = out_dtype(self.G, ops)
        work = torch.full((b.track_at_work_bytes(steps, ops),), 0xA5, dtype=torch.uint8, device="cuda")
        out = torch.zeros((steps, self.streams * 2, w), dtype=dt, device="cuda")
        (b.track_rates_f32 if self.f32 else b.track_rates_s16)(self.d_pcm, self.pitch, self.d_starts.data_ptr() + 4 * t0, self.d_ur.data_ptr() + 4 * t0, steps, out, work, ops)
        torch.cuda.synchronize()
        return out

    def keyframes(self):
        """float32 [STEPS][units][n]: the finished float rows of every step, from a gl_storage 0 twin"""
        G = self.G
        b = _batch(G, self.n, self.streams, "texels", storage=0)
        rows = self.rates(b, G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE, self.n).cpu().numpy()
        b.close()
        return rows

    def frames(self, b, frm, to, mod, d_keys, keep, ops, w, steps=STEPS, t0=0, rates=True, stream=None, sync=True):
        """glv_batch_track_frames_* on `b`: [frames][units][w]; the guards behind the workspace and the output are checked"""
        import torch
        frames = len(frm)
        dt = out_dtype(self.G, ops)
        nbytes = b.track_frames_work_bytes(steps, frames, ops)
        work = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        assert work.data_ptr() % 256 == 0
        count = frames * self.streams * 2 * w
        flat = torch.zeros((count + GUARD,), dtype=dt, device="cuda")
        flat[count:] = 77
        self.tables = (_dev(frm, np.uint32), _dev(to, np.uint32), _dev(mod, np.float32))
        d_ur = self.d_ur.data_ptr() + 4 * t0 if rates else None
        (b.track_frames_f32 if self.f32 else b.track_frames_s16)(self.d_pcm, self.pitch, self.d_starts.data_ptr() + 4 * t0, d_ur, steps, *self.tables, frames, d_keys, keep,
                                                                 flat, work, ops, stream=stream)
        if sync:
            torch.cuda.synchronize()
            assert bool((work[nbytes:] == 0xA5).all()), "the call wrote behind the workspace it asked for"
            assert bool((flat[count:] == 77).all()), "the call wrote behind its output"
        self.flat, self.work = flat, work
        return flat[:count].view(frames, self.streams * 2, w)

    def state_eq(self, a, b, ops, w):
        """the state two batches are left in, through one more update on each"""
        dt = out_dtype(self.G, ops)
        return eq(seq(a, self.wins[STEPS:], ops, w, dt, self.f32), seq(b, self.wins[STEPS:], ops, w, dt, self.f32))


def _keys(n, streams, seed=None):
    """d_keys float32 [2][units][n]: zeros, or seeded values that straddle [0, 1]"""
    import torch
    if seed is None:
        return torch.zeros((2, streams * 2, n), dtype=torch.float32, device="cuda")
    return torch.from_numpy((np.random.default_rng(seed).random((2, streams * 2, n), dtype=np.float32) * F32(1.3) - F32(0.1)).astype(np.float32)).cuda()


def _lerp(keys, rows, frm, to, mod, steps=STEPS):
    """w float32 [frames][units][n] in numpy: the keyframe itself, or s + ((e - s) * mod) in three float32 operations; indices clamped to steps + 1"""
    key = lambda k: keys[k] if k < 2 else rows[k - 2]                          # noqa: E731
    out = []
    with np.errstate(all="ignore"):
        for a, b, m in zip(frm, to, mod):
            a, b = min(a, steps + 1), min(b, steps + 1)
            s, e = key(a), key(b)
            out.append(s.copy() if a == b else (s + ((e - s).astype(F32) * F32(m)).astype(F32)).astype(F32))
    return np.stack(out)


def _want(G, form, n, U, cache=None, key=None):
    """what the form's bars give for one upload row U uint16 [n], as tests/test_upload_chain.py states them (cache: the oracle's pass over a row, once per key)"""
    kw, table, w, r16 = _forms(n)[form]
    if form == "texels": return U
    if form == "maximum": return Oracle.bars_mode(texel_floats(U), 80, 1, 0.65, 0.025, 0.0)
    if cache is None: cache, key = {}, 0
    if key not in cache: cache[key] = Oracle.bars_int(U, n, 0.025, 0.5)
    t, f = cache[key]
    if form == "pass": return t
    if form in ("bar", "bar_floats"): return (t if r16 else f)[np.asarray(table[1], dtype=np.int64)]
    tab = np.asarray(table[1], dtype=np.int64)
    T = texel_floats(t)
    return (((T[tab[:, 0]] + T[tab[:, 1]]).astype(F32) + T[tab[:, 2]]).astype(F32) / F32(3.0)).astype(F32)


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype == np.int16: got = got.view(np.uint16)
    if got.dtype == np.float32: got, want = got.view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    return got.shape == want.shape and bool((got == want).all())


def _launches(form):
    return 2 + 1 + 1 + (0 if form == "texels" else 1)      # the transform and the scan, the frames, the write-back, the bars


# ---- 1. identity tables ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("n,streams", SHAPES, ids=SHAPE_IDS)
def test_identity_tables_give_the_rates_call_s_blocks(glvlib, n, streams, f32):
    """from == to == 2 + step_of_frame: frame j is block step_of_frame[j] of glv_batch_track_rates_* on a twin batch, in every output form; so is the state"""
    G = glvlib
    S = _Session(G, n, streams, f32, 301)
    idx = [2 + t for t in STEP_OF_FRAME]
    for form, (_, _, w, r16) in _forms(n).items():
        ops = _ops(G, form, r16)
        bt, bs = _batch(G, n, streams, form), _batch(G, n, streams, form)
        keys = _keys(n, streams, 5)
        before = keys.clone()
        got = S.frames(bt, idx, idx, [0.25] * FRAMES, keys, (0, 1), ops, w)
        assert bt.last_launches() == _launches(form) and bt.kernel_name() == "glv_track_frames_kernel", (form, bt.last_launches(), bt.kernel_name())
        want = S.rates(bs, ops, w)
        for j in range(FRAMES):
            assert eq(got[j], want[STEP_OF_FRAME[j]]), (form, j)
        assert eq(keys, before), form                                          # keep = (0, 1): the keyframes stay
        assert S.state_eq(bt, bs, ops, w), form
        bt.close(); bs.close()


# ---- 2. lerped frames -------------------------------------------------------------------------------------------------------------------------------------
#        (0, 1)  (1, k)  (k, k')  backwards  the keyframe itself  the last step's row
FROM = [0, 0, 1, 1, 2, 3, 3, 7, 10, 4, 4, 5, 1, 0, 6, 6, 9, 10, 2, 8, 8, 0, 9]
TO = [1, 1, 2, 2, 3, 4, 4, 2, 3, 4, 5, 5, 0, 0, 7, 7, 10, 10, 9, 9, 9, 10, 10]
MOD = [0.0, 0.59310347, 0.0, 1.0, 0.25, 0.5, 1.0, 0.3, 0.75, 0.9, 0.1, 0.6, 0.4, 0.2, 0.0, 0.5931035, 1.0, 0.7, 0.33333334, 0.0, 0.8, 0.45, 1.0]
assert len(FROM) == len(TO) == len(MOD) == FRAMES and max(FROM + TO) == STEPS + 1


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("n,streams", SHAPES, ids=SHAPE_IDS)
def test_lerped_frames_against_numpy_and_the_oracle(glvlib, oracle, n, streams, f32):
    G = glvlib
    S = _Session(G, n, streams, f32, 302)
    rows = S.keyframes()
    keys = _keys(n, streams, 6)
    k_host = keys.cpu().numpy()
    w_all = _lerp(k_host, rows, FROM, TO, MOD)
    U = Oracle.texels_r16(w_all.reshape(-1, n)).reshape(FRAMES, streams * 2, n)
    check_rows = sorted({0, streams * 2 - 1})
    cache = {}
    for form, (_, _, w, r16) in _forms(n).items():
        ops = _ops(G, form, r16)
        bt = _batch(G, n, streams, form)
        d_keys = keys.clone()
        got = S.frames(bt, FROM, TO, MOD, d_keys, (9, 10), ops, w).cpu().numpy()
        assert bt.last_launches() == _launches(form), (form, bt.last_launches())
        if form == "texels":
            assert _same(got, U), form                                         # every frame, row and bin
        else:
            for j in range(FRAMES):
                for r in check_rows:
                    assert _same(got[j, r], _want(G, form, n, U[j, r], cache, (j, r))), (form, j, r)
        assert _same(d_keys.cpu().numpy(), rows[7:9]), form                    # keep = (9, 10): the rows of steps 7 and 8
        bt.close()


def test_a_stateless_chain_and_a_null_rate_table(glvlib, oracle):
    """GLV_OP_FFT | GLV_OP_R16 [| GLV_OP_BARS] with d_ur NULL: the table call underneath, the keyframes are the transform's own rows; three launches, four with bars"""
    import torch
    G = glvlib
    n, streams = 256, 3
    S = _Session(G, n, streams, False, 309)
    twin = G.Batch(G.Params(n=n), streams, G.OP_FFT)
    rows = torch.zeros((STEPS, streams * 2, n), dtype=torch.float32, device="cuda")
    twin.track_at_s16(S.d_pcm, S.pitch, S.d_starts, STEPS, rows, torch.zeros((twin.track_at_work_bytes(STEPS, G.OP_FFT),), dtype=torch.uint8, device="cuda"), G.OP_FFT)
    torch.cuda.synchronize()
    rows = rows.cpu().numpy()
    twin.close()
    keys = _keys(n, streams, 13)
    U = Oracle.texels_r16(_lerp(keys.cpu().numpy(), rows, FROM, TO, MOD).reshape(-1, n)).reshape(FRAMES, streams * 2, n)
    for form, launches in (("texels", 3), ("pass", 4)):
        bt = _batch(G, n, streams, form)
        ops = G.OP_FFT | G.OP_R16 | (G.OP_BARS if form == "pass" else 0)
        got = S.frames(bt, FROM, TO, MOD, keys.clone(), (0, 1), ops, n, rates=False).cpu().numpy()
        assert bt.last_launches() == launches, (form, bt.last_launches())
        for j in range(FRAMES):
            for r in range(streams * 2):
                assert _same(got[j, r], _want(G, form, n, U[j, r])), (form, j, r)
        bt.close()


# ---- 3. chunk composition--------------------------------------------------------------------------------------------------------------------------------
MODIFIED = [True, False, True, True, False, False, True, False, False, False, True, True, False, True, False, False, False, False, True, False, True, False, False]
assert len(MODIFIED) == FRAMES and sum(MODIFIED) == STEPS
CUT = [j for j, m in enumerate(MODIFIED) if m][4]                                # the frame that runs step 4: chunks of 4 and 5 steps
ON = {"on": [True] * FRAMES,                                                    # a push with every update: both chunks keep (k, k')
      "late": [j >= 20 for j in range(FRAMES)]}                                 # off until the last update: the first chunk keeps (0, 1), the second (1, k)


@pytest.mark.parametrize("on", ["on", "late"])
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("n,streams", [(256, 3), (4096, 1)], ids=["n256-s3", "n4096-s1"])
def test_nine_steps_cut_as_4_and_5_at_a_frame_boundary(glvlib, n, streams, f32, on):
    G = glvlib
    S = _Session(G, n, streams, f32, 303)
    uratio = [0.4] * FRAMES
    whole = keyframe_tables(MODIFIED, ON[on], uratio)
    first = keyframe_tables(MODIFIED[:CUT], ON[on][:CUT], uratio[:CUT])
    idle = CUT - 1 - max(j for j in range(CUT) if MODIFIED[j])                  # frames without an update in front of the cut: the second chunk's kcounter
    assert idle == 3
    rest = keyframe_tables(MODIFIED[CUT:], ON[on][CUT:], uratio[CUT:], kcounter=idle)
    assert (first[3:], rest[3:], whole[3:]) == (((4, 5), (5, 6), (9, 10)) if on == "on" else ((0, 1), (1, 6), (1, 10)))
    for form in ("texels", "pass"):
        _, _, w, r16 = _forms(n)[form]
        ops = _ops(G, form, r16)
        bw, bc = _batch(G, n, streams, form), _batch(G, n, streams, form)
        kw_, kc = _keys(n, streams, 7), _keys(n, streams, 7)
        want = S.frames(bw, *whole[:3], kw_, whole[3:], ops, w)
        a = S.frames(bc, *first[:3], kc, first[3:], ops, w, steps=4)
        b = S.frames(bc, *rest[:3], kc, rest[3:], ops, w, steps=5, t0=4)
        assert eq(a, want[:CUT]) and eq(b, want[CUT:]), (form, on)
        assert eq(kc, kw_), (form, on)
        assert S.state_eq(bc, bw, ops, w), (form, on)
        bw.close(); bc.close()


# ---- 4. special values ------------------------------------------------------------------------------------------------------------------------------------
def test_special_values_in_the_recording_and_the_keyframes(glvlib, oracle):
    """Inf, NaN and -0 samples in a float recording, and in d_keys: the rows they reach, the lerp over them and the quantiser, bit for bit"""
    G = glvlib
    n, streams = 256, 3
    S = _Session(G, n, streams, True, 304)
    x = np.array(S.x, copy=True)
    last = S.starts[STEPS - 1]
    x[0, last + n - 3, 0] = np.inf; x[1, S.starts[6] + n - 2, 1] = np.nan; x[2, 5:40, :] = -0.0; x[2, S.starts[4] + 7, 0] = -np.inf
    S.set_recording(x)
    rows = S.keyframes()                                                         # (gravity keeps a NaN out of a finished row, as the reference's comparison does: the keyframes below carry one)
    k_host = _keys(n, streams, 8).cpu().numpy()
    k_host[0, 0, :8] = [-0.0, np.nan, np.inf, -np.inf, 0.0, 1.0, 2.0, -1.0]
    k_host[1, 0, :8] = [0.5, 0.5, 0.5, 0.5, -0.0, np.nan, np.inf, np.inf]
    import torch
    w_all = _lerp(k_host, rows, FROM, TO, MOD)
    U = Oracle.texels_r16(w_all.reshape(-1, n)).reshape(FRAMES, streams * 2, n)
    for form in ("texels", "pass", "maximum"):
        _, _, w, r16 = _forms(n)[form]
        bt = _batch(G, n, streams, form)
        got = S.frames(bt, FROM, TO, MOD, torch.from_numpy(k_host.copy()).cuda(), (1, 5), _ops(G, form, r16), w).cpu().numpy()
        for j in range(FRAMES):
            for r in range(streams * 2):
                assert _same(got[j, r], _want(G, form, n, U[j, r])), (form, j, r)
        bt.close()


# ---- 5. table clamping ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,streams", [(256, 3), (4096, 1)], ids=["n256-s3", "n4096-s1"])
def test_indices_beyond_the_last_keyframe_are_clamped(glvlib, n, streams):
    G = glvlib
    S = _Session(G, n, streams, False, 305)
    big = [STEPS + 2, 1000, 2 ** 31, 2 ** 32 - 1]
    frm = [big[j % 4] if j % 3 == 0 else FROM[j] for j in range(FRAMES)]
    to = [big[(j + 1) % 4] if j % 5 in (0, 3) else TO[j] for j in range(FRAMES)]
    clamp = lambda t: [min(v, STEPS + 1) for v in t]                           # noqa: E731
    assert clamp(frm) != frm and clamp(to) != to
    for form in ("texels", "bar"):
        _, _, w, r16 = _forms(n)[form]
        ops = _ops(G, form, r16)
        ba, bb = _batch(G, n, streams, form), _batch(G, n, streams, form)
        ka, kb = _keys(n, streams, 9), _keys(n, streams, 9)
        got = S.frames(ba, frm, to, MOD, ka, (2, 3), ops, w)
        want = S.frames(bb, clamp(frm), clamp(to), MOD, kb, (2, 3), ops, w)
        assert eq(got, want) and eq(ka, kb), form
        ba.close(); bb.close()


# ---- 6. launch caps ---------------------------------------------------------------------------------------------------------------------------------------
def test_more_work_items_than_the_grid_has_workgroups(glvlib, oracle):
    """n = 256, one stream, segments of one frame: 2 * 5003 work items of the frames kernel against its 8192 workgroups (glv_track_frames.hip kFramesGridCap) --
    the grid loops; the write-back's 128 lanes are below its cap at any number of frames.  That cap is crossed through streams, not frames: from 4097
    streams of n = 256 on, which tests/test_track_each_launch_geometry.py runs"""
    G = glvlib
    n, streams, frames = 256, 1, 5003
    assert 2 * frames > 256 * 32
    S = _Session(G, n, streams, False, 306)
    rows = S.keyframes()
    rng = np.random.default_rng(17)
    frm = [int(v) for v in rng.integers(0, STEPS + 2, frames)]
    to = [int(v) for v in rng.integers(0, STEPS + 2, frames)]
    mod = [float(v) for v in rng.random(frames, dtype=np.float32)]
    keys = _keys(n, streams, 10)
    k_host = keys.cpu().numpy()
    bt = _batch(G, n, streams, "texels", segment=1)
    got = S.frames(bt, frm, to, mod, keys, (0, 1), _ops(G, "texels", True), n).cpu().numpy()
    sample = sorted({0, 1, 2, 4095, 4096, 4097, frames - 2, frames - 1} | {int(v) for v in rng.integers(0, frames, 40)})
    want = Oracle.texels_r16(_lerp(k_host, rows, [frm[j] for j in sample], [to[j] for j in sample], [mod[j] for j in sample]).reshape(-1, n)).reshape(len(sample), 2, n)
    for i, j in enumerate(sample):
        assert _same(got[j], want[i]), j
    bt.close()


# ---- 7. graph capture -------------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_call_replayed_after_rewriting_d_mod(glvlib, oracle):
    """kernels only: the first frames call of a batch can be captured; the tables are read when the kernels run"""
    import torch
    G = glvlib
    n, streams = 4096, 3
    S = _Session(G, n, streams, False, 307)
    rows = S.keyframes()
    keys = _keys(n, streams, 11)
    k_host = keys.cpu().numpy()
    bt = _batch(G, n, streams, "texels")
    ops = _ops(G, "texels", True)
    work = torch.zeros((bt.track_frames_work_bytes(STEPS, FRAMES, ops),), dtype=torch.uint8, device="cuda")
    out = torch.zeros((FRAMES, streams * 2, n), dtype=torch.int16, device="cuda")
    d_from, d_to, d_mod = _dev(FROM, np.uint32), _dev(TO, np.uint32), _dev(MOD, np.float32)
    other = [float(F32(1.0) - F32(m)) for m in MOD]
    d_other = _dev(other, np.float32)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        bt.track_frames_s16(S.d_pcm, S.pitch, S.d_starts, S.d_ur, STEPS, d_from, d_to, d_mod, FRAMES, keys, (0, 1), out, work, ops, stream=s.cuda_stream)
    assert bt.last_launches() == 4
    torch.cuda.synchronize()
    assert not bool(out.any())                                                    # captured, not run
    with torch.cuda.stream(s):
        d_mod.copy_(d_other)                                                      # in stream order, in front of the replay
        g.replay()
    torch.cuda.synchronize()
    want = Oracle.texels_r16(_lerp(k_host, rows, FROM, TO, other).reshape(-1, n)).reshape(FRAMES, streams * 2, n)
    assert _same(out.cpu().numpy(), want)
    del g
    bt.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_batch_as_it_was(glvlib):
    import torch
    G = glvlib
    n, streams = 256, 3
    S = _Session(G, n, streams, False, 308)
    form = "pass"
    _, _, w, r16 = _forms(n)[form]
    ops = _ops(G, form, r16)
    bt, bs = _batch(G, n, streams, form), _batch(G, n, streams, form)
    keys = _keys(n, streams, 12)
    before = keys.clone()
    tabs = (_dev(FROM, np.uint32), _dev(TO, np.uint32), _dev(MOD, np.float32))
    work = torch.zeros((bt.track_frames_work_bytes(STEPS, FRAMES, ops) + 64,), dtype=torch.uint8, device="cuda")
    out = torch.zeros((FRAMES * streams * 2 * w + 64,), dtype=torch.int16, device="cuda")
    L = G.lib()

    def call(b=bt, pcm=S.d_pcm.data_ptr(), pitch=S.pitch, where=S.d_starts.data_ptr(), ur=S.d_ur.data_ptr(), steps=STEPS, frm=tabs[0].data_ptr(), to=tabs[1].data_ptr(),
             mod=tabs[2].data_ptr(), frames=FRAMES, d_keys=keys.data_ptr(), keep=(9, 10), fr=True, d_out=out.data_ptr(), d_work=work.data_ptr(), ops=ops):
        s = G.TrackFrames(frm, to, mod, frames, d_keys, keep[0], keep[1])
        return L.glv_batch_track_frames_s16(b._h, pcm, pitch, where, ur, steps, C.byref(s) if fr else None, d_out, d_work, ops, None)

    INVALID, STATE = G.ERR_INVALID, G.ERR_STATE
    refused = [("fr NULL", INVALID, dict(fr=False)), ("d_from NULL", INVALID, dict(frm=None)), ("d_to NULL", INVALID, dict(to=None)), ("d_mod NULL", INVALID, dict(mod=None)),
               ("d_keys NULL", INVALID, dict(d_keys=None)), ("frames 0", INVALID, dict(frames=0)), ("d_keys alignment", INVALID, dict(d_keys=keys.data_ptr() + 4)),
               ("d_from alignment", INVALID, dict(frm=tabs[0].data_ptr() + 2)), ("d_to alignment", INVALID, dict(to=tabs[1].data_ptr() + 1)),
               ("d_mod alignment", INVALID, dict(mod=tabs[2].data_ptr() + 2)),
               ("no R16 or BARS", INVALID, dict(ops=G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE)), ("WAVE", INVALID, dict(ops=G.OP_WAVE | G.OP_R16, ur=None)),
               ("rows", INVALID, dict(frames=2 ** 31 // streams + 1)),
               # the table call's own
               ("steps 0", INVALID, dict(steps=0, keep=(0, 1))), ("d_where NULL", INVALID, dict(where=None)), ("pitch", INVALID, dict(pitch=n - 1)),
               ("d_ur alignment", INVALID, dict(ur=S.d_ur.data_ptr() + 2)), ("rates without gravity", INVALID, dict(ops=G.OP_FFT | G.OP_AVERAGE | G.OP_BARS | G.OP_R16)),
               ("d_pcm NULL", INVALID, dict(pcm=None)), ("d_out NULL", INVALID, dict(d_out=None)), ("d_work alignment", INVALID, dict(d_work=work.data_ptr() + 64)),
               ("RAW", INVALID, dict(ops=ops | G.OP_RAW))]
    for kf, kt in ((1, 0), (0, 0), (0, 2), (1, 1), (2, 2), (3, 2), (2, 1), (1, STEPS + 2), (2, STEPS + 2), (STEPS + 1, STEPS + 2), (0, 2 ** 32 - 1)):
        refused.append(("keep %d %d" % (kf, kt), INVALID, dict(keep=(kf, kt))))
    for name, code, kw in refused:
        assert call(**kw) == code, (name, L.glv_last_error().decode())
        assert L.glv_last_error().decode(), name
    # any gl_storage but 3, and state the batch was not created with
    for storage in (0, 1):
        other = G.Batch(G.Params(n=n, avg_frames=F, gl_storage=storage, bars=n, bar_phase=0.5), streams, G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS)
        assert call(b=other, ops=G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_R16) == STATE, storage
        with pytest.raises(G.GlvError) as ei:
            other.track_frames_work_bytes(STEPS, FRAMES, G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_R16)
        assert ei.value.code == STATE
        other.close()
    gravity_only = G.Batch(G.Params(n=n, avg_frames=F, gl_storage=G.GL_STORAGE_UPLOAD, bars=n, bar_phase=0.5), streams, G.OP_GRAVITY | G.OP_BARS)
    assert call(b=gravity_only) == STATE
    gravity_only.close()
    for bad in (dict(steps=0), dict(frames=0), dict(ops=G.OP_FFT | G.OP_GRAVITY), dict(ops=G.OP_WAVE | G.OP_R16)):
        with pytest.raises(G.GlvError) as ei:
            bt.track_frames_work_bytes(**dict(dict(steps=STEPS, frames=FRAMES, ops=ops), **bad))
        assert ei.value.code == INVALID, bad
    torch.cuda.synchronize()
    assert eq(keys, before) and not bool(out.any()) and not bool(work.any())      # nothing was launched
    # ... and the batch is where a batch that saw none of it is: the accepted pairs (1, k) and (k, k') run, output, keyframes and state agree
    k2 = before.clone()
    got = S.frames(bt, FROM, TO, MOD, keys, (1, STEPS + 1), ops, w)
    want = S.frames(bs, FROM, TO, MOD, k2, (1, STEPS + 1), ops, w)
    assert eq(got, want) and eq(keys, k2) and S.state_eq(bt, bs, ops, w)
    bt.close(); bs.close()
