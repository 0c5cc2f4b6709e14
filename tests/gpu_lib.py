"""Helpers shared by several GPU test files: a plain module, like oracle_lib.py and src_scan.py (default collection does not pick it up; torch is imported
inside the functions, as in the tests).  A test file imports what it shares with another from here or from track_lib.py, never from that file."""
import ctypes as C

import numpy as np

from oracle_lib import Oracle, Ref, lcg_pcm_fast

F32 = np.float32
# (n, kernel configuration): every size and every configuration the frame kernel is built for
SIZES = [(256, 0)] + [(n, v) for n in (512, 1024, 2048, 4096, 8192, 16384, 32768) for v in (0, 1)]


# ---- bit equality ---------------------------------------------------------------------------------------------------------------------------------
def eq(a, b):
    """two device tensors, bit for bit: float32 compared as int32"""
    import torch
    ia = a.view(torch.int32) if a.dtype == torch.float32 else a
    ib = b.view(torch.int32) if b.dtype == torch.float32 else b
    return bool(torch.equal(ia, ib))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the wave bind's models (tests/test_wave.py, tests/test_track_wave.py) ------------------------------------------------------------------------------
def wrange(x, use_ref=False):
    """transform_wrange (render.c:773-781) of every row of x through the oracle, or through the compiled reference"""
    import ctypes as C
    x = np.array(x, dtype=np.float32, copy=True)
    flat = x.reshape(-1, x.shape[-1])
    for i in range(flat.shape[0]):
        row = np.ascontiguousarray(flat[i])
        if use_ref:
            p = Ref.params()
            Ref.lib().glvref_wrange(C.byref(p), row, row.size)
        else:
            Oracle.lib().glvo_wrange(row, row.size)
        flat[i] = row
    return x


def upload(planar):
    """the GL_R16 texels of the wave bind for planar rows [rows][n] (already unpacked): wrange, then the upload rounding"""
    return Oracle.texels_r16(wrange(planar))


def texel_floats(c):
    return (c.astype(np.float64) / 65535).astype(np.float32)


def planar_of_s16(pcm, streams, n, channels=2):
    rows = np.empty((streams * 2, n), np.float32)
    for s in range(streams):
        rows[2 * s], rows[2 * s + 1] = Oracle.unpack_s16(pcm[s * 2 * n:(s + 1) * 2 * n], channels)
    return rows


def texel_bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint16)


def same(got, want):
    return texel_bits(got).shape == texel_bits(want).shape and bool((texel_bits(got) == texel_bits(want)).all())


# ---- one update of every input kind, and the creation mask it needs (tests/test_snapped_bars.py, tests/test_column_texels.py) -------------------------------
def update_inputs(kind, streams, n, fr):
    """(method, input tensor, extra args) of one update of input kind `kind`"""
    import torch
    div = (1, 8, 64)[fr % 3]
    pcm = (lcg_pcm_fast(9100 + fr + n, streams * 2 * n) // div).astype(np.int16)
    if kind == "s16":
        return "process_s16", torch.from_numpy(pcm).cuda(), ()
    f = torch.from_numpy(pcm.astype(np.float32) / np.float32(32768)).cuda()
    if kind == "f32":
        return "process_f32", f.reshape(streams * 2, n).contiguous(), ()
    if kind == "f32_stereo":
        return "process_f32_stereo", f, ()
    new = 256                                                       # ring updates: 256 new stereo frames per stream
    if kind == "ring_s16":
        return "ring_update_s16", torch.from_numpy(pcm[: streams * new * 2].copy()).cuda(), (new,)
    return "ring_update_f32", f[: streams * new * 2].contiguous(), (new,)


def bars_mask(G, kind, bars_only):
    m = G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS
    if bars_only: m |= G.OP_BARS_ONLY
    if kind == "ring_s16": m |= G.OP_RING_S16
    if kind == "ring_f32": m |= G.OP_RING_F32
    return m


# ---- the oracle's bars under a shape (tests/test_smooth_shape.py, tests/test_knob_changes.py) ---------------------------------------------------------------
def oracle_bars(row, bars, factor, phase, shape, chunked=False):
    """the oracle's smooth_audio() of one float row under `shape` = (round_formula, sample_mode, hybrid_weight, scale, range)"""
    formula, mode, hw, scale, rng = shape
    with Oracle.smooth_shape(formula, scale, rng):
        if mode:
            return Oracle.bars_mode(row, bars, mode, hw or 0.65, factor, phase)
        out = np.empty(bars, np.float32)
        (Oracle.lib().glvo_bars_chunked_at if chunked else Oracle.lib().glvo_bars_at)(np.ascontiguousarray(row, np.float32), row.size, out, bars, factor, phase)
        return out


# ---- the knob schedules (tests/test_knob_changes_host.py pins the oracle to the compiled reference under them, tests/test_knob_changes.py the device) --------
def updates_of(F):
    return 2 * F + 4


def float_schedule(updates, seed=2387):
    """one dict of knobs per update for the float chains.  `ur` and `gravity_step` differ on every update (seeded); fixed positions carry the edge steps --
    update 1: ur = 0 (the step is +inf, the output -inf; update 2 recovers), 3: gravity_step = 0, 4: a negative step (values rise), 5: a step larger than
    any magnitude; fft_scale / fft_cutoff change at update 2 and at the last but one; avg_window is switched off at update 3 (and on again at update 9 of
    schedules that long); channels go 2 -> 1 -> 2 every six updates.  A prefix of a longer schedule is the shorter schedule."""
    assert updates >= 6
    rng = np.random.default_rng(seed)
    out, scale, cutoff, window = [], 10.2, 0.3, True
    for u in range(updates):
        ur = float(F32(rng.uniform(40.0, 160.0)))
        step = float(F32(rng.uniform(0.5, 9.0)))
        if u == 1: ur = 0.0
        if u == 3: step = 0.0
        if u == 4: step = -step
        if u == 5: step = 1.0e4
        if u == 2: scale, cutoff = 6.5, 0.55
        if u == updates - 2: scale, cutoff = 14.0, 0.125
        if u == 3: window = False
        if u == 9: window = True
        out.append(dict(ur=ur, gravity_step=step, fft_scale=scale, fft_cutoff=cutoff, avg_window=window, channels=1 if u % 6 in (2, 3) else 2))
    return out


# the first six updates of the GL schedule: every kind of step, in an order that goes integer -> float -> integer and shows the recovery from ur = 0
_GL_HEAD = [
    dict(gravity_step=4.2, ur=86.1328125),                       # the shipped step: integer, D = 3196
    dict(gravity_step=float(F32(100.5) / F32(65535)), ur=1.0),   # g * 65535 = 100.5: float rounding decides texel by texel
    dict(gravity_step=1.7, ur=61.0),                             # integer, another D
    dict(gravity_step=4.2, ur=0.0),                              # +inf: every texel falls to 0
    dict(gravity_step=-0.9, ur=75.0),                            # g < 0: values rise, evaluated in float
    dict(gravity_step=150.0, ur=60.0),                           # g = 2.5: larger than any texel
]


def gl_schedule(updates, seed=728):
    """one dict per update for the GL_R16 chains: (gravity_step, ur) from _GL_HEAD, then seeded -- every third of those at a half-integer of g * 65535;
    avg_window off at updates 2 and 3 (and 8); the tilt (fft_scale, fft_cutoff) changes at updates 1 and 4 (and 9)"""
    assert updates >= len(_GL_HEAD)
    rng = np.random.default_rng(seed)
    out, scale, cutoff = [], 10.2, 0.3
    for u in range(updates):
        if u < len(_GL_HEAD): k = dict(_GL_HEAD[u])
        else:
            k = dict(gravity_step=float(F32(rng.uniform(0.3, 9.0))), ur=float(F32(rng.uniform(40.0, 160.0))))
            if u % 3 == 1: k = dict(gravity_step=float(F32(int(rng.integers(50, 4000)) + 0.5) / F32(65535)), ur=1.0)
        if u == 1: scale, cutoff = 7.0, 0.5
        if u == 4: scale, cutoff = 12.5, 0.2
        if u == 9: scale, cutoff = 10.2, 0.3
        out.append(dict(k, fft_scale=scale, fft_cutoff=cutoff, avg_window=u not in (2, 3, 8)))
    return out


# ---- what the files that change parameters between updates share (tests/test_knob_changes.py, tests/test_live_bins_changes.py) ------------------------------
KNOBS = ("ur", "gravity_step", "fft_scale", "fft_cutoff", "avg_window", "channels", "avg_window_kind")


def knob_params(G, base, k, **more):
    return G.Params(**{**base, **{key: v for key, v in k.items() if key in KNOBS}, **more})


def frames(seed, u, streams, n, levels=(1, 8, 64)):
    """int16 [streams][n][2] of update u: every stream at a level of its own, which moves from update to update"""
    x = lcg_pcm_fast(seed + 31 * u, streams * n * 2).reshape(streams, n, 2).copy()
    for s in range(streams):
        x[s] //= levels[(s + u) % len(levels)]
    return x


def nan_rows(rows, w):
    import torch
    return torch.full((rows, w), float("nan"), dtype=torch.float32, device="cuda")


def texel_rows(rows, w):
    import torch
    return torch.full((rows, w), -1, dtype=torch.int16, device="cuda")


def u16(t):
    return t.cpu().numpy().view(np.uint16)


def refused(G, b, p, code):
    import pytest
    with pytest.raises(G.GlvError) as ei:
        b.set_params(p)
    assert ei.value.code == code, (ei.value.code, str(ei.value))


class GLModel:
    """the oracle's model of the GL passes for `rows` channel rows: transform_fft + glvo_gl_chain_r16 with each update's knobs, on float arrays of texel values"""

    def __init__(self, rows, n, F, average):
        self.n, self.F, self.average = n, F, average
        self.store = np.zeros((rows, n), np.float32); self.hist = np.zeros((rows, F, n), np.float32)
        self.heads = [C.c_size_t(0) for _ in range(rows)]

    def row(self, r, samples, k):
        """row r one update further on n float samples -> its GL_R16 texels"""
        want = Oracle.transform_fft(samples, k["fft_scale"], k["fft_cutoff"])
        Oracle.lib().glvo_gl_chain_r16(want, self.store[r], self.hist[r], C.byref(self.heads[r]), self.n, self.F, int(k["avg_window"]), int(self.average),
                                       k["gravity_step"], k["ur"])
        return Oracle.texels_r16(want)

    def update(self, x, k):
        """every row one update further on int16 [streams][n][2] -> texels [streams * 2][n]"""
        out = np.empty((2 * len(x), self.n), np.uint16)
        for s in range(len(x)):
            for c, samples in enumerate(Oracle.unpack_s16(x[s], 2)):
                out[2 * s + c] = self.row(2 * s + c, samples, k)
        return out
