"""GPU: the per-stream, pool and render-frame track calls past every launch cap -- and their lockstep frames and table siblings, which no large batch had run.

tests/test_track_launch_geometry.py drives the hop entries at 3457 streams; the entries below were added after it and their contract tests run 3 to 7 streams, so
every grid-stride loop behind them took one trip under test.  Here only the stream count is large; n = 256, steps and frames stay in single digits:

    SPEC   4100 streams   the FFT chains: 2 * 4100 * 64 = 524 800 quads of the frames calls' write-back against 2048 x 256 lanes (the second trip begins exactly
                          at stream 4096); 3 steps under bufscale 2 are 12 300 windows against the 8192 of one decimation trip (window 8192 lies in stream
                          2730); 8200 channel rows are 8200 work items of a segment of the frames kernels against 8192 workgroups
    WAVE   8200 streams   the wave module: 8200 * 64 = 524 800 quads of its write-backs (the second trip begins at stream 8192); 3 steps are 24 600 windows x 32
                          groups of 8 frames against 524 288 lanes of the waveform kernels, and in front of the bars (64 bins at the least) 9 steps are 73 800
                          windows x 8 groups; 8200 work items of a segment of the frames kernels

Which case takes which kernel past which cap (kGridCap and kDecimateGridCap: 2048 workgroups of 256 lanes; kFramesGridCap: 8192 workgroups of one item):
    glv_track_keys_kernel                       kGridCap           test_frames_lockstep_at_spec
    glv_track_keys_each_kernel                  kGridCap           test_frames_per_stream_at_spec
    glv_wave_keys_kernel<s16 | f32>, glv_wave_keys_planar_kernel        kGridCap           test_wave_frames_lockstep_at_wave
    glv_wave_keys_each_kernel<KIND, POOL>       kGridCap           test_wave_frames_per_stream_at_wave
    glv_track_frames_kernel                     kFramesGridCap     test_frames_lockstep_at_spec (rest % units up to 8199, two segments)
    glv_track_frames_each_kernel                kFramesGridCap     test_frames_per_stream_at_spec
    glv_wave_frames_kernel, glv_wave_frames_planar_kernel               kFramesGridCap     test_wave_frames_lockstep_at_wave (rest % streams up to 8199)
    glv_wave_frames_each_kernel                 kFramesGridCap     test_wave_frames_per_stream_at_wave
    glv_decimate_kernel, a table row per stream kDecimateGridCap   test_frames_per_stream_at_spec[each-*-bufscale2], test_updates_per_stream_at_spec[each-*-bufscale2]
    glv_decimate_kernel, one table row          kDecimateGridCap   test_shared_tables_at_spec
    glv_decimate_pool_kernel<3 kinds>           kDecimateGridCap   test_updates_per_stream_at_spec[pool-*-bufscale2], test_frames_per_stream_at_spec[pool-*-bufscale2]
    glv_wave_kernel kinds 3, 4, 5, a row per stream                     kGridCap           test_wave_updates_per_stream_at_wave[each-*]
    glv_wave_pool_kernel<3 kinds, R16 | float>  kGridCap           test_wave_updates_per_stream_at_wave[pool-*]
    glv_track_each_scan_kernel, glv_bars_rows_i8_kernel behind it       (8200 rows of a step, 24 600 in all: 385 blocks of 64 rows)   test_updates_per_stream_at_spec

Checkers, everything == on bits (floats as int32), no tolerance anywhere.  The wave forms are checked WHOLE against the numpy restatement of the contract modules
(rows_each, lerp_each, Oracle.texels_r16, keep_each): every stream, frame and sample, and all of d_keys.  The spectrum forms are compared with the same entry on
batches of 6 streams fed exactly the large call's inputs for those streams -- the first six, the last six, the six that straddle the write-back's trip boundary and
the six around the decimation boundary -- through every step's or frame's rows, the rows of d_keys and one more update of both sides (the contract tests pin those
small calls to one-stream twins and the oracle); in addition the frames forms' whole write-back is held to keep_each and their whole texel output to lerp_each over
the step rows the call left in its workspace.  One stream's inputs are planted on both sides of every boundary: the copies' results equal the source's.  Every
per-stream input is a function of the stream index with a period that does not divide 4096 (tests/track_geometry_lib.py); behind every count the tables hold
0xFFFFFFFF and NaN; every test asserts that the two streams on either side of each trip boundary differ in output and in kept keyframes, so a read of the
neighbour's row cannot pass.  Recordings begin one frame (planar: one float) behind a load boundary and both load forms occur (asserted).  Every call gets a
workspace of exactly the queried size and an output of exactly the documented size, a guard behind each."""
import numpy as np
import pytest

from gpu_lib import eq, same, texel_floats
from oracle_lib import Oracle
from test_track_each import _chain, _dev_u32, _dev_ur, _each, _make, _process, _shared
from test_track_frames import F, _batch as _spec_batch, _forms as _spec_forms, _lerp, _ops as _spec_ops, _same
from test_track_frames_each import KNAME, _Each, _device, _layout
from test_track_pool import _pool_call
from test_track_wave_frames import _batch as _wave_batch, _forms as _wave_forms, _launches as _wave_launches
from test_track_wave_frames_each import ELEMENT, _Wave, _lockstep as _wave_lockstep
from test_track_wave_frames_host import np_keyframes
from track_frames_each_lib import keep_each, lerp_each
from track_geometry_lib import (BIG, FLOAT_RATES, FRAMES_LANES, K_DECIMATE_GRID_CAP, K_FRAMES_GRID_CAP, K_GRID_CAP, LANES, N, ROWS_PER_BLOCK, SEGMENT, SMALL, SOURCE, SPEC,
                                SPEC_COPIES, SPEC_FRAMES, SPEC_STEPS, TEXEL_RATES, WAVE, WAVE_BARS_STEPS, WAVE_COPIES, WAVE_GROUP, WAVE_LIMIT_MIN, WAVE_STEPS, counts_of,
                                decimate_boundary_stream, frame_counts_of, frame_tables_of, keep_of, keys_of, plant, rates_of, recording, rows_of, small_batches,
                                spans_of, starts_of)
from track_lib import GUARD, differing, out_dtype, rec
from track_rates_lib import FLOAT_STEP, TEXEL_STEP
from track_wave_frames_each_lib import each_starts, pool_starts

gpu = pytest.mark.gpu
F32 = np.float32
KINDS = ["s16", "f32", "planar"]
QUADS = N // 4                                   # work items of a row in the write-backs, of a window in the decimation
TRIP = K_GRID_CAP * LANES                        # work items of one trip of a capped grid of 256-lane workgroups
SPEC_BOUNDARY, WAVE_BOUNDARY = 4096, 8192        # the stream with which the write-backs' second trip begins
POOL_FRAMES = 4001                               # one small pool: odd, so that the planar pool's second row is 4-byte aligned and no more
WAVE_BARS_WINDOW = TRIP // (WAVE_LIMIT_MIN // WAVE_GROUP)                      # the step-major window with which the waveform's second trip begins in front of the bars


# ---- the caps against the shapes: no GPU work ----------------------------------------------------------------------------------------------------------------------
def test_the_large_calls_lie_beyond_every_cap_and_the_small_ones_below():
    assert K_GRID_CAP == K_DECIMATE_GRID_CAP == 2048 and K_FRAMES_GRID_CAP == 8192 and TRIP == 524288
    # SPEC: the write-back of the spectrum frames calls, quads = units * n / 4, a stream is 2 * n / 4 of them: the second trip begins with a whole stream
    assert 2 * SPEC * QUADS == 524800 > TRIP and TRIP % (2 * QUADS) == 0 and TRIP // (2 * QUADS) == SPEC_BOUNDARY < SPEC
    # ... the decimation: items = windows * n / 4 in [stream][step] order
    assert SPEC * SPEC_STEPS == 12300 > K_DECIMATE_GRID_CAP * LANES // QUADS == 8192
    d = decimate_boundary_stream(SPEC_STEPS)
    assert d == 2730 and d * SPEC_STEPS <= 8192 < (d + 1) * SPEC_STEPS and 8192 % SPEC_STEPS != 0      # ... window 8192 is step 2 of stream 2730: a stream is cut
    # ... the frames kernels: items = segments * units * groups, one wave of 64 lanes x 4 bins a row of n = 256
    groups = -(-(N // 4) // FRAMES_LANES)
    segments = -(-SPEC_FRAMES // SEGMENT)
    assert groups == 1 and segments == 2 and SPEC_FRAMES % SEGMENT != 0 and 2 * SPEC * groups == 8200 > K_FRAMES_GRID_CAP
    # ... the bars behind the per-stream calls: rows of all steps, blocks of 64 of them, some of them the zero rows behind a count
    assert SPEC_STEPS * SPEC * 2 == 24600 > K_GRID_CAP and -(-24600 // ROWS_PER_BLOCK) == 385
    # WAVE: the write-back of the wave frames calls, quads = streams * n / 4 (a lane takes both channel rows)
    assert WAVE * QUADS == 524800 > TRIP and TRIP // QUADS == WAVE_BOUNDARY < WAVE and TRIP % QUADS == 0
    assert WAVE * WAVE_STEPS * (N // WAVE_GROUP) == 24600 * 32 > TRIP                                   # the waveform kernels without bars
    assert WAVE * WAVE_BARS_STEPS * (WAVE_LIMIT_MIN // WAVE_GROUP) == 73800 * 8 > TRIP                  # ... and in front of the bars, at the least their limit can be
    assert WAVE_BARS_WINDOW == 65536 and WAVE_BARS_WINDOW // WAVE == 7 and WAVE_BARS_WINDOW % WAVE == 8136      # step 7, stream 8136
    assert WAVE * groups == 8200 > K_FRAMES_GRID_CAP
    # the small batches lie under every cap
    assert 2 * SMALL * QUADS < TRIP and SMALL * WAVE_BARS_STEPS * QUADS < TRIP and SMALL * WAVE_BARS_STEPS * (N // WAVE_GROUP) < TRIP
    assert segments * 2 * SMALL * groups < K_FRAMES_GRID_CAP and SMALL * WAVE_BARS_STEPS * 2 <= ROWS_PER_BLOCK * 2
    # ... and where they lie: the ends, the six that straddle the write-back's boundary, the six around the decimation boundary
    assert small_batches(SPEC, SPEC_BOUNDARY) == (0, 4094, 4093, 2727) and small_batches(WAVE, WAVE_BOUNDARY) == (0, 8194, 8189, 2727)
    for s0, streams in [(s0, SPEC) for s0 in small_batches(SPEC, SPEC_BOUNDARY)] + [(s0, WAVE) for s0 in small_batches(WAVE, WAVE_BOUNDARY)] + [(8136 - 3, WAVE)]:
        assert 0 <= s0 and s0 + SMALL <= streams
    assert 4093 <= SPEC_BOUNDARY - 1 and SPEC_BOUNDARY < 4093 + SMALL and 2727 <= d < 2727 + SMALL and 8189 < WAVE_BOUNDARY < 8189 + SMALL
    # the planted copies: on both sides of every boundary, never a boundary's own two streams
    for copies, streams, marks in ((SPEC_COPIES, SPEC, (2048, d, SPEC_BOUNDARY)), (WAVE_COPIES, WAVE, (d, 4096, WAVE_BOUNDARY))):
        for m in marks:
            assert any(c < m - 1 for c in copies if c >= m - 3) and any(c > m for c in copies if c <= m + 2), m
            assert m - 1 not in copies and m not in copies
        assert all(SOURCE < c < streams for c in copies) and SOURCE >= SMALL
        assert counts_of(np.asarray([SOURCE]), SPEC_STEPS)[0] == SPEC_STEPS and frame_counts_of(np.asarray([SOURCE]), SPEC_FRAMES)[0] == SPEC_FRAMES
    # the variety: both streams of every boundary pair run steps, show frames and are handed different rows of everything
    for streams, copies, steps, marks in ((SPEC, SPEC_COPIES, SPEC_STEPS, (SPEC_BOUNDARY, d)), (WAVE, WAVE_COPIES, WAVE_STEPS, (WAVE_BOUNDARY,))):
        idx = plant(streams, copies)
        counts, fcounts, keep = counts_of(idx, steps), frame_counts_of(idx, SPEC_FRAMES), keep_of(idx, steps)
        frm, to, mod = frame_tables_of(idx, steps, SPEC_FRAMES)
        starts = starts_of(idx, steps, 300)
        assert {0, steps}.issubset(set(counts.tolist())) and counts.max() > steps and {0, SPEC_FRAMES}.issubset(set(fcounts.tolist())) and fcounts.max() > SPEC_FRAMES
        assert (keep.astype(np.int64).max(axis=1) > np.minimum(counts, steps).astype(np.int64) + 1).any() and (keep == BIG).any() and (starts > 300).any()
        for m in marks:
            a, b = m - 1, m
            assert counts[a] != counts[b] and fcounts[a] != fcounts[b] and fcounts[a] >= 1 and fcounts[b] >= 1
            assert (keep[a] != keep[b]).any() and (frm[a] != frm[b]).any() and (to[a] != to[b]).any() and (mod[a] != mod[b]).any() and (starts[a] != starts[b]).any()
        for c in copies:
            assert counts[c] == counts[SOURCE] and (frm[c] == frm[SOURCE]).all() and (starts[c] == starts[SOURCE]).all() and (keep[c] == keep[SOURCE]).all()


# ---- what every case asserts of its results --------------------------------------------------------------------------------------------------------------------------
def _neighbours_differ(x, boundaries, what):
    """x [..][streams * 2][w], tensor or array: the rows of the two streams on either side of each boundary differ"""
    for m in boundaries:
        a, b = rows_of(x, m - 1, 1), rows_of(x, m, 1)
        agree = eq(a.contiguous(), b.contiguous()) if hasattr(x, "is_cuda") else same(a, b)
        assert not agree, (*what, "streams", m - 1, "and", m, "agree")


def _copies_are_the_source(x, copies, what):
    src = rows_of(x, SOURCE, 1)
    for c in copies:
        mine = rows_of(x, c, 1)
        agree = eq(mine.contiguous(), src.contiguous()) if hasattr(x, "is_cuda") else same(mine, src)
        assert agree, (*what, "copy", c)


def _loads_of_both_forms(d_pcm, frames_in, kind):
    """frames_in: the absolute first frame (planar: float) of every window in the buffer -- groups that take the wide loads, and groups that do not"""
    at = {int(v) for v in np.unique((d_pcm.data_ptr() + np.asarray(frames_in, dtype=np.int64).reshape(-1) * ELEMENT[kind]) % 16)}
    assert 0 in at and len(at) > 1, at


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _spans_device(spans):
    import torch
    from glava_amd.track_starts import SPAN_DTYPE
    a = np.zeros((len(spans) + 1,), dtype=np.dtype(SPAN_DTYPE))
    a["first"][:-1] = [first for first, _ in spans]
    a["frames"][:-1] = [frames for _, frames in spans]
    a["reserved"][:-1] = 0xDEADBEEF
    a[-1] = (0xFFFFFFFFFFFFFFF0, 0xFFFFFFFF, 0)                                  # one record behind the last stream: never read
    t = torch.from_numpy(a.view(np.int32).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


# ---- the wave module: recordings or a pool for 8200 streams, made once ---------------------------------------------------------------------------------------------
class _BigWave(_Wave):
    """test_track_wave_frames_each._Wave with every stream's recording (or span), starts and planted copies from tests/track_geometry_lib.py; `call`, `tables`, `head`
    and `keyframes` are _Wave's"""

    def __init__(self, G, kind, pool, channels, steps, seed=601):
        idx = plant(WAVE, WAVE_COPIES)
        self.G, self.n, self.kind, self.pool, self.streams, self.steps, self.idx = G, N, kind, pool, WAVE, steps, idx
        self.f32 = kind != "s16"
        self.channels = 2 if kind == "planar" else channels
        if pool:
            self.pool_frames = POOL_FRAMES
            self.spans = spans_of(idx, POOL_FRAMES, N)
            self.starts = starts_of(idx, steps, N + 700)
            self.x = rec(seed, 1, POOL_FRAMES, self.f32)[0]                       # [pool_frames][2]
            self.d_pcm = _device(np.ascontiguousarray(self.x.T) if kind == "planar" else self.x, kind, 2 * N)
            self.d_spans = _spans_device(self.spans)
            self.where = pool_starts(self.spans, self.starts, POOL_FRAMES, N)
            self.recordings = [self.x] * WAVE
            assert int(self.where.max()) == POOL_FRAMES - N and len({tuple(s) for s in self.spans}) == 8      # a few clamp to the pool's last window; two share a span
            _loads_of_both_forms(self.d_pcm, self.where, kind)
        else:
            self.pitch = (N + 300) | 1
            self.starts = starts_of(idx, steps, self.pitch - N)
            self.x = recording(seed, idx, self.pitch, self.f32)                   # [streams][pitch][2]
            self.d_pcm = _device(_layout(self.x, kind), kind, 2 * N)
            self.where = each_starts(self.starts, self.pitch, N)
            self.recordings = list(self.x)
            assert (self.where != self.starts).any()                              # entries beyond the last window of a recording: they clamp
            rows = 2 if kind == "planar" else 1
            _loads_of_both_forms(self.d_pcm, np.arange(WAVE, dtype=np.int64)[:, None] * rows * self.pitch + self.where, kind)
        self.made = {}

    def reference(self, key, make):
        """numpy results that several forms of one case share, made once"""
        if key not in self.made: self.made[key] = make()
        return self.made[key]


@pytest.fixture(scope="module")
def waves(glvlib):
    """(kind, pool, channels, steps) -> _BigWave, each made once and freed with the module"""
    made = {}

    def get(kind, pool=False, channels=2, steps=WAVE_STEPS):
        key = (kind, pool, channels, steps)
        if key not in made: made[key] = _BigWave(glvlib, kind, pool, channels, steps)
        return made[key]
    yield get
    made.clear()


# ---- 5. glv_batch_track_wave_frames_*: lockstep ----------------------------------------------------------------------------------------------------------------------
WAVE_ROW = dict(starts=[5, 0xFFFFFFF0, 133], frm=[0, 1, 2, 4, 3, BIG, 2], to=[1, 2, 3, 4, 0, 3, 2], mod=[0.25, 0.59310347, 1.0, 0.0, 0.5, 0.125, 0.75], keep=(3, 4))


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_wave_frames_lockstep_at_wave(glvlib, oracle, waves, kind):
    """glv_wave_frames_kernel / _planar_kernel over 8200 streams x 2 segments (rest % streams up to 8199, rest / streams = 1), glv_wave_keys_kernel / _planar_kernel
    over 524 800 quads: texels and floats, whole, against numpy"""
    G = glvlib
    S = waves(kind)
    T = WAVE_ROW
    kh = keys_of(S.idx, N, 71)
    clamped = [G.track_at_start(S.pitch, N, a) for a in T["starts"]]
    assert clamped[1] == S.pitch - N
    rows = np_keyframes(S.x, clamped, N, S.f32, S.channels)
    wl = _lerp(kh, rows, T["frm"], T["to"], T["mod"], WAVE_STEPS)
    U = Oracle.texels_r16(wl.reshape(-1, N)).reshape(len(T["frm"]), WAVE * 2, N)
    kept = np.stack([rows[k - 2] for k in T["keep"]])
    for form in ("texels", "floats"):
        _, _, w, ops = _wave_forms(G, N)[form]
        b = _wave_batch(G, N, WAVE, form, segment=SEGMENT)
        keys = _cuda(kh)
        got = _wave_lockstep(G, b, kind, S.d_pcm, S.pitch, T["starts"], WAVE_STEPS, T["frm"], T["to"], T["mod"], keys, T["keep"], ops, w)
        assert b.last_launches() == _wave_launches(ops, G) == 2 and b.kernel_name() == "glv_wave_frames_kernel", (form, b.last_launches(), b.kernel_name())
        got = got.cpu().numpy()
        assert _same(got, U if form == "texels" else texel_floats(U)), (kind, form)
        assert _same(keys.cpu().numpy(), kept), (kind, form, "d_keys")
        _neighbours_differ(got, (WAVE_BOUNDARY,), (kind, form)); _neighbours_differ(keys, (WAVE_BOUNDARY,), (kind, form, "d_keys"))
        _copies_are_the_source(got, WAVE_COPIES, (kind, form)); _copies_are_the_source(keys, WAVE_COPIES, (kind, form, "d_keys"))
        b.close()


# ---- 6. glv_batch_track_each_wave_frames_* / glv_batch_track_pool_wave_frames_* ----------------------------------------------------------------------------------------
WAVE_EACH = [(k, p, 2, False) for p in (False, True) for k in KINDS] + [("s16", False, 1, False), ("f32", True, 1, False), ("s16", True, 2, True), ("planar", False, 2, True)]


@gpu
@pytest.mark.parametrize("kind,pool,channels,null", WAVE_EACH,
                         ids=["%s-%s%s%s" % ("pool" if p else "each", k, "-mono" if c == 1 else "", "-null-counts" if z else "") for k, p, c, z in WAVE_EACH])
def test_wave_frames_per_stream_at_wave(glvlib, oracle, waves, kind, pool, channels, null):
    """glv_wave_frames_each_kernel over 2 x 8200 work items and glv_wave_keys_each_kernel over 524 800 quads, each stream with its own starts, tables, counts and
    keep pair (null: d_counts and d_frame_counts NULL, every stream takes all): texels and floats, whole, against numpy"""
    G = glvlib
    S = waves(kind, pool, channels)
    idx, steps, frames = S.idx, WAVE_STEPS, SPEC_FRAMES
    counts, fcounts = (None, None) if null else (counts_of(idx, steps), frame_counts_of(idx, frames))
    keep = keep_of(idx, steps)
    frm, to, mod = frame_tables_of(idx, steps, frames, fcounts)
    kh = keys_of(idx, N, 72)

    def reference():
        rows = S.keyframes(counts)
        wl, shown = lerp_each(kh, rows, frm, to, mod, counts, fcounts, steps)
        if not null: assert not shown.all() and shown[0].sum() == (np.minimum(fcounts, frames) >= 1).sum()
        return Oracle.texels_r16(wl.reshape(-1, N)).reshape(frames, WAVE * 2, N), keep_each(kh, rows, keep, counts, steps)
    U, kept = S.reference(("frames", null), reference)
    for form in ("texels", "floats"):
        _, _, w, ops = _wave_forms(G, N)[form]
        b = _wave_batch(G, N, WAVE, form, channels, segment=SEGMENT)
        keys = _cuda(kh)
        got = S.call(b, S.tables(counts), (frm, to, mod, fcounts, keep), keys, ops, w)
        assert b.last_launches() == 2 and b.kernel_name() == "glv_wave_frames_each_kernel", (form, b.last_launches(), b.kernel_name())
        got = got.cpu().numpy()
        assert _same(got, U if form == "texels" else texel_floats(U)), (kind, pool, form)      # (a frame not shown: zero texels, which U holds for w = 0)
        assert _same(keys.cpu().numpy(), kept), (kind, pool, form, "d_keys")
        _neighbours_differ(got, (WAVE_BOUNDARY,), (kind, form)); _neighbours_differ(keys, (WAVE_BOUNDARY,), (kind, form, "d_keys"))
        _copies_are_the_source(got, WAVE_COPIES, (kind, form)); _copies_are_the_source(keys, WAVE_COPIES, (kind, form, "d_keys"))
        b.close()


# ---- 7. the wave form of glv_batch_track_each_* / glv_batch_track_pool_* -------------------------------------------------------------------------------------------------
def _wave_updates(S, b, d_starts, steps, ops, dt):
    if S.pool: return _pool_call(b, S.kind, S.d_pcm, S.pool_frames, S.d_spans, d_starts, None, None, steps, ops, N, dt)
    return _each(b, S.kind, S.d_pcm, S.pitch, d_starts, None, None, steps, ops, N, dt)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pool", [False, True], ids=["each", "pool"])
def test_wave_updates_per_stream_at_wave(glvlib, oracle, waves, pool, kind):
    """GLV_OP_WAVE [| GLV_OP_R16], 3 steps: 24 600 windows x 32 groups over glv_wave_kernel's kinds 3 / 4 / 5 with a row of starts per stream, or over
    glv_wave_pool_kernel -- one launch, whole, against numpy"""
    G = glvlib
    S = waves(kind, pool)
    steps = WAVE_STEPS
    U = S.reference("updates", lambda: Oracle.texels_r16(S.keyframes(None).reshape(-1, N)).reshape(steps, WAVE * 2, N))
    for r16 in (True, False):
        ops = G.OP_WAVE | (G.OP_R16 if r16 else 0)
        b = G.Batch(G.Params(n=N, gl_storage=1, bars=N, bar_phase=0.5), WAVE, G.OP_WAVE | G.OP_BARS)
        got = _wave_updates(S, b, _dev_u32(S.starts, steps), steps, ops, out_dtype(G, ops))
        assert b.last_launches() == 1 and b.kernel_name() == "glv_wave_kernel", (b.last_launches(), b.kernel_name())
        got = got.cpu().numpy()
        assert _same(got, U if r16 else texel_floats(U)), (kind, pool, r16)
        _neighbours_differ(got, (WAVE_BOUNDARY, 16384 - WAVE), (kind, r16)); _copies_are_the_source(got, WAVE_COPIES, (kind, r16))
        b.close()


@gpu
@pytest.mark.parametrize("kind,pool", [("s16", False), ("f32", True), ("planar", False), ("s16", True)], ids=["each-s16", "pool-f32", "each-planar", "pool-s16"])
def test_wave_updates_in_front_of_the_bars_at_wave(glvlib, waves, kind, pool):
    """GLV_OP_WAVE | GLV_OP_BARS | GLV_OP_R16, 9 steps: the waveform up to the bars' limit (73 800 windows x 8 groups at the least) into the workspace, then the
    integer pass over 147 600 rows.  Against batches of 6 streams: the ends, the streams around the write-backs' boundary, and those around step-major window
    65 536 (step 7, stream 8136), where the waveform's second trip begins if its limit is 64 bins"""
    G = glvlib
    steps = WAVE_BARS_STEPS
    S = waves(kind, pool, 2, steps)
    ops = G.OP_WAVE | G.OP_BARS | G.OP_R16
    dt = out_dtype(G, ops)
    make = lambda streams: G.Batch(G.Params(n=N, gl_storage=1, bars=N, bar_phase=0.5), streams, G.OP_WAVE | G.OP_BARS)      # noqa: E731
    b = make(WAVE)
    assert b.bars_arithmetic() == G.BARS_I8_EXACT
    got = _wave_updates(S, b, _dev_u32(S.starts, steps), steps, ops, dt)
    assert b.last_launches() == 2 and b.kernel_name() == "glv_wave_kernel", (b.last_launches(), b.kernel_name())
    b.close()
    for s0 in small_batches(WAVE, WAVE_BOUNDARY)[:3] + (WAVE_BARS_WINDOW % WAVE - 3,):
        sel = slice(s0, s0 + SMALL)
        small = object.__new__(_BigWave)
        small.kind, small.pool, small.pitch = kind, pool, getattr(S, "pitch", None)
        if pool: small.d_pcm, small.pool_frames, small.d_spans = S.d_pcm, S.pool_frames, _spans_device(S.spans[sel])
        else: small.d_pcm = _device(_layout(S.x[sel], kind), kind, 2 * N)
        bs = make(SMALL)
        want = _wave_updates(small, bs, _dev_u32(S.starts[sel], steps), steps, ops, dt)
        mine = rows_of(got, s0).contiguous()
        assert bool((mine != 0).any()) and eq(mine, want), (kind, pool, s0, differing(mine, want))
        bs.close()
    _neighbours_differ(got, (WAVE_BOUNDARY, WAVE_BARS_WINDOW % WAVE), (kind, pool)); _copies_are_the_source(got, WAVE_COPIES, (kind, pool))


# ---- the FFT chains: recordings or a pool for 4100 streams, made once ----------------------------------------------------------------------------------------------
class _BigEach(_Each):
    """test_track_frames_each._Each with every stream's recording (or span), starts, rates and planted copies from tests/track_geometry_lib.py, windows of
    bufscale * n frames; `call`, `warm_up` and `tables` are _Each's.  sub(s0): the same inputs for streams [s0, s0 + 6), on the device anew"""

    def __init__(self, G, kind, pool, bufscale, seed=701):
        idx = plant(SPEC, SPEC_COPIES)
        self.G, self.n, self.kind, self.pool, self.streams, self.steps, self.idx, self.span = G, N, kind, pool, SPEC, SPEC_STEPS, idx, bufscale * N
        self.f32 = kind != "s16"
        span = self.span
        if pool:
            self.pool_frames = POOL_FRAMES
            self.spans = spans_of(idx, POOL_FRAMES, span)
            self.starts = starts_of(idx, SPEC_STEPS, span + 700)
            self.x = rec(seed, 1, POOL_FRAMES, self.f32)[0]
            self.d_pcm = _device(np.ascontiguousarray(self.x.T) if kind == "planar" else self.x, kind, 2 * N)
            self.d_spans = _spans_device(self.spans)
            where = pool_starts(self.spans, self.starts, POOL_FRAMES, span)
            assert int(where.max()) == POOL_FRAMES - span
            _loads_of_both_forms(self.d_pcm, where, kind)
        else:
            self.pitch = (span + 300) | 1
            self.starts = starts_of(idx, SPEC_STEPS, self.pitch - span)
            self.x = recording(seed, idx, self.pitch, self.f32)
            self.d_pcm = _device(_layout(self.x, kind), kind, 2 * N)
            where = each_starts(self.starts, self.pitch, span)
            assert (where != self.starts).any()
            rows = 2 if kind == "planar" else 1
            _loads_of_both_forms(self.d_pcm, np.arange(SPEC, dtype=np.int64)[:, None] * rows * self.pitch + where, kind)
        self.warm = _layout(recording(seed + 1, idx, span + 64, self.f32), kind)

    def window(self, start, s=None):
        import torch
        sel = slice(None) if s is None else slice(s, s + 1)
        w = self.warm[sel, :, start:start + self.span] if self.kind == "planar" else self.warm[sel, start:start + self.span, :]
        return torch.from_numpy(np.ascontiguousarray(w)).cuda()

    def sub(self, s0):
        sel = slice(s0, s0 + SMALL)
        t = object.__new__(_BigEach)
        t.G, t.n, t.kind, t.pool, t.streams, t.steps, t.span, t.f32 = self.G, N, self.kind, self.pool, SMALL, self.steps, self.span, self.f32
        t.starts, t.warm = self.starts[sel], self.warm[sel]
        if self.pool: t.pool_frames, t.d_pcm, t.spans, t.d_spans = self.pool_frames, self.d_pcm, self.spans[sel], _spans_device(self.spans[sel])
        else: t.pitch, t.d_pcm = self.pitch, _device(_layout(self.x[sel], self.kind), self.kind, 2 * N)
        return t

    def head(self):
        if self.pool: return [self.d_pcm, self.pool_frames, self.d_spans]
        return [self.d_pcm] if self.kind == "planar" else [self.d_pcm, self.pitch]


@pytest.fixture(scope="module")
def specs(glvlib):
    """(kind, pool, bufscale) -> _BigEach, each made once and freed with the module"""
    made = {}

    def get(kind, pool=False, bufscale=1):
        key = (kind, pool, bufscale)
        if key not in made: made[key] = _BigEach(glvlib, kind, pool, bufscale)
        return made[key]
    yield get
    made.clear()


def _cut(v, sel):
    """rows [sel] of a per-stream table, None as it is"""
    return None if v is None else np.ascontiguousarray(v[sel])


def _step_rows(work, nbytes, bufscale, steps, streams, frames, bars):
    """float32 [steps][units][n] on the host: every step's finished float rows, which a gl_storage 3 frames call leaves in its workspace -- behind the decimated rows
    (bufscale > 1) and the transform's rows, each region steps * units * n floats (glv_track.cpp windows_geometry; the sizes already are multiples of 256)"""
    import torch
    region = steps * streams * 2 * N * 4
    assert region % 256 == 0 and frames * streams * 2 * N * 2 % 256 == 0
    dec = region if bufscale > 1 else 0
    assert nbytes == dec + 2 * region + (frames * streams * 2 * N * 2 if bars else 0), nbytes
    return work[dec + region:dec + 2 * region].view(torch.float32).view(steps, streams * 2, N).cpu().numpy()


def _spec_make(G, form, bufscale):
    def make(streams):
        b = _spec_batch(G, N, streams, form, segment=SEGMENT)
        if bufscale > 1: b.set_bufscale(bufscale)
        return b
    return make


# ---- 1. glv_batch_track_frames_*: lockstep ------------------------------------------------------------------------------------------------------------------------------
SPEC_ROW = dict(starts=[5, 0xFFFFFFF0, 133], ur=[1.0, 59.0, 60.0], frm=[0, 1, 2, 4, 3, BIG, 2], to=[1, 2, 3, 4, 0, 3, 2], mod=[0.25, 0.59310347, 1.0, 0.0, 0.5, 0.125, 0.75],
                keep=(3, 4))


def _spec_lockstep(S, b, T, keys, ops, w):
    """glv_batch_track_frames_* on `b`, one row of every table for all: ([frames][units][w], the workspace, its bytes); exact sizes, a guard behind each"""
    import torch
    steps, frames = len(T["starts"]), len(T["frm"])
    dt = out_dtype(S.G, ops)
    nbytes = b.track_frames_work_bytes(steps, frames, ops)
    work = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert work.data_ptr() % 256 == 0
    count = frames * b.streams * 2 * w
    fill = 23130 if dt == torch.int16 else -7.0
    flat = torch.full((count + GUARD,), fill, dtype=dt, device="cuda")
    getattr(b, "track_frames_" + KNAME[S.kind])(*S.head(), _dev_u32(T["starts"], 0), _dev_ur(T["ur"]), steps, _dev_u32(T["frm"], 0), _dev_u32(T["to"], 0), _dev_ur(T["mod"]),
                                                frames, keys, T["keep"], flat, work, ops)
    torch.cuda.synchronize()
    assert bool((work[nbytes:] == 0xA5).all()), "the call wrote behind the workspace it asked for"
    assert bool((flat[count:] == fill).all()), "the call wrote behind its output"
    return flat[:count].view(frames, b.streams * 2, w), work, nbytes


@gpu
@pytest.mark.parametrize("kind,form,bufscale", [("s16", "texels", 1), ("f32", "pass", 1), ("planar", "texels", 2), ("s16", "pass", 2)],
                         ids=["s16-texels", "f32-pass", "planar-texels-bufscale2", "s16-pass-bufscale2"])
def test_frames_lockstep_at_spec(glvlib, oracle, specs, kind, form, bufscale):
    """glv_track_frames_kernel over 2 x 8200 work items and glv_track_keys_kernel over 524 800 quads; under bufscale 2 glv_decimate_kernel with one table row over
    12 300 windows"""
    G = glvlib
    S = specs(kind, False, bufscale)
    T = SPEC_ROW
    steps, frames = SPEC_STEPS, SPEC_FRAMES
    _, _, w, r16 = _spec_forms(N)[form]
    ops = _spec_ops(G, form, r16)
    dt = out_dtype(G, ops)
    make = _spec_make(G, form, bufscale)
    kh = keys_of(S.idx, N, 73)
    b = make(SPEC)
    S.warm_up([b], ops, w)
    keys = _cuda(kh)
    got, work, nbytes = _spec_lockstep(S, b, T, keys, ops, w)
    launches = 2 + 2 + (0 if form == "texels" else 1) + (1 if bufscale > 1 else 0)
    assert b.last_launches() == launches and b.kernel_name() == "glv_track_frames_kernel", (b.last_launches(), b.kernel_name())
    rows = _step_rows(work, nbytes, bufscale, steps, SPEC, frames, form != "texels")
    del work
    assert _same(keys.cpu().numpy(), np.stack([rows[k - 2] for k in T["keep"]])), "d_keys"                # the whole write-back, every stream
    if form == "texels":
        U = Oracle.texels_r16(_lerp(kh, rows, T["frm"], T["to"], T["mod"], steps).reshape(-1, N)).reshape(frames, SPEC * 2, N)
        assert _same(got.cpu().numpy(), U), "every frame of every stream from the step rows"
    more = _process(b, kind, S.window(17), ops, w, dt)
    for s0 in small_batches(SPEC, SPEC_BOUNDARY):
        Q = S.sub(s0)
        bs = make(SMALL)
        Q.warm_up([bs], ops, w)
        ks = _cuda(rows_of(kh, s0))
        want, _, _ = _spec_lockstep(Q, bs, T, ks, ops, w)
        mine = rows_of(got, s0).contiguous()
        assert bool((mine != 0).any()) and eq(mine, want), (s0, differing(mine, want))
        assert eq(rows_of(keys, s0).contiguous(), ks), (s0, "d_keys")
        assert eq(more[2 * s0:2 * (s0 + SMALL)], _process(bs, kind, Q.window(17), ops, w, dt)), (s0, "next update")
        bs.close()
    marks = (SPEC_BOUNDARY, decimate_boundary_stream(steps))
    for x, what in ((got, "frames"), (keys, "d_keys"), (more[None], "next update")):
        _neighbours_differ(x, marks, (kind, form, what)); _copies_are_the_source(x, SPEC_COPIES, (kind, form, what))
    b.close()


# ---- 2. glv_batch_track_each_frames_* / glv_batch_track_pool_frames_* -------------------------------------------------------------------------------------------------
SPEC_EACH = [(k, p, "texels", 1, False) for p in (False, True) for k in KINDS] + [
    ("s16", False, "pass", 1, True), ("f32", True, "texels", 1, True), ("s16", False, "texels", 2, False), ("f32", True, "pass", 2, False), ("planar", True, "texels", 2, False)]


@gpu
@pytest.mark.parametrize("kind,pool,form,bufscale,null", SPEC_EACH,
                         ids=["%s-%s-%s%s%s" % ("pool" if p else "each", k, f, "-bufscale2" if k2 > 1 else "", "-null-counts" if z else "") for k, p, f, k2, z in SPEC_EACH])
def test_frames_per_stream_at_spec(glvlib, oracle, specs, kind, pool, form, bufscale, null):
    """glv_track_frames_each_kernel over 2 x 8200 work items and glv_track_keys_each_kernel over 524 800 quads, on the updates of the per-stream or the pool call
    (glv_track_each_scan_kernel at 8200 rows; under bufscale 2 glv_decimate_kernel with a table row per stream, or glv_decimate_pool_kernel, over 12 300 windows)"""
    G = glvlib
    S = specs(kind, pool, bufscale)
    idx, steps, frames = S.idx, SPEC_STEPS, SPEC_FRAMES
    _, _, w, r16 = _spec_forms(N)[form]
    ops = _spec_ops(G, form, r16)
    dt = out_dtype(G, ops)
    make = _spec_make(G, form, bufscale)
    counts, fcounts = (None, None) if null else (counts_of(idx, steps), frame_counts_of(idx, frames))
    keep = keep_of(idx, steps)
    frm, to, mod = frame_tables_of(idx, steps, frames, fcounts)
    starts = np.array(S.starts)
    if counts is not None: starts[np.arange(steps)[None, :] >= np.minimum(counts, steps)[:, None]] = BIG
    urs = rates_of(idx, steps, FLOAT_RATES, counts)
    kh = keys_of(idx, N, 74)

    def run(Q, b, sel):
        ks = _cuda(kh[:, 2 * sel.start:2 * sel.stop])
        tables = (_dev_u32(starts[sel], steps), _dev_ur(urs[sel]), _dev_u32(counts[sel], 1) if counts is not None else None)
        out = Q.call(b, tables, (frm[sel], to[sel], mod[sel], _cut(fcounts, sel), keep[sel]), ks, ops, w)
        return out, ks
    b = make(SPEC)
    S.warm_up([b], ops, w)
    got, keys = run(S, b, slice(0, SPEC))
    launches = 2 + 2 + (0 if form == "texels" else 1) + (1 if bufscale > 1 else 0)
    assert b.last_launches() == launches and b.kernel_name() == "glv_track_frames_each_kernel", (b.last_launches(), b.kernel_name())
    work = S.held[3]
    rows = _step_rows(work[:work.numel() - GUARD], work.numel() - GUARD, bufscale, steps, SPEC, frames, form != "texels")
    S.held = work = None
    if counts is not None:
        behind = np.repeat(np.arange(steps)[:, None] >= np.minimum(counts, steps)[None, :], 2, axis=1)
        assert not rows[behind].any() and rows[~behind].any()                     # the zero rows behind a count, which no frame and no keep pair may show
    assert _same(keys.cpu().numpy(), keep_each(kh, rows, keep, counts, steps)), "d_keys"                  # the whole write-back, every stream
    if form == "texels":
        wl, _ = lerp_each(kh, rows, frm, to, mod, counts, fcounts, steps)
        assert _same(got.cpu().numpy(), Oracle.texels_r16(wl.reshape(-1, N)).reshape(frames, SPEC * 2, N)), "every frame of every stream from the step rows"
    more = _process(b, kind, S.window(17), ops, w, dt)
    for s0 in small_batches(SPEC, SPEC_BOUNDARY):
        Q = S.sub(s0)
        bs = make(SMALL)
        Q.warm_up([bs], ops, w)
        want, ks = run(Q, bs, slice(s0, s0 + SMALL))
        mine = rows_of(got, s0).contiguous()
        assert bool((mine != 0).any()) and eq(mine, want), (s0, differing(mine, want))
        assert eq(rows_of(keys, s0).contiguous(), ks), (s0, "d_keys")
        assert eq(more[2 * s0:2 * (s0 + SMALL)], _process(bs, kind, Q.window(17), ops, w, dt)), (s0, "next update")
        bs.close()
    marks = (SPEC_BOUNDARY, decimate_boundary_stream(steps))
    for x, what in ((got, "frames"), (keys, "d_keys"), (more[None], "next update")):
        _neighbours_differ(x, marks, (kind, pool, form, what)); _copies_are_the_source(x, SPEC_COPIES, (kind, pool, form, what))
    b.close()


# ---- 3. glv_batch_track_each_* / glv_batch_track_pool_*, 4. glv_batch_track_at_* / glv_batch_track_rates_* ----------------------------------------------------------------
def _updates_case(G, S, entry, chain, with_ur, with_counts=True):
    """one large call of `entry` (each, pool, at, rates) against the four small batches: every step's rows, then the state through one more update; the copies and
    the boundary neighbours"""
    kind, steps, idx = S.kind, SPEC_STEPS, S.idx
    bufscale = S.span // N
    kw, mask, ops, table, w, texel = _chain(G, chain, N)
    pkw = dict(dict(n=N, avg_frames=F, gravity_step=TEXEL_STEP if texel else FLOAT_STEP), **kw)
    dt = out_dtype(G, ops)
    make = lambda streams: _make(G, pkw, mask, table, streams, bufscale)          # noqa: E731
    shared = entry in ("at", "rates")
    counts = None if shared or not with_counts else counts_of(idx, steps)
    base = TEXEL_RATES if texel else FLOAT_RATES
    if shared: starts, urs = np.asarray(SPEC_ROW["starts"], dtype=np.uint32), np.asarray(base[:steps], dtype=np.float32)
    else:
        starts = np.array(S.starts)
        if counts is not None: starts[np.arange(steps)[None, :] >= np.minimum(counts, steps)[:, None]] = BIG
        urs = rates_of(idx, steps, base, counts)
    with_ur = with_ur or entry == "rates"

    def run(Q, b, sel):
        if shared: return _shared(b, kind, Q.d_pcm, getattr(Q, "pitch", None), _dev_u32(starts, 0), _dev_ur(urs) if with_ur else None, steps, ops, w, dt)
        tables = (_dev_u32(starts[sel], steps), _dev_ur(urs[sel]) if with_ur else None, _dev_u32(counts[sel], 1) if counts is not None else None)
        if Q.pool: return _pool_call(b, kind, Q.d_pcm, Q.pool_frames, Q.d_spans, *tables, steps, ops, w, dt)
        return _each(b, kind, Q.d_pcm, Q.pitch, *tables, steps, ops, w, dt)
    b = make(SPEC)
    S.warm_up([b], ops, w)
    got = run(S, b, slice(0, SPEC))
    launches = 1 + 1 + (1 if ops & G.OP_BARS else 0) + (1 if bufscale > 1 else 0)
    name = "glv_track_scan_kernel" if shared else "glv_track_each_scan_kernel"
    assert b.last_launches() == launches and b.kernel_name() == name, (b.last_launches(), b.kernel_name())
    more = _process(b, kind, S.window(17), ops, w, dt)
    for s0 in small_batches(SPEC, SPEC_BOUNDARY):
        Q = S.sub(s0)
        bs = make(SMALL)
        Q.warm_up([bs], ops, w)
        want = run(Q, bs, slice(s0, s0 + SMALL))
        mine = rows_of(got, s0).contiguous()
        assert bool((mine != 0).any()), s0
        for t in range(steps): assert eq(mine[t], want[t]), (entry, chain, s0, t, differing(mine[t], want[t]))
        assert eq(more[2 * s0:2 * (s0 + SMALL)], _process(bs, kind, Q.window(17), ops, w, dt)), (entry, chain, s0, "next update")
        bs.close()
    marks = (SPEC_BOUNDARY, decimate_boundary_stream(steps))
    for x, what in ((got, "steps"), (more[None], "next update")):
        _neighbours_differ(x, marks, (entry, chain, what)); _copies_are_the_source(x, SPEC_COPIES, (entry, chain, what))
    b.close()


UPDATES = [("each", "s16", "chain", True, 2), ("each", "planar", "gl_chain_r16", False, 2), ("each", "f32", "gl_bars", True, 2), ("pool", "s16", "gl_chain_r16", True, 2),
           ("pool", "f32", "chain", False, 2), ("pool", "planar", "gl_bars", True, 2), ("each", "f32", "gl_chain_r16", True, 1), ("pool", "s16", "chain", True, 1)]


@gpu
@pytest.mark.parametrize("entry,kind,chain,with_ur,bufscale", UPDATES,
                         ids=["%s-%s-%s-%s%s" % (e, k, c, "rates" if u else "counts-alone", "-bufscale2" if k2 > 1 else "") for e, k, c, u, k2 in UPDATES])
def test_updates_per_stream_at_spec(glvlib, specs, entry, kind, chain, with_ur, bufscale):
    """3 steps, under bufscale 2 12 300 windows through the decimation (a table row per stream, or the pool kernel): glv_track_each_scan_kernel at 8200 rows with rate
    rows or with counts alone, on the float chain and the texel chain, and the integer pass behind it over 24 600 rows, some of them the zero rows behind a count"""
    _updates_case(glvlib, specs(kind, entry == "pool", bufscale), entry, chain, with_ur)


@gpu
@pytest.mark.parametrize("entry,kind,chain", [("at", "s16", "gl_chain_r16"), ("rates", "f32", "chain")], ids=["at-s16-gl_chain_r16", "rates-f32-chain"])
def test_shared_tables_at_spec(glvlib, specs, entry, kind, chain):
    """one shared table for 4100 streams under bufscale 2 (glv_decimate_kernel's one-row form past its cap): these entries had never run above 3 streams"""
    _updates_case(glvlib, specs(kind, False, 2), entry, chain, entry == "rates")
