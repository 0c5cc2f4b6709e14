"""GPU: track calls past every launch cap -- a stream's results do not depend on the streams around it.

Streams are independent, so stream s of a LARGE track call is, bit for bit, what the same recording gives in a SMALL batch: on every step, and in
the state the call leaves.  The contract tests (test_track*.py) pin the arithmetic to sequential process calls at 3 streams x 11-14 steps, at most 84
rows, below every cap of every launcher; here one LARGE call past all of them is compared with SMALL batches fed exactly its first and its last five
streams and driven through sequential process calls, window by window (track_lib.seq) -- the path the older tests pin to the oracle:

    large   3457 streams x 19 steps = 65 683 windows, 131 366 rows: more than kGridCap workgroups of one row (glv_columns_kernel, glv_bars_kernel) and of
            two (glv_bars_short_kernel), 2053 >= 512 blocks of 64 rows (split_rounds' unsplit form), more than kGridCap x 256 groups of 8 frames
            (glv_wave_kernel KIND 3 / 4, with and without bars behind it), 6914 x ceil(n / 128) workgroups of the scan, and several trips per workgroup
            of the transform
    small   5 streams, process calls of 10 rows: one block of 64 rows (the rounds split over blockIdx.y), one trip everywhere

Inside the range the recording of stream 3 is planted in streams on both sides of the 64-row blocks, of row 2048 and of row 512 x 64 = 32 768: every
step's rows of each copy equal stream 3's.  n = 256 wherever the form exists at that size (the live forms probe upwards, as test_track_live._choose
does); hop 45, F = 5, odd pitches; the s16 recording one frame behind an 8-byte boundary (its windows alternate load forms), the f32 one 8 bytes behind
a 16-byte boundary.  Every call gets a workspace of exactly the queried size and an output of exactly the documented size, a guard region behind each;
every case asserts the launch count and the kernel name the header documents for its form.  Every assertion is bit equality, floats as int32.

What the names cannot show: glv_batch_track_windows_* names the scan whatever bars follow it -- which bars kernel runs rests on
glv_batch_bars_arithmetic, on the step counts of the 80-bar work lists (tests/test_bars_launch_geometry.py) and on the live entry, which names its
third kernel; GLV_TRACK_WAVE_ORDER changes no name.

The last test is one call whose regions lie beyond 4 GiB, at the shape include/glv_spectrum.h gives measurements for (n = 4096, 1024 streams)."""
import pytest

from glava_amd.bar_positions import graph_column_texels, radial_bar_texels
from track_lib import bars_batch, eq as _eq, out_dtype, pitch_odd, s16_chains, seq as _seq, track, with_table, work_regions

pytestmark = pytest.mark.gpu

N = 256
FR = 5
HOP = 45
STREAMS, STEPS, SMALL = 3457, 19, 5
ENDS = (0, STREAMS - SMALL)                                  # the small batches' first streams
# stream 3's recording again: around row 64 of step 0 (31, 32), row 32 768 of the stream-major workspace rows (862, 863), row 2048 of step 0 (1023 to 1025),
# a block boundary in mid-range (1728), row 32 768 of the step-major output rows (2555, 2556, at step 4), and inside the last small batch (3455)
SOURCE, COPIES = 3, (31, 32, 862, 863, 1023, 1024, 1025, 1728, 2555, 2556, 3455)
WINDOWS, ROWS = STREAMS * STEPS, STREAMS * STEPS * 2

# ---- the caps, restated, and the arithmetic that puts LARGE beyond them and SMALL below -------------------------------------------------------------------
K_GRID_CAP = 256 * 8          # glv_launch_util.h kGridCap: capped_grid of glv_wave_kernel (256 lanes x 8 frames), glv_columns_kernel and glv_bars_kernel
                              # (1 row per workgroup), glv_bars_short_kernel (2), glv_bars_mode_kernel
ROWS_PER_BLOCK = 64           # glv_bars.hip with_rows_i8_ring: RB of glv_bars_rows_i8_kernel for every ring n <= 16384 takes
SPLIT_FROM = 512              # glv_launch_util.h split_rounds: from 512 x-workgroups on the rounds are not split over blockIdx.y
WAVE_LANES, WAVE_GROUP = 256, 8   # glv_misc.hip glv_wave_kernel: __launch_bounds__(256), one lane per group of 8 frames (grid_256)
WAVE_LIMIT_MIN = 64           # glv_chain.cpp plan_wave: in front of the bars the waveform stops at bins_needed, a whole multiple of 64 bins
K_TRACK_DEPTH = 8             # glv_misc.hip kTrackDepth: steps whose loads are in flight ahead of the scan
SCAN_BINS = 128               # glv_misc.hip kTrackLanes = 64 lanes x one pair of bins: workgroups of the scan per row = ceil(kept / 128)


def test_the_large_call_lies_beyond_every_cap_and_the_small_one_below():
    assert ROWS == 131366 and WINDOWS == 65683
    assert ROWS > K_GRID_CAP and ROWS > 2 * K_GRID_CAP                                       # one and two rows per workgroup
    assert -(-ROWS // ROWS_PER_BLOCK) >= SPLIT_FROM > -(-(SMALL * 2 * STEPS) // ROWS_PER_BLOCK)
    assert -(-(SMALL * 2) // ROWS_PER_BLOCK) < SPLIT_FROM                                    # (the sequential side: process calls of 10 rows)
    assert WINDOWS * (N // WAVE_GROUP) / WAVE_LANES > K_GRID_CAP                             # the waveform kernel without bars
    assert WINDOWS * (WAVE_LIMIT_MIN // WAVE_GROUP) / WAVE_LANES > K_GRID_CAP                # ... and in front of the bars, at the least its limit can be
    assert STEPS > K_TRACK_DEPTH + FR                                                        # the look-ahead refills and the ring wraps
    assert STREAMS * 2 * (N // SCAN_BINS) > K_GRID_CAP
    for c in COPIES: assert SOURCE < c < STREAMS and c not in range(SMALL)
    assert {2 * 31 + 1, 2 * 32} == {63, 64} and 2 * 1023 < 2048 <= 2 * 1024 and ENDS[1] <= 3455   # rows of step 0: both sides of a block of 64 and of row 2048
    assert 2 * 1728 % ROWS_PER_BLOCK == 0
    mark = SPLIT_FROM * ROWS_PER_BLOCK                                                       # row 32 768, where block 512 begins
    assert 862 * STEPS * 2 <= mark < 863 * STEPS * 2                                         # stream-major: [stream][step][channel]
    assert 4 * STREAMS * 2 + 2 * 2555 + 1 == mark - 1 and 4 * STREAMS * 2 + 2 * 2556 == mark # step-major: [step][stream][channel]


# ---- the recordings: made once per shape, on the device -------------------------------------------------------------------------------------------------
class _Rec:
    """[STREAMS][pitch][2] frames on the device.  layout `odd`: an odd pitch, the first frame 4 bytes behind an 8-byte boundary (f32: 8 behind a 16-byte one);
    `grouped`: a pitch that is a multiple of 8 at a 32-byte boundary; `residue`: a pitch that is a multiple of 64"""
    def __init__(self, n, hop, f32, layout, streams=STREAMS, steps=STEPS, copies=((SOURCE, COPIES),), seed=0):
        import torch
        self.n, self.hop, self.f32, self.streams = n, hop, f32, streams
        pitch = pitch_odd(n, hop, steps + 1)                             # odd, holds one more window than the call takes: the state check's
        if layout == "grouped": pitch = (pitch + 7) // 8 * 8
        if layout == "residue": pitch = (pitch + 63) // 64 * 64
        self.pitch = pitch
        g = torch.Generator(device="cuda")
        g.manual_seed(4000 + 7 * n + hop + seed)
        size = streams * pitch * 2
        lead = 0 if layout == "grouped" else 2
        flat = torch.zeros((size + 16,), dtype=torch.float32 if f32 else torch.int16, device="cuda")
        assert flat.data_ptr() % 256 == 0
        self.view = flat[lead:lead + size]
        self.x = self.view.view(streams, pitch, 2)
        level = torch.arange(streams, device="cuda") % 3                 # every stream at a level of its own: 1, 1 / 8, 1 / 64
        if f32:
            self.x.copy_(torch.randn((streams, pitch, 2), generator=g, device="cuda") * 0.3 * torch.pow(0.125, level.float())[:, None, None])
            self.view.view(streams, -1)[:, 7::97] = -0.0
            assert self.view.data_ptr() % 16 == 8
        else:
            x = torch.randint(-32768, 32768, (streams, pitch, 2), generator=g, device="cuda", dtype=torch.int32)
            self.x.copy_((x >> (3 * level.int())[:, None, None]).to(torch.int16))
            assert self.view.data_ptr() % 32 == (0 if layout == "grouped" else 4)
        for source, copies in copies:
            self.x[list(copies)] = self.x[source].clone()
        torch.cuda.synchronize()

    def window(self, t, streams=slice(None)):
        """window t of the streams, [streams][n][2] contiguous: a process call's input"""
        return self.x[streams, t * self.hop:t * self.hop + self.n].contiguous()


@pytest.fixture(scope="module")
def recordings():
    """(n, hop, f32, layout) -> _Rec, each made once and freed with the module"""
    made = {}

    def get(n, hop=HOP, f32=False, layout="odd"):
        key = (n, hop, f32, layout)
        if key not in made: made[key] = _Rec(n, hop, f32, layout)
        return made[key]
    yield get
    made.clear()


# ---- one call, exactly sized buffers --------------------------------------------------------------------------------------------------------------------------
def _track(b, entry, rec, ops, w, dt, steps=STEPS, fill=0xA5):
    """steps [0, steps) of the recording in one call (track_lib.track: workspace and output exactly as large as the library asks and documents, a guard
    behind each); returns the output and the workspace"""
    return track(b, entry, rec.view, rec.pitch, rec.hop, steps, ops, w, dt, f32=rec.f32, fill=fill, keep_work=True)


def _rows(x, s0, count=SMALL):
    """the channel rows of streams [s0, s0 + count) of every step of a step-major output"""
    return x[:, 2 * s0:2 * (s0 + count)].contiguous()


def _check(G, make, entry, rec, ops, w, launches, name, stateful, what, streams=STREAMS, steps=STEPS, ends=ENDS, small=SMALL, copies=((SOURCE, COPIES),)):
    """the LARGE call against SMALL batches through sequential process calls, the copies inside the range, and (stateful) one more process call on all"""
    import torch
    dt = out_dtype(G, ops)
    large = make(streams)
    got, work = _track(large, entry, rec, ops, w, dt, steps=steps)
    assert large.last_launches() == launches and large.kernel_name() == name, (what, large.last_launches(), large.kernel_name())
    if launches == 1: assert bool((work == 0xA5).all()), "a call that runs in one launch touched the workspace"
    del work
    after = _seq(large, [rec.window(steps)], ops, w, dt, rec.f32) if stateful else None
    for source, planted in copies:
        for c in planted:
            assert _eq(_rows(got, c, 1), _rows(got, source, 1)), (what, "copy", c, int((_rows(got, c, 1) != _rows(got, source, 1)).sum()))
            if stateful: assert _eq(_rows(after, c, 1), _rows(after, source, 1)), (what, "state of copy", c)
    for s0 in ends:
        b = make(small)
        wins = [rec.window(t, slice(s0, s0 + small)) for t in range(steps + 1)]
        want = _seq(b, wins[:steps], ops, w, dt, rec.f32)
        mine = _rows(got, s0, small)
        assert bool((mine != 0).any()), (what, s0)
        for t in range(steps):
            assert _eq(mine[t], want[t]), (what, s0, t, int((mine[t] != want[t]).sum()))
        if stateful:
            assert _eq(_rows(after, s0, small), _seq(b, wins[steps:], ops, w, dt, rec.f32)), (what, s0, "state")
        b.close()
    large.close()
    del got
    torch.cuda.empty_cache()


def _first_size(G, build, entry, hop=HOP):
    """the smallest n at which the form exists: the batch can be created and the sizing query takes the call"""
    for n in (N, 512, 1024, 2048, 4096):
        try:
            make, ops, w = build(n)
            probe = make(1)
        except (G.GlvError, ValueError, AssertionError):
            continue
        try:
            query = "track_work_bytes" if entry == "residue" else f"track_{entry}_work_bytes"
            pitch = pitch_odd(n, hop, STEPS + 1)
            getattr(probe, query)((pitch + 63) // 64 * 64 if entry == "residue" else pitch, hop, STEPS, ops)
            return n, make, ops, w
        except G.GlvError:
            continue
        finally:
            probe.close()
    raise AssertionError("no size takes this form")


def _maker(G, n, kw, mask, table=None, F=FR):
    def make(streams):
        return with_table(G.Batch(G.Params(n=n, avg_frames=F, **kw), streams, mask), table)
    return make


# ---- 1. glv_batch_track_windows_s16 / _f32 ----------------------------------------------------------------------------------------------------------------------
def _windows_forms(G):
    """name -> (n -> (parameters, creation mask, ops, table), launches, bars arithmetic or None)"""
    FFT, R16, B = G.OP_FFT, G.OP_R16, G.OP_BARS
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    gl = dict(gl_storage=1, avg_window_kind=1)
    radial = lambda n: ("bar", radial_bar_texels(n, 160)[0])            # noqa: E731
    return {
        "fft":              (lambda n: (dict(), FFT, FFT, None), 1, None),                                               # one launch, step-major straight into d_out
        "chain":            (lambda n: (dict(), GA, FFT | GA, None), 2, None),                                            # scan<false>
        "gl_chain_r16":     (lambda n: (gl, GA, FFT | GA | R16, None), 2, None),                                          # scan<true>
        "gl_pass_r16":      (lambda n: (dict(bars=n, bar_phase=0.5, **gl), GA | B, FFT | GA | B | R16, None), 3, G.BARS_I8_EXACT),   # the i8 pass over texel rows, unsplit
        "float_80_short":   (lambda n: (dict(bars=80), GA | B, FFT | GA | B, None), 3, None),                            # glv_bars_short_kernel, 2 rows per workgroup
        "float_80_chunked": (lambda n: (dict(bars=80, smooth_factor=0.5), GA | B, FFT | GA | B, None), 3, None),         # glv_bars_kernel, 1 row per workgroup
        "snap_r16":         (lambda n: (dict(bars=len(radial(n)[1]), **gl), GA | B, FFT | GA | B | R16, radial(n)), 3, G.BARS_I8_EXACT),   # glv_bars_snap_kernel
        "snap_floats":      (lambda n: (dict(bars=len(radial(n)[1]), **gl), GA | B, FFT | GA | B, radial(n)), 3, G.BARS_I8_EXACT),
        "maximum_r16":      (lambda n: (dict(bars=n, bar_phase=0.5, sample_mode=1, **gl), GA | B, FFT | GA | B | R16, None), 3, G.BARS_F32_SEQ),   # glv_bars_mode_kernel
        "hybrid_floats":    (lambda n: (dict(bars=n, bar_phase=0.5, sample_mode=2, sample_hybrid_weight=0.25, **gl), GA | B, FFT | GA | B, None), 3, G.BARS_F32_SEQ),
        "chain_mono":       (lambda n: (dict(channels=1), GA, FFT | GA, None), 2, None),
        "gl_chain_mono":    (lambda n: (dict(channels=1, **gl), GA, FFT | GA | R16, None), 2, None),
    }


WINDOWS_FORMS = ["fft", "chain", "gl_chain_r16", "gl_pass_r16", "float_80_short", "float_80_chunked", "snap_r16", "snap_floats", "maximum_r16",
                 "hybrid_floats", "chain_mono", "gl_chain_mono"]


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("form", WINDOWS_FORMS)
def test_track_windows_of_a_stream_do_not_depend_on_the_streams_around_it(glvlib, recordings, form, f32):
    G = glvlib
    spec, launches, arithmetic = _windows_forms(G)[form]

    def build(n):
        kw, mask, ops, table = spec(n)
        return _maker(G, n, kw, mask, table), ops, kw.get("bars", n) if ops & G.OP_BARS else n
    n, make, ops, w = _first_size(G, build, "windows")
    if arithmetic is not None:
        probe = make(1)
        assert probe.bars_arithmetic() == arithmetic, probe.bars_arithmetic()
        probe.close()
    stateful = bool(ops & (G.OP_GRAVITY | G.OP_AVERAGE))
    _check(G, make, "windows", recordings(n, f32=f32), ops, w, launches, "glv_track_scan_kernel" if stateful else "glv_frame_kernel", stateful, (form, n, f32))


# ---- 2. glv_batch_track_s16, the residue form --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["gl_chain_r16", "chain"])
def test_residue_track_of_a_stream_does_not_depend_on_the_streams_around_it(glvlib, recordings, chain):
    """hop 64, a pitch that is a multiple of 64: n / hop residue launches over the whole frame sequence, then the scan's log_q / residue_rows map at a large k0"""
    G = glvlib
    kw, mask, ops = s16_chains(G)[chain]
    hop = 64
    n, make, ops, w = _first_size(G, lambda n: (_maker(G, n, kw, mask), ops, n), "residue", hop=hop)
    rec = recordings(n, hop=hop, layout="residue")
    assert rec.pitch % hop == 0 and 2 * ((STREAMS - 1) * rec.pitch // n) > K_GRID_CAP          # rows of one residue launch
    _check(G, make, "residue", rec, ops, w, n // hop + 1, "glv_track_scan_kernel", True, (chain, n))


# ---- 3. glv_batch_track_columns_s16 / _f32 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("sample_mode", [0, 1, 2])
def test_track_columns_of_a_stream_do_not_depend_on_the_streams_around_it(glvlib, recordings, sample_mode, f32):
    """glv_columns_kernel's texel-row kind: 131 366 rows over kGridCap workgroups, the exact integer sums and the two float walks"""
    G = glvlib
    GA = G.OP_GRAVITY | G.OP_AVERAGE

    def build(n):
        table = graph_column_texels(n, 200)[0]
        kw = dict(bars=len(table), gl_storage=1, avg_window_kind=1, sample_mode=sample_mode)
        return _maker(G, n, kw, GA | G.OP_BARS, ("col", table)), G.OP_FFT | GA | G.OP_BARS, len(table)
    n, make, ops, w = _first_size(G, build, "columns")
    _check(G, make, "columns", recordings(n, f32=f32), ops, w, 3, "glv_columns_kernel", True, ("columns", n, sample_mode, f32))


# ---- 4. glv_batch_track_live_s16 / _f32: the scan over the kept bins -----------------------------------------------------------------------------------
def _live_candidates(G, case):
    """test_track_live._cases' chains at every size from 256 on: (n, parameters, table) in ascending size, and the ops"""
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    gl = dict(avg_window_kind=1, gl_storage=1)
    chain = G.OP_FFT | GA | G.OP_BARS
    sizes = (N, 512, 1024, 2048, 4096)
    if case == "gl_smallest":
        return [(n, dict(bars=n, bar_phase=0.5, smooth_factor=0.025, **gl), None) for n in sizes], chain | G.OP_R16
    if case == "float_80":
        return [(n, dict(bars=80), None) for n in sizes], chain
    tables = [(n, graph_column_texels(n, 320)[0]) for n in sizes]
    return [(n, dict(bars=len(t), **gl), ("col", t)) for n, t in tables], chain


def _scan_keeps_less_than_a_row(G, n, kw, table, ops, rec_of):
    """one stream, F + 1 steps on a workspace of 0xFF bytes: the last 64 bins of every row of the scan's region still hold them (a texel or a float the
    scan had written there would have to be 0xFFFF / a NaN of all ones in every row)"""
    b = bars_batch(G, n, kw, table, FR, 1)
    if b.live_bins() == 0:
        b.close()
        return False
    rec = rec_of(n)
    steps, elem = FR + 1, 2 if kw.get("gl_storage") == 1 else 4
    _, work = _track(b, "live", rec, ops, kw["bars"], out_dtype(G, ops), steps=steps, fill=0xFF)
    b.close()
    (_, _), (scan, _) = work_regions(work, steps * 2, n, elem, elem)
    tail = scan[:steps * 2 * n * elem].view(steps * 2, n * elem)[:, -64 * elem:]
    return bool((tail == 0xFF).all())


@pytest.mark.parametrize("case,f32", [("gl_smallest", False), ("float_80", False), ("columns", False), ("gl_smallest", True)])
def test_live_track_of_a_stream_does_not_depend_on_the_streams_around_it(glvlib, recordings, case, f32):
    """the smallest size at which the chain has live bins and its scan keeps fewer than n of them: units * ceil(kept / 128) workgroups, kept < n"""
    G = glvlib
    candidates, ops = _live_candidates(G, case)
    rec_of = lambda n: recordings(n, f32=f32)                           # noqa: E731
    for n, kw, table in candidates:
        try:
            if _scan_keeps_less_than_a_row(G, n, kw, table, ops, rec_of): break
        except G.GlvError:
            continue
    else:
        raise AssertionError(f"no candidate size of {case} has live bins")
    probe = bars_batch(G, n, kw, table, FR, 1)
    assert probe.live_bins() != 0 and probe.live_bins() < n
    probe.close()
    name = {"gl_smallest": "glv_bars_rows_i8_kernel", "float_80": "glv_bars_kernel", "columns": "glv_columns_kernel"}[case]
    _check(G, lambda streams: bars_batch(G, n, kw, table, FR, streams), "live", recordings(n, f32=f32), ops, kw["bars"], 3, name, True, (case, n, f32))


# ---- 5. - 7. glv_batch_track_wave_s16 / _f32: stateless --------------------------------------------------------------------------------------------------
def _wave_maker(G, n, monkeypatch=None, order=None):
    def make(streams):
        if order and streams == STREAMS: monkeypatch.setenv("GLV_TRACK_WAVE_ORDER", order)      # (read at creation: diagnostics)
        b = G.Batch(G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5), streams, G.OP_WAVE | G.OP_BARS)
        if order and streams == STREAMS: monkeypatch.delenv("GLV_TRACK_WAVE_ORDER")
        assert b.bars_arithmetic() == G.BARS_I8_EXACT
        return b
    return make


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("r16", [True, False], ids=["texels", "floats"])
def test_wave_track_without_bars(glvlib, recordings, r16, f32):
    """glv_wave_kernel KIND 3 / 4 past its cap: 65 683 x 32 groups of 8 frames over 2048 workgroups of 256 lanes"""
    G = glvlib
    ops = G.OP_WAVE | (G.OP_R16 if r16 else 0)
    _check(G, _wave_maker(G, N), "wave", recordings(N, f32=f32), ops, N, 1, "glv_wave_kernel", False, ("wave", r16, f32))


@pytest.mark.parametrize("form", ["rows", "steps", "unaligned"])
def test_wave_track_with_the_integer_pass(glvlib, monkeypatch, recordings, form):
    """GLV_OP_WAVE | GLV_OP_BARS | GLV_OP_R16.  rows / steps: a 32-byte aligned recording, hop 48, a pitch that is a multiple of 8 -- one launch of
    glv_bars_rows_i8_kernel straight from the frames, 64 consecutive output rows per workgroup or (GLV_TRACK_WAVE_ORDER=steps at creation) the 19 steps of
    one channel row, a partial block each.  unaligned: hop 45 one frame off -- the waveform kernel into the workspace, the integer pass over its rows"""
    G = glvlib
    ops = G.OP_WAVE | G.OP_BARS | G.OP_R16
    if form == "unaligned":
        rec, launches, name = recordings(N), 2, "glv_wave_kernel"
    else:
        rec, launches, name = recordings(N, hop=48, layout="grouped"), 1, "glv_bars_rows_i8_kernel"
        assert rec.view.data_ptr() % 32 == 0 and rec.pitch % 8 == 0 and rec.hop % 8 == 0
        assert (4 * STREAMS * 2 + 2) * N * 4 <= 2 ** 32 - 1                                   # glv_track.cpp track_wave: the steps order's lane offset fits, the order is taken
        assert STEPS % ROWS_PER_BLOCK != 0
    _check(G, _wave_maker(G, N, monkeypatch, "steps" if form == "steps" else None), "wave", rec, ops, N, launches, name, False, ("wave pass", form))


@pytest.mark.parametrize("r16", [True, False], ids=["texels", "floats"])
def test_wave_track_f32_with_the_integer_pass(glvlib, recordings, r16):
    """KIND 4 up to the bars' limit, then the i8 pass over its 131 366 rows: always two launches"""
    G = glvlib
    ops = G.OP_WAVE | G.OP_BARS | (G.OP_R16 if r16 else 0)
    _check(G, _wave_maker(G, N), "wave", recordings(N, f32=True), ops, N, 2, "glv_wave_kernel", False, ("wave f32 pass", r16))


# ---- one track call past 4 GiB ----------------------------------------------------------------------------------------------------------------------------
def test_track_call_with_regions_beyond_4_GiB(glvlib):
    """n = 4096, 1024 streams x 257 steps, hop 735, an odd pitch (the shape include/glv_spectrum.h gives measurements for, one step more): 526 336 rows.
    The GL chain with the pre-smoothing pass, texels out: both workspace regions and d_out are 526 336 x 4096 x 2 bytes > 2^32 -- row 524 288 starts at
    4 GiB: stream 1020 of the stream-major workspace rows (514 per stream), step 256 of the step-major output (2048 rows per step).  The float chain
    without bars: the workspace and d_out are 8 GiB each, 16 KiB per row -- 4 GiB at row 262 144, stream 510 of the workspace and step 128 of the
    output; 8 GiB at stream 1020 and step 256.  Streams [0, 3) and [1021, 1024) against a 6-stream batch through 257 sequential process calls; stream
    2's recording again in streams 511, 512 (just beyond the float workspace's 4 GiB) and 1022 (beyond every mark)"""
    import torch
    G = glvlib
    n, streams, steps, hop, small = 4096, 1024, 257, 735, 3
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    rec = _Rec(n, hop, False, "odd", streams=streams, steps=steps, copies=((2, (511, 512, 1022)),), seed=99)
    assert rec.pitch % 2 == 1
    rows = steps * streams * 2
    assert rows == 526336 and rows * n * 2 > 2 ** 32
    assert 2 ** 32 // (n * 2) // (steps * 2) == 1020 and 2 ** 32 // (n * 2) // (streams * 2) == 256
    assert 2 ** 32 // (n * 4) // (steps * 2) == 510 and 2 ** 32 // (n * 4) // (streams * 2) == 128
    ends = (0, streams - small)
    both = torch.tensor([0, 1, 2, 1021, 1022, 1023], device="cuda")
    wins = [rec.window(t, both) for t in range(steps + 1)]              # the 6-stream batch's inputs, cut on the device
    forms = [
        ("gl pass", dict(bars=n, bar_phase=0.5, gl_storage=1, avg_window_kind=1), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16, 3, 2, 2),
        ("float chain", dict(), GA, G.OP_FFT | GA, 2, 4, 4),
    ]
    for what, kw, mask, ops, launches, in_bytes, out_bytes in forms:
        dt = out_dtype(G, ops)
        make = _maker(G, n, kw, mask)
        large, ref = make(streams), make(2 * small)
        up = lambda v: (v + 255) & ~255                                  # noqa: E731
        nbytes = large.track_windows_work_bytes(rec.pitch, hop, steps, ops)
        assert nbytes == up(rows * n * in_bytes) * (2 if ops & G.OP_BARS else 1) and up(rows * n * in_bytes) > 2 ** 32, (what, nbytes)
        got, work = _track(large, "windows", rec, ops, n, dt, steps=steps)
        assert got.numel() * out_bytes > 2 ** 32 and got.element_size() == out_bytes
        assert large.last_launches() == launches and large.kernel_name() == "glv_track_scan_kernel", (what, large.last_launches(), large.kernel_name())
        del work
        want = _seq(ref, wins[:steps], ops, n, dt)
        mine = torch.cat([_rows(got, s0, small) for s0 in ends], dim=1)
        assert bool((mine != 0).any())
        for t in range(steps):
            assert _eq(mine[t], want[t]), (what, t, int((mine[t] != want[t]).sum()))
        for c in (511, 512, 1022):
            assert _eq(_rows(got, c, 1), _rows(got, 2, 1)), (what, "copy", c, int((_rows(got, c, 1) != _rows(got, 2, 1)).sum()))
        after = _seq(large, [rec.window(steps)], ops, n, dt)
        assert _eq(torch.cat([_rows(after, s0, small) for s0 in ends], dim=1), _seq(ref, wins[steps:], ops, n, dt)), (what, "state")
        for c in (511, 512, 1022):
            assert _eq(_rows(after, c, 1), _rows(after, 2, 1)), (what, "state of copy", c)
        large.close(); ref.close()
        del got, mine, want, after
        torch.cuda.empty_cache()
