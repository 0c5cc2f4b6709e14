"""The bars passes of a second launch: results do not depend on launch geometry.

Rows are independent, so the bars of row r from a launch of R rows are, bit for bit, the bars of the same input row from a launch of R'
rows -- however the launcher cut the rows into workgroups, split a table's rounds over blockIdx.y or capped the grid.  The parity tests
anchor the arithmetic to the oracle at a few hundred rows, below every cap; here a LARGE run past every cap is compared with SMALL runs
fed exactly its first and its last 130 rows:

    small   65 streams =    130 rows: no multiple of 64 or 32 (a partial last workgroup), fewer than 512 workgroups of 64 rows (the rounds
                                      are split over y)
    large   16 417 streams = 32 834 rows: 514 workgroups of 64 rows (>= 512: the unsplit form), more than 2048 workgroups of 1, 2 and 8 rows
                                      (the grid-stride loops run), and 4 units per row (8 tiles at n = 256) = 131 336 units of the
                                      one-lane-per-bar kernel against its cap of 4096 workgroups x 4 units.

n = 256 is the smallest size with 256 bars.  Its 80-bar work lists (glv_tables.h make_bar_items for 128 groups) are 2 steps long at
smooth_factor 0.025, 4 at 0.12 and 6 at 0.5: glv_bars_short_kernel<2>, <4> and the chunked glv_bars_kernel.

What the test cannot see: glv_batch_bars reports no kernel name and no launch count, and glv_batch_bars_arithmetic names the arithmetic,
not the kernel -- the three chunked-list cases all answer BARS_F32_CHAIN, the matrix-core kernel and the one-lane-per-bar kernel
(GLV_NO_BARS_ROWS at creation) both BARS_F32_MATRIX.  Which kernel a case runs rests on the step counts above and on that switch; only the
wave cases tell their two forms apart, by glv_batch_last_launches.

The last section takes the same sizes through glv_batch_process_s16, two updates each (state rows are read as well as written), for the kernels of a
process call's last launch that glv_batch_bars over float spectra never reaches: glv_bars_mode_kernel over a GL chain's texel rows, glv_bars_snap_kernel
and the I8_FLOATS kind of the integer pass over the float rows of the pass-by-pass chain (gl_storage 2), glv_columns_kernel over float rows."""
import numpy as np
import pytest

from glava_amd.bar_positions import graph_column_texels, radial_bar_texels
from oracle_lib import lcg_pcm_fast

gpu = pytest.mark.gpu

N = 256
SMALL_STREAMS, LARGE_STREAMS = 65, 16417
SMALL_ROWS, LARGE_ROWS = 2 * SMALL_STREAMS, 2 * LARGE_STREAMS


@pytest.fixture(scope="module")
def spectra():
    """[LARGE_ROWS][N] float spectra on the device, made once and freed with the module: values on both sides of [0, 1], a NaN here and there"""
    import torch
    rng = np.random.default_rng(7000 + N)
    spec = (rng.random((LARGE_ROWS, N), dtype=np.float32) ** 2 * np.float32(1.25) - np.float32(0.04)).astype(np.float32)
    spec[::97, ::9] = np.nan
    spec[-1, 5] = np.nan
    return torch.from_numpy(spec).cuda()


@pytest.fixture(scope="module")
def pcm_frames():
    """interleaved s16 frames of LARGE_STREAMS streams of N frames, on the device, made once and freed with the module"""
    import torch
    return torch.from_numpy(lcg_pcm_fast(8128, LARGE_STREAMS * 2 * N)).cuda()


def assert_same_bits(got, want, what):
    import torch
    bits = torch.int32 if got.dtype == torch.float32 else got.dtype
    differ = got.view(bits) != want.view(bits)
    assert not bool(differ.any()), (what, int(differ.sum()), differ.nonzero()[:4].tolist())


def bars_of(G, params, streams, spec, monkeypatch, env=None):
    """Batch.bars over `spec` ([2 * streams][n], on the device) by a batch of `streams` streams"""
    import torch
    if env:
        monkeypatch.setenv(env, "1")
    b = G.Batch(params, streams, G.OP_FFT | G.OP_BARS)
    if env:
        monkeypatch.delenv(env)
    out = torch.full((2 * streams, params.bars), -1.0, dtype=torch.float32, device="cuda")
    b.bars(spec, out)
    torch.cuda.synchronize()
    arithmetic = b.bars_arithmetic()
    b.close()
    return out, arithmetic


@gpu
@pytest.mark.parametrize("family,kw,env,arithmetic", [
    ("short kernel, 2 steps", dict(bars=80), None, "BARS_F32_CHAIN"),
    ("short kernel, 4 steps", dict(bars=80, smooth_factor=0.12), None, "BARS_F32_CHAIN"),
    ("chunked kernel (6 steps)", dict(bars=80, smooth_factor=0.5), None, "BARS_F32_CHAIN"),
    ("rows kernel", dict(bars=256), None, "BARS_F32_MATRIX"),
    ("one lane per bar", dict(bars=256), "GLV_NO_BARS_ROWS", "BARS_F32_MATRIX"),
    ("mode kernel", dict(bars=80, sample_mode=1), None, "BARS_F32_SEQ"),
])
def test_bars_of_a_row_do_not_depend_on_the_rows_around_it(glvlib, monkeypatch, spectra, family, kw, env, arithmetic):
    """glv_batch_bars over float spectra: every kernel family launch_bars picks"""
    G = glvlib
    p = G.Params(n=N, **kw)
    spec = spectra
    large, a_large = bars_of(G, p, LARGE_STREAMS, spec, monkeypatch, env)
    assert a_large == getattr(G, arithmetic)
    assert not bool((large == -1.0).any())                                      # every bar of every row was written
    for name, rows in (("first", slice(0, SMALL_ROWS)), ("last", slice(LARGE_ROWS - SMALL_ROWS, LARGE_ROWS))):
        small, a_small = bars_of(G, p, SMALL_STREAMS, spec[rows].contiguous(), monkeypatch, env)
        assert a_small == a_large
        assert_same_bits(small, large[rows], (family, name))


def wave_texture(G, streams, pcm, monkeypatch, unfused):
    import torch
    if unfused:
        monkeypatch.setenv("GLV_UNFUSED_WAVE", "1")
    b = G.Batch(G.Params(n=N, bars=N, bar_phase=0.5, gl_storage=1), streams, G.OP_WAVE | G.OP_BARS)
    monkeypatch.delenv("GLV_UNFUSED_WAVE", raising=False)
    assert b.bars_arithmetic() == G.BARS_I8_EXACT
    out = torch.zeros((2 * streams, N), dtype=torch.int16, device="cuda")
    b.process_s16(pcm, out, G.OP_WAVE | G.OP_BARS | G.OP_R16)
    torch.cuda.synchronize()
    assert b.last_launches() == (2 if unfused else 1), b.last_launches()         # the i8 kernel from the frames / the wave kernel, then the i8 kernel over texel rows
    if not unfused:
        assert b.kernel_name() == "glv_bars_rows_i8_kernel"
    b.close()
    return out


@gpu
@pytest.mark.parametrize("unfused", [False, True])
def test_wave_texture_of_a_stream_does_not_depend_on_the_streams_around_it(glvlib, monkeypatch, pcm_frames, unfused):
    """GLV_OP_WAVE | GLV_OP_BARS | GLV_OP_R16 from s16 frames: the integer matrix-core pass in its one-launch form, and (GLV_UNFUSED_WAVE) over the
    waveform kernel's texel rows"""
    G = glvlib
    pcm = pcm_frames
    large = wave_texture(G, LARGE_STREAMS, pcm, monkeypatch, unfused)
    assert int(large.ne(0).sum()) > 0
    per_stream = 2 * N                                                          # int16 values of a stream's frames
    for name, s0 in (("first", 0), ("last", LARGE_STREAMS - SMALL_STREAMS)):
        small = wave_texture(G, SMALL_STREAMS, pcm[s0 * per_stream:(s0 + SMALL_STREAMS) * per_stream].contiguous(), monkeypatch, unfused)
        assert_same_bits(small, large[2 * s0:2 * (s0 + SMALL_STREAMS)], (unfused, name))


# ---- the last launch of a process call: the kernels glv_batch_bars never reaches ------------------------------------------------------------------------
LANES_PER_ROW = 16                      # glv_inst.hip: lanes per row of the one kernel configuration of n = 256 -- no process call fuses bars or columns behind it


@pytest.fixture(scope="module")
def pcm_updates(pcm_frames):
    """the frames of two updates of LARGE_STREAMS streams: pcm_frames, and the same frames in reverse stream order at a third of the level"""
    import torch
    second = torch.div(pcm_frames.view(LARGE_STREAMS, 2 * N).flip(0), 3, rounding_mode="floor").reshape(-1).contiguous()
    return pcm_frames, second


def _second_launch_families(G):
    """family -> (parameters, table, GLV_OP_R16, launches, bars arithmetic).  launches: the transform and the kernel named -- and between them, for
    gl_storage 2, the pass-by-pass chain's own pass (glv_post_kernel), which makes the kernel under test the third launch, not the second"""
    bar = ("bar", radial_bar_texels(N, 160)[0])
    wide, narrow = ("col", graph_column_texels(N, 200)[0]), ("col", graph_column_texels(N, 40)[0])
    assert len(np.unique(wide[1])) + 1 > 4 * LANES_PER_ROW                       # more distinct texels than fit behind a row as 16-bit values
    nb, nw, nn = len(bar[1]), len(wide[1]), len(narrow[1])
    return {
        "mode kernel on texel rows": (dict(gl_storage=1, bars=nb, sample_mode=1), bar, True, 2, G.BARS_F32_SEQ),
        "snap kernel on float rows, texels out": (dict(gl_storage=2, bars=nb), bar, True, 3, G.BARS_I8_EXACT),
        "snap kernel on float rows, floats out": (dict(gl_storage=2, bars=nb), bar, False, 3, G.BARS_I8_EXACT),
        "columns kernel on float rows, over the fuse limit": (dict(gl_storage=1, bars=nw), wide, False, 2, G.BARS_I8_EXACT),
        "columns kernel pass by pass, average": (dict(gl_storage=2, bars=nn, sample_mode=0), narrow, False, 3, G.BARS_I8_EXACT),
        "columns kernel pass by pass, maximum": (dict(gl_storage=2, bars=nn, sample_mode=1), narrow, False, 3, G.BARS_F32_SEQ),
        "columns kernel pass by pass, hybrid": (dict(gl_storage=2, bars=nn, sample_mode=2, sample_hybrid_weight=0.25), narrow, False, 3, G.BARS_F32_SEQ),
        "i8 pass over float rows": (dict(gl_storage=2, bars=N, bar_phase=0.5), None, True, 3, G.BARS_I8_EXACT),
    }


def two_updates(G, kw, table, r16, streams, updates, launches, arithmetic):
    """the outputs of two glv_batch_process_s16 calls of the GL chain with bars on a batch of `streams` streams"""
    import torch
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    b = G.Batch(G.Params(n=N, avg_window_kind=1, **kw), streams, GA | G.OP_BARS)
    if table: (b.set_bar_texels if table[0] == "bar" else b.set_column_texels)(table[1])
    assert b.bars_arithmetic() == arithmetic, b.bars_arithmetic()
    outs = []
    for pcm in updates:
        out = torch.zeros((2 * streams, kw["bars"]), dtype=torch.int16 if r16 else torch.float32, device="cuda")
        b.process_s16(pcm, out, G.OP_FFT | GA | G.OP_BARS | (G.OP_R16 if r16 else 0))
        assert b.last_launches() == launches and b.kernel_name() == "glv_frame_kernel", (b.last_launches(), b.kernel_name())    # (a GL chain names its transform)
        outs.append(out)
    torch.cuda.synchronize()
    b.close()
    return outs


@gpu
@pytest.mark.parametrize("family", ["mode kernel on texel rows", "snap kernel on float rows, texels out", "snap kernel on float rows, floats out",
                                    "columns kernel on float rows, over the fuse limit", "columns kernel pass by pass, average",
                                    "columns kernel pass by pass, maximum", "columns kernel pass by pass, hybrid", "i8 pass over float rows"])
def test_last_launch_of_a_process_call_does_not_depend_on_the_streams_around_it(glvlib, pcm_updates, family):
    """two updates of 16 417 streams against two updates of its first and its last 65.  n = 256 fuses none of these (16 lanes per row), so every family
    stays at this size; glv_batch_last_launches is 2 on gl_storage 1 and 3 on gl_storage 2, whose chain runs its state pass as a launch of its own"""
    G = glvlib
    kw, table, r16, launches, arithmetic = _second_launch_families(G)[family]
    large = two_updates(G, kw, table, r16, LARGE_STREAMS, pcm_updates, launches, arithmetic)
    assert int(large[1].ne(0).sum()) > 0
    per_stream = 2 * N                                                          # int16 values of a stream's frames
    for name, s0 in (("first", 0), ("last", LARGE_STREAMS - SMALL_STREAMS)):
        cut = [pcm[s0 * per_stream:(s0 + SMALL_STREAMS) * per_stream].contiguous() for pcm in pcm_updates]
        small = two_updates(G, kw, table, r16, SMALL_STREAMS, cut, launches, arithmetic)
        for u in range(2):
            assert_same_bits(small[u], large[u][2 * s0:2 * (s0 + SMALL_STREAMS)], (family, name, u))
