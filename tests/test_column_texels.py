"""GPU: the graph module's columns (glv_batch_set_column_texels) and the circle module's texels through glv_batch_set_bar_texels.

Contract: with a column table set, out[row][x] == fdiv(fadd(fadd(T(l), T(m)), T(r)), 3.0f) bit for bit, where T(t) = c / 65535 (correctly
rounded) of GL_R16 texel c = texel t of the twin -- the same batch created with bars = n, bar_phase 0.5, run with GLV_OP_R16.  Every check here
gathers the twin's texel output and averages it in numpy float32.  The GL_R16 chain with sample_mode average computes the columns in the
transform's launch where the distinct texels fit behind the row; everything else takes one more launch (glv_columns_kernel)."""

import numpy as np
import pytest

from glava_amd.bar_positions import circle_texels, graph_column_texels
from gpu_lib import bars_mask as _mask, eq as _eq, update_inputs as _inputs
from oracle_lib import lcg_pcm_fast

pytestmark = pytest.mark.gpu
F = np.float32


def _contract(twin_texels, table):
    """twin_texels uint16 [rows][n], table [count][3] -> float32 [rows][count]"""
    T = (twin_texels.astype(F) / F(65535)).astype(F)
    lm = (T[:, table[:, 0]] + T[:, table[:, 1]]).astype(F)
    return ((lm + T[:, table[:, 2]]).astype(F) / F(3.0)).astype(F)


def _fits_fused(n, table):
    """the plan: the distinct texels (+ the dump slot) as 16-bit values behind the row of the size's default kernel configuration"""
    lanes = {1024: 64, 4096: 128, 16384: 256}[n]
    return len(np.unique(table)) + 1 <= 4 * lanes


def _run_pair(G, n, table, streams=3, kind="s16", bars_only=True, log_mode=1, gl_storage=1, sample_mode=0, updates=3, expect_launches=None):
    import torch
    table = np.asarray(table, np.int64)
    kw = dict(n=n, avg_window_kind=1, log_mode=log_mode, gl_storage=gl_storage, sample_mode=sample_mode)
    mask = _mask(G, kind, bars_only)
    cols = G.Batch(G.Params(bars=len(table), **kw), streams, mask)
    twin = G.Batch(G.Params(bars=n, bar_phase=0.5, **kw), streams, mask)
    cols.set_column_texels(table)
    assert cols.bars_arithmetic() == twin.bars_arithmetic()
    ops = G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS
    out_c = torch.zeros((streams * 2, len(table)), dtype=torch.float32, device="cuda")
    out_t = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda")
    launches = None
    for fr in range(updates):
        meth, x, extra = _inputs(kind, streams, n, fr)
        getattr(cols, meth)(x, *extra, out_c, ops)
        launches = cols.last_launches()
        if expect_launches is not None:
            assert launches == expect_launches, (fr, launches)
        getattr(twin, meth)(x, *extra, out_t, ops | G.OP_R16)
        torch.cuda.synchronize()
        want = _contract(out_t.cpu().numpy().view(np.uint16), table)
        got = out_c.cpu().numpy()
        assert (got.view(np.uint32) == want.view(np.uint32)).all(), (fr, kind, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        assert np.isfinite(got).all() and (got.max() > 0 or fr == 0)
    cols.close(); twin.close()
    return launches


def test_graph_tables_bit_equal_and_launch_counts(glvlib):
    seen = set()
    for n in (1024, 4096, 16384):
        for W in (320, 800, 1920):
            table = graph_column_texels(n, W)[0]
            fused = _fits_fused(n, table)
            got = _run_pair(glvlib, n, table, streams=3 if n < 16384 else 2, expect_launches=1 if fused else 2)
            print(f"n={n} W={W}: {len(table)} columns over {len(np.unique(table))} texels, launches {got}")
            seen.add(got)
    assert seen == {1, 2}


@pytest.mark.parametrize("bars_only", [True, False])
@pytest.mark.parametrize("log_mode", [0, 1])
def test_bars_only_and_log_modes(glvlib, bars_only, log_mode):
    _run_pair(glvlib, 4096, graph_column_texels(4096, 320)[0], streams=5, bars_only=bars_only, log_mode=log_mode, expect_launches=1)
    _run_pair(glvlib, 4096, graph_column_texels(4096, 800)[0], streams=5, bars_only=bars_only, log_mode=log_mode, expect_launches=2)


@pytest.mark.parametrize("kind", ["s16", "f32", "f32_stereo", "ring_s16", "ring_f32"])
def test_every_input_kind(glvlib, kind):
    _run_pair(glvlib, 4096, graph_column_texels(4096, 320)[0], kind=kind, expect_launches=1)
    _run_pair(glvlib, 1024, graph_column_texels(1024, 320)[0], kind=kind, log_mode=0, expect_launches=2)


def test_gl_storage_2_second_launch(glvlib):
    _run_pair(glvlib, 4096, graph_column_texels(4096, 320)[0], gl_storage=2, bars_only=False)
    _run_pair(glvlib, 1024, graph_column_texels(1024, 800)[0], gl_storage=2, bars_only=False, log_mode=0)


@pytest.mark.parametrize("mode", [1, 2])
def test_maximum_hybrid_second_launch(glvlib, mode):
    _run_pair(glvlib, 4096, graph_column_texels(4096, 320)[0], sample_mode=mode, expect_launches=2)
    _run_pair(glvlib, 4096, graph_column_texels(4096, 800)[0], sample_mode=mode, bars_only=False, expect_launches=2)


def test_refusals_and_clear(glvlib):
    import torch
    G = glvlib
    n, streams, W = 4096, 3, 320
    table = graph_column_texels(n, W)[0]
    cnt = len(table)
    mask = G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS
    kw = dict(n=n, bars=cnt, gl_storage=1, avg_window_kind=1)
    b = G.Batch(G.Params(**kw), streams, mask)

    def refused(code, fn):
        with pytest.raises(G.GlvError) as ei:
            fn()
        assert ei.value.code == code, (ei.value.code, str(ei.value))
        assert str(ei.value)

    refused(G.ERR_INVALID, lambda: b.set_column_texels(table[:-1]))
    bad = table.copy(); bad[7, 2] = n
    refused(G.ERR_INVALID, lambda: b.set_column_texels(bad))
    f32 = G.Batch(G.Params(n=n, bars=cnt, gl_storage=0), streams, mask)
    refused(G.ERR_STATE, lambda: f32.set_column_texels(table))
    nob = G.Batch(G.Params(**kw), streams, G.OP_GRAVITY | G.OP_AVERAGE)
    refused(G.ERR_STATE, lambda: nob.set_column_texels(table))
    ops = G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS
    pcm = torch.from_numpy(lcg_pcm_fast(78, streams * 2 * n)).cuda()
    ref = G.Batch(G.Params(**kw), streams, mask)
    o1 = torch.zeros((streams * 2, cnt), device="cuda"); o2 = torch.zeros_like(o1)
    o16 = torch.zeros((streams * 2, cnt), dtype=torch.int16, device="cuda")
    # the two tables exclude each other, either way round; clearing the kind that is not set changes nothing
    b.set_bar_texels(table[:, 1])
    refused(G.ERR_STATE, lambda: b.set_column_texels(table))
    b.set_column_texels(None)
    refused(G.ERR_STATE, lambda: b.set_column_texels(table))
    b.set_bar_texels(None)
    b.set_column_texels(table)
    refused(G.ERR_STATE, lambda: b.set_bar_texels(table[:, 1]))
    b.set_bar_texels(None)
    assert b.bars_arithmetic() == G.BARS_I8_EXACT
    # refused while set: texel output, a float chain, glv_batch_bars, another table length
    refused(G.ERR_STATE, lambda: b.process_s16(pcm, o16, ops | G.OP_R16))
    refused(G.ERR_STATE, lambda: b.process_s16(pcm, o1, G.OP_FFT | G.OP_BARS))
    refused(G.ERR_STATE, lambda: b.bars(torch.zeros((streams * 2, n), device="cuda"), o1))
    refused(G.ERR_STATE, lambda: b.set_params(G.Params(n=n, bars=40, gl_storage=1, avg_window_kind=1)))
    # glv_batch_reset keeps the table
    b.process_s16(pcm, o1, ops)
    b.reset()
    b.process_s16(pcm, o1, ops)
    assert b.last_launches() == 1
    twin = G.Batch(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=1, avg_window_kind=1), streams, mask)
    ot = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda")
    twin.process_s16(pcm, ot, ops | G.OP_R16)
    torch.cuda.synchronize()
    assert (o1.cpu().numpy().view(np.uint32) == _contract(ot.cpu().numpy().view(np.uint16), table.astype(np.int64)).view(np.uint32)).all()
    # cleared: the unsnapped bars again, bit for bit
    b.set_column_texels(None)
    b.reset()
    b.process_s16(pcm, o1, ops)
    ref.process_s16(pcm, o2, ops)
    torch.cuda.synchronize()
    assert _eq(o1, o2)
    b.process_s16(pcm, o16, ops | G.OP_R16)                            # texel bars are allowed again
    for x in (b, f32, nob, ref, twin): x.close()


def test_smooth_factor_change_rebuilds(glvlib):
    import torch
    G = glvlib
    n, streams, sf = 4096, 3, 0.04
    for W in (320, 800):                                              # the fused route and the second launch
        table = graph_column_texels(n, W)[0].astype(np.int64)
        mask = G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS
        b = G.Batch(G.Params(n=n, bars=len(table), gl_storage=1, avg_window_kind=1), streams, mask)
        b.set_column_texels(table)
        b.set_params(G.Params(n=n, bars=len(table), gl_storage=1, avg_window_kind=1, smooth_factor=sf))
        twin = G.Batch(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=1, avg_window_kind=1, smooth_factor=sf), streams, mask)
        ops = G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS
        o = torch.zeros((streams * 2, len(table)), device="cuda"); ot = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda")
        for fr in range(3):
            pcm = torch.from_numpy(lcg_pcm_fast(300 + fr, streams * 2 * n)).cuda()
            b.process_s16(pcm, o, ops); twin.process_s16(pcm, ot, ops | G.OP_R16)
            torch.cuda.synchronize()
            assert (o.cpu().numpy().view(np.uint32) == _contract(ot.cpu().numpy().view(np.uint16), table).view(np.uint32)).all(), (W, fr)
        b.close(); twin.close()


@pytest.mark.parametrize("W", [320, 800])
def test_graph_capture_of_first_columns_call(glvlib, W):
    import torch
    G = glvlib
    n, streams = 4096, 5
    table = graph_column_texels(n, W)[0].astype(np.int64)
    mask = G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS | G.OP_BARS_ONLY
    b = G.Batch(G.Params(n=n, bars=len(table), gl_storage=1, avg_window_kind=1), streams, mask)
    b.set_column_texels(table)
    twin = G.Batch(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=1, avg_window_kind=1), streams, mask)
    ops = G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS
    pcm = torch.from_numpy(lcg_pcm_fast(4321, streams * 2 * n)).cuda()
    o = torch.zeros((streams * 2, len(table)), device="cuda"); ot = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        b.process_s16(pcm, o, ops, stream=s.cuda_stream)
    g.replay()
    twin.process_s16(pcm, ot, ops | G.OP_R16)
    torch.cuda.synchronize()
    assert (o.cpu().numpy().view(np.uint32) == _contract(ot.cpu().numpy().view(np.uint16), table).view(np.uint32)).all()
    del g
    b.close(); twin.close()


def test_create_set_destroy_cycles_return_memory(glvlib):
    import torch
    G = glvlib
    n = 4096
    t320, t800 = graph_column_texels(n, 320)[0], graph_column_texels(n, 1920)[0]
    mask = G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS

    def cycle(mode):
        b = G.Batch(G.Params(n=n, bars=len(t320), gl_storage=1, avg_window_kind=1, sample_mode=mode), 64, mask)
        b.set_column_texels(t320)
        b.set_column_texels(None)
        b.set_column_texels(t320)
        b.close()
        b = G.Batch(G.Params(n=n, bars=len(t800), gl_storage=1, avg_window_kind=1, sample_mode=mode), 64, mask)
        b.set_column_texels(t800)
        b.close()
    cycle(0); cycle(1)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for i in range(20):
        cycle(i % 2)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (2 << 20)


@pytest.mark.parametrize("n", [1024, 4096])
def test_circle_texels_through_set_bar_texels(glvlib, n):
    import torch
    G = glvlib
    streams = 3
    theta = np.linspace(-np.pi, np.pi, 120, endpoint=False)
    tex, left, ties = circle_texels(n, theta)
    assert not ties.any() and left.any() and (~left).any()
    mask = G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS | G.OP_BARS_ONLY
    kw = dict(n=n, gl_storage=1, avg_window_kind=1)
    b = G.Batch(G.Params(bars=len(tex), **kw), streams, mask)
    b.set_bar_texels(tex)
    twin = G.Batch(G.Params(bars=n, bar_phase=0.5, **kw), streams, mask)
    ops = G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS | G.OP_R16
    o = torch.zeros((streams * 2, len(tex)), dtype=torch.int16, device="cuda"); ot = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda")
    idx = torch.from_numpy(tex.astype(np.int64)).cuda()
    for fr in range(3):
        pcm = torch.from_numpy(lcg_pcm_fast(500 + fr, streams * 2 * n)).cuda()
        b.process_s16(pcm, o, ops); twin.process_s16(pcm, ot, ops)
        torch.cuda.synchronize()
        assert _eq(o, ot[:, idx].contiguous()), fr
    # a pixel's value: the channel row the shader picks (idx > 0: left = row 0 of the stream, else right = row 1), texel tex[k]
    got = o.cpu().numpy().view(np.uint16).reshape(streams, 2, len(tex))
    want = ot.cpu().numpy().view(np.uint16).reshape(streams, 2, n)
    ch = np.where(left, 0, 1)
    assert (got[:, ch, np.arange(len(tex))] == want[:, ch, tex.astype(np.int64)]).all()
    b.close(); twin.close()
