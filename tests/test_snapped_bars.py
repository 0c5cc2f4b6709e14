"""GPU: bars at texels of the pre-smoothing pass (glv_batch_set_bar_texels).

Contract: with a bar texel table t set, bars_out[row][k] == twin_out[row][t[k]] bit for bit, where the twin is the same batch created
with bars = n and bar_phase = 0.5 (the pre-smoothing pass GLava's modules sample with setsmoothpass true) -- as GL_R16 texels and as
floats, with and without GLV_OP_BARS_ONLY, for every input kind, both log modes, across stateful updates.  The GL_R16 chain with
sample_mode average computes them in the transform's launch; everything else takes a second launch."""

import numpy as np
import pytest

from glava_amd.bar_positions import bars_module_bar_texels, radial_bar_texels
from gpu_lib import bars_mask as _mask, eq as _eq, update_inputs as _inputs
from oracle_lib import Oracle, lcg_pcm_fast

pytestmark = pytest.mark.gpu


def _run_pair(G, n, tex, streams=5, kind="s16", r16=True, bars_only=True, log_mode=1, gl_storage=1, sample_mode=0, updates=3,
              expect_launches=None, twin_check_oracle=False):
    import torch
    kw = dict(n=n, avg_window_kind=1, log_mode=log_mode, gl_storage=gl_storage, sample_mode=sample_mode)
    mask = _mask(G, kind, bars_only)
    snap = G.Batch(G.Params(bars=len(tex), **kw), streams, mask)
    twin = G.Batch(G.Params(bars=n, bar_phase=0.5, **kw), streams, mask)
    snap.set_bar_texels(tex)
    assert snap.bars_arithmetic() == twin.bars_arithmetic()
    ops = G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS | (G.OP_R16 if r16 else 0)
    dt = torch.int16 if r16 else torch.float32
    out_s = torch.zeros((streams * 2, len(tex)), dtype=dt, device="cuda")
    out_t = torch.zeros((streams * 2, n), dtype=dt, device="cuda")
    t_idx = torch.from_numpy(np.asarray(tex, np.int64)).cuda()
    for fr in range(updates):
        meth, x, extra = _inputs(kind, streams, n, fr)
        getattr(snap, meth)(x, *extra, out_s, ops)
        if expect_launches is not None:
            assert snap.last_launches() == expect_launches, (fr, snap.last_launches())
        getattr(twin, meth)(x, *extra, out_t, ops)
        torch.cuda.synchronize()
        assert _eq(out_s, out_t[:, t_idx].contiguous()), (fr, kind, r16)
    if twin_check_oracle:
        # the twin's own texels: the oracle's exact integer mean over the chain's `av` rows (an unsnapped GL_R16 chain's texel output)
        av_b = G.Batch(G.Params(bars=80, **kw), streams, mask & ~G.OP_BARS_ONLY)
        av = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda")
        for fr in range(updates):
            meth, x, extra = _inputs(kind, streams, n, fr)
            getattr(av_b, meth)(x, *extra, av, G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_R16)
        torch.cuda.synchronize()
        rows = av.cpu().numpy().view(np.uint16)
        got = out_t.cpu().numpy()
        for r in range(0, streams * 2, 3):
            t, f = Oracle.bars_int(rows[r], n, smooth_factor=0.025, phase=0.5)
            if r16: assert (got[r].view(np.uint16) == t).all(), r
            else: assert (got[r].view(np.uint32) == f.view(np.uint32)).all(), r
        av_b.close()
    snap.close(); twin.close()


@pytest.mark.parametrize("n", [1024, 4096, 16384])
@pytest.mark.parametrize("r16", [True, False])
def test_radial_texels_fused_one_launch(glvlib, oracle, n, r16):
    tex, ties = radial_bar_texels(n, 160)
    assert not ties.any()
    _run_pair(glvlib, n, tex, streams=5 if n < 16384 else 3, r16=r16, expect_launches=1, twin_check_oracle=(n == 4096))


@pytest.mark.parametrize("bars_only", [True, False])
@pytest.mark.parametrize("log_mode", [0, 1])
def test_bars_only_and_log_modes(glvlib, bars_only, log_mode):
    _run_pair(glvlib, 4096, radial_bar_texels(4096, 160)[0], streams=7, bars_only=bars_only, log_mode=log_mode, expect_launches=1)


@pytest.mark.parametrize("kind", ["s16", "f32", "f32_stereo", "ring_s16", "ring_f32"])
def test_every_input_kind(glvlib, kind):
    _run_pair(glvlib, 4096, radial_bar_texels(4096, 160)[0], streams=3, kind=kind, expect_launches=1)
    _run_pair(glvlib, 1024, radial_bar_texels(1024, 160)[0], streams=3, kind=kind, r16=False, log_mode=0, expect_launches=1)


@pytest.mark.parametrize("W,bw,gap", [(1280, 5, 1), (801, 4, 2)])
@pytest.mark.parametrize("n", [1024, 4096])
def test_bars_module_texels(glvlib, W, bw, gap, n):
    tex, _ = bars_module_bar_texels(n, W, bw, gap, 2)
    G = glvlib
    # as many bars as the module draws: fused where the slack behind the row holds them (bars + 1 <= 2 lanes), a second launch else
    _run_pair(G, n, tex, streams=3, r16=True)
    _run_pair(G, n, tex, streams=3, r16=False, bars_only=False)


@pytest.mark.parametrize("mode", [1, 2])
def test_maximum_hybrid_second_launch(glvlib, mode):
    _run_pair(glvlib, 4096, radial_bar_texels(4096, 160)[0], streams=3, sample_mode=mode, expect_launches=2)
    _run_pair(glvlib, 4096, radial_bar_texels(4096, 160)[0], streams=3, sample_mode=mode, r16=False, bars_only=False, expect_launches=2)


@pytest.mark.parametrize("r16", [True, False])
def test_gl_storage_2_second_launch(glvlib, r16):
    _run_pair(glvlib, 4096, radial_bar_texels(4096, 160)[0], streams=3, gl_storage=2, bars_only=False, r16=r16)
    _run_pair(glvlib, 1024, radial_bar_texels(1024, 160)[0], streams=3, gl_storage=2, bars_only=False, r16=r16, log_mode=0)


def test_refusals_and_clear(glvlib):
    import torch
    G = glvlib
    n, streams = 4096, 3
    tex = radial_bar_texels(n, 160)[0]
    mask = G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS
    b = G.Batch(G.Params(n=n, bars=80, gl_storage=1, avg_window_kind=1), streams, mask)

    def refused(code, fn):
        with pytest.raises(G.GlvError) as ei:
            fn()
        assert ei.value.code == code, (ei.value.code, str(ei.value))
        assert str(ei.value)

    refused(G.ERR_INVALID, lambda: b.set_bar_texels(tex[:79]))
    bad = tex.copy(); bad[5] = n
    refused(G.ERR_INVALID, lambda: b.set_bar_texels(bad))
    f32 = G.Batch(G.Params(n=n, bars=80, gl_storage=0), streams, mask)
    refused(G.ERR_STATE, lambda: f32.set_bar_texels(tex))
    nob = G.Batch(G.Params(n=n, bars=80, gl_storage=1, avg_window_kind=1), streams, G.OP_GRAVITY | G.OP_AVERAGE)
    refused(G.ERR_STATE, lambda: nob.set_bar_texels(tex))
    wide = G.Batch(G.Params(n=16384, bars=80, gl_storage=1, avg_window_kind=1, smooth_factor=0.1), 1, mask)
    assert wide.bars_arithmetic() == G.BARS_F32_CHAIN
    refused(G.ERR_INVALID, lambda: wide.set_bar_texels(radial_bar_texels(16384, 160)[0]))
    assert "F32_MATRIX" in G.lib().glv_last_error().decode()
    # unsnapped bits first
    ops = G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS | G.OP_R16
    pcm = torch.from_numpy(lcg_pcm_fast(77, streams * 2 * n)).cuda()
    ref = G.Batch(G.Params(n=n, bars=80, gl_storage=1, avg_window_kind=1), streams, mask)
    o1 = torch.zeros((streams * 2, 80), dtype=torch.int16, device="cuda"); o2 = torch.zeros_like(o1)
    b.set_bar_texels(tex)
    assert b.bars_arithmetic() == G.BARS_I8_EXACT
    # refused while set
    refused(G.ERR_STATE, lambda: b.set_params(G.Params(n=n, bars=40, gl_storage=1, avg_window_kind=1)))
    refused(G.ERR_STATE, lambda: b.bars(torch.zeros((streams * 2, n), device="cuda"), torch.zeros((streams * 2, 80), device="cuda")))
    refused(G.ERR_STATE, lambda: b.process_s16(pcm, torch.zeros((streams * 2, 80), device="cuda"), G.OP_FFT | G.OP_BARS))
    # bar_phase is ignored, smooth_factor rebuilds
    b.set_params(G.Params(n=n, bars=80, gl_storage=1, avg_window_kind=1, bar_phase=0.3))
    b.reset()                                                        # keeps the table
    b.process_s16(pcm, o1, ops)
    twin = G.Batch(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=1, avg_window_kind=1), streams, mask)
    ot = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda")
    twin.process_s16(pcm, ot, ops)
    torch.cuda.synchronize()
    assert _eq(o1, ot[:, torch.from_numpy(tex.astype(np.int64)).cuda()].contiguous())
    # cleared: the unsnapped bits again
    b.set_params(G.Params(n=n, bars=80, gl_storage=1, avg_window_kind=1))
    b.set_bar_texels(None)
    assert b.bars_arithmetic() == G.BARS_F32_CHAIN
    b.reset()
    b.process_s16(pcm, o1, ops)
    ref.process_s16(pcm, o2, ops)
    torch.cuda.synchronize()
    assert _eq(o1, o2)
    for x in (b, f32, nob, wide, ref, twin): x.close()


def test_smooth_factor_change_rebuilds(glvlib):
    import torch
    G = glvlib
    n, streams, sf = 4096, 3, 0.04
    tex = radial_bar_texels(n, 160)[0]
    mask = G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS
    b = G.Batch(G.Params(n=n, bars=80, gl_storage=1, avg_window_kind=1), streams, mask)
    b.set_bar_texels(tex)
    b.set_params(G.Params(n=n, bars=80, gl_storage=1, avg_window_kind=1, smooth_factor=sf))
    twin = G.Batch(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=1, avg_window_kind=1, smooth_factor=sf), streams, mask)
    ops = G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS
    o = torch.zeros((streams * 2, 80), device="cuda"); ot = torch.zeros((streams * 2, n), device="cuda")
    for fr in range(3):
        pcm = torch.from_numpy(lcg_pcm_fast(300 + fr, streams * 2 * n)).cuda()
        b.process_s16(pcm, o, ops); twin.process_s16(pcm, ot, ops)
        torch.cuda.synchronize()
        assert _eq(o, ot[:, torch.from_numpy(tex.astype(np.int64)).cuda()].contiguous()), fr
    b.close(); twin.close()


def test_graph_capture_of_first_snapped_call(glvlib):
    import torch
    G = glvlib
    n, streams = 4096, 5
    tex = radial_bar_texels(n, 160)[0]
    mask = G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS | G.OP_BARS_ONLY
    b = G.Batch(G.Params(n=n, bars=80, gl_storage=1, avg_window_kind=1), streams, mask)
    b.set_bar_texels(tex)
    twin = G.Batch(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=1, avg_window_kind=1), streams, mask)
    ops = G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS | G.OP_R16
    pcm = torch.from_numpy(lcg_pcm_fast(4321, streams * 2 * n)).cuda()
    o = torch.zeros((streams * 2, 80), dtype=torch.int16, device="cuda"); ot = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        b.process_s16(pcm, o, ops, stream=s.cuda_stream)
    g.replay()
    twin.process_s16(pcm, ot, ops)
    torch.cuda.synchronize()
    assert _eq(o, ot[:, torch.from_numpy(tex.astype(np.int64)).cuda()].contiguous())
    del g
    b.close(); twin.close()


def test_create_set_destroy_cycles_return_memory(glvlib):
    import torch
    G = glvlib
    n = 4096
    tex = radial_bar_texels(n, 160)[0]
    mask = G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS

    def cycle():
        b = G.Batch(G.Params(n=n, bars=80, gl_storage=1, avg_window_kind=1, sample_mode=1), 64, mask)
        b.set_bar_texels(tex)
        b.set_bar_texels(None)
        b.set_bar_texels(tex)
        b.close()
    cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(20):
        cycle()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (2 << 20)
