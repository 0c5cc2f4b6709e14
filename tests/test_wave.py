"""The wave module on the device (GLV_OP_WAVE): PCM -> wrange -> GL_R16 upload -> pre-smoothed texels.

Every expectation is bit equality against the models of tests/oracle_lib.py: the unpack (glvo_unpack_s16 / glvo_unpack_f32), wrange
(glvo_wrange, and the compiled reference's transform_wrange where it is available), the upload rounding (glvo_texels_r16), the pre-smoothing
pass in its exact integer form (glvo_bars_int_at) and, for sample_mode maximum / hybrid, the shader's float loop (glvo_bars_mode_at).  No
tolerances.  The GPU tests need GLV_OP_WAVE; the CPU tests at the end need the helper, the constant and the exported symbol."""
import os
import re

import numpy as np
import pytest

from gpu_lib import planar_of_s16, same, texel_floats, upload, wrange
from oracle_lib import Oracle, Ref, lcg_pcm, lcg_pcm_fast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu


def planar_of_f32(frames, streams, n, channels=2):
    rows = np.empty((streams * 2, n), np.float32)
    for s in range(streams):
        l = np.empty(n, np.float32); r = np.empty(n, np.float32)
        Oracle.lib().glvo_unpack_f32(np.ascontiguousarray(frames[s * 2 * n:(s + 1) * 2 * n]), n, channels, l, r)
        rows[2 * s], rows[2 * s + 1] = l, r
    return rows


def dev_u16(t):
    return t.cpu().numpy().view(np.uint16)


# ---- 1. every s16 value -------------------------------------------------------------------------------------------------------------
@gpu
def test_every_s16_value(glvlib, oracle):
    import torch
    G = glvlib
    streams, n = 16, 4096
    v = (np.arange(65536, dtype=np.int64) - 32768).astype(np.int16)
    pcm = np.empty((streams * n, 2), np.int16)
    pcm[:, 0] = v; pcm[:, 1] = v[::-1]
    pcm = pcm.reshape(-1)
    b = G.Batch(G.Params(n=n), streams, G.OP_WAVE)
    d_pcm = torch.from_numpy(pcm).cuda()
    o16 = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda")
    of = torch.zeros((streams * 2, n), dtype=torch.float32, device="cuda")
    b.process_s16(d_pcm, o16, G.OP_WAVE | G.OP_R16)
    assert b.last_launches() == 1 and b.kernel_name() == "glv_wave_kernel"
    b.process_s16(d_pcm, of, G.OP_WAVE)
    torch.cuda.synchronize()
    planar = planar_of_s16(pcm, streams, n)
    want = Oracle.texels_r16(wrange(planar))
    assert same(dev_u16(o16), want)
    if Ref.available():
        assert same(dev_u16(o16), Oracle.texels_r16(wrange(planar, use_ref=True)))
    assert same(of.cpu().numpy(), texel_floats(want))
    assert len(np.unique(want)) > 30000                          # (the waveform spans the texel range)
    assert b.algorithmic_bytes(G.OP_WAVE | G.OP_R16, True) == streams * 8 * n and b.algorithmic_bytes(G.OP_WAVE, False) == streams * 16 * n
    b.close()
    # channels = 1: the mono mix into both rows
    m = G.Batch(G.Params(n=n, channels=1), 4, G.OP_WAVE)
    pcm = lcg_pcm(99, 4 * 2 * n)
    o = torch.zeros((8, n), dtype=torch.int16, device="cuda")
    m.process_s16(torch.from_numpy(pcm).cuda(), o, G.OP_WAVE | G.OP_R16)
    torch.cuda.synchronize()
    want = upload(planar_of_s16(pcm, 4, n, channels=1))
    assert same(dev_u16(o), want) and (want[0] == want[1]).all()
    m.close()


# ---- 2. input kinds -----------------------------------------------------------------------------------------------------------------
def _special_floats(count, seed):
    rng = np.random.default_rng(seed)
    x = (rng.random(count, dtype=np.float32) * np.float32(2.6) - np.float32(1.3)).astype(np.float32)      # inside and outside [-1, 1]
    sp = np.array([-0.0, 0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 3.0, -3.0, 1e-45, -1e-45, 0.99999994, -0.99999994, 1e30, -1e30], np.float32)
    x[: sp.size] = sp
    x[-sp.size:] = sp[::-1]
    x[count // 2: count // 2 + sp.size] = sp
    return x


@gpu
def test_f32_inputs_with_special_values(glvlib, oracle):
    import torch
    G = glvlib
    streams, n = 5, 1024
    b = G.Batch(G.Params(n=n), streams, G.OP_WAVE)
    x = _special_floats(streams * 2 * n, 3)
    o16 = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda")
    of = torch.zeros((streams * 2, n), dtype=torch.float32, device="cuda")
    # planar rows are taken as they are
    planar = x.reshape(streams * 2, n)
    b.process_f32(torch.from_numpy(x).cuda(), o16, G.OP_WAVE | G.OP_R16)
    b.process_f32(torch.from_numpy(x).cuda(), of, G.OP_WAVE)
    torch.cuda.synchronize()
    want = upload(planar)
    assert same(dev_u16(o16), want) and same(of.cpu().numpy(), texel_floats(want))
    assert want.reshape(-1)[6] == 0 and want.reshape(-1)[4] == 65535 and want.reshape(-1)[5] == 0         # NaN -> 0, +Inf -> 1, -Inf -> 0
    # interleaved frames
    b.process_f32_stereo(torch.from_numpy(x).cuda(), o16, G.OP_WAVE | G.OP_R16)
    b.process_f32_stereo(torch.from_numpy(x).cuda(), of, G.OP_WAVE)
    torch.cuda.synchronize()
    want = upload(planar_of_f32(x, streams, n))
    assert same(dev_u16(o16), want) and same(of.cpu().numpy(), texel_floats(want))
    b.close()
    # ... and their mono mix (L + R) / 2 in float
    m = G.Batch(G.Params(n=n, channels=1), streams, G.OP_WAVE)
    y = (np.random.default_rng(8).random(streams * 2 * n, dtype=np.float32) * np.float32(2.2) - np.float32(1.1)).astype(np.float32)
    m.process_f32_stereo(torch.from_numpy(y).cuda(), o16, G.OP_WAVE | G.OP_R16)
    torch.cuda.synchronize()
    assert same(dev_u16(o16), upload(planar_of_f32(y, streams, n, channels=1)))
    m.close()


@gpu
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("channels", [2, 1])
def test_rings_follow_the_rotation(glvlib, oracle, f32, channels):
    """the window of a ring update starts at the ring's oldest frame: the model's rows are ring_planar of a second, identically fed batch"""
    import torch
    G = glvlib
    streams, n = 3, 1024
    ring = G.OP_RING_F32 if f32 else G.OP_RING_S16
    b = G.Batch(G.Params(n=n, channels=channels), streams, G.OP_WAVE | ring)
    twin = G.Batch(G.Params(n=n, channels=channels), streams, ring)
    o16 = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda")
    of = torch.zeros((streams * 2, n), dtype=torch.float32, device="cuda")
    rows = torch.zeros((streams * 2, n), dtype=torch.float32, device="cuda")
    for i, new in enumerate([256, 100, 256, n, 100, 8, 3]):
        pcm = lcg_pcm_fast(500 + i, streams * new * 2)
        x = torch.from_numpy(pcm.astype(np.float32) / np.float32(30000)).cuda() if f32 else torch.from_numpy(pcm).cuda()
        r16 = i % 2 == 0
        if f32:
            b.ring_update_f32(x, new, o16 if r16 else of, G.OP_WAVE | (G.OP_R16 if r16 else 0)); twin.ring_append_f32(x, new)
        else:
            b.ring_update_s16(x, new, o16 if r16 else of, G.OP_WAVE | (G.OP_R16 if r16 else 0)); twin.ring_append_s16(x, new)
        twin.ring_planar(rows, f32_ring=f32)
        torch.cuda.synchronize()
        want = upload(rows.cpu().numpy())
        if r16: assert same(dev_u16(o16), want), (i, new)
        else: assert same(of.cpu().numpy(), texel_floats(want)), (i, new)
    b.close(); twin.close()


# ---- 3. the texture -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("factor", [0.025, 0.05])
@pytest.mark.parametrize("n", [1024, 4096, 16384])
def test_the_texture_the_wave_module_samples(glvlib, oracle, n, factor):
    """GLV_OP_WAVE | GLV_OP_BARS with bars = n, bar_phase 0.5 on gl_storage 1: the pre-smoothing pass over the upload's texels, the exact integer
    mean of glvo_bars_int_at for every row -- as texels and as floats, in one launch from s16 frames and from the s16 ring"""
    import torch
    G = glvlib
    streams = 3
    p = G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=1, smooth_factor=factor)
    b = G.Batch(p, streams, G.OP_WAVE | G.OP_BARS | G.OP_RING_S16)
    assert b.bars_arithmetic() == G.BARS_I8_EXACT
    pcm = lcg_pcm_fast(40 + n, streams * 2 * n)
    d_pcm = torch.from_numpy(pcm).cuda()
    o16 = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda")
    of = torch.zeros((streams * 2, n), dtype=torch.float32, device="cuda")
    b.process_s16(d_pcm, o16, G.OP_WAVE | G.OP_BARS | G.OP_R16)
    assert b.last_launches() == 1, b.last_launches()
    assert b.kernel_name() == "glv_bars_rows_i8_kernel"
    b.process_s16(d_pcm, of, G.OP_WAVE | G.OP_BARS)
    assert b.last_launches() == 1
    torch.cuda.synchronize()
    up = upload(planar_of_s16(pcm, streams, n))
    got16, gotf = dev_u16(o16), of.cpu().numpy()
    for r in range(streams * 2):
        t, f = Oracle.bars_int(up[r], n, factor, 0.5)
        assert same(got16[r], t), (r, np.flatnonzero(got16[r] != t)[:5])
        assert same(gotf[r], f), r
    # the input bytes counted are the frames the bars sample
    assert b.algorithmic_bytes(G.OP_WAVE | G.OP_BARS | G.OP_R16, True) < streams * (4 * n * 0.4 + 4 * n)
    # the s16 ring, rotated by whole groups of frames: one launch
    twin = G.Batch(G.Params(n=n), streams, G.OP_RING_S16)
    rows = torch.zeros((streams * 2, n), dtype=torch.float32, device="cuda")
    for i in range(3):
        new = torch.from_numpy(lcg_pcm_fast(70 + i, streams * 256 * 2)).cuda()
        b.ring_update_s16(new, 256, o16, G.OP_WAVE | G.OP_BARS | G.OP_R16)
        assert b.last_launches() == 1
        twin.ring_append_s16(new, 256)
    twin.ring_planar(rows)
    torch.cuda.synchronize()
    up = upload(rows.cpu().numpy())
    got16 = dev_u16(o16)
    for r in range(streams * 2):
        assert same(got16[r], Oracle.bars_int(up[r], n, factor, 0.5)[0]), r
    # ... by a number of frames that is not a multiple of 8: the waveform kernel, then the pass -- the same texels' model
    new = torch.from_numpy(lcg_pcm_fast(75, streams * 100 * 2)).cuda()
    b.ring_update_s16(new, 100, o16, G.OP_WAVE | G.OP_BARS | G.OP_R16)
    assert b.last_launches() == 2
    twin.ring_append_s16(new, 100)
    twin.ring_planar(rows)
    torch.cuda.synchronize()
    up = upload(rows.cpu().numpy())
    got16 = dev_u16(o16)
    for r in range(streams * 2):
        assert same(got16[r], Oracle.bars_int(up[r], n, factor, 0.5)[0]), r
    b.close(); twin.close()


@gpu
@pytest.mark.parametrize("kind", ["f32", "f32_stereo", "ring_f32", "s16_mono"])
def test_the_texture_from_the_other_inputs(glvlib, oracle, kind):
    import torch
    G = glvlib
    streams, n = 3, 4096
    ch = 1 if kind == "s16_mono" else 2
    b = G.Batch(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=1, channels=ch), streams, G.OP_WAVE | G.OP_BARS | G.OP_RING_F32)
    pcm = lcg_pcm_fast(91, streams * 2 * n)
    x = (pcm.astype(np.float32) / np.float32(29000)).astype(np.float32)
    o16 = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda")
    if kind == "f32":
        b.process_f32(torch.from_numpy(x).cuda(), o16, G.OP_WAVE | G.OP_BARS | G.OP_R16); planar = x.reshape(streams * 2, n)
    elif kind == "f32_stereo":
        b.process_f32_stereo(torch.from_numpy(x).cuda(), o16, G.OP_WAVE | G.OP_BARS | G.OP_R16); planar = planar_of_f32(x, streams, n)
    elif kind == "ring_f32":
        b.ring_update_f32(torch.from_numpy(x).cuda(), n, o16, G.OP_WAVE | G.OP_BARS | G.OP_R16); planar = planar_of_f32(x, streams, n)
    else:
        b.process_s16(torch.from_numpy(pcm).cuda(), o16, G.OP_WAVE | G.OP_BARS | G.OP_R16); planar = planar_of_s16(pcm, streams, n, channels=1)
    assert b.last_launches() == (1 if kind == "s16_mono" else 2)
    torch.cuda.synchronize()
    up = upload(planar)
    got = dev_u16(o16)
    for r in range(streams * 2):
        assert same(got[r], Oracle.bars_int(up[r], n, 0.025, 0.5)[0]), (kind, r)
    b.close()


@gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_maximum_and_hybrid(glvlib, oracle, mode):
    import torch
    G = glvlib
    streams, n = 3, 4096
    b = G.Batch(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=1, sample_mode=mode), streams, G.OP_WAVE | G.OP_BARS)
    assert b.bars_arithmetic() == G.BARS_F32_SEQ
    pcm = lcg_pcm_fast(17 + mode, streams * 2 * n)
    o16 = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda")
    of = torch.zeros((streams * 2, n), dtype=torch.float32, device="cuda")
    b.process_s16(torch.from_numpy(pcm).cuda(), o16, G.OP_WAVE | G.OP_BARS | G.OP_R16)
    assert b.last_launches() == 2
    b.process_s16(torch.from_numpy(pcm).cuda(), of, G.OP_WAVE | G.OP_BARS)
    torch.cuda.synchronize()
    up = upload(planar_of_s16(pcm, streams, n))
    for r in range(streams * 2):
        want = Oracle.bars_mode(texel_floats(up[r]), n, mode, 0.65, 0.025, 0.5)
        assert same(of.cpu().numpy()[r], want), r
        assert same(dev_u16(o16)[r], Oracle.texels_r16(want)), r
    b.close()


@gpu
@pytest.mark.parametrize("r16", [True, False])
def test_fewer_than_256_bars_take_the_float_chain(glvlib, oracle, r16):
    """GLV_OP_WAVE | GLV_OP_BARS with the modules' 80 bars: the waveform kernel writes the texels' floats, glv_bars_kernel samples them -- the same
    bits as glv_batch_bars over those floats (GLV_BARS_F32_CHAIN; the chain's own arithmetic is pinned by the existing bars tests)"""
    import torch
    G = glvlib
    streams, n = 3, 4096
    b = G.Batch(G.Params(n=n, bars=80, gl_storage=1), streams, G.OP_WAVE | G.OP_BARS)
    assert b.bars_arithmetic() == G.BARS_F32_CHAIN
    pcm_h = lcg_pcm_fast(61, streams * 2 * n)
    pcm = torch.from_numpy(pcm_h).cuda()
    o = torch.zeros((streams * 2, 80), dtype=torch.int16 if r16 else torch.float32, device="cuda")
    b.process_s16(pcm, o, G.OP_WAVE | G.OP_BARS | (G.OP_R16 if r16 else 0))
    assert b.last_launches() == 2
    torch.cuda.synchronize()
    up = upload(planar_of_s16(pcm_h, streams, n))
    rows = torch.from_numpy(texel_floats(up)).cuda()
    ref = torch.zeros((streams * 2, 80), dtype=torch.float32, device="cuda")
    b.bars(rows, ref)
    torch.cuda.synchronize()
    want = ref.cpu().numpy()
    for r in range(streams * 2):                                  # ... which is the oracle's chunked chain over the texel floats
        w = np.empty(80, np.float32)
        Oracle.lib().glvo_bars_chunked_at(np.ascontiguousarray(texel_floats(up[r])), n, w, 80, 0.025, 0.0)
        assert same(want[r], w), r
    if r16: assert same(dev_u16(o), Oracle.texels_r16(want))
    else: assert same(o.cpu().numpy(), want)
    b.close()


@gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_bar_texels_with_maximum_and_hybrid(glvlib, oracle, mode):
    import torch
    from glava_amd.bar_positions import wave_column_texels
    G = glvlib
    streams, n = 3, 4096
    tex, _ = wave_column_texels(n, 320)
    kw = dict(n=n, gl_storage=1, sample_mode=mode)
    snap = G.Batch(G.Params(bars=len(tex), **kw), streams, G.OP_WAVE | G.OP_BARS)
    twin = G.Batch(G.Params(bars=n, bar_phase=0.5, **kw), streams, G.OP_WAVE | G.OP_BARS)
    snap.set_bar_texels(tex)
    assert snap.bars_arithmetic() == twin.bars_arithmetic() == G.BARS_F32_SEQ
    pcm = torch.from_numpy(lcg_pcm_fast(62 + mode, streams * 2 * n)).cuda()
    idx = torch.from_numpy(tex.astype(np.int64)).cuda()
    for r16 in (True, False):
        dt = torch.int16 if r16 else torch.float32
        ops = G.OP_WAVE | G.OP_BARS | (G.OP_R16 if r16 else 0)
        o_s = torch.zeros((streams * 2, len(tex)), dtype=dt, device="cuda"); o_t = torch.zeros((streams * 2, n), dtype=dt, device="cuda")
        snap.process_s16(pcm, o_s, ops); twin.process_s16(pcm, o_t, ops)
        assert snap.last_launches() == 2
        torch.cuda.synchronize()
        want = o_t[:, idx].contiguous()
        assert same(o_s.cpu().numpy(), want.cpu().numpy()), (mode, r16)
    snap.close(); twin.close()


@gpu
def test_mono_ring_rotated_inside_a_group_of_frames(glvlib, oracle):
    """channels = 1 and an s16 ring whose oldest frame is not at a multiple of 8: two launches, the texture of the ring's mono rows"""
    import torch
    G = glvlib
    streams, n = 3, 4096
    b = G.Batch(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=1, channels=1), streams, G.OP_WAVE | G.OP_BARS | G.OP_RING_S16)
    twin = G.Batch(G.Params(n=n, channels=1), streams, G.OP_RING_S16)
    o16 = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda")
    rows = torch.zeros((streams * 2, n), dtype=torch.float32, device="cuda")
    for i, (new, launches) in enumerate([(256, 1), (99, 2), (13, 1), (5, 2)]):        # positions 256, 355, 368, 373
        x = torch.from_numpy(lcg_pcm_fast(80 + i, streams * new * 2)).cuda()
        b.ring_update_s16(x, new, o16, G.OP_WAVE | G.OP_BARS | G.OP_R16)
        assert b.last_launches() == launches, (i, b.last_launches())
        twin.ring_append_s16(x, new)
        twin.ring_planar(rows)
        torch.cuda.synchronize()
        up = upload(rows.cpu().numpy())
        assert (up[0] == up[1]).all()
        got = dev_u16(o16)
        for r in range(streams * 2):
            assert same(got[r], Oracle.bars_int(up[r], n, 0.025, 0.5)[0]), (i, r)
    b.close(); twin.close()


# ---- 4. bar texels ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w", [320, 800, 1920])
def test_bar_texels_over_the_wave_texture(glvlib, oracle, w):
    import torch
    from glava_amd.bar_positions import wave_column_texels
    G = glvlib
    streams, n = 3, 4096
    tex, _ = wave_column_texels(n, w)
    assert len(tex) == w + 2
    kw = dict(n=n, gl_storage=1)
    snap = G.Batch(G.Params(bars=len(tex), **kw), streams, G.OP_WAVE | G.OP_BARS)
    twin = G.Batch(G.Params(bars=n, bar_phase=0.5, **kw), streams, G.OP_WAVE | G.OP_BARS)
    plain = G.Batch(G.Params(bars=len(tex), **kw), streams, G.OP_WAVE | G.OP_BARS)
    pcm = torch.from_numpy(lcg_pcm_fast(23 + w, streams * 2 * n)).cuda()
    idx = torch.from_numpy(tex.astype(np.int64)).cuda()
    before = {}
    for r16 in (True, False):
        dt = torch.int16 if r16 else torch.float32
        ops = G.OP_WAVE | G.OP_BARS | (G.OP_R16 if r16 else 0)
        o = torch.zeros((streams * 2, len(tex)), dtype=dt, device="cuda")
        snap.process_s16(pcm, o, ops)
        torch.cuda.synchronize()
        before[r16] = o.clone()
    snap.set_bar_texels(tex)
    assert snap.bars_arithmetic() == twin.bars_arithmetic() == G.BARS_I8_EXACT
    for r16 in (True, False):
        dt = torch.int16 if r16 else torch.float32
        ops = G.OP_WAVE | G.OP_BARS | (G.OP_R16 if r16 else 0)
        o_s = torch.zeros((streams * 2, len(tex)), dtype=dt, device="cuda")
        o_t = torch.zeros((streams * 2, n), dtype=dt, device="cuda")
        snap.process_s16(pcm, o_s, ops)
        assert snap.last_launches() == 2
        twin.process_s16(pcm, o_t, ops)
        torch.cuda.synchronize()
        want = o_t[:, idx].contiguous()
        assert torch.equal(o_s.view(torch.int32) if not r16 else o_s, want.view(torch.int32) if not r16 else want), (w, r16)
        assert int(o_t.view(torch.int32 if not r16 else torch.int16).ne(0).sum()) > 0
    # cleared: the unsnapped result again, bit for bit
    snap.set_bar_texels(None)
    for r16 in (True, False):
        dt = torch.int16 if r16 else torch.float32
        ops = G.OP_WAVE | G.OP_BARS | (G.OP_R16 if r16 else 0)
        o = torch.zeros((streams * 2, len(tex)), dtype=dt, device="cuda"); o_p = torch.zeros_like(o)
        snap.process_s16(pcm, o, ops); plain.process_s16(pcm, o_p, ops)
        torch.cuda.synchronize()
        v = (lambda t: t.view(torch.int32)) if not r16 else (lambda t: t)
        assert torch.equal(v(o), v(before[r16])) and torch.equal(v(o), v(o_p))
    for x in (snap, twin, plain): x.close()


# ---- 5. the single-stream drop-in -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [1024, 4096])
def test_wave_texture_drop_in(glvlib, oracle, n):
    G = glvlib
    st = G.State(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=1, avg_window_kind=1))
    rng = np.random.default_rng(n)
    for k in range(2):
        buf = (rng.random(n, dtype=np.float32) * np.float32(2.4) - np.float32(1.2)).astype(np.float32)
        keep = buf.copy()
        tex = np.zeros(n, np.uint16)
        st.wave_texture(buf, tex, smooth_pass=False)
        up = upload(keep.reshape(1, n))[0]
        assert same(tex, up)
        st.wave_texture(buf, tex, smooth_pass=True)
        assert same(tex, Oracle.bars_int(up, n, 0.025, 0.5)[0])
        assert same(buf, keep)
    st.close()
    # the upload alone works on any state; the pass needs GL_R16 storage and bars = n
    plain = G.State(G.Params(n=n))
    buf = np.linspace(-1, 1, n, dtype=np.float32)
    tex = np.zeros(n, np.uint16)
    plain.wave_texture(buf, tex, smooth_pass=False)
    assert same(tex, upload(buf.reshape(1, n))[0])
    with pytest.raises(G.GlvError) as ei:
        plain.wave_texture(buf, tex, smooth_pass=True)
    assert ei.value.code == G.ERR_STATE
    plain.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals(glvlib, oracle):
    import torch
    from glava_amd.bar_positions import graph_column_texels
    G = glvlib
    streams, n = 2, 1024
    pcm_h = lcg_pcm_fast(5, streams * 2 * n)
    pcm = torch.from_numpy(pcm_h).cuda()
    f32 = torch.from_numpy(pcm_h.astype(np.float32) / np.float32(32768)).cuda()
    out = torch.zeros((streams * 2, n), dtype=torch.float32, device="cuda")
    o16 = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda")
    want = upload(planar_of_s16(pcm_h, streams, n))

    def refused(code, fn):
        with pytest.raises(G.GlvError) as ei:
            fn()
        assert ei.value.code == code, (ei.value.code, str(ei.value))
        assert G.lib().glv_last_error().decode() != ""

    def still_works(b):
        b.process_s16(pcm, o16, G.OP_WAVE | G.OP_R16)
        torch.cuda.synchronize()
        assert same(dev_u16(o16), want)

    full = G.Batch(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=1, avg_window_kind=1), streams,
                   G.OP_WAVE | G.OP_BARS | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_SMOOTH)
    for extra in (G.OP_FFT, G.OP_GRAVITY, G.OP_AVERAGE, G.OP_FFT | G.OP_RAW, G.OP_WRANGE, G.OP_MAGNITUDE, G.OP_SMOOTH, G.OP_GRAVITY | G.OP_OUTPUT_IS_STATE,
                  G.OP_OUTPUT_IS_STATE):
        refused(G.ERR_INVALID, lambda: full.process_s16(pcm, out, G.OP_WAVE | extra))
        refused(G.ERR_INVALID, lambda: full.process_f32(f32, out, G.OP_WAVE | extra))
    still_works(full)
    # a float chain has no texel rows
    fl = G.Batch(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=0), streams, G.OP_WAVE | G.OP_BARS)
    refused(G.ERR_STATE, lambda: fl.process_s16(pcm, out, G.OP_WAVE | G.OP_BARS))
    still_works(fl)
    # either bit missing from the creation mask
    for mask in (G.OP_WAVE, G.OP_BARS, G.OP_BARS | G.OP_GRAVITY | G.OP_AVERAGE):
        nb = G.Batch(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=1, avg_window_kind=1), streams, mask)
        refused(G.ERR_STATE, lambda: nb.process_s16(pcm, o16, G.OP_WAVE | G.OP_BARS | G.OP_R16))
        still_works(nb)
        nb.close()
    # column texels: the wave shader does not average three texels
    table, _, _ = graph_column_texels(n, 320)
    col = G.Batch(G.Params(n=n, bars=len(table), gl_storage=1, avg_window_kind=1), streams, G.OP_WAVE | G.OP_BARS | G.OP_GRAVITY | G.OP_AVERAGE)
    col.set_column_texels(table)
    refused(G.ERR_STATE, lambda: col.process_s16(pcm, out, G.OP_WAVE | G.OP_BARS))
    refused(G.ERR_STATE, lambda: col.process_s16(pcm, o16, G.OP_WAVE | G.OP_R16))
    refused(G.ERR_STATE, lambda: col.process_f32(f32, out, G.OP_WAVE))
    col.process_s16(pcm, out, G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS)   # the batch still works: its columns
    col.set_column_texels(None)
    still_works(col)
    col.process_s16(pcm, out, G.OP_WAVE | G.OP_BARS)              # ... and without the table the call is taken
    # without the feature's bit nothing changed: GLV_OP_BARS alone is still no chain
    refused(G.ERR_INVALID, lambda: full.process_s16(pcm, out, G.OP_BARS))
    for x in (full, fl, col): x.close()


# ---- 7. hipGraph ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("unfused", [False, True])
def test_graph_capture(glvlib, oracle, unfused, monkeypatch):
    """the first WAVE | BARS | R16 call of a batch is captured and replayed on new PCM: nothing allocates, the results are those of direct calls"""
    import torch
    G = glvlib
    streams, n = 5, 4096
    if unfused:
        monkeypatch.setenv("GLV_UNFUSED_WAVE", "1")
    p = G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=1)
    b = G.Batch(p, streams, G.OP_WAVE | G.OP_BARS)
    monkeypatch.delenv("GLV_UNFUSED_WAVE", raising=False)
    direct = G.Batch(p, streams, G.OP_WAVE | G.OP_BARS)
    ops = G.OP_WAVE | G.OP_BARS | G.OP_R16
    pcm = torch.from_numpy(lcg_pcm_fast(4321, streams * 2 * n)).cuda()
    o = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda"); od = torch.zeros_like(o)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        b.process_s16(pcm, o, ops, stream=s.cuda_stream)
    assert b.last_launches() == (2 if unfused else 1)
    for i in range(2):
        pcm.copy_(torch.from_numpy(lcg_pcm_fast(600 + i, streams * 2 * n)).cuda())
        torch.cuda.synchronize()
        g.replay()
        direct.process_s16(pcm, od, ops)
        torch.cuda.synchronize()
        assert torch.equal(o, od), i
        assert int(o.ne(0).sum()) > 0
    del g
    b.close(); direct.close()


# ---- 8. existing behaviour --------------------------------------------------------------------------------------------------------------
@gpu
def test_wrange_is_what_it_was_on_a_wave_batch(glvlib, oracle):
    import torch
    G = glvlib
    streams, n = 4, 2048
    x = _special_floats(streams * 2 * n, 11)
    d = torch.from_numpy(x).cuda()
    res = []
    for mask in (G.OP_WAVE | G.OP_BARS, G.OP_BARS, 0):
        b = G.Batch(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=1), streams, mask | G.OP_FFT)
        of = torch.zeros((streams * 2, n), dtype=torch.float32, device="cuda")
        o16 = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda")
        b.process_f32(d, of, G.OP_WRANGE)
        b.process_f32(d, o16, G.OP_WRANGE | G.OP_R16)
        torch.cuda.synchronize()
        res.append((of.cpu().numpy(), dev_u16(o16)))
        b.close()
    for f, t in res[1:]:
        assert same(res[0][0], f) and same(res[0][1], t)
    w = wrange(x.reshape(streams * 2, n))
    fin = ~np.isnan(w)                                            # (a NaN stays a NaN; its payload is the device's business)
    assert same(res[0][0][fin], w[fin]) and np.isnan(res[0][0][~fin]).all()
    assert same(res[0][1], upload(x.reshape(streams * 2, n)))


# ---- 9. CPU -----------------------------------------------------------------------------------------------------------------------------
def test_wave_column_texels_follow_the_specification():
    from glava_amd.bar_positions import wave_column_texels
    for n in (1024, 4096):
        t, edge = wave_column_texels(n, n)
        assert len(t) == n + 2 and t.dtype == np.uint32
        assert (t[1:-1] == np.arange(n)).all() and t[0] == n - 1 and t[-1] == 0
        assert not edge.any()
    for n, w in ((4096, 320), (4096, 800), (4096, 1920), (1024, 1366), (4096, 4097), (16384, 7)):
        t, edge = wave_column_texels(n, w)
        assert len(t) == w + 2 and (t < n).all()
        inner = t[1:-1].astype(np.int64)
        assert (np.diff(inner) >= 0).all() and inner[0] == 0                     # monotone on 0 .. w - 1
        assert t[-1] == 0                                                         # screen_w wraps to texel 0
        # GL 4.5 section 8.14 in exact arithmetic wherever the float coordinate is not within an ulp of a texel boundary
        x = np.arange(-1, w + 1, dtype=np.int64)
        exact = np.mod(np.floor_divide(x * n, w), n)
        assert (t[~edge] == exact[~edge]).all()
    # a width whose odd part is large puts coordinates within one float ulp of a boundary without being on it: flagged
    t, edge = wave_column_texels(4096, 4097)
    assert edge.any() and edge[4096 + 1]


def test_constant_header_and_symbol():
    from glava_amd import spectrum
    assert spectrum.OP_WAVE == 1 << 14
    hdr = open(os.path.join(ROOT, "include", "glv_spectrum.h")).read()
    assert re.search(r"GLV_OP_WAVE\s*=\s*1u << 14", hdr)
    assert re.search(r"int glv_wave_texture\(const glv_params\* p, glv_state\* s, const float\* buf, int smooth_pass, uint16_t\* texels\);", hdr)
    from glava_amd import build as B
    B.build()
    L = spectrum.lib()
    assert hasattr(L, "glv_wave_texture")
    assert L.glv_abi_version() == 7
    assert hasattr(spectrum.State, "wave_texture")
