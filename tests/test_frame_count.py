"""GPU: every averaging path at frame counts 1 to 64.

`avg_frames` (F) is a run-time parameter the ABI accepts anywhere in [1, GLV_MAX_AVG_FRAMES = 64]; every stateful kernel has loops, ring indices and table
sizes that depend on it.  The rest of the suite runs F <= 7 on texel chains, F <= 5 in the live classes and in track calls.  This module walks

    FS = (1, 2, 5, 6, 7, 8, 16, 17, 33, 63, 64)

    1        no average pass; the gravity store is the ring slot itself
    2        one old slot (and the one frame count whose windowed weights are all 1: the shader's product is skipped)
    5        the live classes' prefetch alone: npre = F - 1 = kLivePre (glv_frame.h gl16_state_prefetch), no leftover trip
    6        the first leftover trip behind the prefetch (`for (; f + 1 < F; ++f)` from f = npre): the gravity store comes out of that trip, not out of
             a prefetched slot (`k + 2 == F` is never true)
    7        two leftover trips
    8 .. 33  both parities: the two-frames-per-trip loops (apply_state_block PAIR, gl16_state_block TWO) walk F - 1 old slots -- an odd F ends on a
             pair, an even F on a single slot taken by the one-frame loop behind
    63, 64   the last entries of the 64-entry weight tables (FrameArgs::wts / wts32 [F - 1]) and the largest LDS ring of glv_track_scan_kernel
             (F x 64 lanes x 8 bytes = 32 KiB on float rows)

through every kernel class and entry that keeps a ring.  Every stateful sequence runs F + 3 updates -- loud, quiet (PCM / 64), all-zero, then on -- so that
the ring fills, wraps, and the head passes slot 0.  Every comparison is bit for bit (floats as their 32-bit patterns, texels as uint16); no tolerance
anywhere.  The checkers: the oracle's chain (StreamOracle, log_mode 0: the compiled reference's bits) for float chains, its GL model (transform_fft +
glvo_gl_chain_r16, no texel excluded) for texel chains, and for everything else a second device path documented as bit-identical (the pass-by-pass form,
a batch without GLV_OP_BARS_ONLY, the sequential calls of a track, a one-stream batch, the automatic grid).

Sizes are the smallest at which the path can still go wrong: n = 256, and n = 8192 / 16384 on either side of GLV_STATE_PAIR_MAX (log2(n / 2) = 12) where the
two-frames-per-trip loops are compiled in or out; 7 streams at n = 256 and 3 above (odd: a workgroup's last group of rows is ragged); the live classes at
the smallest size that takes them.  Where a size has several kernel configurations (glv_batch_variants) every one runs, and configuration 0 is asserted to."""
import ctypes as C

import numpy as np
import pytest

from glava_amd.bar_positions import graph_column_texels, radial_bar_texels
from oracle_lib import Oracle, StreamOracle, lcg_pcm_fast
from track_lib import eq as _eq, hop_windows as _windows, pcm as _pcm, seq as _seq, to_device, track, with_table as _with_table

pytestmark = pytest.mark.gpu

FS = (1, 2, 5, 6, 7, 8, 16, 17, 33, 63, 64)
CHAIN_SIZES = (256, 8192, 16384)                 # ... and the sizes next to GLV_STATE_PAIR_MAX on either side
GS, UR = 4.2, 86.1328125


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _streams(n):
    return 7 if n <= 4096 else 3


# ---- inputs and references, computed once per (size, update) and shared by every test that needs them; never modified ------------------------------
_PCM, _SPEC = {}, {}


def _update(n, streams, u):
    """update u of every sequence of this size: int16 [streams * 2 * n]; u = 0 loud, 1 quiet (PCM / 64), 2 all-zero, then / 8, loud, quiet, ..."""
    key = (n, streams, u)
    if key not in _PCM:
        pcm = (lcg_pcm_fast(4200 + u + n, streams * 2 * n) // (1, 64, 8)[u % 3]).astype(np.int16)
        if u == 2: pcm[:] = 0
        pcm.setflags(write=False)
        _PCM[key] = pcm
    return _PCM[key]


def _spectra(n, streams, u):
    """transform_fft of update u (the oracle's; no state): float32 [streams * 2][n]"""
    key = (n, streams, u)
    if key not in _SPEC:
        pcm = _update(n, streams, u)
        spec = np.concatenate([StreamOracle(n, gravity=False, average=False).frame(pcm[s * 2 * n:(s + 1) * 2 * n]) for s in range(streams)])
        spec.setflags(write=False)
        _SPEC[key] = spec
    return _SPEC[key]


def _gl_model(n, streams, F, win):
    """the GL_R16 chain's texels of F + 3 updates: glvo_gl_chain_r16 on the oracle's spectra, row by row"""
    rows = streams * 2
    store = np.zeros((rows, n), np.float32); hist = np.zeros((rows, F, n), np.float32)
    heads = [C.c_size_t(0) for _ in range(rows)]
    out = []
    for u in range(F + 3):
        spec = _spectra(n, streams, u)
        tex = np.empty((rows, n), np.uint16)
        for r in range(rows):
            row = spec[r].copy()
            Oracle.lib().glvo_gl_chain_r16(row, store[r], hist[r], C.byref(heads[r]), n, F, int(win), 1, GS, UR)
            tex[r] = Oracle.texels_r16(row)
        out.append(tex)
    return out


def _float_model(n, streams, F, win, gravity):
    """fft (-> gravity) -> average of F + 3 updates, float32 [streams * 2][n] per update: StreamOracle.frame's own steps (oracle/glv_oracle.c glvo_frame_s16:
    transform_fft, glvo_gravity, glvo_average per channel row) with the transform taken from the cache above -- it does not depend on F.  At n = 256 the
    composition is checked against StreamOracle itself on every call."""
    rows = streams * 2
    grav = np.zeros((rows, n), np.float32); hist = np.zeros((rows, F, n), np.float32)
    heads = [C.c_size_t(0) for _ in range(rows)]
    sos = [StreamOracle(n, avg_frames=F, avg_window=win, gravity=gravity, average=True) for _ in range(streams)] if n == 256 else None
    out = []
    with np.errstate(all="ignore"):
        for u in range(F + 3):
            want = _spectra(n, streams, u).copy()
            for r in range(rows):
                if gravity: Oracle.gravity(want[r], grav[r], GS, UR)
                Oracle.average(want[r], hist[r], heads[r], F, win)
            if sos:
                pcm = _update(n, streams, u)
                whole = np.concatenate([sos[s].frame(pcm[s * 2 * n:(s + 1) * 2 * n]) for s in range(streams)])
                assert (bits(whole) == bits(want)).all(), "the composed reference is not StreamOracle's"
            out.append(want)
    return out


def _variants(G, p, mask):
    b = G.Batch(p, 1, mask)
    nv = b.variants(); b.close()
    assert nv >= 1
    return nv


def _batch(G, p, streams, mask, variant):
    b = G.Batch(p, streams, mask)
    b.set_variant(variant)
    return b


# ---- 1. the GL_R16 chain in one launch (FC_GL16), and glv_post_kernel's pass-by-pass branch; 8. the algorithmic bytes -------------------------------
@pytest.mark.parametrize("win", [True, False])
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("n", CHAIN_SIZES)
def test_gl_r16_chain_equals_the_oracle_model_and_the_pass_by_pass_form(glvlib, oracle, n, F, win):
    """FFT | GRAVITY | AVERAGE | R16 on gl_storage 1, avg_window_kind 1, window on and off: texels equal to the oracle's model on every texel of every
    update, and to a gl_storage 2 batch (the transform, then glv_post_kernel's apply_state on float state with the same F); the float-output form gives the
    texels' read-back values c / 65535.  Every F of FS.  glv_batch_algorithmic_bytes of the texel form is (8 + 4 F) n per frame and stream: 4 n in,
    4 (F - 1) n of ring slots read, 4 n written, 4 n out (28 n at F = 5)."""
    import torch
    G = glvlib
    streams = _streams(n)
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    ops = G.OP_FFT | GA
    kw = dict(n=n, avg_frames=F, avg_window=win, avg_window_kind=1, log_mode=0)
    want = _gl_model(n, streams, F, win)
    nv = _variants(G, G.Params(gl_storage=1, **kw), GA)
    for v in range(nv):
        tex, flt = _batch(G, G.Params(gl_storage=1, **kw), streams, GA, v), _batch(G, G.Params(gl_storage=1, **kw), streams, GA, v)
        split = _batch(G, G.Params(gl_storage=2, **kw), streams, GA | G.OP_BARS, v)
        o_t = torch.full((streams * 2, n), -1, dtype=torch.int16, device="cuda"); o_s = torch.full_like(o_t, -2)
        o_f = torch.full((streams * 2, n), float("nan"), dtype=torch.float32, device="cuda")
        for u in range(F + 3):
            d = torch.tensor(_update(n, streams, u)).cuda()
            tex.process_s16(d, o_t, ops | G.OP_R16)
            assert tex.last_launches() == 1 and tex.last_variant() == v
            flt.process_s16(d, o_f, ops)
            assert flt.last_launches() == 1 and flt.last_variant() == v
            split.process_s16(d, o_s, ops | G.OP_R16)
            assert split.last_launches() >= 2
            got = o_t.cpu().numpy().view(np.uint16)
            bad = got != want[u]
            assert not bad.any(), (n, F, win, v, u, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            assert _eq(o_t, o_s), (n, F, win, v, u, int((o_t != o_s).sum()))
            assert (bits(o_f.cpu().numpy()) == bits(got.astype(np.float32) / np.float32(65535))).all(), (n, F, win, v, u)
        if F >= 2:
            assert tex.algorithmic_bytes(ops | G.OP_R16) == streams * (8 + 4 * F) * n, (F, tex.algorithmic_bytes(ops | G.OP_R16))
        for b in (tex, flt, split): b.close()


# ---- 2. float chains against the oracle's chain (the compiled reference's bits), log_mode 0 ----------------------------------------------------------
def _float_chain_case(G, n, F, gravity, win):
    """FC_STATE, FC_STATE_R16 and FC_STATE_BARS of one (n, F, chain, window) against the reference, in every kernel configuration of the size"""
    import torch
    streams, bars = _streams(n), 80
    mask = (G.OP_GRAVITY if gravity else 0) | G.OP_AVERAGE
    ops = G.OP_FFT | mask
    p = G.Params(n=n, avg_frames=F, avg_window=win, log_mode=0, bars=bars)
    want = _float_model(n, streams, F, win, gravity)
    for v in range(_variants(G, p, mask | G.OP_BARS)):
        flt, r16, fused = _batch(G, p, streams, mask | G.OP_BARS, v), _batch(G, p, streams, mask, v), _batch(G, p, streams, mask | G.OP_BARS, v)
        o_f = torch.full((streams * 2, n), float("nan"), dtype=torch.float32, device="cuda")
        o_q = torch.full((streams * 2, n), -1, dtype=torch.int16, device="cuda")
        d_b1 = torch.full((streams * 2, bars), float("nan"), dtype=torch.float32, device="cuda"); d_b2 = torch.full_like(d_b1, float("nan"))
        for u in range(F + 3):
            d = torch.tensor(_update(n, streams, u)).cuda()
            flt.process_s16(d, o_f, ops); r16.process_s16(d, o_q, ops | G.OP_R16)
            assert flt.last_launches() == 1 and flt.last_variant() == v and r16.last_launches() == 1 and r16.last_variant() == v
            bad = bits(o_f.cpu().numpy()) != bits(want[u])
            assert not bad.any(), (n, F, gravity, win, v, u, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            bad = o_q.cpu().numpy().view(np.uint16) != Oracle.texels_r16(want[u])
            assert not bad.any(), ("r16", n, F, gravity, win, v, u, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            flt.bars(o_f, d_b1)                                             # glv_batch_bars over spectra that equal the reference's
            fused.process_s16(d, d_b2, ops | G.OP_BARS)
            assert fused.last_variant() == v
            if v == 0 and n >= 1024: assert fused.last_launches() == 1, fused.last_launches()
            assert _eq(d_b1, d_b2), ("bars", n, F, gravity, win, v, u, int((d_b1.view(torch.int32) != d_b2.view(torch.int32)).sum()))
        for b in (flt, r16, fused): b.close()


@pytest.mark.parametrize("win", [True, False])
@pytest.mark.parametrize("gravity", [True, False])
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("n", CHAIN_SIZES + (1024,))
def test_float_chains_equal_the_reference(glvlib, oracle, n, F, gravity, win):
    """FFT | AVERAGE and FFT | GRAVITY | AVERAGE, avg_window (kind 0) on and off, in kernel classes FC_STATE (floats out) and FC_STATE_R16 (GLV_OP_R16: the
    texels of the reference's row): every value of every update.  FC_STATE_BARS: 80 bars computed inside the frame kernel from the finished row in LDS, one
    launch -- against glv_batch_bars over the FC_STATE batch's spectra, which were just asserted equal to the reference.  Bars fuse where whole waves own a
    row: n = 1024 is the smallest such size and runs for that class; at n = 256 the same comparison holds with the bars in a second launch, and a
    configuration that cannot fuse (n = 16384, configuration 1) takes two launches as well.  Every F of FS."""
    _float_chain_case(glvlib, n, F, gravity, win)


# ---- 3. the unfused post kernel on float state -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", [True, False])
@pytest.mark.parametrize("F", FS)
def test_post_kernel_on_planar_rows(glvlib, oracle, F, win):
    """glv_batch_process_f32 with GRAVITY | AVERAGE and no FFT (glv_post_kernel, apply_state on float state): planar rows in, against Oracle.gravity then
    Oracle.average row by row.  n = 256, 7 streams; every F of FS."""
    import torch
    G = glvlib
    n, streams = 256, 7
    rows = streams * 2
    rng = np.random.default_rng(1000 + F)
    b = G.Batch(G.Params(n=n, avg_frames=F, avg_window=win), streams, G.OP_GRAVITY | G.OP_AVERAGE)
    grav = np.zeros((rows, n), np.float32); hist = np.zeros((rows, F, n), np.float32)
    heads = [C.c_size_t(0) for _ in range(rows)]
    d_out = torch.full((rows, n), float("nan"), dtype=torch.float32, device="cuda")
    for u in range(F + 3):
        x = (rng.random((rows, n), dtype=np.float32) * np.float32(2.0) - np.float32(0.5)) / np.float32((1, 64, 8)[u % 3])
        if u == 2: x[:] = 0
        x = x.astype(np.float32)
        b.process_f32(torch.from_numpy(x).cuda(), d_out, G.OP_GRAVITY | G.OP_AVERAGE)
        assert b.last_launches() == 1 and b.kernel_name() == "glv_post_kernel"
        want = x.copy()
        for r in range(rows):
            Oracle.gravity(want[r], grav[r], GS, UR)
            Oracle.average(want[r], hist[r], heads[r], F, win)
        bad = bits(d_out.cpu().numpy()) != bits(want)
        assert not bad.any(), (F, win, u, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    b.close()


# ---- 4. the live classes (GLV_OP_BARS_ONLY) ----------------------------------------------------------------------------------------------------------
def _live_cases(G):
    """name -> (kernel class, candidate (n, parameters, table) in ascending size, ops, launches of configuration 0).  The first candidate whose
    glv_batch_live_bins is not 0 runs -- the smallest size that takes the live class; the fused forms' candidates are the sizes of
    tests/test_gl_fused.py test_bars_only_with_the_bars_fused_is_the_full_chain, the table forms' the smallest sizes at which tests/test_snapped_bars.py and
    tests/test_column_texels.py see their table fused."""
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    gl = dict(avg_window_kind=1, gl_storage=1)
    chain = G.OP_FFT | GA | G.OP_BARS
    sizes = (256, 512, 1024, 2048, 4096)
    radial = lambda n: ("bar", radial_bar_texels(n, 160)[0])            # noqa: E731
    cols = lambda n: ("col", graph_column_texels(n, 320)[0])            # noqa: E731
    return {
        "7_smallest": (7, [(n, dict(bars=n, bar_phase=0.5, smooth_factor=0.025, **gl), None) for n in sizes], chain | G.OP_R16, 2),
        "7_shipped": (7, [(4096, dict(bars=4096, bar_phase=0.5, smooth_factor=0.025, **gl), None)], chain | G.OP_R16, 2),
        "8": (8, [(1024, dict(bars=80), None), (4096, dict(bars=80), None), (8192, dict(bars=100), None), (16384, dict(bars=80), None)], chain, 1),
        "9": (9, [(2048, dict(bars=64, **gl), None), (4096, dict(bars=80, **gl), None), (16384, dict(bars=80, **gl), None)], chain | G.OP_R16, 1),
        "11": (11, [(n, dict(bars=len(radial(n)[1]), **gl), radial(n)) for n in (1024, 4096)], chain | G.OP_R16, 1),
        "13": (13, [(4096, dict(bars=len(cols(4096)[1]), **gl), cols(4096))], chain, 1),
    }


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("case", ["7_smallest", "7_shipped", "8", "9", "11", "13"])
def test_live_classes_are_the_full_chain(glvlib, case, F):
    """A GLV_OP_BARS_ONLY batch against the same batch without the flag, update by update: FC_GL16_LIVE (7; the pre-smoothing pass in a second launch, at
    the smallest size with live bins and at the shipped 4096), FC_STATE_BARS_LIVE (8) and FC_GL16_BARS_LIVE (9; 80 / 64 bars fused), the bar-texel and
    column-texel live classes (11, 13; tables of glava_amd.bar_positions).  The GL live classes request min(F - 1, 4) ring slots before the transform; from
    F = 6 on the rest -- and the gravity store -- come out of the leftover loop, which no F <= 5 enters.  The test asserts that the live class ran:
    glv_batch_live_bins != 0 and the launch count of the class (configuration 0: one launch where the bars are fused, two for class 7; another
    configuration may not fuse and then takes class 7 or the full chain plus a bars launch, as the unflagged batch does).  Every F of FS."""
    import torch
    G = glvlib
    cls, candidates, ops, launches = _live_cases(G)[case]
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    mask = GA | G.OP_BARS
    chosen = None
    for n, kw, table in candidates:
        probe = _with_table(G.Batch(G.Params(n=n, avg_frames=F, **kw), 1, mask | G.OP_BARS_ONLY), table)
        L = probe.live_bins(); probe.close()
        if L != 0:
            chosen = (n, kw, table)
            break
    assert chosen is not None, f"no candidate size takes live class {cls}"
    n, kw, table = chosen
    streams = _streams(n)
    p = G.Params(n=n, avg_frames=F, **kw)
    w = kw["bars"]
    dt = torch.int16 if ops & G.OP_R16 else torch.float32
    nv = _variants(G, p, mask)
    for v in range(nv):
        full, live = _with_table(_batch(G, p, streams, mask, v), table), _with_table(_batch(G, p, streams, mask | G.OP_BARS_ONLY, v), table)
        assert full.live_bins() == 0 and live.live_bins() != 0 and live.live_bins() < n, (case, n, live.live_bins())
        o_f = torch.full((streams * 2, w), -1, dtype=dt, device="cuda"); o_l = torch.full_like(o_f, -2)
        for u in range(F + 3):
            d = torch.tensor(_update(n, streams, u)).cuda()
            full.process_s16(d, o_f, ops); live.process_s16(d, o_l, ops)
            assert live.last_variant() == v and full.last_variant() == v
            if v == 0 or cls == 7: assert live.last_launches() == launches, (case, n, v, live.last_launches())
            assert live.last_launches() == full.last_launches()
            assert _eq(o_f, o_l), (case, n, F, v, u, int((o_f != o_l).sum()))
        assert live.live_bins() != 0
        assert bool((o_f != 0).any()), (case, "nothing but zeros came out")
        full.close(); live.close()


# ---- 5. track calls ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("chain", ["chain", "gl_chain_r16"])
@pytest.mark.parametrize("entry", ["track", "track_windows"])
def test_track_calls_equal_sequential_calls(glvlib, entry, chain, F):
    """glv_batch_track_s16 (n = 256, hop 64) and glv_batch_track_windows_s16 (hop 45), 3 streams, the float chain FFT | GRAVITY | AVERAGE and the GL chain with
    texels out: glv_track_scan_kernel keeps the F-slot ring in LDS (F x 64 lanes x 4 or 8 bytes) and the host advances the head by (head + steps) % F.
    Per F: steps = F - 1 (F > 1: the ring does not wrap inside the call), F (the head returns to where it was), F + 9 (one more than kTrackDepth + F: the
    ring wraps and the look-ahead refills), and track(F + 1) then track(8) -- the second chunk starts at head 1 (at F = 1 every chunk length is a multiple
    of F; the chunks are 2 and 8).  Every run against glv_batch_process_s16 on the same windows one by one: every step's output, then one more
    process_s16 call on both batches (the ring contents and the head the track call left).  Window 2 of every stream is all-zero; the streams' levels are
    1, 1 / 8 and 1 / 64.  Every F of FS."""
    import torch
    G = glvlib
    n, streams = 256, 3
    old = entry == "track"
    hop = 64 if old else 45
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    kw, ops = (dict(), G.OP_FFT | GA) if chain == "chain" else (dict(gl_storage=1, avg_window_kind=1), G.OP_FFT | GA | G.OP_R16)
    dt = torch.int16 if ops & G.OP_R16 else torch.float32
    p = G.Params(n=n, avg_frames=F, **kw)
    most = F + 10                                                      # windows the longest run touches: F + 9 steps and the update behind them
    pitch = n + (most + 3) * hop if old else (n + most * hop + 38) | 1  # (the residue entry takes multiples of the hop only)
    x = _pcm(600 + F + hop, streams, pitch)
    x[:, 2 * hop:2 * hop + n, :] = 0
    d_pcm = to_device(x, not old, False)                               # (the windows entry: one frame behind an 8-byte boundary)
    wins = _windows(x, n, hop, 0, most)
    bt, bs = G.Batch(p, streams, GA), G.Batch(p, streams, GA)
    first = F + 1 if F > 1 else 2
    runs = ([(F - 1,)] if F > 1 else []) + [(F,), (F + 9,), (first, F + 9 - first)]
    assert first % F != 0 or F == 1
    for chunks in runs:
        bt.reset(); bs.reset()
        steps, t0, got = sum(chunks), 0, []
        for c in chunks:
            got.append(track(bt, "residue" if old else "windows", d_pcm, pitch, hop, c, ops, n, dt, t0=t0))
            assert bt.kernel_name() == "glv_track_scan_kernel" and bt.last_variant() == 0
            t0 += c
        got = torch.cat(got)
        want = _seq(bs, wins[:steps], ops, n, dt)
        for t in range(steps):
            assert _eq(got[t], want[t]), (entry, chain, F, chunks, t, int((got[t] != want[t]).sum()))
        assert _eq(_seq(bt, wins[steps:steps + 1], ops, n, dt), _seq(bs, wins[steps:steps + 1], ops, n, dt)), (entry, chain, F, chunks, "state")
    bt.close(); bs.close()


# ---- 6. the single-row drop-ins ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [6, 64])
def test_single_row_chain_is_the_one_stream_batch(glvlib, F):
    """glv_fft_gravity_average (host samples in, the spectrum out; one state per channel) against a one-stream batch on the same planar rows, F + 3
    updates.  F = 6 and 64: the drop-in runs the batch's kernels on one row, so the other values of FS take no branch here that section 2 does not."""
    import torch
    G = glvlib
    n = 256
    p = G.Params(n=n, avg_frames=F)
    st = [G.State(p) for _ in range(2)]
    b = G.Batch(p, 1, G.OP_GRAVITY | G.OP_AVERAGE)
    out = torch.full((2, n), float("nan"), dtype=torch.float32, device="cuda")
    for u in range(F + 3):
        x = (_update(n, 1, u).reshape(n, 2).T.astype(np.float32) / np.float32(65535)).copy()
        b.process_f32(torch.from_numpy(x).cuda(), out, G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE)
        want = out.cpu().numpy()
        for ch in range(2):
            row = x[ch].copy()
            st[ch].fft_gravity_average(row)
            assert (bits(row) == bits(want[ch])).all(), (F, u, ch)
    for s in st: s.close()
    b.close()


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("F", [6, 64])
def test_single_row_gl_texture_is_the_one_stream_batch(glvlib, F, smooth):
    """glv_gl_texture (smooth_pass 0 and 1) against a one-stream batch of the GL-default chain on the same planar rows, F + 3 updates; n = 1024.  F = 6
    and 64, for the reason given above."""
    import torch
    G = glvlib
    n = 1024
    kw = dict(n=n, avg_frames=F, avg_window_kind=1, gl_storage=1, bars=n, bar_phase=0.5)
    mask = G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS
    st = [G.State(G.Params(**kw)) for _ in range(2)]
    b = G.Batch(G.Params(**kw), 1, mask)
    ops = G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_R16 | (G.OP_BARS if smooth else 0)
    out = torch.full((2, n), -1, dtype=torch.int16, device="cuda")
    for u in range(F + 3):
        x = (_update(n, 1, u).reshape(n, 2).T.astype(np.float32) / np.float32(65535)).copy()
        b.process_f32(torch.from_numpy(x).cuda(), out, ops)
        want = out.cpu().numpy().view(np.uint16)
        for ch in range(2):
            row = x[ch].copy(); tex = np.zeros(n, np.uint16)
            st[ch].gl_texture(row, tex, smooth)
            assert (row == x[ch]).all() and (tex == want[ch]).all(), (F, smooth, u, ch, int((tex != want[ch]).sum()))
    assert want.max() > 0
    for s in st: s.close()
    b.close()


# ---- 7. forced grids ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["chain", "gl_chain_r16"])
@pytest.mark.parametrize("F", [6, 64])
def test_forced_grid_at_large_frame_counts(glvlib, F, chain):
    """glv_batch_set_grid(1) and (2) against the automatic grid, n = 4096 (two rows per workgroup in both configurations), 7 streams: one workgroup makes
    four trips, the last with one frame; the ring's F - 1 loads per row run on every trip.  The float chain and the GL chain with texels out, F + 3
    updates, compared after every update.  F = 6 and 64: the grid changes which workgroup takes a row, not the row's loops."""
    import torch
    G = glvlib
    n, streams = 4096, 7
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    kw, ops = (dict(), G.OP_FFT | GA) if chain == "chain" else (dict(gl_storage=1, avg_window_kind=1), G.OP_FFT | GA | G.OP_R16)
    dt = torch.int16 if ops & G.OP_R16 else torch.float32
    p = G.Params(n=n, avg_frames=F, **kw)
    for v in range(_variants(G, p, GA)):
        auto, one, two = (_batch(G, p, streams, GA, v) for _ in range(3))
        one.set_grid(1); two.set_grid(2)
        outs = [torch.full((streams * 2, n), -1 - i, dtype=dt, device="cuda") for i in range(3)]
        for u in range(F + 3):
            d = torch.tensor(_update(n, streams, u)).cuda()
            for b, o in zip((auto, one, two), outs): b.process_s16(d, o, ops)
            assert one.last_grid() == 1 and two.last_grid() == 2 and auto.last_grid() >= 1
            assert all(b.last_variant() == v and b.last_launches() == 1 for b in (auto, one, two))
            assert _eq(outs[1], outs[0]) and _eq(outs[2], outs[0]), (chain, F, v, u)
        assert bool((outs[0] != 0).any())
        for b in (auto, one, two): b.close()
