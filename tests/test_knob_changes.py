"""GPU: knob changes BETWEEN updates on kept state, on every stateful path.

The host GLava binds to measures `ur` on every frame (render.c:2387; 0 after an interval without updates) and lets a user re-define fft_scale, gravity_step,
avg_window or smooth_factor while it runs.  The library's layer for that -- sync_params (the drop-ins' fast path for ur / gravity_step, the slow path
through glv_batch_set_params), update_gravity_step (the cached integer form of the gravity step on GL_R16 texels), batch_prepare (tables regenerated in
place), the launch-plan cache reset, the restore after a refused change, the track executor's state checks -- is held here to the oracle under the
schedules of tests/test_knob_changes_host.py (pinned there to the compiled reference), update after update, with history in the state.

Everything is bit for bit (floats as uint32, texels as uint16); log_mode 0 wherever the oracle's bits are the expectation.  The one tolerance is the
project's chain_close for the updates a batch spends in log_mode 1."""
import ctypes as C

import numpy as np
import pytest

from glava_amd.bar_positions import graph_column_texels, radial_bar_texels
from gpu_lib import (SIZES, GLModel as _GLModel, bits, float_schedule, frames as _frames, gl_schedule, knob_params as _params, nan_rows as _nan,
                     oracle_bars as _oracle_bars, refused as _refused, texel_rows as _texels, u16 as _u16, updates_of)
from oracle_lib import Oracle, StreamOracle
from track_lib import eq, hop_windows, pcm, pitch_odd, rec, seq, to_device, track

pytestmark = pytest.mark.gpu


def _same(got, want, what):
    bad = bits(got) != bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:3].tolist(), np.asarray(got)[bad][:3], np.asarray(want)[bad][:3])


def _set(so, k):
    so.channels, so.fft_scale, so.fft_cutoff = k.get("channels", 2), k["fft_scale"], k["fft_cutoff"]
    so.gravity_step, so.ur, so.avg_window = k["gravity_step"], k["ur"], k["avg_window"]


def _oracle_rows(so, rows, k):
    """StreamOracle `so` one update further on its two unpacked rows under the knobs k, operator by operator (transform_fft, gravity, average) on its own
    state arrays; avg_window_kind 1: the ring with the GL twin's weights (glvo_average_gl = make_frame_weights kind 1 on float state)"""
    _set(so, k)
    out = np.empty((2, so.n), np.float32)
    for c in range(2):
        row = Oracle.transform_fft(rows[c], so.fft_scale, so.fft_cutoff)
        if so.grav is not None: Oracle.gravity(row, so.grav[c], so.gravity_step, so.ur)
        if so.hist is not None:
            head = C.c_size_t(so.heads[c])
            average = Oracle.lib().glvo_average_gl if k.get("avg_window_kind") else Oracle.lib().glvo_average
            average(row, so.hist[c], C.byref(head), so.n, so.F, int(so.avg_window))
            so.heads[c] = head.value
        out[c] = row
    return out


def _oracle_frame(so, pcm, k):
    """... from one interleaved s16 frame: StreamOracle.frame with its attributes reassigned, except where the ring takes the kind-1 weights"""
    _set(so, k)
    if k.get("avg_window_kind") and so.hist is not None:
        return _oracle_rows(so, Oracle.unpack_s16(pcm, so.channels), k)
    return so.frame(pcm)


def _a_schedule(F):
    """the float schedule plus avg_window_kind 0 -> 1 -> 0 on the float ring"""
    return [dict(k, avg_window_kind=1 if u % 7 in (3, 4) else 0) for u, k in enumerate(float_schedule(updates_of(F)))]


# ---- a. float chains through glv_batch_set_params ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,variant,F", [(n, v, 5) for n, v in SIZES] + [(1024, 0, 1), (1024, 1, 8)])
def test_float_chains_follow_the_oracle_through_set_params(glvlib, oracle, n, variant, F):
    """fft, fft -> gravity, fft -> gravity -> average in both kernel configurations of every size: glv_batch_set_params before every process_s16 call
    (ur and gravity_step on every update, ur = 0, a zero, a negative and a huge step, fft_scale / fft_cutoff twice, avg_window, channels 2 -> 1 -> 2,
    avg_window_kind 0 -> 1 -> 0), every stream against a StreamOracle under the same schedule"""
    import torch
    G = glvlib
    streams = 3 if n < 16384 else 2
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    base = dict(n=n, avg_frames=F, log_mode=0)
    sched = _a_schedule(F)
    chains = [("fft", G.OP_FFT, False, False), ("gravity", G.OP_GRAVITY, True, False), ("chain", GA, True, True)]
    bs, sos = {}, {}
    for name, mask, g, a in chains:
        bs[name] = G.Batch(_params(G, base, sched[0]), streams, mask)
        bs[name].set_variant(variant)
        sos[name] = [StreamOracle(n, avg_frames=F, gravity=g, average=a) for _ in range(streams)]
    for u, k in enumerate(sched):
        x = _frames(1100 + n, u, streams, n)
        d = torch.from_numpy(x).cuda()
        for name, mask, _, _ in chains:
            b = bs[name]
            b.set_params(_params(G, base, k))
            o = _nan(streams * 2, n)
            b.process_s16(d, o, G.OP_FFT | mask)
            assert b.last_variant() == variant and b.last_launches() == 1
            got = o.cpu().numpy()
            for s in range(streams):
                _same(got[2 * s:2 * s + 2], _oracle_frame(sos[name][s], x[s], k), (name, u, s, k))
            if u == 1 and name != "fft": assert np.isneginf(got).all()        # ur = 0
    for b in bs.values(): b.close()


def test_float_chain_knob_changes_from_f32_frames_and_from_the_ring(glvlib, oracle):
    """the same schedule at n = 1024 through glv_batch_process_f32_stereo (the oracle's pulse unpack in front) and through glv_batch_ring_update_s16
    (300 new frames per update: the window is the last n frames of everything appended so far)"""
    import torch
    G = glvlib
    n, F, streams, part = 1024, 5, 3, 300
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    base = dict(n=n, avg_frames=F, log_mode=0)
    sched = _a_schedule(F)
    bf, br = G.Batch(_params(G, base, sched[0]), streams, GA), G.Batch(_params(G, base, sched[0]), streams, GA | G.OP_RING_S16)
    sf, sr = ([StreamOracle(n, avg_frames=F) for _ in range(streams)] for _ in range(2))
    tail = np.zeros((streams, n, 2), np.int16)
    for u, k in enumerate(sched):
        for b in (bf, br): b.set_params(_params(G, base, k))
        x = (_frames(2100, u, streams, n).astype(np.float32) / np.float32(65535)).astype(np.float32)
        x[0, 5::97] = np.float32(-0.0)
        o = _nan(streams * 2, n)
        bf.process_f32_stereo(torch.from_numpy(x).cuda(), o, G.OP_FFT | GA)
        got = o.cpu().numpy()
        for s in range(streams):
            l, r = np.empty(n, np.float32), np.empty(n, np.float32)
            Oracle.lib().glvo_unpack_f32(np.ascontiguousarray(x[s]).reshape(-1), n, k["channels"], l, r)
            _same(got[2 * s:2 * s + 2], _oracle_rows(sf[s], (l, r), k), ("f32 stereo", u, s, k))
        new = _frames(2200, u, streams, part)
        tail = np.concatenate([tail, new], axis=1)[:, -n:]
        o = _nan(streams * 2, n)
        br.ring_update_s16(torch.from_numpy(new).cuda(), part, o, G.OP_FFT | GA)
        got = o.cpu().numpy()
        for s in range(streams):
            _same(got[2 * s:2 * s + 2], _oracle_frame(sr[s], np.ascontiguousarray(tail[s]), k), ("ring", u, s, k))
    bf.close(); br.close()


# ---- b. fused float bars and stateless bars ---------------------------------------------------------------------------------------------------------
def _bar_schedule():
    """bar knobs per update: smooth_factor, bar_phase, the shape (sample_mode average -> maximum -> hybrid -> average, round_formula, sample_scale) and
    bars 80 -> 40 -> 80"""
    S = dict(bars=80, smooth_factor=0.025, bar_phase=0.0, sample_mode=0, round_formula=0, sample_scale=0.0, sample_hybrid_weight=0.0)
    return [dict(S), dict(S, smooth_factor=0.06), dict(S, smooth_factor=0.06, bar_phase=0.5), dict(S, sample_mode=1), dict(S, sample_mode=2, sample_hybrid_weight=0.4),
            dict(S, round_formula=1), dict(S, round_formula=2, sample_scale=6.0), dict(S, bars=40), dict(S, bars=40, smooth_factor=0.01), dict(S)]


def _want_bars(G, row, k, arithmetic):
    """the oracle's bars of one float row in the arithmetic the batch reports: the chunked chains (averaging) or the shader's loop (maximum / hybrid)"""
    assert arithmetic == (G.BARS_F32_SEQ if k["sample_mode"] else G.BARS_F32_CHAIN), (arithmetic, k)
    clean = np.nan_to_num(np.clip(row, 0, 1), nan=0.0).astype(np.float32)                 # the rows enter like texels: clamped
    shape = (k["round_formula"], k["sample_mode"], k["sample_hybrid_weight"], k["sample_scale"], 0.0)
    return _oracle_bars(clean, k["bars"], k["smooth_factor"], k["bar_phase"], shape, chunked=True)


def test_bar_knobs_change_between_updates_of_a_chain_that_fuses_its_bars(glvlib, oracle):
    """fft -> gravity -> average -> 80 bars of a float chain (the transform kernel computes the bars itself where the form allows): after every change of
    the bar knobs the update equals the oracle's bars of the oracle's spectra, and a fresh batch created with those parameters that replays every input --
    output, launches, arithmetic and kernel name"""
    import torch
    G = glvlib
    n, F, streams = 4096, 3, 3
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    base = dict(n=n, avg_frames=F, log_mode=0)
    sched = _bar_schedule()
    b = G.Batch(G.Params(**base, **sched[0]), streams, GA | G.OP_BARS)
    sos = [StreamOracle(n, avg_frames=F) for _ in range(streams)]
    inputs, fused = [], 0
    for u, k in enumerate(sched):
        b.set_params(G.Params(**base, **k))
        inputs.append(torch.from_numpy(_frames(3100, u, streams, n, levels=(4, 16, 64))).cuda())
        o = _nan(streams * 2, k["bars"])
        b.process_s16(inputs[u], o, G.OP_FFT | GA | G.OP_BARS)
        got = o.cpu().numpy()
        fresh = G.Batch(G.Params(**base, **k), streams, GA | G.OP_BARS)
        of = _nan(streams * 2, k["bars"])
        for d in inputs: fresh.process_s16(d, of, G.OP_FFT | GA | G.OP_BARS)
        assert (b.last_launches(), b.bars_arithmetic(), b.kernel_name()) == (fresh.last_launches(), fresh.bars_arithmetic(), fresh.kernel_name()), (u, k)
        fused += b.last_launches() == 1
        _same(got, of.cpu().numpy(), ("fresh batch", u, k))
        for s in range(streams):
            spec = sos[s].frame(inputs[u][s].cpu().numpy())
            for c in range(2):
                _same(got[2 * s + c], _want_bars(G, spec[c], k, b.bars_arithmetic()), ("oracle", u, s, c, k))
        fresh.close()
    assert fused >= 4, fused                                                           # the averaging forms run inside the transform's launch
    b.close()


def test_bar_knobs_change_between_calls_of_stateless_bars(glvlib, oracle):
    """glv_batch_bars on caller rows under the same changes: the oracle's bars, and a fresh batch's"""
    import torch
    G = glvlib
    n, rows = 2048, 6
    spec = (np.random.default_rng(8).random((rows, n), dtype=np.float32) ** 2 * np.float32(1.2) - np.float32(0.03)).astype(np.float32)
    d_spec = torch.from_numpy(spec).cuda()
    sched = _bar_schedule()
    b = G.Batch(G.Params(n=n, **sched[0]), rows // 2, G.OP_FFT | G.OP_BARS)
    for u, k in enumerate(sched):
        b.set_params(G.Params(n=n, **k))
        fresh = G.Batch(G.Params(n=n, **k), rows // 2, G.OP_FFT | G.OP_BARS)
        o, of = _nan(rows, k["bars"]), _nan(rows, k["bars"])
        b.bars(d_spec, o); fresh.bars(d_spec, of)
        assert (b.last_launches(), b.bars_arithmetic()) == (fresh.last_launches(), fresh.bars_arithmetic()), (u, k)
        got = o.cpu().numpy()
        _same(got, of.cpu().numpy(), ("fresh batch", u, k))
        for r in range(rows):
            _same(got[r], _want_bars(G, spec[r], k, b.bars_arithmetic()), ("oracle", u, r, k))
        fresh.close()
    b.close()


# ---- c. the GL_R16 chain in one launch -----------------------------------------------------------------------------------------------------------------
def _want_sm(G, b, texels, factor, phase=0.5):
    """the pre-smoothing pass over one row of `av` texels in the arithmetic the batch reports: the exact integer mean, or the fma chain of the texels' floats"""
    bars = b.params.bars
    if b.bars_arithmetic() == G.BARS_I8_EXACT:
        return Oracle.bars_int(texels, bars, factor, phase)[0]
    assert b.bars_arithmetic() == G.BARS_F32_MATRIX, b.bars_arithmetic()
    want = np.empty(bars, np.float32)
    Oracle.lib().glvo_bars_chunked_at((texels.astype(np.float32) / np.float32(65535)).copy(), texels.size, want, bars, factor, phase)
    return Oracle.texels_r16(want)


@pytest.mark.parametrize("average", [True, False], ids=["average", "gravity"])
@pytest.mark.parametrize("F", [1, 2, 5])
@pytest.mark.parametrize("n,variant", [(512, 0), (4096, 0), (4096, 1), (16384, 0)])
def test_gl_chain_follows_the_model_through_set_params(glvlib, oracle, n, variant, F, average):
    """gl_storage 1 under the GL schedule -- integer and float-evaluated gravity steps in turn, g < 0, g >= 1, ur = 0, avg_window toggles, tilt changes:
    the `av` texels against transform_fft + glvo_gl_chain_r16 with each update's values; the same schedule through the pre-smoothing pass (bars = n,
    bar_phase 0.5), 80 fused bars, a GLV_OP_BARS_ONLY batch (live bins before and after every change) and gl_storage 2 -- all of them agree"""
    import torch
    G = glvlib
    streams = 3 if n < 16384 else 2
    mask = G.OP_GRAVITY | (G.OP_AVERAGE if average else 0)
    ops = G.OP_FFT | mask
    base = dict(n=n, avg_frames=F, avg_window_kind=1, log_mode=0)
    sched = gl_schedule(updates_of(F))
    smooth = dict(bars=n, bar_phase=0.5)
    live_kw = smooth
    mk = lambda gl, more, extra=0: G.Batch(_params(G, base, sched[0], gl_storage=gl, **more), streams, mask | extra)   # noqa: E731
    tex, split = mk(1, {}), mk(2, {})
    sm, b80, s80 = mk(1, smooth, G.OP_BARS), mk(1, dict(bars=80), G.OP_BARS), mk(2, dict(bars=80), G.OP_BARS)
    live, full = mk(1, live_kw, G.OP_BARS | G.OP_BARS_ONLY), mk(1, live_kw, G.OP_BARS)
    every = {"tex": (tex, 1, {}), "split": (split, 2, {}), "sm": (sm, 1, smooth), "b80": (b80, 1, dict(bars=80)), "s80": (s80, 2, dict(bars=80)),
             "live": (live, 1, live_kw), "full": (full, 1, live_kw)}
    for b, _, _ in every.values(): b.set_variant(variant)
    model = _GLModel(streams * 2, n, F, average)
    for u, k in enumerate(sched):
        assert live.live_bins() > 0
        for b, gl, more in every.values(): b.set_params(_params(G, base, k, gl_storage=gl, **more))
        assert live.live_bins() > 0 and full.live_bins() == 0
        x = _frames(4100 + n, u, streams, n, levels=(16, 4, 64))
        d = torch.from_numpy(x).cuda()
        want = model.update(x, k)
        o = _texels(streams * 2, n)
        tex.process_s16(d, o, ops | G.OP_R16)
        assert tex.last_launches() == 1 and tex.last_variant() == variant
        av = _u16(o)
        bad = av != want
        assert not bad.any(), ("model", u, k, int(bad.sum()), np.argwhere(bad)[:3].tolist(), av[bad][:3], want[bad][:3])
        o = _texels(streams * 2, n)
        split.process_s16(d, o, ops | G.OP_R16)
        assert (_u16(o) == want).all(), ("gl_storage 2", u, k)
        o = _texels(streams * 2, n)
        sm.process_s16(d, o, ops | G.OP_BARS | G.OP_R16)
        got_sm = _u16(o)
        for r in range(streams * 2):
            assert (got_sm[r] == _want_sm(G, sm, av[r], 0.025)).all(), ("pre-smoothing pass", u, r, k)
        o, o2 = _nan(streams * 2, 80), _nan(streams * 2, 80)
        b80.process_s16(d, o, ops | G.OP_BARS); s80.process_s16(d, o2, ops | G.OP_BARS)
        got = o.cpu().numpy()
        _same(got, o2.cpu().numpy(), ("80 bars, gl_storage 2", u, k))
        assert b80.bars_arithmetic() == G.BARS_F32_CHAIN
        for r in range(streams * 2):
            _same(got[r], _oracle_bars((av[r].astype(np.float32) / np.float32(65535)).copy(), 80, 0.025, 0.0, (0, 0, 0.0, 0.0, 0.0), chunked=True), ("80 bars", u, r, k))
        w = live_kw["bars"]
        o, o2 = _texels(streams * 2, w), _texels(streams * 2, w)
        live.process_s16(d, o, ops | G.OP_BARS | G.OP_R16); full.process_s16(d, o2, ops | G.OP_BARS | G.OP_R16)
        assert (_u16(o) == _u16(o2)).all(), ("GLV_OP_BARS_ONLY", u, k)
        if w == n: assert (_u16(o) == got_sm).all(), ("GLV_OP_BARS_ONLY against the pre-smoothing pass", u, k)
    for b, _, _ in every.values(): b.close()


# ---- d. the drop-ins with a ur that changes on every call --------------------------------------------------------------------------------------------
def test_float_drop_ins_follow_the_oracle_while_ur_changes_on_every_call(glvlib, oracle):
    """one glv_state per channel, its parameters reassigned before every call as the integration does: glv_fft + glv_gravity + glv_average one by one, and
    glv_fft_gravity_average, against StreamOracle.  Most updates differ from the previous call in ur / gravity_step alone (sync_params' fast path), some
    in fft_scale, avg_window or smooth_factor (the slow path); the three calls of one update, and a repeated update, differ in nothing"""
    G = glvlib
    n, F = 1024, 3
    sched = float_schedule(updates_of(F))
    sched = [dict(k, smooth_factor=0.05 if u in (6, 7) else 0.025) for u, k in enumerate(sched)]
    sched.append(dict(sched[-1]))                                       # ... identical to the call before
    base = dict(n=n, avg_frames=F, log_mode=0)
    sep = [G.State(_params(G, base, sched[0], channels=2)) for _ in range(2)]
    fus = [G.State(_params(G, base, sched[0], channels=2)) for _ in range(2)]
    so_sep, so_fus = StreamOracle(n, avg_frames=F), StreamOracle(n, avg_frames=F)
    for u, k in enumerate(sched):
        pcm = np.ascontiguousarray(_frames(5100, u, 1, n)[0])
        rows = Oracle.unpack_s16(pcm, k["channels"])
        p = _params(G, base, k, channels=2, smooth_factor=k["smooth_factor"])
        want = _oracle_frame(so_sep, pcm, k)
        _same(_oracle_frame(so_fus, pcm, k), want, "the two oracles")
        for c in range(2):
            buf = rows[c].copy()
            sep[c].params = p
            sep[c].fft(buf); sep[c].gravity(buf); sep[c].average(buf)
            _same(buf, want[c], ("one by one", u, c, k))
            buf = rows[c].copy()
            fus[c].params = p
            fus[c].fft_gravity_average(buf)
            _same(buf, want[c], ("fused", u, c, k))
    for s in sep + fus: s.close()


def test_smooth_drop_in_follows_its_bounds_between_calls(glvlib, oracle):
    """glv_smooth with smooth_distance / smooth_ratio (and ur in between) reassigned before every call, against the oracle's transform_smooth"""
    G = glvlib
    n = 1024
    st = G.State(G.Params(n=n))
    x = np.abs(np.random.default_rng(n).standard_normal(n)).astype(np.float32)
    x[::7] = 0
    for dist, ratio, ur in ((0.01, 4.0, 86.0), (0.01, 4.0, 61.5), (0.05, 2.0, 61.5), (0.05, 2.0, 0.0), (0.2, 2.0, 99.0), (0.01, 4.0, 99.0), (0.01, 3.0, 99.0)):
        want = x.copy()
        with np.errstate(all="ignore"):
            Oracle.lib().glvo_smooth(want, n, dist, ratio)
        st.params = G.Params(n=n, smooth_distance=dist, smooth_ratio=ratio, ur=ur)
        got = x.copy(); st.smooth(got)
        assert ((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all(), (dist, ratio, ur)
    st.close()


@pytest.mark.parametrize("smooth", [False, True], ids=["av", "sm"])
def test_gl_texture_drop_in_follows_the_model_while_ur_changes_on_every_call(glvlib, oracle, smooth):
    """glv_gl_texture, one state per channel, under the GL schedule: every call's (gravity_step, ur) differs from the one before -- integer steps, steps the
    kernel evaluates in float, ur = 0 -- through sync_params' fast path; avg_window, the tilt and smooth_factor through the slow one; a repeated update.
    Texels of the model of the batched chain, and with the pre-smoothing pass the exact integer mean over them"""
    G = glvlib
    n, F = 1024, 5
    sched = [dict(k, smooth_factor=0.04 if u in (7, 8) else 0.025) for u, k in enumerate(gl_schedule(updates_of(F)))]
    sched.append(dict(sched[-1]))
    base = dict(n=n, avg_frames=F, avg_window_kind=1, gl_storage=1, log_mode=0, bars=n, bar_phase=0.5)
    st = [G.State(_params(G, base, sched[0])) for _ in range(2)]
    model = _GLModel(2, n, F, True)
    for u, k in enumerate(sched):
        rows = Oracle.unpack_s16(_frames(5200, u, 1, n, levels=(16, 4, 64))[0], 2)
        for c in range(2):
            want = model.row(c, rows[c], k)
            if smooth: want = Oracle.bars_int(want, n, k["smooth_factor"], 0.5)[0]
            st[c].params = _params(G, base, k, smooth_factor=k["smooth_factor"])
            buf, tex = rows[c].copy(), np.zeros(n, np.uint16)
            st[c].gl_texture(buf, tex, smooth)
            assert (buf == rows[c]).all()
            bad = tex != want
            assert not bad.any(), (u, c, k, int(bad.sum()), np.flatnonzero(bad)[:4], tex[bad][:4], want[bad][:4])
    for s in st: s.close()


# ---- e. log_mode and gl_storage 0 <-> 2 on a batch with history ------------------------------------------------------------------------------------
def _tuned_entries(G, tmp_path, n, streams, F, d, o):
    """the wisdom keys of this device for the stateless transform and for the float chain of (n, streams, F), read back from two measured entries"""
    G.wisdom_clear()
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    for mask, ops in ((G.OP_FFT, G.OP_FFT), (GA, G.OP_FFT | GA)):
        b = G.Batch(G.Params(n=n, avg_frames=F, log_mode=0), streams, mask)
        b.autotune(d, o, ops); b.close()
    f = tmp_path / "measured.txt"
    G.wisdom_save(str(f)); G.wisdom_clear()
    entries = [l.split() for l in f.read_text().splitlines() if not l.startswith("#")]
    assert len(entries) == 2 and all(int(e[5]) == 0 for e in entries), entries
    return entries


@pytest.mark.parametrize("n", [4096, 16384])
def test_log_mode_changes_on_a_running_batch(glvlib, oracle, tmp_path, n):
    """log_mode 0 -> 1 -> 0 on a running fft -> gravity -> average batch (at n = 16384 the tilt table changes form: folded under log_mode 1).  With a
    launch wisdom that names another kernel configuration and grid per log mode: after each change a stateless transform on the same batch equals a fresh
    batch's of those parameters bit for bit, in its kernel configuration, grid and kernel name.  The stateful output: the oracle's bits in mode 0, the
    project's 1e-5 contract (chain_close) in mode 1, and after the return to mode 0 the oracle's bits again, its state arrays overwritten with the
    device's (the outputs of a gravity-only batch under the same schedule: what the chain's ring holds)"""
    import torch
    G = glvlib
    streams, F = (3 if n < 16384 else 2), 3
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    base = dict(n=n, avg_frames=F)
    o, og, of, o2 = (_nan(streams * 2, n) for _ in range(4))
    d0 = torch.from_numpy(_frames(6100 + n, 0, streams, n)).cuda()
    try:
        entries = _tuned_entries(G, tmp_path, n, streams, F, d0, o)
        lines = [" ".join(e[:5] + [str(mode), e[6], e[7], str(1 - mode), str(2 + mode), "1.0"]) for e in entries for mode in (0, 1)]
        (tmp_path / "per_mode.txt").write_text("\n".join(lines) + "\n")
        G.wisdom_load(str(tmp_path / "per_mode.txt"))
        assert G.wisdom_count() == 4
        b = G.Batch(G.Params(log_mode=0, **base), streams, GA)
        grav = G.Batch(G.Params(log_mode=0, **base), streams, G.OP_GRAVITY)
        sos = [StreamOracle(n, avg_frames=F) for _ in range(streams)]
        gouts, u = [], 0
        for mode in (0, 1, 0):
            for x in (b, grav): x.set_params(G.Params(log_mode=mode, **base))
            fresh = G.Batch(G.Params(log_mode=mode, **base), streams, G.OP_FFT)
            b.process_s16(d0, of, G.OP_FFT); fresh.process_s16(d0, o2, G.OP_FFT)
            assert (b.last_variant(), b.last_grid(), b.kernel_name()) == (fresh.last_variant(), fresh.last_grid(), fresh.kernel_name()) \
                and b.last_variant() == 1 - mode, (mode, b.last_variant(), b.last_grid(), fresh.last_variant(), fresh.last_grid())
            _same(of.cpu().numpy(), o2.cpu().numpy(), ("stateless transform after the change", mode))
            fresh.close()
            if mode == 0 and u:                                         # the oracle continues from the device's state
                for s in range(streams):
                    sos[s].grav[:] = gouts[-1][2 * s:2 * s + 2]
                    for j in range(u - F, u):
                        sos[s].hist[:, j % F] = gouts[j][2 * s:2 * s + 2]
            for _ in range(F + 1):
                x = _frames(6100 + n, u + 1, streams, n)
                d = torch.from_numpy(x).cuda()
                b.process_s16(d, o, G.OP_FFT | GA); grav.process_s16(d, og, G.OP_FFT | G.OP_GRAVITY)
                assert b.last_variant() == 1 - mode
                got = o.cpu().numpy(); gouts.append(og.cpu().numpy().copy())
                for s in range(streams):
                    want = sos[s].frame(x[s])
                    if mode == 0: _same(got[2 * s:2 * s + 2], want, ("mode 0", u, s))
                    else: assert sos[s].close(got[2 * s:2 * s + 2], want), ("mode 1", u, s, float(np.abs(got[2 * s:2 * s + 2] - want).max()))
                u += 1
        b.close(); grav.close()
    finally:
        G.wisdom_clear()


def test_gl_storage_changes_between_the_float_and_the_pass_by_pass_form_keep_the_state(glvlib, oracle):
    """gl_storage 2 -> 0 -> 2 on a running fft -> gravity -> average batch: "State (gravity, history, rings) is kept" (include/glv_spectrum.h).  The
    expectation is the composition of the oracle's two models over the SAME arrays: StreamOracle's grav / hist / heads are glvo_gl_chain_r16's store / hist
    / head, and back"""
    import torch
    G = glvlib
    n, F, streams = 1024, 3, 3
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    base = dict(n=n, avg_frames=F, avg_window_kind=1, log_mode=0)
    k = dict(float_schedule(6)[0], avg_window_kind=1)
    b = G.Batch(_params(G, base, k, gl_storage=2), streams, GA)
    sos = [StreamOracle(n, avg_frames=F) for _ in range(streams)]
    u = 0
    for gl in (2, 0, 2):
        b.set_params(_params(G, base, k, gl_storage=gl))
        for _ in range(F + 1):
            x = _frames(6500, u, streams, n, levels=(16, 4, 64))
            o = _nan(streams * 2, n)
            b.process_s16(torch.from_numpy(x).cuda(), o, G.OP_FFT | GA)
            got = o.cpu().numpy()
            for s in range(streams):
                so = sos[s]
                if gl == 0: want = _oracle_frame(so, x[s], k)
                else:
                    want = np.empty((2, n), np.float32)
                    for c, samples in enumerate(Oracle.unpack_s16(x[s], 2)):
                        row = Oracle.transform_fft(samples, k["fft_scale"], k["fft_cutoff"])
                        head = C.c_size_t(so.heads[c])
                        Oracle.lib().glvo_gl_chain_r16(row, so.grav[c], so.hist[c], C.byref(head), n, F, 1, 1, k["gravity_step"], k["ur"])
                        so.heads[c] = head.value
                        want[c] = row
                _same(got[2 * s:2 * s + 2], want, ("gl_storage", gl, u, s))
            u += 1
    b.close()


# ---- f. track calls cut at a knob change --------------------------------------------------------------------------------------------------------------
def _pieces(gl):
    """three parameter sets for the three pieces of a recording: ur, gravity_step and avg_window differ, the tilt in the last; on GL_R16 state an integer
    step, one evaluated in float and ur = 0"""
    if gl:
        s = gl_schedule(6)
        return [dict(s[0]), dict(s[1], avg_window=False), dict(s[3], fft_scale=7.0, fft_cutoff=0.5, avg_window=True)]
    s = float_schedule(6)
    return [dict(s[0], channels=2), dict(s[2], channels=2, avg_window=False, fft_scale=10.2, fft_cutoff=0.3), dict(s[4], channels=2, avg_window=True)]


TRACK_N, TRACK_STREAMS, TRACK_F = 1024, 4, 3
TRACK_STEPS = TRACK_F + 2


def _track_case(G, entry):
    """-> (make, base parameters, ops, output width, hop, f32, pieces, call(b, d_pcm, pitch, t0) of one piece)"""
    n, F = TRACK_N, TRACK_F
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    S = TRACK_STEPS
    if entry in ("track", "track_windows", "track_windows_f32"):
        base = dict(n=n, avg_frames=F, log_mode=0)
        ops, hop, f32 = G.OP_FFT | GA, (256 if entry == "track" else 735), entry.endswith("f32")
        make = lambda p: G.Batch(p, TRACK_STREAMS, GA)                                                                    # noqa: E731
        form = "residue" if entry == "track" else "windows"
        call = lambda b, d, pitch, t0: track(b, form, d, pitch, hop, S, ops, n, _f32dt(), t0=t0, f32=f32)                  # noqa: E731
        return make, base, ops, n, hop, f32, _pieces(False), call
    if entry == "track_live":
        base = dict(n=n, avg_frames=F, log_mode=0, bars=80)
        ops, hop = G.OP_FFT | GA | G.OP_BARS, 735
        make = lambda p: G.Batch(p, TRACK_STREAMS, GA | G.OP_BARS | G.OP_BARS_ONLY)                                       # noqa: E731
        call = lambda b, d, pitch, t0: track(b, "live", d, pitch, hop, S, ops, 80, _f32dt(), t0=t0)    # noqa: E731
        pieces = [dict(k, smooth_factor=f) for k, f in zip(_pieces(False), (0.025, 0.05, 0.0125))]
        return make, base, ops, 80, hop, False, pieces, call
    table = np.ascontiguousarray(graph_column_texels(n, 100)[0], np.int64)
    base = dict(n=n, avg_frames=F, avg_window_kind=1, gl_storage=1, log_mode=0, bars=len(table))
    ops, hop = G.OP_FFT | GA | G.OP_BARS, 735

    def make(p):
        b = G.Batch(p, TRACK_STREAMS, GA | G.OP_BARS)
        b.set_column_texels(table)
        return b
    call = lambda b, d, pitch, t0: track(b, "columns", d, pitch, hop, S, ops, len(table), _f32dt(), t0=t0)    # noqa: E731
    pieces = [dict(k, smooth_factor=f) for k, f in zip(_pieces(True), (0.025, 0.05, 0.0125))]
    return make, base, ops, len(table), hop, False, pieces, call


def _f32dt():
    import torch
    return torch.float32


@pytest.mark.parametrize("entry", ["track", "track_windows", "track_windows_f32", "track_live", "track_columns"])
def test_track_calls_cut_at_a_knob_change_equal_the_sequential_calls(glvlib, oracle, entry):
    """a recording in three pieces of F + 2 steps, glv_batch_set_params between the pieces (ur, gravity_step, avg_window, the tilt; smooth_factor too for
    the live bars and the columns): every step of every piece and the state afterwards -- one more process call on both batches -- equal the one-by-one
    process calls under the same schedule; the windows entry also equals the oracle"""
    import torch
    G = glvlib
    make, base, ops, w, hop, f32, pieces, call = _track_case(G, entry)
    n, S = TRACK_N, TRACK_STEPS
    more = lambda k: {key: k[key] for key in ("smooth_factor",) if key in k}                                             # noqa: E731
    bt, bs = make(_params(G, base, pieces[0], **more(pieces[0]))), make(_params(G, base, pieces[0], **more(pieces[0])))
    if entry == "track_live": assert bt.live_bins() > 0
    # glv_batch_track_s16 wants a pitch that is a multiple of its hop; the other entries take an odd pitch and a recording one frame behind an aligned address
    pitch = n + (3 * S + 3) * hop if entry == "track" else pitch_odd(n, hop, 3 * S + 1)
    x = np.array(rec(7100, TRACK_STREAMS, pitch), copy=True) if f32 else pcm(7100, TRACK_STREAMS, pitch)
    d_pcm = to_device(x, entry != "track", f32)
    wins = hop_windows(x, n, hop, 0, 3 * S + 1)
    sos = [StreamOracle(n, avg_frames=TRACK_F) for _ in range(TRACK_STREAMS)] if entry == "track_windows" else []
    for i, k in enumerate(pieces):
        for b in (bt, bs): b.set_params(_params(G, base, k, **more(k)))
        got = call(bt, d_pcm, pitch, i * S)
        want = seq(bs, wins[i * S:(i + 1) * S], ops, w, torch.float32, f32)
        for t in range(S):
            assert eq(got[t], want[t]), (entry, i, t, int((got[t].view(torch.int32) != want[t].view(torch.int32)).sum()))
        assert bool((got != 0).any())
        host = got.cpu().numpy()
        for s, so in enumerate(sos):
            for t in range(S):
                _same(host[t, 2 * s:2 * s + 2], _oracle_frame(so, np.ascontiguousarray(x[s, (i * S + t) * hop:(i * S + t) * hop + n]), k), ("oracle", i, t, s))
        if entry == "track_live": assert bt.live_bins() > 0
    assert eq(seq(bt, wins[3 * S:], ops, w, torch.float32, f32), seq(bs, wins[3 * S:], ops, w, torch.float32, f32)), (entry, "state")
    bt.close(); bs.close()


# ---- g. refused and forced ----------------------------------------------------------------------------------------------------------------------------
def test_a_refused_change_leaves_a_batch_with_bar_texels_as_it_was(glvlib):
    """glv_batch_set_params refused by the validation (channels = 3) and with GLV_ERR_STATE (n, avg_frames, gl_storage across the storage class, gl_storage 0
    and another bar count while a bar-texel table is set), each asking for other tables as well: the next F + 2 updates equal an unperturbed twin's"""
    import torch
    G = glvlib
    n, F, streams = 1024, 3, 3
    tex = radial_bar_texels(n, 160)[0]
    kw = dict(n=n, avg_frames=F, avg_window_kind=1, gl_storage=1, bars=len(tex))
    mask = G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS
    ops = G.OP_FFT | mask | G.OP_R16
    b, twin = G.Batch(G.Params(**kw), streams, mask), G.Batch(G.Params(**kw), streams, mask)
    for x in (b, twin): x.set_bar_texels(tex)
    o, o2 = _texels(streams * 2, len(tex)), _texels(streams * 2, len(tex))

    def step(u):
        d = torch.from_numpy(_frames(8100, u, streams, n, levels=(16, 4, 64))).cuda()
        b.process_s16(d, o, ops); twin.process_s16(d, o2, ops)
        assert eq(o, o2), u
        assert b.last_launches() == twin.last_launches()
    for u in range(2): step(u)
    other = dict(fft_scale=7.0, fft_cutoff=0.5, smooth_factor=0.06, gravity_step=1.0, ur=50.0, log_mode=0)
    _refused(G, b, G.Params(**{**kw, **other, "channels": 3}), G.ERR_INVALID)
    _refused(G, b, G.Params(**{**kw, **other, "n": 2048}), G.ERR_STATE)
    _refused(G, b, G.Params(**{**kw, **other, "avg_frames": F + 1}), G.ERR_STATE)
    _refused(G, b, G.Params(**{**kw, **other, "gl_storage": 2}), G.ERR_STATE)
    _refused(G, b, G.Params(**{**kw, **other, "gl_storage": 0}), G.ERR_STATE)
    _refused(G, b, G.Params(**{**kw, **other, "bars": len(tex) - 1}), G.ERR_STATE)
    for u in range(2, F + 4): step(u)
    b.close(); twin.close()


def test_a_refused_change_leaves_a_batch_that_ran_its_live_class_as_it_was(glvlib):
    """a GLV_OP_BARS_ONLY batch that has run its live class refuses parameters that take the live class away -- AFTER its tables were regenerated for them
    (tilt, bar tables, the gravity step): the restore must bring every one of them back.  The next F + 2 updates equal an unperturbed twin's, the live
    bins are what they were; the refusals that touch nothing (validation, n, avg_frames) likewise"""
    import torch
    G = glvlib
    n, F, streams = 4096, 3, 3
    kw = dict(n=n, avg_frames=F, avg_window_kind=1, gl_storage=1, bars=n, bar_phase=0.5, gravity_step=float(np.float32(100.5) / np.float32(65535)), ur=1.0)
    mask = G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS | G.OP_BARS_ONLY
    ops = G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS | G.OP_R16
    b, twin = G.Batch(G.Params(**kw), streams, mask), G.Batch(G.Params(**kw), streams, mask)
    o, o2 = _texels(streams * 2, n), _texels(streams * 2, n)

    def step(u):
        d = torch.from_numpy(_frames(8200, u, streams, n, levels=(16, 4, 64))).cuda()
        b.process_s16(d, o, ops); twin.process_s16(d, o2, ops)
        assert eq(o, o2), (u, int((o != o2).sum()))
        assert b.last_launches() == twin.last_launches() == 2
    for u in range(F + 1): step(u)
    L = b.live_bins()
    assert L > 0
    other = dict(fft_scale=7.0, fft_cutoff=0.5, smooth_factor=0.06, gravity_step=4.2, ur=86.0, avg_window=False)
    _refused(G, b, G.Params(**{**kw, **other, "log_mode": 2}), G.ERR_STATE)
    assert b.live_bins() == L
    step(F + 1)
    _refused(G, b, G.Params(**{**kw, **other, "channels": 3}), G.ERR_INVALID)
    _refused(G, b, G.Params(**{**kw, **other, "n": 2048}), G.ERR_STATE)
    _refused(G, b, G.Params(**{**kw, **other, "avg_frames": F + 1}), G.ERR_STATE)
    assert b.live_bins() == L and b.bars_arithmetic() == twin.bars_arithmetic()
    for u in range(F + 2, 2 * F + 4): step(u)
    b.close(); twin.close()


def test_a_forced_grid_survives_set_params(glvlib, oracle):
    """glv_batch_set_grid(2), then glv_batch_set_params between updates: the grid stays forced, the output is the automatic grid's (and the oracle's)"""
    import torch
    G = glvlib
    n, F, streams = 1024, 3, 37
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    base = dict(n=n, avg_frames=F, log_mode=0)
    sched = float_schedule(updates_of(F))
    forced, auto = G.Batch(_params(G, base, sched[0]), streams, GA), G.Batch(_params(G, base, sched[0]), streams, GA)
    forced.set_grid(2)
    so = StreamOracle(n, avg_frames=F)
    for u, k in enumerate(sched):
        for b in (forced, auto): b.set_params(_params(G, base, k))
        x = _frames(8300, u, streams, n)
        d = torch.from_numpy(x).cuda()
        o, o2 = _nan(streams * 2, n), _nan(streams * 2, n)
        forced.process_s16(d, o, G.OP_FFT | GA); auto.process_s16(d, o2, G.OP_FFT | GA)
        assert forced.last_grid() == 2 and auto.last_grid() != 2, (u, forced.last_grid(), auto.last_grid())
        assert eq(o, o2), u
        _same(o.cpu().numpy()[:2], _oracle_frame(so, x[0], k), ("oracle", u))
    forced.close(); auto.close()
