"""GPU: the frame kernel's later trips -- forced grids (glv_batch_set_grid) at every size and kernel configuration.

glv_frame_kernel is persistent: a workgroup takes a group of rows, transforms them and strides on by gridDim.x * SLOTS until its share is done.  The
automatic grid gives every workgroup ONE trip until the chip is full, so at the small shapes of the parity tests nothing that lives between two trips
ever runs: the look-ahead load of the slot's next frame, the clamp of an idle slot to the last frame and the `active` flag that keeps its stores away,
the workgroup-uniform break, the track windows' row hand-over, the state prefetch for the next trip's row, the exchange counter carried across trips.
Here the grid is forced to 1, 2 or 3 workgroups (and once to more workgroups than there is work) and the stream count is chosen so that workgroup 0
makes at least three trips, the last trip is ragged and one workgroup stops a trip before another -- computed from the rows per workgroup the library
reports and asserted, so that a retuned configuration cannot quietly turn these into one-trip tests.

Every comparison is bit for bit (floats as int32, texels as uint16): the result does not depend on the grid.

Which loop an input takes (glava_amd/csrc/glv_kernel_tmpl.h): s16 frames, the s16 ring and track windows take the s16 pipeline (one slot = one frame
per trip); planar f32 the planar pipeline (one slot = one row per trip) up to n = 8192; interleaved f32 and the f32 ring the interleaved pipeline (one
slot = one frame) up to n = 8192; the f32 mono mix at every size and every f32 input at n >= 16384 the generic loop (one slot = one row; a single-slot
workgroup both rows of a frame).  The shapes satisfy the three conditions under both ways of counting."""

import ctypes as C
import re

import numpy as np
import pytest

from glava_amd.bar_positions import graph_column_texels, radial_bar_texels
from oracle_lib import Oracle, StreamOracle, lcg_pcm_fast
from gpu_lib import SIZES, bits
from track_lib import compare_hop, eq as _eq, fft_kernel, hop_windows as _windows, launches_fft, pcm as _pcm, pitch_odd as _pitch
from track_lib import s16_chains as _chains, seq as _seq, to_device, track

pytestmark = pytest.mark.gpu

GRIDS = (1, 2, 3)
STEPS = 11


# ---- shapes: what each workgroup does at a forced grid --------------------------------------------------------------------------------------
def _slots(b, variant):
    m = re.search(r"(\d+) row\(s\) per workgroup", b.describe_variant(variant))
    assert m, b.describe_variant(variant)
    return int(m.group(1))


def _trips(work, grid, cap):
    """items (frames or rows) workgroup w takes on each of its trips: trip m of workgroup w covers [(m * grid + w) * cap, + cap) of [0, work), and the
    workgroup leaves at the first trip that starts behind the work (the kernel's uniform break)"""
    out = []
    for w in range(grid):
        mine, m = [], 0
        while (m * grid + w) * cap < work:
            mine.append(min(cap, work - (m * grid + w) * cap))
            m += 1
        out.append(mine)
    return out


def _models(streams, slots, frames_only=False, frames=None):
    """(work, items per workgroup and trip, granularity of the work): the frame-per-slot pipelines count frames; the row-per-slot loops count the
    2 * streams channel rows, a single-slot workgroup taking both rows of a frame per trip"""
    frame = (streams if frames is None else frames, slots, 1)
    return [frame] if frames_only else [frame, (2 * streams, slots if slots > 1 else 2, 2)]


def _conditions(work, grid, cap, unit):
    """the three conditions of a forced grid: workgroup 0 makes at least three trips; the last trip is ragged -- some slots of a workgroup idle, or,
    where the work only comes in whole trips of a workgroup (cap == unit), workgroups make unequal numbers of trips; one workgroup stops a trip before
    another.  One workgroup has nobody to differ from: the last two reduce to the idle slots."""
    t = _trips(work, grid, cap)
    counts = [len(x) for x in t]
    ok = counts[0] >= 3
    if cap > unit: ok = ok and any(0 < x < cap for mine in t for x in mine)
    if grid > 1: ok = ok and min(counts) < max(counts)
    return ok


def _pick_streams(slots, grids, frames_only=False, steps=None, first=1):
    """the smallest stream count at which every grid of `grids` meets the conditions under every way of counting (steps: a track call's
    streams * steps frames)"""
    for streams in range(first, 64 * slots + 64):
        models = _models(streams, slots, frames_only, None if steps is None else streams * steps)
        if all(_conditions(w, g, cap, unit) for g in grids for w, cap, unit in models):
            return streams
    raise AssertionError(f"no stream count meets the trip conditions: {slots} slot(s), grids {grids}")


def _assert_shape(streams, slots, grids, frames_only=False, steps=None):
    """the conditions, asserted on what the test is about to run (and printed: -s shows the shapes)"""
    for w, cap, unit in _models(streams, slots, frames_only, None if steps is None else streams * steps):
        for g in grids:
            t = _trips(w, g, cap)
            assert len(t[0]) >= 3, (w, g, cap, t)
            assert _conditions(w, g, cap, unit), (w, g, cap, t)
    frames = streams if steps is None else streams * steps
    print(f"slots {slots} streams {streams} frames {frames}: trips per workgroup " +
          ", ".join(f"grid {g}: {[len(x) for x in _trips(frames, g, slots)]}" for g in grids))


def _batch(G, p, streams, mask, variant):
    b = G.Batch(p, streams, mask)
    assert b.variants() > variant
    b.set_variant(variant)
    return b


def _frames(seed, streams, n, silent=False):
    """int16 [streams][n][2]: every stream at a level of its own; silent: every fourth stream's frame is all zero"""
    x = lcg_pcm_fast(seed, streams * n * 2).reshape(streams, n, 2).copy()
    for s in range(streams):
        x[s] //= (1, 8, 64)[s % 3]
    if silent: x[1::4] = 0
    return x


def _f32(seed, streams, n):
    """float [streams][n][2] interleaved frames and the same samples as planar rows [streams * 2][n]"""
    x = (np.random.default_rng(seed).standard_normal((streams, n, 2)) * 0.25).astype(np.float32)
    return x, np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(streams * 2, n)


def _fill(rows, w, dt, value):
    import torch
    return torch.full((rows, w), float("nan") if dt == torch.float32 and value is None else (-1 if value is None else value), dtype=dt, device="cuda")


# ---- 1. stateless classes: forced grid == automatic grid --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,variant", SIZES)
def test_stateless_classes_do_not_depend_on_the_grid(glvlib, n, variant):
    """classes 0 and 3 (FFT | RAW, FFT, FFT | R16) of every input kind -- s16 frames, their mono mix, the s16 ring at an odd and at an even rotation,
    planar f32, interleaved f32, its mono mix (the generic loop), the f32 ring -- at the automatic grid, at 1, 2 and 3 workgroups, at more workgroups
    than there is work, and at the automatic grid again after glv_batch_set_grid(0); outputs prefilled with NaN / 0xFFFF"""
    import torch
    G = glvlib
    probe = G.Batch(G.Params(n=n), 1, G.OP_FFT)
    slots = _slots(probe, variant); probe.close()
    streams = _pick_streams(slots, GRIDS)
    _assert_shape(streams, slots, GRIDS)
    # more workgroups than there is work under EITHER way of counting (the row loops stride over 2 * streams rows): ceil(work / per trip) + 3, so at
    # least three workgroups have nothing to do in every loop -- they leave at the first uniform check, their prologue skipped
    big = max(-(-work // cap) for work, cap, _ in _models(streams, slots)) + 3
    for work, cap, _ in _models(streams, slots):
        assert sum(1 for mine in _trips(work, big, cap) if not mine) >= 3, (work, big, cap)
    d_pcm = torch.from_numpy(_frames(100 + n, streams, n)).cuda()
    x_st, x_pl = _f32(200 + n, streams, n)
    d_st, d_pl = torch.from_numpy(x_st).cuda(), torch.from_numpy(x_pl).cuda()
    part = n // 4 + 1                                                # an odd number of frames: one such update leaves an odd rotation, two an even one
    d_part16 = torch.from_numpy(_frames(300 + n, streams, part)).cuda()
    d_part32 = torch.from_numpy(_f32(400 + n, streams, part)[0]).cuda()
    for log_mode in (0, 1, 2) if variant == 0 else (0, 1):
        mask = G.OP_FFT | G.OP_RING_S16 | G.OP_RING_F32
        b = _batch(G, G.Params(n=n, log_mode=log_mode), streams, mask, variant)
        bm = _batch(G, G.Params(n=n, log_mode=log_mode, channels=1), streams, mask, variant)
        kinds = [   # name, the call on (out, ops); a ring's whole-window update leaves its rotation where it was
            ("s16", lambda o, ops: b.process_s16(d_pcm, o, ops)),
            ("s16 mono", lambda o, ops: bm.process_s16(d_pcm, o, ops)),
            ("s16 ring, odd rotation", lambda o, ops: b.ring_update_s16(d_pcm, n, o, ops)),
            ("s16 ring, even rotation", lambda o, ops: b.ring_update_s16(d_pcm, n, o, ops)),
            ("f32 planar", lambda o, ops: b.process_f32(d_pl, o, ops)),
            ("f32 interleaved", lambda o, ops: b.process_f32_stereo(d_st, o, ops)),
            ("f32 interleaved mono", lambda o, ops: bm.process_f32_stereo(d_st, o, ops)),
            ("f32 ring", lambda o, ops: b.ring_update_f32(d_st, n, o, ops)),
        ]
        scratch = torch.empty((streams * 2, n), dtype=torch.float32, device="cuda")
        for name, call in kinds:
            if name.startswith("s16 ring"): b.ring_update_s16(d_part16, part, scratch, G.OP_FFT)
            if name == "f32 ring": b.ring_update_f32(d_part32, part, scratch, G.OP_FFT)
            for ops in (G.OP_FFT | G.OP_RAW, G.OP_FFT, G.OP_FFT | G.OP_R16):
                dt = torch.int16 if ops & G.OP_R16 else torch.float32
                who = bm if "mono" in name else b

                def run(grid):
                    who.set_grid(grid)
                    o = _fill(streams * 2, n, dt, None)
                    call(o, ops)
                    assert who.last_variant() == variant, (name, grid)
                    if grid: assert who.last_grid() == grid, (name, grid, who.last_grid())
                    return o

                call(auto := _fill(streams * 2, n, dt, None), ops)    # before any glv_batch_set_grid on this batch where it is the first call
                auto_grid = who.last_grid()
                if name == "s16": assert 0 < auto_grid <= -(-streams * 2 // slots)
                assert not _eq(auto, _fill(streams * 2, n, dt, None)), (name, "nothing was written")
                for grid in GRIDS + (big,):
                    got = run(grid)
                    assert _eq(got, auto), (name, log_mode, ops, grid, int((got != auto).sum()))
                again = run(0)
                assert who.last_grid() == auto_grid, (name, who.last_grid(), auto_grid)
                assert _eq(again, auto), (name, log_mode, ops, "automatic again")
        b.close(); bm.close()


def test_set_grid_zero_is_the_untouched_batch(glvlib):
    """glv_batch_set_grid(0) (and a negative grid) after a forced grid: the grid an untouched batch of the same shape reports"""
    import torch
    G = glvlib
    n, streams = 1024, 37
    d_pcm = torch.from_numpy(_frames(1, streams, n)).cuda()
    o = torch.empty((streams * 2, n), dtype=torch.float32, device="cuda")
    fresh, b = G.Batch(G.Params(n=n), streams, G.OP_FFT), G.Batch(G.Params(n=n), streams, G.OP_FFT)
    fresh.process_s16(d_pcm, o, G.OP_FFT)
    for grid in (2, 0, 3, -1):
        b.set_grid(grid)
        b.process_s16(d_pcm, o, G.OP_FFT)
        assert b.last_grid() == (grid if grid > 0 else fresh.last_grid()), grid
    fresh.close(); b.close()


# ---- 2. against the oracle directly -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,variant", SIZES)
def test_forced_grid_equals_the_oracle_on_every_stream(glvlib, oracle, n, variant):
    """s16 frames at 1 and 2 workgroups, EVERY stream: the raw FFT against StreamOracle(..., want_raw); with the bit-faithful log (log_mode 0) the float
    chain fft -> gravity -> average against StreamOracle.frame and the GL_R16 chain's texels against glvo_gl_chain_r16 + Oracle.texels_r16, update after
    update, no value excluded"""
    import torch
    G = glvlib
    grids = (1, 2)
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    probe = G.Batch(G.Params(n=n), 1, G.OP_FFT)
    slots = _slots(probe, variant); probe.close()
    streams = _pick_streams(slots, grids, frames_only=True)
    _assert_shape(streams, slots, grids, frames_only=True)
    F = 3 if n >= 16384 else 5
    # raw
    x = _frames(500 + n, streams, n)
    want = [StreamOracle(n, gravity=False, average=False).frame(x[s], want_raw=True)[1] for s in range(streams)]
    for g in grids:
        b = _batch(G, G.Params(n=n), streams, G.OP_FFT, variant)
        b.set_grid(g)
        o = _fill(streams * 2, n, torch.float32, None)
        b.process_s16(torch.from_numpy(x).cuda(), o, G.OP_FFT | G.OP_RAW)
        assert b.last_grid() == g and b.last_variant() == variant
        got = o.cpu().numpy()
        for s in range(streams):
            assert (bits(got[2 * s:2 * s + 2]) == bits(want[s])).all(), ("raw", g, s)
        b.close()
    # the float chain
    bs = [_batch(G, G.Params(n=n, avg_frames=F, log_mode=0), streams, GA, variant) for _ in grids]
    for b, g in zip(bs, grids): b.set_grid(g)
    sos = [StreamOracle(n, avg_frames=F) for _ in range(streams)]
    for u in range(F + 2):
        x = _frames(600 + 7 * u + n, streams, n, silent=u == 2)
        want = [sos[s].frame(x[s]) for s in range(streams)]
        d = torch.from_numpy(x).cuda()
        for b, g in zip(bs, grids):
            o = _fill(streams * 2, n, torch.float32, None)           # (a buffer of its own per grid: a skipped store shows as NaN)
            b.process_s16(d, o, G.OP_FFT | GA)
            assert b.last_grid() == g and b.last_variant() == variant
            got = o.cpu().numpy()
            for s in range(streams):
                diff = bits(got[2 * s:2 * s + 2]) != bits(want[s])
                assert not diff.any(), ("chain", g, u, s, int(diff.sum()), np.argwhere(diff)[:3].tolist())
    for b in bs: b.close()
    # the GL_R16 chain (PCM // 16: the texels do not saturate)
    bs = [_batch(G, G.Params(n=n, avg_frames=F, avg_window_kind=1, gl_storage=1, log_mode=0), streams, GA, variant) for _ in grids]
    for b, g in zip(bs, grids): b.set_grid(g)
    store = np.zeros((streams * 2, n), np.float32); hist = np.zeros((streams * 2, F, n), np.float32)
    heads = [C.c_size_t(0) for _ in range(streams * 2)]
    for u in range(F + 2):
        x = _frames(700 + 7 * u + n, streams, n, silent=u == 2) // 16
        want = np.empty((streams * 2, n), np.uint16)
        for s in range(streams):
            spec = StreamOracle(n, gravity=False, average=False).frame(x[s])
            for c in range(2):
                row = np.ascontiguousarray(spec[c])
                Oracle.lib().glvo_gl_chain_r16(row, store[2 * s + c], hist[2 * s + c], C.byref(heads[2 * s + c]), n, F, 1, 1, 4.2, 86.1328125)
                want[2 * s + c] = Oracle.texels_r16(row)
        d = torch.from_numpy(x).cuda()
        for b, g in zip(bs, grids):
            q = _fill(streams * 2, n, torch.int16, None)
            b.process_s16(d, q, G.OP_FFT | GA | G.OP_R16)
            assert b.last_grid() == g and b.last_variant() == variant and b.last_launches() == 1
            bad = q.cpu().numpy().view(np.uint16) != want
            assert not bad.any(), ("gl chain", g, u, int(bad.sum()), np.argwhere(bad)[:3].tolist())
    for b in bs: b.close()


# ---- 3. stateful and fused classes: forced grid == automatic grid, update by update ---------------------------------------------------------------
def _float_state_cases(G, n):
    S, GA = G.OP_GRAVITY, G.OP_GRAVITY | G.OP_AVERAGE
    return [    # name, params, creation mask, ops, output width, table to set, input kinds
        ("gravity (class 1)", dict(), S, G.OP_FFT | S, n, None, ("s16",)),
        ("gravity | average (class 1)", dict(), GA, G.OP_FFT | GA, n, None, ("s16", "ring_s16", "planar", "stereo")),
        ("gravity | average | r16 (class 4)", dict(), GA, G.OP_FFT | GA | G.OP_R16, n, None, ("s16",)),
        ("80 bars (class 2)", dict(bars=80), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS, 80, None, ("s16",)),
        ("bars only, 80 bars (class 8)", dict(bars=80), GA | G.OP_BARS | G.OP_BARS_ONLY, G.OP_FFT | GA | G.OP_BARS, 80, None, ("s16",)),
    ]


def _gl_state_cases(G, n):
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    gl = dict(gl_storage=1, avg_window_kind=1)
    full, live = GA | G.OP_BARS, GA | G.OP_BARS | G.OP_BARS_ONLY
    chain = G.OP_FFT | GA
    radial, cols = radial_bar_texels(n, 160)[0], graph_column_texels(n, 320)[0]
    return [
        ("GL chain, texels (class 5)", gl, GA, chain | G.OP_R16, n, None, ("s16", "ring_s16", "planar", "stereo")),
        ("GL chain, floats (class 5)", gl, GA, chain, n, None, ("s16",)),
        ("GL chain, 80 bars (class 6)", dict(bars=80, **gl), full, chain | G.OP_BARS, 80, None, ("s16",)),
        ("GL chain, bars = n (the integer pass)", dict(bars=n, bar_phase=0.5, **gl), full, chain | G.OP_BARS | G.OP_R16, n, None, ("s16",)),
        ("bars only, bars = n (class 7)", dict(bars=n, bar_phase=0.5, **gl), live, chain | G.OP_BARS | G.OP_R16, n, None, ("s16",)),
        ("bars only, GL chain, 80 bars (class 9)", dict(bars=80, **gl), live, chain | G.OP_BARS | G.OP_R16, 80, None, ("s16",)),
        ("bar texels (class 10)", dict(bars=len(radial), **gl), full, chain | G.OP_BARS | G.OP_R16, len(radial), ("bar", radial), ("s16",)),
        ("bar texels, bars only (class 11)", dict(bars=len(radial), **gl), live, chain | G.OP_BARS, len(radial), ("bar", radial), ("s16",)),
        ("column texels (class 12)", dict(bars=len(cols), **gl), full, chain | G.OP_BARS, len(cols), ("col", cols), ("s16",)),
        ("column texels, bars only (class 13)", dict(bars=len(cols), **gl), live, chain | G.OP_BARS, len(cols), ("col", cols), ("s16",)),
    ]


def _run_stateful(G, n, variant, cases):
    """two batches from the same parameters, one forced and one automatic; F + 2 updates of fresh input each, compared after every update -- a state
    row written to the wrong place on a later trip shows on the next update"""
    import torch
    probe = G.Batch(G.Params(n=n), 1, G.OP_FFT)
    slots = _slots(probe, variant); probe.close()
    streams = _pick_streams(slots, GRIDS)
    _assert_shape(streams, slots, GRIDS)
    F = 3 if n >= 16384 else 5
    new = min(300, n - 1)                                           # frames per ring update (at most n; n - 1 at n = 256: the rotation moves every update)
    inputs = {}

    def data(kind, u):
        if (kind, u) not in inputs:
            if kind in ("s16", "ring_s16"):
                x = _frames(800 + 7 * u + n, streams, n, silent=u == 2)
                inputs[kind, u] = torch.from_numpy(x if kind == "s16" else np.ascontiguousarray(x[:, :new])).cuda()
            else:
                st, pl = _f32(900 + 7 * u + n, streams, n)
                if u == 2: st[1::4] = 0; pl = np.ascontiguousarray(st.transpose(0, 2, 1)).reshape(streams * 2, n)
                inputs["stereo", u], inputs["planar", u] = torch.from_numpy(st).cuda(), torch.from_numpy(pl).cuda()
        return inputs[kind, u]

    def update(b, kind, u, o, ops):
        if kind == "s16": b.process_s16(data(kind, u), o, ops)
        elif kind == "ring_s16": b.ring_update_s16(data(kind, u), new, o, ops)
        elif kind == "planar": b.process_f32(data(kind, u), o, ops)
        else: b.process_f32_stereo(data(kind, u), o, ops)

    turn = 0
    for name, kw, mask, ops, w, table, kinds in cases:
        for kind in kinds:
            for log_mode in (0, 1):
                g = GRIDS[turn % len(GRIDS)]; turn += 1
                p = G.Params(n=n, avg_frames=F, log_mode=log_mode, **kw)
                m = mask | (G.OP_RING_S16 if kind == "ring_s16" else 0)
                bf, ba = _batch(G, p, streams, m, variant), _batch(G, p, streams, m, variant)
                for b in (bf, ba):
                    if table: (b.set_bar_texels if table[0] == "bar" else b.set_column_texels)(table[1])
                bf.set_grid(g)
                if mask & G.OP_BARS_ONLY:
                    # the live classes (7, 8, 9, 11, 13) run where glv_batch_live_bins != 0: the bins the bars sample -- below 0.288 n plus half a
                    # smoothing window at the shipped parameters -- fit the share of the row every configuration keeps alive (3/8, one half where
                    # the last pass is radix 2 or 4): every size.  A float chain's live class (8) is the fused one, and bars fuse where whole waves
                    # own a row: n >= 1024; below, the batch runs the full chain plus a bars launch under the same contract.  (A configuration
                    # that cannot fuse bars -- n = 16384 configuration 1 -- takes the full chain for classes 8 / 9 as well.)
                    assert bf.live_bins() == ba.live_bins()
                    print(f"{name}: n {n} variant {variant} live bins {bf.live_bins()}")
                    if kw.get("gl_storage", 0) == 1 or n >= 1024: assert bf.live_bins() > 0, (name, n)
                    else: assert bf.live_bins() == 0, (name, n)
                dt = torch.int16 if ops & G.OP_R16 else torch.float32
                of, oa = _fill(streams * 2, w, dt, -1), _fill(streams * 2, w, dt, -2)
                for u in range(F + 2):
                    update(bf, kind, u, of, ops); update(ba, kind, u, oa, ops)
                    assert bf.last_grid() == g and bf.last_variant() == variant and ba.last_variant() == variant, (name, kind, bf.last_grid(), g)
                    assert bf.last_launches() == ba.last_launches()
                    assert _eq(of, oa), (name, kind, log_mode, g, u, int((of != oa).sum()))
                assert bool((of != 0).any()), (name, kind)
                bf.close(); ba.close()


@pytest.mark.parametrize("n,variant", SIZES)
def test_float_state_classes_do_not_depend_on_the_grid(glvlib, n, variant):
    """gravity; gravity | average from s16 frames, the s16 ring, planar and interleaved f32; as texels; with 80 bars (fused where whole waves own a row,
    a second launch elsewhere: the same contract); a GLV_OP_BARS_ONLY batch with 80 bars -- log modes 0 and 1, the forced grid cycling over 1, 2, 3"""
    _run_stateful(glvlib, n, variant, _float_state_cases(glvlib, n))


@pytest.mark.parametrize("n,variant", SIZES)
def test_gl_state_classes_do_not_depend_on_the_grid(glvlib, n, variant):
    """the GL_R16 chain as texels (from s16 frames, the s16 ring, planar and interleaved f32) and as floats; with 80 bars; with the pre-smoothing pass
    (bars = n, bar_phase 0.5: the integer pass) -- log modes 0 and 1, the forced grid cycling over 1, 2, 3"""
    _run_stateful(glvlib, n, variant, _gl_state_cases(glvlib, n)[:4])


@pytest.mark.parametrize("n,variant", SIZES)
def test_gl_bars_only_classes_do_not_depend_on_the_grid(glvlib, n, variant):
    """GLV_OP_BARS_ONLY batches of the GL_R16 chain, with the pre-smoothing pass in a second launch (class 7) and with 80 bars fused (class 9)"""
    _run_stateful(glvlib, n, variant, _gl_state_cases(glvlib, n)[4:6])


@pytest.mark.parametrize("n,variant", SIZES)
def test_bar_texel_classes_do_not_depend_on_the_grid(glvlib, n, variant):
    """bar texels (glv_batch_set_bar_texels), without and with GLV_OP_BARS_ONLY (classes 10 / 11)"""
    _run_stateful(glvlib, n, variant, _gl_state_cases(glvlib, n)[6:8])


@pytest.mark.parametrize("n,variant", SIZES)
def test_column_texel_classes_do_not_depend_on_the_grid(glvlib, n, variant):
    """column texels (glv_batch_set_column_texels), without and with GLV_OP_BARS_ONLY (classes 12 / 13)"""
    _run_stateful(glvlib, n, variant, _gl_state_cases(glvlib, n)[8:])


# ---- 4. track windows -----------------------------------------------------------------------------------------------------------------------
def _track_shape(G, n, variant, grids):
    probe = G.Batch(G.Params(n=n), 1, G.OP_FFT)
    slots = _slots(probe, variant); probe.close()
    streams = _pick_streams(slots, grids, frames_only=True, steps=STEPS, first=2)       # (two streams at least: rows of a second stream exist)
    _assert_shape(streams, slots, grids, frames_only=True, steps=STEPS)
    return streams


@pytest.mark.parametrize("n,variant", SIZES)
def test_track_windows_at_forced_grids(glvlib, n, variant):
    """glv_batch_track_windows_s16 at 1 and 2 workgroups, 11 steps, hop 45 and n + 3, the recording aligned and one frame off: `fft` (step-major rows
    straight into d_out), `fft_r16`, `chain` (stream-major rows, then the scan) and `gl_chain_r16` against sequential glv_batch_process_s16 calls at the
    automatic grid on a second batch, output and -- through one more update on both -- state (track_lib.compare)"""
    G = glvlib
    grids = (1, 2)
    streams = _track_shape(G, n, variant, grids)
    for chain in ("fft", "fft_r16", "chain", "gl_chain_r16"):
        kw, mask, ops = _chains(G)[chain]
        p = G.Params(n=n, **kw)
        bt, bs = _batch(G, p, streams, mask, variant), G.Batch(p, streams, mask)
        for hop in (45, n + 3):
            for odd in (False, True):
                for g in grids:
                    bt.reset(); bs.reset()
                    bt.set_grid(g)
                    pitch = _pitch(n, hop, STEPS + 1)
                    compare_hop(G, bt, bs, "windows", _pcm(41 + g + n + hop, streams, pitch), odd, pitch, hop, n, STEPS, ops, n, launches_fft(G, ops),
                                fft_kernel(G, ops))
                    assert bt.last_grid() == g and bt.last_variant() == variant, (chain, hop, odd, bt.last_grid())
        bt.close(); bs.close()


@pytest.mark.parametrize("n,variant", SIZES)
def test_track_windows_at_a_forced_grid_equals_the_oracle(glvlib, oracle, n, variant):
    """log_mode 0, fft -> gravity -> average at hop 45 and one workgroup: every step of the LAST stream (its frames are the last trips') equals
    StreamOracle.frame on that window bit for bit"""
    import torch
    G = glvlib
    hop, F = 45, 5
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    streams = _track_shape(G, n, variant, (1,))
    pitch = _pitch(n, hop, STEPS)
    x = _pcm(5150 + n, streams, pitch)
    b = _batch(G, G.Params(n=n, avg_frames=F, log_mode=0), streams, GA, variant)
    b.set_grid(1)
    got = track(b, "windows", to_device(x, True, False), pitch, hop, STEPS, G.OP_FFT | GA, n, torch.float32).cpu().numpy()
    assert b.last_grid() == 1 and b.last_variant() == variant
    s = streams - 1
    so = StreamOracle(n, avg_frames=F)
    for t in range(STEPS):
        want = so.frame(x[s, t * hop:t * hop + n, :])
        assert (got[t, 2 * s:2 * s + 2].view(np.uint32) == want.view(np.uint32)).all(), t
    b.close()


@pytest.mark.parametrize("n", [256, 1024, 8192])
def test_track_residue_launches_at_a_forced_grid(glvlib, n):
    """glv_batch_track_s16 at hop n / 4 and one workgroup: each of its four residue launches makes three trips or more, the last one ragged; `chain` and
    `gl_chain_r16` against sequential calls at the automatic grid, output and state"""
    import torch
    G = glvlib
    hop = n // 4
    pitch = (STEPS + 4) * hop + n                                   # a multiple of the hop: the residue entry asks for it
    probe = G.Batch(G.Params(n=n), 1, G.OP_FFT)
    slots = _slots(probe, 0); probe.close()

    def shape_ok(streams):
        ks = G.track_residues(n, hop, pitch, streams, STEPS)
        return all(len(_trips(k, 1, slots)[0]) >= 3 for k in ks) and (slots == 1 or any(k % slots for k in ks))

    streams = next(s for s in range(2, 64) if shape_ok(s))
    assert shape_ok(streams)
    print(f"n {n}: slots {slots} streams {streams}, windows per residue launch {G.track_residues(n, hop, pitch, streams, STEPS)}")
    x = _pcm(77 + n, streams, pitch)
    d_pcm = to_device(x, False, False)
    wins = _windows(x, n, hop, 0, STEPS + 1)
    for chain in ("chain", "gl_chain_r16"):
        kw, mask, ops = _chains(G)[chain]
        p = G.Params(n=n, **kw)
        dt = torch.int16 if ops & G.OP_R16 else torch.float32
        bt, bs = G.Batch(p, streams, mask), G.Batch(p, streams, mask)
        bt.set_grid(1)
        got = track(bt, "residue", d_pcm, pitch, hop, STEPS, ops, n, dt)
        assert bt.last_grid() == 1 and bt.last_launches() == n // hop + 1
        want = _seq(bs, wins[:STEPS], ops, n, dt)
        for t in range(STEPS):
            assert _eq(got[t], want[t]), (chain, t, int((got[t] != want[t]).sum()))
        assert _eq(_seq(bt, wins[STEPS:], ops, n, dt), _seq(bs, wins[STEPS:], ops, n, dt)), (chain, "state")
        bt.close(); bs.close()
